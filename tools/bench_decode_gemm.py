"""The one-pass GEMM decode step (pcy_llama_decode_gemm) against the default step above 32 rows, ONE process, interleaved A/B.

Per geometry the prompts of the widest case are prefilled once; every row count decodes the first `rows` rows of that cache, at the same
position.  Per case `--pairs` times: `--steps` default steps (pcy_llama_decode_graph: the replayed launch-per-stage loop, 32-row passes over
the weights), then `--steps` new steps (eager: one launch per stage, never captured) -- in ABBA order, each block behind one untimed step.
Neither side picks or advances: every step appends at the same slot.  `--beam BxK,...`: the beam search's step all-in (decode + logits record +
beam step + K / V reorder) on the shared-prefix cache, the replayed chain (pcy_llama_beam_steps) against the four calls with the new step.
Prints one line per block and a summary per case (median ms per step of both sides, new / default per pair, the spread of the pairs).

  python tools/bench_decode_gemm.py --geom full  --T 512 --rows 33,40,64,80,160 --beam 8x10,16x10
  python tools/bench_decode_gemm.py --geom split --T 704 --rows 33,40,64,80,160 --beam 8x10,16x10"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from procyon_amd import _lib, synth
from procyon_amd.engine import BeamState, Context, GenState, LlamaConfig, LlamaEngine, decode_gemm_plan

GEOMS = {"full": dict(vocab=128263, d=4096, n_layers=32, n_heads=32, n_kv_heads=8, ffn=14336),
         "split": dict(vocab=32007, d=4096, n_layers=32, n_heads=32, n_kv_heads=32, ffn=11008)}
ap = argparse.ArgumentParser()
ap.add_argument("--geom", default="full", choices=list(GEOMS))
ap.add_argument("--T", type=int, default=512, help="cached tokens per row")
ap.add_argument("--rows", default="33,40,64,80,160", help="row counts of the decode-step cases, comma separated ('' = none)")
ap.add_argument("--beam", default="", help="beam-search cases B x beam, comma separated, e.g. 8x10,16x10")
ap.add_argument("--layers", type=int, default=0, help="decoder layers (0: the geometry's 32)")
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--group", type=int, default=2)
args = ap.parse_args()
kw = dict(GEOMS[args.geom])
if args.layers:
    kw["n_layers"] = args.layers
eng = LlamaEngine(synth.llama_state_dict(**kw, device="cuda"), LlamaConfig(**kw, max_pos=4096), free_source=True)
ctx, lib = Context.get(), _lib.load()
V, T = kw["vocab"], args.T
mha = kw["n_heads"] == kw["n_kv_heads"]
rows = [int(x) for x in args.rows.split(",") if x]
beams = [tuple(int(x) for x in c.split("x")) for c in args.beam.split(",") if c]
assert args.pairs >= 1 and args.steps >= 1


def summary(what, ms, extra=""):
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratios = [n / o for n, o in zip(ms["gemm"], ms["default"])]
    wins = sum(r < 1 for r in ratios)
    print(f"SUMMARY {args.geom} L{kw['n_layers']} T{T} {what}: default {med['default']:.4f} gemm {med['gemm']:.4f} ms/step (median of {args.pairs}); "
          f"gemm/default per pair min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f}; gemm won {wins} of {len(ratios)} pairs; "
          f"default spread {min(ms['default']):.4f}..{max(ms['default']):.4f} gemm spread {min(ms['gemm']):.4f}..{max(ms['gemm']):.4f}{extra}", flush=True)


def abba(what, blocks):
    ms = {k: [] for k in blocks}
    for p in range(args.pairs):
        for k in (("default", "gemm") if p % 2 == 0 else ("gemm", "default")):      # ABBA: neither side always runs first
            ms[k].append(blocks[k]())
            print(f"{args.geom} T{T} {what} pair {p} {k:7s} {ms[k][-1]:.4f} ms/step", flush=True)
    return ms


# ---- the decode step alone
if rows:
    Bmax = max(rows)
    cache = eng.new_cache(Bmax, T + 2)
    emb = (torch.randn(Bmax, T, kw["d"], device="cuda") * 0.02).bfloat16()
    # the prefill in slices of 16 rows (its workspace grows with rows x T), each into a cache of its own, copied into the wide cache
    lg = torch.empty(Bmax, V, dtype=torch.bfloat16, device="cuda")
    for r0 in range(0, Bmax, 16):
        n = min(16, Bmax - r0)
        part = eng.new_cache(n, T + 2)
        lg[r0:r0 + n], _ = eng.prefill(emb[r0:r0 + n], None, part, "last")
        ctx.sync()
        cache.k[:, r0:r0 + n].copy_(part.k); cache.v[:, r0:r0 + n].copy_(part.v)
        del part
    torch.cuda.synchronize()
    for B in rows:
        st = GenState(B, V, 2, "cuda")
        st.pos.fill_(T)
        st.next_tok.copy_(lg[:B].float().argmax(-1).to(torch.int32))

        def block(fn, B=B, st=st):
            fn(cache, st, B)                         # untimed: captures the graph / warms the launches
            ctx.sync()
            ctx.timer_start()
            for _ in range(args.steps):
                fn(cache, st, B)
            return ctx.timer_stop() / args.steps

        n0 = lib.pcy_debug_decode_gemm_count()
        ms = abba(f"rows {B}", {"default": lambda: block(eng.decode_graph), "gemm": lambda: block(eng.decode_gemm)})
        assert lib.pcy_debug_decode_gemm_count() - n0 == args.pairs * (args.steps + 1)
        summary(f"rows {B}", ms, f"; plan(auto)={decode_gemm_plan(B, False, mha)}")
    del cache, emb
    torch.cuda.empty_cache()

# ---- the beam search's step all-in, on the shared-prefix cache
max_new = args.pairs * (args.steps + 1) + 2
for B, beam in beams:
    BB = B * beam
    emb = (torch.randn(B, T, kw["d"], device="cuda") * 0.02).bfloat16()
    prefix = eng.new_cache(B, T)
    lg, _ = eng.prefill(emb, None, prefix, "last")
    ctx.sync()
    logits = lg.repeat_interleave(beam, dim=0).contiguous()

    class Side:
        def __init__(self, gemm):
            self.gemm, self.i = gemm, 0
            self.cache = eng.new_beam_cache(prefix, beam, max_new)
            self.bs = BeamState(B, beam, max_new, -1, prompt_len=T, device="cuda")      # (eos -1: the search never stops)
            self.st = self.bs.gen_state(V)
            eng.beam_step(logits, self.bs, args.group, 0.8)
            eng.kv_reorder(self.cache, self.bs.src, T, t0=T)

        def run(self, n):
            if not self.gemm:
                eng.beam_steps(self.cache, self.st, self.bs, args.group, 0.8, None, n, kv_t0=T)
                self.i += n
                return
            for _ in range(n):                       # generate_beam's four-call body without the record copy's destination: a scratch row
                self.i += 1
                eng.decode_gemm(self.cache, self.st, BB)
                rec.copy_(self.st.logits)
                eng.beam_step(self.st.logits, self.bs, args.group, 0.8)
                eng.kv_reorder(self.cache, self.bs.src, T + self.i, t0=T)

        def block(self):
            self.run(1)
            ctx.sync()
            ctx.timer_start(); self.run(args.steps); return ctx.timer_stop() / args.steps

    rec = torch.empty(BB, V, dtype=torch.bfloat16, device="cuda")
    sides = {"default": Side(False), "gemm": Side(True)}
    ms = abba(f"beam {B}x{beam}", {k: s.block for k, s in sides.items()})
    ctx.sync()
    same = torch.equal(sides["default"].bs.out, sides["gemm"].bs.out)
    summary(f"beam {B}x{beam} ({BB} rows) all-in", ms, f"; same tokens as the default chain: {same} (not promised)")
    del sides, prefix, rec
    torch.cuda.empty_cache()
