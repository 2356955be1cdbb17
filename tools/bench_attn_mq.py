"""The GEMM decode step with the many-queries attention (pcy_llama_decode_gemm_mq) against the same step with the default
attention launch (pcy_llama_decode_gemm: the yardstick, unchanged code), ONE process, interleaved A/B on shared-prefix beam caches.

Per case B x beam the B prompts are prefilled once; both sides decode from beam caches over that prefix, at the same position.  `--pairs`
times: `--steps` steps without shared_attn, then `--steps` with it -- in ABBA order, each block behind one untimed step.  `--cases`: the step
alone (neither side picks or advances: every step appends at the same slot).  `--allin`: generate_beam's four-call body (decode + logits record
+ beam step + K / V reorder) per step.  Prints one line per block and a summary per case (median ms per step of both sides, mq / plain per
pair, the spread of the pairs).

  python tools/bench_attn_mq.py --geom full  --T 512 --cases 16x10,8x10,4x10,2x20 --allin 16x10,8x10
  python tools/bench_attn_mq.py --geom split --T 704 --cases 16x10,8x10,4x10,2x20 --allin 16x10,8x10"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from procyon_amd import _lib, synth
from procyon_amd.engine import BeamState, Context, GenState, LlamaConfig, LlamaEngine

GEOMS = {"full": dict(vocab=128263, d=4096, n_layers=32, n_heads=32, n_kv_heads=8, ffn=14336),
         "split": dict(vocab=32007, d=4096, n_layers=32, n_heads=32, n_kv_heads=32, ffn=11008)}
ap = argparse.ArgumentParser()
ap.add_argument("--geom", default="full", choices=list(GEOMS))
ap.add_argument("--T", type=int, default=512, help="prompt tokens (the shared prefix)")
ap.add_argument("--cases", default="16x10,8x10,4x10,2x20", help="B x beam cases of the step alone, comma separated ('' = none)")
ap.add_argument("--allin", default="16x10,8x10", help="B x beam cases of the beam search's step all-in ('' = none)")
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
parse = lambda s: [tuple(int(x) for x in c.split("x")) for c in s.split(",") if c]
assert args.pairs >= 1 and args.steps >= 1
SIDES = ("plain", "mq")


def summary(what, ms, extra=""):
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratios = [n / o for n, o in zip(ms["mq"], ms["plain"])]
    wins = sum(r < 1 for r in ratios)
    print(f"SUMMARY {args.geom} L{kw['n_layers']} T{T} {what}: plain {med['plain']:.4f} mq {med['mq']:.4f} ms/step (median of {args.pairs}); "
          f"mq/plain per pair min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f}; mq won {wins} of {len(ratios)} pairs; "
          f"plain spread {min(ms['plain']):.4f}..{max(ms['plain']):.4f} mq spread {min(ms['mq']):.4f}..{max(ms['mq']):.4f}{extra}", flush=True)


def abba(what, blocks):
    ms = {k: [] for k in blocks}
    for p in range(args.pairs):
        for k in (SIDES if p % 2 == 0 else SIDES[::-1]):      # ABBA: neither side always runs first
            ms[k].append(blocks[k]())
            print(f"{args.geom} T{T} {what} pair {p} {k:5s} {ms[k][-1]:.4f} ms/step", flush=True)
    return ms


def prefill(B):
    emb = (torch.randn(B, T, kw["d"], device="cuda") * 0.02).bfloat16()
    prefix = eng.new_cache(B, T)
    lg, _ = eng.prefill(emb, None, prefix, "last")
    ctx.sync()
    return prefix, lg


max_new = args.pairs * (args.steps + 1) + 2
prefixes = {}
for B, beam in parse(args.cases):
    BB = B * beam
    if B not in prefixes:
        prefixes[B] = prefill(B)
    prefix, lg = prefixes[B]
    st = GenState(BB, V, 2, "cuda")
    st.pos.fill_(T)
    st.next_tok.copy_(lg.float().argmax(-1).to(torch.int32).repeat_interleave(beam))
    caches = {k: eng.new_beam_cache(prefix, beam, 2) for k in SIDES}

    def block(k, BB=BB, st=st, caches=caches):
        eng.decode_gemm(caches[k], st, BB, shared_attn=k == "mq")      # untimed: warms the launches
        ctx.sync()
        ctx.timer_start()
        for _ in range(args.steps):
            eng.decode_gemm(caches[k], st, BB, shared_attn=k == "mq")
        return ctx.timer_stop() / args.steps

    n0 = lib.pcy_debug_attn_mq_count()
    ms = abba(f"step {B}x{beam}", {k: (lambda k=k: block(k)) for k in SIDES})
    assert lib.pcy_debug_attn_mq_count() - n0 == args.pairs * (args.steps + 1)
    summary(f"step {B}x{beam} ({BB} rows)", ms)
    del caches

for B, beam in parse(args.allin):
    BB = B * beam
    if B not in prefixes:
        prefixes[B] = prefill(B)
    prefix, lg = prefixes[B]
    logits = lg.repeat_interleave(beam, dim=0).contiguous()
    rec = torch.empty(BB, V, dtype=torch.bfloat16, device="cuda")

    class Side:
        def __init__(self, mq):
            self.mq, self.i = mq, 0
            self.cache = eng.new_beam_cache(prefix, beam, max_new)
            self.bs = BeamState(B, beam, max_new, -1, prompt_len=T, device="cuda")      # (eos -1: the search never stops)
            self.st = self.bs.gen_state(V)
            eng.beam_step(logits, self.bs, args.group, 0.8)
            eng.kv_reorder(self.cache, self.bs.src, T, t0=T)

        def run(self, n):
            for _ in range(n):                       # generate_beam's four-call body without the record copy's destination: a scratch row
                self.i += 1
                eng.decode_gemm(self.cache, self.st, BB, shared_attn=self.mq)
                rec.copy_(self.st.logits)
                eng.beam_step(self.st.logits, self.bs, args.group, 0.8)
                eng.kv_reorder(self.cache, self.bs.src, T + self.i, t0=T)

        def block(self):
            self.run(1)
            ctx.sync()
            ctx.timer_start(); self.run(args.steps); return ctx.timer_stop() / args.steps

    sides = {"plain": Side(False), "mq": Side(True)}
    ms = abba(f"beam {B}x{beam}", {k: s.block for k, s in sides.items()})
    ctx.sync()
    same = torch.equal(sides["plain"].bs.out, sides["mq"].bs.out)
    summary(f"beam {B}x{beam} ({BB} rows) all-in", ms, f"; same tokens as the plain side: {same} (not promised)")
    del sides, rec
    torch.cuda.empty_cache()
