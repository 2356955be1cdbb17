"""The split-key decode attention against the code it would replace, ONE process per geometry, interleaved A/B on shared-prefix
beam caches over the same prefilled prompts at the same position.

`--pairs` times: `--steps` steps of one side, then of the other -- in ABBA order, each block behind one untimed step.
  --chain  B x beam cases of the default batched loop (9..32 rows), two measurements each:
             "step":   the decode step alone, eager on both sides (pcy_llama_decode against pcy_llama_decode_split; neither side picks or
                       advances: every step appends at the same slot) -- the library has no captured decode-only graph on the split side;
             "all-in": the replayed beam-search chain (pcy_llama_beam_steps, the yardstick and unchanged code, against
                       pcy_llama_beam_steps_split): decode + logits record + beam step + K / V reorder, one graph launch per step.
  --gemm   B x beam cases of the GEMM step: decode_gemm(shared_attn=True) against decode_gemm(shared_attn="split"), the step alone.
Prints one line per block and a summary per case (median ms per step of both sides, new / old per pair, the spread of the pairs).

  python tools/bench_attn_split.py --geom full  --T 512
  python tools/bench_attn_split.py --geom split --T 704"""
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
ap.add_argument("--chain", default="1x10,1x20,2x10,1x32", help="B x beam cases of the default loop, comma separated ('' = none)")
ap.add_argument("--gemm", default="4x10,16x10", help="B x beam cases of the GEMM step ('' = none)")
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
assert args.pairs >= 1 and 1 <= args.steps <= 8
SIDES = ("old", "split")


def summary(what, old_name, ms, extra=""):
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratios = [n / o for n, o in zip(ms["split"], ms["old"])]
    wins = sum(r < 1 for r in ratios)
    print(f"SUMMARY {args.geom} L{kw['n_layers']} T{T} {what}: {old_name} {med['old']:.4f} split {med['split']:.4f} ms/step (median of {args.pairs}); "
          f"split/{old_name} per pair min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f}; split won {wins} of {len(ratios)} "
          f"pairs; {old_name} spread {min(ms['old']):.4f}..{max(ms['old']):.4f} split spread {min(ms['split']):.4f}..{max(ms['split']):.4f}{extra}", flush=True)


def abba(what, blocks):
    ms = {k: [] for k in blocks}
    for p in range(args.pairs):
        for k in (SIDES if p % 2 == 0 else SIDES[::-1]):      # ABBA: neither side always runs first
            ms[k].append(blocks[k]())
            print(f"{args.geom} T{T} {what} pair {p} {k:5s} {ms[k][-1]:.4f} ms/step", flush=True)
    return ms


prefixes = {}


def prefill(B):
    if B not in prefixes:
        emb = (torch.randn(B, T, kw["d"], device="cuda") * 0.02).bfloat16()
        prefix = eng.new_cache(B, T)
        lg, _ = eng.prefill(emb, None, prefix, "last")
        ctx.sync()
        prefixes[B] = (prefix, lg)
    return prefixes[B]


def step_alone(what, old_name, B, beam, steps_fn):
    """steps_fn: side -> (cache, st, BB) -> None"""
    BB = B * beam
    prefix, lg = prefill(B)
    st = GenState(BB, V, 2, "cuda")
    st.pos.fill_(T)
    st.next_tok.copy_(lg.float().argmax(-1).to(torch.int32).repeat_interleave(beam))
    caches = {k: eng.new_beam_cache(prefix, beam, 2) for k in SIDES}

    def block(k):
        steps_fn[k](caches[k], st, BB)                       # untimed: warms the launches
        ctx.sync()
        ctx.timer_start()
        for _ in range(args.steps):
            steps_fn[k](caches[k], st, BB)
        return ctx.timer_stop() / args.steps

    n0 = lib.pcy_debug_attn_split_count()
    ms = abba(f"{what} {B}x{beam}", {k: (lambda k=k: block(k)) for k in SIDES})
    assert lib.pcy_debug_attn_split_count() - n0 == args.pairs * (args.steps + 1)
    summary(f"{what} {B}x{beam} ({BB} rows)", old_name, ms)


max_new = args.pairs * (args.steps + 1) + 2
for B, beam in parse(args.chain):
    BB = B * beam
    step_alone("step", "default", B, beam, {"old": eng.decode, "split": eng.decode_split})
    prefix, lg = prefill(B)
    logits = lg.repeat_interleave(beam, dim=0).contiguous()

    class Side:
        def __init__(self, split):
            self.split = split
            self.cache = eng.new_beam_cache(prefix, beam, max_new)
            self.bs = BeamState(B, beam, max_new, -1, prompt_len=T, device="cuda")      # (eos -1: the search never stops)
            self.st = self.bs.gen_state(V)
            self.rec = torch.empty(max_new, BB, V, dtype=torch.bfloat16, device="cuda")
            eng.beam_step(logits, self.bs, args.group, 0.8)
            eng.kv_reorder(self.cache, self.bs.src, T, t0=T)

        def run(self, n):
            eng.beam_steps(self.cache, self.st, self.bs, args.group, 0.8, self.rec, n, kv_t0=T, split=self.split)

        def block(self):
            self.run(1)                                      # untimed: captures this side's chain (the two never share a graph)
            ctx.sync()
            ctx.timer_start(); self.run(args.steps); return ctx.timer_stop() / args.steps

    sides = {"old": Side(False), "split": Side(True)}
    ms = abba(f"chain {B}x{beam}", {k: s.block for k, s in sides.items()})
    ctx.sync()
    same = torch.equal(sides["old"].bs.out, sides["split"].bs.out)
    summary(f"chain {B}x{beam} ({BB} rows) all-in", "default", ms, f"; same tokens as the default side: {same} (not promised)")
    del sides
    torch.cuda.empty_cache()

for B, beam in parse(args.gemm):
    step_alone("gemm step", "mq", B, beam, {"old": lambda c, s, n: eng.decode_gemm(c, s, n, shared_attn=True),
                                             "split": lambda c, s, n: eng.decode_gemm(c, s, n, shared_attn="split")})
