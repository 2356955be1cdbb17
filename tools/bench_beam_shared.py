"""Beam step on a shared-prefix cache against its twin on the plain cache, ONE process, interleaved A/B.

Per case B x beam x T: the prompts are prefilled once; the plain cache gets its B*beam rows by the replicating pcy_kv_reorder (timed: the
one-time cost after the prefill), the shared cache wraps a B-row prefix cache.  Then `--pairs` times: `--steps` replayed beam steps
(pcy_llama_beam_steps: decode + logits record + beam step + K / V reorder, all-in) on the plain cache, the same on the shared cache -- each
block behind one untimed step that captures the chain.  Both sides walk the same positions.  Prints one line per block and a summary per case
(median ms per step of both sides, the spread of the pairs, cache bytes).

  python tools/bench_beam_shared.py --geom full  --cases 1x10x512,1x20x512,16x10x512
  python tools/bench_beam_shared.py --geom split --cases 1x10x704,1x20x704"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from procyon_amd import synth
from procyon_amd.engine import BeamState, Context, LlamaConfig, LlamaEngine, beam_cache_plan

GEOMS = {"full": dict(vocab=128263, d=4096, n_layers=32, n_heads=32, n_kv_heads=8, ffn=14336),
         "split": dict(vocab=32007, d=4096, n_layers=32, n_heads=32, n_kv_heads=32, ffn=11008)}
ap = argparse.ArgumentParser()
ap.add_argument("--geom", default="full", choices=list(GEOMS))
ap.add_argument("--cases", default="1x10x512,1x20x512,16x10x512", help="B x beam x T, comma separated")
ap.add_argument("--layers", type=int, default=0, help="decoder layers (0: the geometry's 32)")
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--steps", type=int, default=16)
ap.add_argument("--group", type=int, default=2)
args = ap.parse_args()
kw = dict(GEOMS[args.geom])
if args.layers:
    kw["n_layers"] = args.layers
eng = LlamaEngine(synth.llama_state_dict(**kw, device="cuda"), LlamaConfig(**kw, max_pos=4096), free_source=True)
ctx = Context.get()
V = kw["vocab"]
max_new = args.pairs * (args.steps + 1) + 2


class Side:
    def __init__(self, cache, B, beam, T, logits):
        self.cache, self.T = cache, T
        self.bs = BeamState(B, beam, max_new, -1, prompt_len=T, device="cuda")      # (eos -1: the search never stops)
        self.st = self.bs.gen_state(V)
        eng.beam_step(logits, self.bs, args.group, 0.8)
        eng.kv_reorder(cache, self.bs.src, T, t0=T)

    def block(self):
        run = lambda n: eng.beam_steps(self.cache, self.st, self.bs, args.group, 0.8, None, n, kv_t0=self.T)
        run(1)                                   # captures the chain for THIS cache (one capture per context)
        ctx.sync()
        ctx.timer_start(); run(args.steps); return ctx.timer_stop() / args.steps


for case in args.cases.split(","):
    B, beam, T = (int(x) for x in case.split("x"))
    BB = B * beam
    emb = (torch.randn(B, T, kw["d"], device="cuda") * 0.02).bfloat16()
    plain = eng.new_cache(BB, T + max_new)
    lg, _ = eng.prefill(emb, None, plain, "last")
    ctx.sync()
    ctx.timer_start(); eng.kv_reorder(plain, torch.arange(BB, dtype=torch.int32) // beam, T); ms_rep = ctx.timer_stop()
    prefix = eng.new_cache(B, T)
    eng.prefill(emb, None, prefix, "last")
    ctx.sync()
    ctx.timer_start(); shared = eng.new_beam_cache(prefix, beam, max_new); ms_new = ctx.timer_stop()
    logits = lg.repeat_interleave(beam, dim=0).contiguous()
    sides = {"plain": Side(plain, B, beam, T, logits), "shared": Side(shared, B, beam, T, logits)}
    ms = {k: [] for k in sides}
    for p in range(args.pairs):
        for k in (("plain", "shared") if p % 2 == 0 else ("shared", "plain")):      # ABBA: neither side always runs first
            ms[k].append(sides[k].block())
            print(f"{args.geom} {case} pair {p} {k:6s} {ms[k][-1]:.4f} ms/step", flush=True)
    ctx.sync()
    same = torch.equal(sides["plain"].bs.out, sides["shared"].bs.out) and torch.equal(sides["plain"].bs.cur, sides["shared"].bs.cur)
    nbytes = lambda c: 2 * c.k.numel() * 2
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratios = [s / p for s, p in zip(ms["shared"], ms["plain"])]
    plan = beam_cache_plan(B, beam, T, max_new, ())
    print(f"SUMMARY {args.geom} L{kw['n_layers']} {case}: plain {med['plain']:.4f} shared {med['shared']:.4f} ms/step all-in (median of {args.pairs}); "
          f"shared/plain per pair min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f}; "
          f"plain spread {min(ms['plain']):.4f}..{max(ms['plain']):.4f}; after prefill: replicate {ms_rep:.3f} ms vs allocate suffix {ms_new:.3f} ms; "
          f"cache bytes plain {nbytes(plain) / 1e9:.3f} GB shared {(nbytes(prefix) + nbytes(shared)) / 1e9:.3f} GB; plan.shared={plan['shared']}; "
          f"same tokens and scores: {same}", flush=True)
    del plain, shared, prefix, sides
    torch.cuda.empty_cache()
