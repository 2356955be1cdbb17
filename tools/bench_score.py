"""Fused lm_head x cross-entropy (pcy_lm_head_xent) against its materialising twin, ONE process, interleaved A/B.

  A  Context.lm_head_xent(x, W, targets): the logits never reach memory
  B  Context.gemm(x, W) into [M, V] bf16, then torch.nn.functional.cross_entropy(logits.float(), targets, reduction="none") on the device --
     what HF's loss does with the logits of `forward(full_logits=True)`

Per shape M x V (d = 4096): `--pairs` pairs of blocks in ABBA order, a block = `reps` back-to-back calls between two device events (reps
sized so that a block lasts about `--block-ms`).  Prints one line per block, and per shape: ms per call of both sides (median), the per-pair
ratio A / B as min . median . max, the peak extra device bytes of each side (torch's allocator peak over the block + the engine workspace of
the operator, which torch does not see) and the largest |nll_A - nll_B|.

  python tools/bench_score.py
  python tools/bench_score.py --shapes 64x128263,2048x32007 --pairs 5"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from procyon_amd.engine import Context

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="64x128263,256x128263,2048x128263,2048x32007", help="M x V, comma separated")
ap.add_argument("--d", type=int, default=4096)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--block-ms", type=float, default=300.0)
args = ap.parse_args()
ctx = Context.get()
d = args.d
weights = {}


def lm_head(V):
    if V not in weights:
        g = torch.Generator(device="cuda").manual_seed(V)
        weights[V] = (torch.randn(V, d, generator=g, device="cuda") / d ** 0.5).bfloat16()      # logits ~ N(0, 1) on unit-RMS rows
    return weights[V]


for shape in args.shapes.split(","):
    M, V = (int(v) for v in shape.split("x"))
    W = lm_head(V)
    g = torch.Generator(device="cuda").manual_seed(M)
    x = torch.randn(M, d, generator=g, device="cuda")
    x = (x / x.pow(2).mean(-1, keepdim=True).sqrt()).bfloat16()
    tg = torch.randint(0, V, (M,), generator=g, device="cuda", dtype=torch.int32)
    tg64 = tg.long()
    fused = lambda: ctx.lm_head_xent(x, W, tg)
    twin = lambda: F.cross_entropy(ctx.gemm(x, W).float(), tg64, reduction="none")
    sides = {"fused": fused, "twin": twin}
    reps, peak, ms = {}, {}, {k: [] for k in sides}
    for k, fn in sides.items():          # warm-up + block size + peak extra bytes of ONE call
        fn(); ctx.sync()
        ctx.timer_start(); fn(); t1 = ctx.timer_stop()
        reps[k] = max(3, int(args.block_ms / max(t1, 1e-3)))
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn(); torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - base
        del out
    peak["fused"] += ctx.lib.pcy_lm_head_xent_ws_bytes(M, V)
    diff = float((fused() - twin()).abs().max())
    for p in range(args.pairs):
        for k in (("fused", "twin") if p % 2 == 0 else ("twin", "fused")):      # ABBA: neither side always runs first
            fn = sides[k]
            ctx.sync()
            ctx.timer_start()
            for _ in range(reps[k]):
                fn()
            ms[k].append(ctx.timer_stop() / reps[k])
            print(f"{shape} pair {p} {k:5s} {ms[k][-1]:.4f} ms/call ({reps[k]} calls)", flush=True)
    ratios = [a / b for a, b in zip(ms["fused"], ms["twin"])]
    med = {k: statistics.median(v) for k, v in ms.items()}
    tflops = 2.0 * M * V * d / (med["fused"] * 1e-3) / 1e12
    print(f"SUMMARY M={M} V={V} d={d}: fused {med['fused']:.4f} twin {med['twin']:.4f} ms/call (median of {args.pairs}); fused/twin per pair "
          f"min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f}; fused {tflops:.0f} TFLOP/s of GEMM work; "
          f"peak extra bytes fused {peak['fused']} twin {peak['twin']}; max |nll_fused - nll_twin| {diff:.3e}", flush=True)
    del x, tg, tg64
    torch.cuda.empty_cache()
