"""fp32 fused lm_head x cross-entropy (pcy_f32_lm_head_xent) against its materialising twin, ONE process, interleaved A/B.

  A  F32Ops.lm_head_xent(x, W, targets): the [M, V] fp32 logits never reach memory
  B  F32Ops.linear(x, W) into [M, V] fp32, then torch.nn.functional.cross_entropy(logits, targets, reduction="none") on the device -- what
     `forward(full_logits=True)` + HF's loss does on an fp32 model

`--pairs` pairs of blocks in ABBA order, a block = `reps` back-to-back calls between two device events (reps sized so that a block lasts
about `--block-ms`).  Prints one line per block, then ms per call of both sides (median), the per-pair ratio A / B as min . median . max,
the peak extra device bytes of each side (torch's allocator peak over a call + the engine workspace of the operator, which torch does not
see) and the largest |nll_A - nll_B|.  No threshold: the numbers are reported as they come out.

  python tools/bench_f32_score.py
  python tools/bench_f32_score.py --M 2048 --V 128263 --d 4096 --pairs 5"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from procyon_amd.engine_f32 import F32Ops

ap = argparse.ArgumentParser()
ap.add_argument("--M", type=int, default=2048)
ap.add_argument("--V", type=int, default=128263)
ap.add_argument("--d", type=int, default=4096)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--block-ms", type=float, default=300.0)
args = ap.parse_args()
ops = F32Ops()
ctx = ops.ctx
M, V, d = args.M, args.V, args.d
g = torch.Generator(device="cuda").manual_seed(V)
W = torch.randn(V, d, generator=g, device="cuda") / d ** 0.5                # logits ~ N(0, 1) on unit-RMS rows
x = torch.randn(M, d, generator=g, device="cuda")
x = (x / x.pow(2).mean(-1, keepdim=True).sqrt()).contiguous()
tg = torch.randint(0, V, (M,), generator=g, device="cuda", dtype=torch.int32)
tg64 = tg.long()
fused = lambda: ops.lm_head_xent(x, W, tg)
twin = lambda: F.cross_entropy(ops.linear(x, W), tg64, reduction="none")
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
peak["fused"] += ops.lm_head_xent_ws_bytes(M, V)
diff = float((fused() - twin()).abs().max())
for p in range(args.pairs):
    for k in (("fused", "twin") if p % 2 == 0 else ("twin", "fused")):      # ABBA: neither side always runs first
        fn = sides[k]
        ctx.sync()
        ctx.timer_start()
        for _ in range(reps[k]):
            fn()
        ms[k].append(ctx.timer_stop() / reps[k])
        print(f"{M}x{V} pair {p} {k:5s} {ms[k][-1]:.4f} ms/call ({reps[k]} calls)", flush=True)
ratios = [a / b for a, b in zip(ms["fused"], ms["twin"])]
med = {k: statistics.median(v) for k, v in ms.items()}
tflops = 2.0 * M * V * d / (med["fused"] * 1e-3) / 1e12
print(f"SUMMARY M={M} V={V} d={d}: fused {med['fused']:.4f} twin {med['twin']:.4f} ms/call (median of {args.pairs}); fused/twin per pair "
      f"min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f}; fused {tflops:.1f} TFLOP/s of GEMM work; "
      f"peak extra bytes fused {peak['fused']} twin {peak['twin']}; max |nll_fused - nll_twin| {diff:.3e}", flush=True)
