"""Ranking N candidate texts per prompt: the prompt prefilled ONCE + one cache extension against what the engine offered
before, ONE process, interleaved A/B, full Llama geometry (seeded random weights; the text decoder only -- the protein encoder runs once
per prompt on one side and N times on the other, which this tool leaves out).

  A  LlamaEngine.score on the [P*N, Tp+S] concatenated rows (every row prefills its prompt again)
  B  LlamaEngine.prefill of the P prompts into a P-row cache + LlamaEngine.extend of the P*N suffixes on a cache that shares it

Per shape PxN (Tp = 512, S = 32 by default): `--pairs` pairs of blocks in ABBA order, a block = `reps` back-to-back calls between two
device events.  Prints one line per block, and per shape: ms per call of both sides (median), the per-pair ratio B / A as min . median . max,
the row arithmetic N (Tp + S) / (Tp + N S) and the largest |token_nll_A - token_nll_B|.  The caches of both sides are allocated outside the
timed blocks.

  python tools/bench_candidates.py
  python tools/bench_candidates.py --shapes 1x16 --pairs 1 --layers 4"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from procyon_amd import synth
from procyon_amd.engine import BF16, LlamaConfig, LlamaEngine
from procyon_amd.synthetic_model import GEOMETRIES

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="1x4,1x16,1x64,4x16", help="P x N, comma separated")
ap.add_argument("--tp", type=int, default=512)
ap.add_argument("--s", type=int, default=32)
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--block-ms", type=float, default=300.0)
ap.add_argument("--layers", type=int, default=0, help="decoder layers (0 = the geometry's 32)")
args = ap.parse_args()

g = dict(GEOMETRIES["full"]["llama"])
if args.layers:
    g["n_layers"] = args.layers
eng = LlamaEngine(synth.llama_state_dict(**g, device="cuda", dtype=BF16), LlamaConfig(**g, max_pos=4096), torch.device("cuda"), free_source=True)
ctx = eng.ctx
Tp, S = args.tp, args.s

for shape in args.shapes.split(","):
    P, N = (int(v) for v in shape.split("x"))
    B = P * N
    gen = torch.Generator().manual_seed(B)
    pre_ids = torch.randint(0, 128000, (P, Tp), generator=gen)
    suf_ids = torch.randint(0, 128000, (B, S), generator=gen)
    labels = suf_ids.clone()
    labels[:, 0] = -100
    pre_emb, suf_emb = eng.embed_tokens(pre_ids), eng.embed_tokens(suf_ids)
    cat_emb = torch.cat([pre_emb.repeat_interleave(N, 0), suf_emb], 1).contiguous()
    cat_labels = torch.cat([torch.full((B, Tp), -100), labels], 1)
    cache_a = eng.new_cache(B, Tp + S)
    prefix = eng.new_cache(P, Tp)
    shared = eng.new_shared_cache(prefix, N, S)

    def side_a():
        return eng.score(cat_emb, None, cat_labels, cache=cache_a)[0][:, Tp:]

    def side_b():
        eng.prefill(pre_emb, None, prefix, logit_rows=None)
        return eng.extend(shared, suf_emb, Tp, labels=labels)[2]

    sides = {"A": side_a, "B": side_b}
    reps, ms = {}, {k: [] for k in sides}
    for k, fn in sides.items():          # warm-up + block size
        fn(); ctx.sync()
        ctx.timer_start(); fn(); t1 = ctx.timer_stop()
        reps[k] = max(1, int(args.block_ms / max(t1, 1e-3)))
    diff = float((side_a() - side_b()).abs().max())
    for p in range(args.pairs):
        for k in (("A", "B") if p % 2 == 0 else ("B", "A")):      # ABBA: neither side always runs first
            fn = sides[k]
            ctx.sync()
            ctx.timer_start()
            for _ in range(reps[k]):
                fn()
            ms[k].append(ctx.timer_stop() / reps[k])
            print(f"{shape} pair {p} {k} {ms[k][-1]:.3f} ms/call ({reps[k]} calls)", flush=True)
    ratios = [b / a for a, b in zip(ms["A"], ms["B"])]
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"SUMMARY P={P} N={N} Tp={Tp} S={S} layers={g['n_layers']}: A {med['A']:.3f} B {med['B']:.3f} ms/call (median of {args.pairs}); B/A per pair "
          f"min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f}; rows A {B * (Tp + S)} B {P * Tp + B * S} "
          f"(x{N * (Tp + S) / (Tp + N * S):.2f}); max |token_nll_A - token_nll_B| {diff:.3e}", flush=True)
    del cache_a, prefix, shared, cat_emb
    torch.cuda.empty_cache()
