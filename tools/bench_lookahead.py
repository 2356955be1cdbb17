"""Greedy decoding with lookahead against plain greedy decoding, ONE process, interleaved A/B.

Synthetic ProCyon-Full decoder (32 layers), one prompt of T tokens, max_len generated ones.  Per window W and per acceptance a (drafts accepted
in EVERY pass, dictated through `forced`: the tokens of an unforced run at that window with every (a+1)-th one made wrong), `--pairs` times: one
`generate_greedy` and one `generate_lookahead`, ABBA.  Both are timed by the host clock around the whole call (they end in a synchronise; the
lookahead loop's host read per pass is part of what it costs) and the opening they share -- cache allocation, prefill, pick of token 0 -- is
timed in the same block and subtracted.  Prints one line per block and per (W, a):
  ms per pass and per committed token, the ratio to the plain run of the same pair as min / median / max, and the break-even acceptance
  pass time / step time - 1 (lookahead pays when more drafts than that are accepted per pass).
Random-init weights do not repeat their prompt: what prompt lookup really accepts on ProCyon text is NOT measured here.

  python tools/bench_lookahead.py                       # windows 4 and 8, T 512, 128 tokens, 5 pairs
  python tools/bench_lookahead.py --layers 2 --pairs 1  # a rehearsal"""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from procyon_amd import synth
from procyon_amd.engine import Context, LlamaConfig, LlamaEngine, lookahead_passes

ap = argparse.ArgumentParser()
ap.add_argument("--windows", default="4,8")
ap.add_argument("--prompt", type=int, default=512)
ap.add_argument("--max-len", type=int, default=128)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--pairs", type=int, default=5)
args = ap.parse_args()
kw = dict(vocab=128263, d=4096, n_layers=args.layers, n_heads=32, n_kv_heads=8, ffn=14336)
eng = LlamaEngine(synth.llama_state_dict(**kw, device="cuda"), LlamaConfig(**kw, max_pos=4096), free_source=True)
ctx = Context.get()
V, T, N = kw["vocab"], args.prompt, args.max_len
ids = torch.randint(0, 128000, (T,), generator=torch.Generator().manual_seed(1))
emb = eng.embed_tokens(ids[None])


def wall(fn):
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def opening():
    cache, st = eng._prefill_for_generation(emb, None, N, False)
    eng.pick(cache, st, 1, advance_pos=False)


plain = lambda: eng.generate_greedy(emb, None, N)
wall(plain)                                                    # warm-up: code objects, the captured decode step
print(f"lookahead A/B: L{args.layers} T {T} max_len {N} pairs {args.pairs}", flush=True)
for W in (int(w) for w in args.windows.split(",")):
    _, (tok_w, _, _, _) = wall(lambda: eng.generate_lookahead(emb, ids, N, W))      # warm-up + the tokens at this window (draft independent)
    tok_w = tok_w.cpu()[0]
    _, (tok_p, _, _, _) = wall(plain)
    agree = (tok_p.cpu()[0] == tok_w)
    first = int((~agree).nonzero()[0]) if not bool(agree.all()) else None
    print(f"W {W}: first token that differs from plain greedy: {first} of {N} (different arithmetic: not promised equal)", flush=True)
    for a in sorted({0, 1, 2, W - 1}):
        forced = tok_w.clone()
        if a < W - 1:
            bad = (torch.arange(N) - 1) % (a + 1) == a         # the draft behind the a accepted ones of every pass
            forced[bad] = (forced[bad] + 1) % V
        want_passes = lookahead_passes(tok_w, ids, W, (3, 1), forced)[0]
        assert want_passes == math.ceil((N - 1) / (a + 1)), (want_passes, a)
        look = lambda: eng.generate_lookahead(emb, ids, N, W, forced=forced)
        rows = []
        for p in range(args.pairs):
            ms = {}
            for side in (("plain", "look") if p % 2 == 0 else ("look", "plain")):      # ABBA: neither side always runs first
                ms[side], out = wall(plain if side == "plain" else look)
                if side == "look":
                    stats, same = out[3][2].stats(), torch.equal(out[0].cpu()[0], tok_w)
            ms_open, _ = wall(opening)
            step_ms = (ms["plain"] - ms_open) / (N - 1)
            pass_ms = (ms["look"] - ms_open) / stats["passes"]
            tok_ms = (ms["look"] - ms_open) / (N - 1)
            rows.append((step_ms, pass_ms, tok_ms))
            print(f"W {W} a {a} pair {p}: plain {ms['plain']:.2f} ms look {ms['look']:.2f} ms opening {ms_open:.2f} ms | step {step_ms:.4f} pass {pass_ms:.4f} "
                  f"ms, per token {tok_ms:.4f} ms, passes {stats['passes']} (want {want_passes}) accepted {stats['accepted']} same tokens {same}", flush=True)
            assert stats["passes"] == want_passes and same
        ratios = [t / s for s, _, t in rows]
        med = [statistics.median(c) for c in zip(*rows)]
        print(f"SUMMARY W {W} accepted {a}/pass: step {med[0]:.4f} ms | pass {med[1]:.4f} ms | per committed token {med[2]:.4f} ms | "
              f"look/plain per token min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f} | "
              f"break-even acceptance {med[1] / med[0] - 1:.3f} drafts per pass", flush=True)
