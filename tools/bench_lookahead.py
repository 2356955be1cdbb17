"""Greedy decoding with lookahead against plain greedy decoding, ONE process, interleaved A/B.

Synthetic ProCyon-Full decoder (32 layers), one prompt of T tokens, max_len generated ones.  Per window W and per acceptance a (drafts accepted
in EVERY pass, dictated through `forced`: the tokens of an unforced run at that window with every (a+1)-th one made wrong), `--pairs` times: one
`generate_greedy` and one `generate_lookahead`, ABBA.  Both are timed by the host clock around the whole call (they end in a synchronise; the
lookahead loop's host read per pass is part of what it costs) and the opening they share -- cache allocation, prefill, pick of token 0 -- is
timed in the same block and subtracted.  Prints one line per block and per (W, a):
  ms per pass and per committed token, the ratio to the plain run of the same pair as min / median / max, and the break-even acceptance
  pass time / step time - 1 (lookahead pays when more drafts than that are accepted per pass).
Random-init weights do not repeat their prompt: what prompt lookup really accepts on ProCyon text is NOT measured here.

--step extend|window|both: what a lookahead pass runs on.  `extend`, the default, is the tool as it always was.  `window`
times step="window" in its place.  `both` times the two in the same block beside the plain run -- plain, extend, window in an order that
rotates with the pair and is mirrored in the second half, so that no side always runs first -- and prints a SUMMARY line per step, the
window one with its ratio to the extend pass of the same block.  --geometry full|split: Llama-3-8B widths (ProCyon-Full) or Llama-2-7B
widths (ProCyon-Split).

  python tools/bench_lookahead.py                       # windows 4 and 8, T 512, 128 tokens, 5 pairs
  python tools/bench_lookahead.py --step both --geometry split
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
ap.add_argument("--step", default="extend", choices=["extend", "window", "both"])
ap.add_argument("--geometry", default="full", choices=["full", "split"])
args = ap.parse_args()
kw = {"full": dict(vocab=128263, d=4096, n_layers=args.layers, n_heads=32, n_kv_heads=8, ffn=14336),
      "split": dict(vocab=32007, d=4096, n_layers=args.layers, n_heads=32, n_kv_heads=32, ffn=11008)}[args.geometry]
STEPS = ["extend", "window"] if args.step == "both" else [args.step]
eng = LlamaEngine(synth.llama_state_dict(**kw, device="cuda"), LlamaConfig(**kw, max_pos=4096), free_source=True)
ctx = Context.get()
V, T, N = kw["vocab"], args.prompt, args.max_len
ids = torch.randint(0, min(128000, V - 7), (T,), generator=torch.Generator().manual_seed(1))
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
tag = "" if (args.step, args.geometry) == ("extend", "full") else f" step {args.step} geometry {args.geometry}"
print(f"lookahead A/B: L{args.layers} T {T} max_len {N} pairs {args.pairs}{tag}", flush=True)
sk = lambda step: {} if step == "extend" else {"step": step}      # (the default call is spelled as it always was)
for W in (int(w) for w in args.windows.split(",")):
    tok_w = {}
    for step in STEPS:
        _, (t, _, _, _) = wall(lambda: eng.generate_lookahead(emb, ids, N, W, **sk(step)))      # warm-up + the tokens at this window (draft independent)
        tok_w[step] = t.cpu()[0]
    _, (tok_p, _, _, _) = wall(plain)
    for step in STEPS:
        agree = (tok_p.cpu()[0] == tok_w[step])
        first = int((~agree).nonzero()[0]) if not bool(agree.all()) else None
        print(f"W {W}{'' if args.step == 'extend' else ' ' + step}: first token that differs from plain greedy: {first} of {N} (different arithmetic: not promised equal)", flush=True)
    for a in sorted({0, 1, 2, W - 1}):
        look = {}
        for step in STEPS:
            forced = tok_w[step].clone()
            if a < W - 1:
                bad = (torch.arange(N) - 1) % (a + 1) == a         # the draft behind the a accepted ones of every pass
                forced[bad] = (forced[bad] + 1) % V
            want_passes = lookahead_passes(tok_w[step], ids, W, (3, 1), forced)[0]
            assert want_passes == math.ceil((N - 1) / (a + 1)), (want_passes, a)
            look[step] = (lambda f, st: (lambda: eng.generate_lookahead(emb, ids, N, W, forced=f, **sk(st))))(forced, step)
        rows = {step: [] for step in STEPS}
        sides = ["plain"] + STEPS
        for p in range(args.pairs):
            # ABBA for two sides; three sides: the order rotates with the pair and the second half of the pairs mirrors it
            order = sides[p % len(sides):] + sides[:p % len(sides)]
            if len(sides) == 2:
                order = sides if p % 2 == 0 else sides[::-1]
            elif p >= (args.pairs + 1) // 2:
                order = order[::-1]
            ms, stats, same = {}, {}, {}
            for side in order:
                ms[side], out = wall(plain if side == "plain" else look[side])
                if side != "plain":
                    stats[side], same[side] = out[3][2].stats(), torch.equal(out[0].cpu()[0], tok_w[side])
            ms_open, _ = wall(opening)
            step_ms = (ms["plain"] - ms_open) / (N - 1)
            for step in STEPS:
                pass_ms = (ms[step] - ms_open) / stats[step]["passes"]
                tok_ms = (ms[step] - ms_open) / (N - 1)
                rows[step].append((step_ms, pass_ms, tok_ms))
                print(f"W {W} a {a} pair {p}{'' if args.step == 'extend' else ' ' + step}: plain {ms['plain']:.2f} ms look {ms[step]:.2f} ms opening {ms_open:.2f} ms | "
                      f"step {step_ms:.4f} pass {pass_ms:.4f} ms, per token {tok_ms:.4f} ms, passes {stats[step]['passes']} (want {want_passes}) "
                      f"accepted {stats[step]['accepted']} same tokens {same[step]}", flush=True)
                assert stats[step]["passes"] == want_passes and same[step]
        for step in STEPS:
            ratios = [t / s_ for s_, _, t in rows[step]]
            med = [statistics.median(c) for c in zip(*rows[step])]
            line = (f"SUMMARY W {W} accepted {a}/pass{'' if args.step == 'extend' else ' ' + step}: step {med[0]:.4f} ms | pass {med[1]:.4f} ms | "
                    f"per committed token {med[2]:.4f} ms | look/plain per token min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f} | "
                    f"break-even acceptance {med[1] / med[0] - 1:.3f} drafts per pass")
            if step == "window" and "extend" in rows:
                wr = [w_[1] / e_[1] for w_, e_ in zip(rows["window"], rows["extend"])]
                line += f" | window/extend pass min {min(wr):.4f} med {statistics.median(wr):.4f} max {max(wr):.4f}"
            print(line, flush=True)
