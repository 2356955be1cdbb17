"""The cached decode step that streams e4m3 weights (pcy_llama_greedy_w8) against the default step, ONE process, interleaved A/B.

Both arms are `n` x (decode step + greedy pick) as ONE replayed graph per step: the default arm is pcy_llama_greedy with decode_w8 off (the
fused bf16 steps), the new arm pcy_llama_greedy_w8 (a launch per stage inside the graph, e4m3 projections, bf16 lm_head).  Full-depth
synthetic weights, T cached tokens per row.  Per row count `--pairs` times: `--steps` steps of one arm, then of the other, in ABBA order; each
block starts at the same position (pos = T, step = 0) behind one untimed call that captures the arm's graph (the context holds one captured
step at a time).  Prints one line per block, a summary per case -- median ms per step of both arms, w8 / default per pair, the weight bytes a
step of either arm reads and the fraction of 6.3 TB/s the new step reaches on them -- and the distance between the two arms' logits on the
same state (synthetic weights that are NOT on the e4m3 grid: the quantisation error of the model, printed, not asserted).

  python tools/bench_decode_w8.py --geom full  --T 512 --rows 1,4
  python tools/bench_decode_w8.py --geom split --T 512 --rows 1,4"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from procyon_amd import _lib, synth
from procyon_amd.engine import Context, GenState, LlamaConfig, LlamaEngine

GEOMS = {"full": dict(vocab=128263, d=4096, n_layers=32, n_heads=32, n_kv_heads=8, ffn=14336),
         "split": dict(vocab=32007, d=4096, n_layers=32, n_heads=32, n_kv_heads=32, ffn=11008)}
HBM_TBS = 6.3
ap = argparse.ArgumentParser()
ap.add_argument("--geom", default="full", choices=list(GEOMS))
ap.add_argument("--T", type=int, default=512, help="cached tokens per row")
ap.add_argument("--rows", default="1,4", help="row counts, comma separated (1..8)")
ap.add_argument("--layers", type=int, default=0, help="decoder layers (0: the geometry's 32)")
ap.add_argument("--pairs", type=int, default=6)
ap.add_argument("--steps", type=int, default=32)
ap.add_argument("--once", default="", choices=["", "default", "w8"], help="one block of one arm and nothing else (for a kernel trace of its own)")
args = ap.parse_args()
kw = dict(GEOMS[args.geom])
if args.layers:
    kw["n_layers"] = args.layers
eng = LlamaEngine(synth.llama_state_dict(**kw, device="cuda"), LlamaConfig(**kw, max_pos=4096), free_source=True)
eng._ensure_fp8_copies()
ctx, lib = Context.get(), _lib.load()
V, T, d, F, L_ = kw["vocab"], args.T, kw["d"], kw["ffn"], kw["n_layers"]
dh = d // kw["n_heads"]
rows = [int(x) for x in args.rows.split(",") if x]
assert args.pairs >= 1 and args.steps >= 1 and all(1 <= b <= 8 for b in rows)

proj_elems = L_ * ((kw["n_heads"] + 2 * kw["n_kv_heads"]) * dh * d + d * d + 2 * F * d + d * F)
proj_rows = L_ * ((kw["n_heads"] + 2 * kw["n_kv_heads"]) * dh + d + 2 * F + d)
head_bytes = V * d * 2
BYTES = {"default": proj_elems * 2 + head_bytes, "w8": proj_elems + proj_rows * 4 + head_bytes}


def kv_bytes(B):
    return 2 * L_ * B * kw["n_kv_heads"] * T * dh * 2


Bmax = max(rows)
cache = eng.new_cache(Bmax, T + args.steps + 2)
emb = (torch.randn(Bmax, T, d, device="cuda") * 0.02).bfloat16()
lg, _ = eng.prefill(emb, None, cache, "last")
ctx.sync()
ARMS = {"default": eng.greedy_steps, "w8": eng.greedy_steps_w8}

for B in rows:
    st = GenState(B, V, args.steps + 2, "cuda")
    tok0 = lg[:B].float().argmax(-1).to(torch.int32)

    def reset():
        st.pos.fill_(T); st.step.zero_(); st.logprob.zero_(); st.next_tok.copy_(tok0)

    def block(arm, B=B, st=st):
        reset()
        ARMS[arm](cache, st, B, 1, True)             # untimed: captures this arm's graph
        ctx.sync()
        reset()
        ctx.sync()
        ctx.timer_start()
        ARMS[arm](cache, st, B, args.steps, True)
        return ctx.timer_stop() / args.steps

    if args.once:
        print(f"{args.geom} L{L_} T{T} rows {B} once {args.once} {block(args.once):.4f} ms/step", flush=True)
        continue
    # the two arms on the same state: how far e4m3 projection weights move the logits of THIS synthetic model
    reset(); eng.decode(cache, st, B); ctx.sync(); ref = st.logits.float().clone()
    reset(); eng.decode_w8(cache, st, B); ctx.sync(); got = st.logits.float()
    dist = float((got - ref).norm() / ref.norm())
    agree = float((got.argmax(-1) == ref.argmax(-1)).float().mean())
    ms = {k: [] for k in ARMS}
    for p in range(args.pairs):
        for k in (("default", "w8") if p % 2 == 0 else ("w8", "default")):      # ABBA: neither arm always runs first
            ms[k].append(block(k))
            print(f"{args.geom} L{L_} T{T} rows {B} pair {p} {k:7s} {ms[k][-1]:.4f} ms/step", flush=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratios = [n / o for n, o in zip(ms["w8"], ms["default"])]
    frac = {k: BYTES[k] / (med[k] * 1e-3) / (HBM_TBS * 1e12) for k in ARMS}
    print(f"SUMMARY {args.geom} L{L_} T{T} rows {B}: default {med['default']:.4f} w8 {med['w8']:.4f} ms/step (median of {args.pairs}); "
          f"w8/default per pair min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f}; w8 won {sum(r < 1 for r in ratios)} of "
          f"{len(ratios)} pairs; default spread {min(ms['default']):.4f}..{max(ms['default']):.4f} w8 spread {min(ms['w8']):.4f}..{max(ms['w8']):.4f}; "
          f"weight bytes per step default {BYTES['default'] / 1e9:.3f} GB w8 {BYTES['w8'] / 1e9:.3f} GB (+ K/V {kv_bytes(B) / 1e9:.3f} GB); "
          f"fraction of {HBM_TBS} TB/s on the weight bytes default {frac['default']:.3f} w8 {frac['w8']:.3f}; "
          f"logits w8 vs bf16 on the same state (weights not on the e4m3 grid): rel. err {dist:.3e}, argmax agreement {agree:.2f}", flush=True)
