"""The device-resident fp32 decode step (pcy_f32_llama_decode_graph) against the operator-per-launch step of
`LlamaEngineF32.decode`, ONE process, interleaved A/B.

Full-width synthetic fp32 weights, T cached tokens per row (the caches hold random K / V: no prefill is timed or needed).  The `ops` arm is
`LlamaEngineF32.decode(cache, ids, T)` exactly as `generate` drives it -- token ids uploaded from the host, ~13 eager launches per layer;
the `stream` arm is `decode_stream(cache, st, B, graph=True)` -- next_tok / *pos in device memory, one replayed graph.  Both arms run the
step alone (no pick), always at position T.  Per row count `--pairs` times: `--steps` steps of one arm, then of the other, in ABBA order,
each block behind one untimed step (the stream arm's captures the graph).  A block is timed with events on the stream around its `--steps`
calls, so the ops arm's host gaps count, as they do in a generation; ms per step = block time / steps.  Prints one line per block and a
summary per case: median ms per step of both arms, stream / ops per pair, the bytes a step reads (fp32 weights = 2 x the bf16 bytes, plus
K / V) and the fraction of the HBM rate the stream step reaches on them, and the distance between the two arms' logits on the same state.

  python tools/bench_decode_f32.py --geom full  --T 512 --rows 1,10,20,32
  python tools/bench_decode_f32.py --geom split --T 512 --rows 1,10,20,32
  rocprofv3 --kernel-trace --stats ... -- python tools/bench_decode_f32.py --geom full --rows 10 --once stream     (the per-launch table)"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from procyon_amd import _lib, synth
from procyon_amd.engine import Context, LlamaConfig
from procyon_amd.engine_f32 import LlamaEngineF32

GEOMS = {"full": dict(vocab=128263, d=4096, n_layers=32, n_heads=32, n_kv_heads=8, ffn=14336),
         "split": dict(vocab=32007, d=4096, n_layers=32, n_heads=32, n_kv_heads=32, ffn=11008)}
HBM_PEAK_TBS, HBM_STREAM_TBS = 8.0, 6.3      # the part's nominal rate; what the project's bf16 streams reach
ap = argparse.ArgumentParser()
ap.add_argument("--geom", default="full", choices=list(GEOMS))
ap.add_argument("--T", type=int, default=512, help="cached tokens per row")
ap.add_argument("--rows", default="1,10,20,32", help="row counts, comma separated")
ap.add_argument("--layers", type=int, default=0, help="decoder layers (0: the geometry's 32)")
ap.add_argument("--pairs", type=int, default=4)
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--once", default="", choices=["", "ops", "stream", "stream_eager"], help="one block of one arm and nothing else (for a kernel trace of its own)")
args = ap.parse_args()
kw = dict(GEOMS[args.geom])
if args.layers:
    kw["n_layers"] = args.layers
torch.manual_seed(0)
eng = LlamaEngineF32(synth.llama_state_dict(**kw, device="cuda", dtype=torch.float32), LlamaConfig(**kw, max_pos=4096))
ctx, lib = Context.get(), _lib.load()
V, T, d, F, L_ = kw["vocab"], args.T, kw["d"], kw["ffn"], kw["n_layers"]
dh = d // kw["n_heads"]
kvw = kw["n_kv_heads"] * dh
rows = [int(x) for x in args.rows.split(",") if x]
assert args.pairs >= 1 and args.steps >= 1 and all(b >= 1 for b in rows)
WEIGHT_BYTES = 4 * (L_ * ((kw["n_heads"] + 2 * kw["n_kv_heads"]) * dh * d + d * d + 2 * F * d + d * F) + V * d)


def kv_bytes(B):
    return 2 * L_ * B * kvw * (T + 1) * 4


for B in rows:
    cache = eng.new_cache(B, T + 2)       # (the ops arm writes every row of the cache it is given: one cache per row count)
    cache.k.normal_(std=0.5)
    cache.v.normal_(std=0.5)
    st = eng.new_gen_state(B, 2)
    ids = torch.randint(0, V, (B,), generator=torch.Generator().manual_seed(B))
    st.set(pos=T, step=0, next_tok=ids.cuda())
    out = {}

    def step(arm, B=B, st=st, ids=ids, cache=cache):
        if arm == "ops":
            out[arm] = eng.decode(cache, ids, T)
        else:
            out[arm] = eng.decode_stream(cache, st, B, graph=arm == "stream")

    def block(arm):
        step(arm)                   # untimed: warms the launches / captures the graph
        ctx.sync()
        ctx.timer_start()
        for _ in range(args.steps):
            step(arm)
        return ctx.timer_stop() / args.steps

    if args.once:
        print(f"{args.geom} L{L_} T{T} rows {B} once {args.once} {block(args.once):.4f} ms/step", flush=True)
        continue
    step("ops"); step("stream"); ctx.sync()
    ref, got = out["ops"].double(), out["stream"].double()
    dist = float((got - ref).norm() / ref.norm())
    agree = float((got.argmax(-1) == ref.argmax(-1)).float().mean())
    ms = {"ops": [], "stream": []}
    for p in range(args.pairs):
        for k in (("ops", "stream") if p % 2 == 0 else ("stream", "ops")):      # ABBA: neither arm always runs first
            ms[k].append(block(k))
            print(f"{args.geom} L{L_} T{T} rows {B} pair {p} {k:6s} {ms[k][-1]:.4f} ms/step", flush=True)
    eager = block("stream_eager")
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratios = [n / o for n, o in zip(ms["stream"], ms["ops"])]
    nbytes = WEIGHT_BYTES + kv_bytes(B)
    rate = nbytes / (med["stream"] * 1e-3) / 1e12
    print(f"SUMMARY {args.geom} L{L_} T{T} rows {B}: ops {med['ops']:.4f} stream {med['stream']:.4f} ms/step (median of {args.pairs} blocks of {args.steps} steps); "
          f"stream/ops per pair min {min(ratios):.4f} med {statistics.median(ratios):.4f} max {max(ratios):.4f}; stream won {sum(r < 1 for r in ratios)} of "
          f"{len(ratios)} pairs; ops spread {min(ms['ops']):.4f}..{max(ms['ops']):.4f} stream spread {min(ms['stream']):.4f}..{max(ms['stream']):.4f}; "
          f"stream without the graph (eager launches, one block) {eager:.4f}; "
          f"bytes per step: fp32 weights {WEIGHT_BYTES / 1e9:.3f} GB (2 x bf16) + K/V {kv_bytes(B) / 1e9:.3f} GB -> stream step {rate:.3f} TB/s = "
          f"{rate / HBM_PEAK_TBS:.3f} of {HBM_PEAK_TBS} TB/s peak, {rate / HBM_STREAM_TBS:.3f} of the {HBM_STREAM_TBS} TB/s the bf16 streams reach; "
          f"logits stream vs ops on the same state: rel. err {dist:.3e}, argmax agreement {agree:.2f}", flush=True)
