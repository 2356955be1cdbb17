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
  rocprofv3 --kernel-trace --stats ... -- python tools/bench_decode_f32.py --geom full --rows 10 --once stream     (the per-launch table)

`--select`: whole generations instead of single steps -- the host-side selection around the replayed step (arm `host`:
`UnifiedProCyon._generate_beam_search_f32` / `_generate_sampling_f32` with decode_f32="stream", the model's own loops, called on a bare text
encoder: prompts replicated x beam before the fp32 prefill, logits to the host every step, torch.cat record, per-group topk / bincount,
advanced-indexing K / V reorder; full-vocabulary sort / cumsum / multinomial for nucleus sampling) against the selection on the device (arm `device`:
`LlamaEngineF32.generate_beam` / `generate_sampling`, what decode_f32="device" runs).  One prompt of T tokens x each beam count of `--beams`
(groups of 5, penalty 0.8), then nucleus sampling (p = 0.9) at each row count of `--sample_rows`; `--gen_steps` tokens.  Per case a warm-up of
both arms, then `--pairs` groups in ABBA order (host, device, device, host); a generation is timed all-in on the host clock between two
synchronisations (prefill, steps, selection, the record on the host) and reported per token of the steps it ran; the arms' prefills are
timed once more on their own per case.  A
group counts as won only when the gap between the arms exceeds the spread of its two host runs.

  python tools/bench_decode_f32.py --select --geom full  --T 512 --beams 10,20 --sample_rows 1,10
  python tools/bench_decode_f32.py --select --geom split --T 512 --beams 10,20 --sample_rows 1,10"""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from procyon_amd import _lib, synth
from procyon_amd.engine import Context, LlamaConfig
from procyon_amd.engine_f32 import LlamaEngineF32
from procyon_amd.model.model_unified import UnifiedProCyon
from procyon_amd.model.pmc_llama import LlamaPostTokenization

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
ap.add_argument("--select", action="store_true", help="whole beam / nucleus generations: host-side selection around the replayed step against the device-side selection")
ap.add_argument("--beams", default="10,20", help="--select: beam counts (one prompt each, groups of 5)")
ap.add_argument("--sample_rows", default="1,10", help="--select: row counts of the nucleus sampling cases")
ap.add_argument("--gen_steps", type=int, default=32, help="--select: generated tokens")
args = ap.parse_args()
kw = dict(GEOMS[args.geom])
if args.layers:
    kw["n_layers"] = args.layers
torch.manual_seed(0)
sd = synth.llama_state_dict(**kw, device="cuda", dtype=torch.float32)
if args.select:      # the model's own loops want its text encoder (which also holds a bf16 engine of the same weights): its fp32 engine serves both arms
    enc = LlamaPostTokenization(sd, LlamaConfig(**kw, max_pos=4096), "cuda", max_new_tokens=args.gen_steps)
    eng = enc.engine_f32
else:
    eng = LlamaEngineF32(sd, LlamaConfig(**kw, max_pos=4096))
del sd
ctx, lib = Context.get(), _lib.load()
V, T, d, F, L_ = kw["vocab"], args.T, kw["d"], kw["ffn"], kw["n_layers"]
dh = d // kw["n_heads"]
kvw = kw["n_kv_heads"] * dh
rows = [int(x) for x in args.rows.split(",") if x]
assert args.pairs >= 1 and args.steps >= 1 and all(b >= 1 for b in rows)
WEIGHT_BYTES = 4 * (L_ * ((kw["n_heads"] + 2 * kw["n_kv_heads"]) * dh * d + d * d + 2 * F * d + d * F) + V * d)


def kv_bytes(B):
    return 2 * L_ * B * kvw * (T + 1) * 4


# ---- --select: whole generations, selection on the host (around the replayed step) against selection on the device
EOS, GROUP, PENALTY, NUCLEUS = V - 1, 5, 0.8, 0.9


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


class HostLoops(UnifiedProCyon):
    """the model's own fp32 generation loops (`_generate_beam_search_f32`, `_generate_sampling_f32`: what decode_f32="stream" runs) on a bare
    text encoder: they read the encoder, the device and the EOS id of the model and nothing else"""

    def __init__(self, enc, eos):
        self.text_encoder, self.device, self.tokenizer = enc, enc.engine.device, SimpleNamespace(eos_token_id=eos)


def beam_host(emb, mask, max_len, beam):
    _, _, rec = loops._generate_beam_search_f32(emb, mask, max_len=max_len, beam_size=beam, beam_group_size=GROUP, diversity_penalty=PENALTY,
                                                decode_f32="stream")
    return rec.shape[2]


def nucleus_host(emb, mask, max_len):
    loops._generate_sampling_f32(emb, mask, max_len=max_len, num_text_per_instance=1, temperature=1.0, greedy=False, nucleus_prob=NUCLEUS,
                                 decode_f32="stream")
    return max_len


def select_case(name, emb, mask, rep, host, device):
    """warm-up of both arms, then --pairs groups of (host, device, device, host); every run is a whole generation, all-in, divided by the
    steps it ran (an EOS in every beam ends a search early); host / device: callables -> steps run; rep: rows the host arm prefills per prompt"""
    n, B = args.gen_steps, emb.shape[0]
    timed(host); timed(device)
    pre_rep, _ = timed(lambda: eng.prefill(emb.repeat_interleave(rep, dim=0), mask.repeat_interleave(rep, dim=0), "last", cache=eng.new_cache(B * rep, T)))
    pre1, _ = timed(lambda: eng.prefill(emb, mask, "last", cache=eng.new_cache(B, T)))
    won, rows_ = 0, []
    for p in range(args.pairs):
        res = {"host": [], "device": []}
        for arm, fn in (("host", host), ("device", device), ("device", device), ("host", host)):
            ms, steps = timed(fn)
            res[arm].append(ms / steps)
            print(f"{name} group {p} {arm:6s} {ms / steps:.4f} ms/token all-in ({steps} steps)", flush=True)
        a, b = statistics.mean(res["host"]), statistics.mean(res["device"])
        spread = abs(res["host"][0] - res["host"][1])
        won += (a - b) > spread
        rows_.append((a, b, spread))
    print(f"SUMMARY select {name}: host {statistics.mean(r[0] for r in rows_):.4f} device {statistics.mean(r[1] for r in rows_):.4f} ms/token all-in "
          f"(up to {n} tokens, T {T}); per group host - device / spread of the two host runs: "
          + ", ".join(f"{a - b:.4f} / {sp:.4f}" for a, b, sp in rows_) + f"; device won {won} of {len(rows_)} groups; "
          f"prefill alone, once: the host arm's {B * rep} rows {pre_rep:.1f} ms = {pre_rep / n:.3f} ms per token of {n}, the device arm's {B} rows {pre1:.1f} ms", flush=True)


if args.select:
    n = args.gen_steps
    loops = HostLoops(enc, EOS)
    g = torch.Generator().manual_seed(1)
    for beam in [int(x) for x in args.beams.split(",") if x]:
        assert beam % GROUP == 0, "--beams: multiples of 5 (the groups)"
        emb, mask = eng.embed_tokens(torch.randint(0, V, (1, T), generator=g)), torch.ones(1, T, dtype=torch.long)
        select_case(f"{args.geom} L{L_} T{T} beam {beam}", emb, mask, beam, lambda: beam_host(emb, mask, n, beam),
                    lambda: eng.generate_beam(emb, mask, n, beam, GROUP, PENALTY, EOS, max_new=n)[2].shape[1])
    for B in [int(x) for x in args.sample_rows.split(",") if x]:
        emb, mask = eng.embed_tokens(torch.randint(0, V, (B, T), generator=g)), torch.ones(B, T, dtype=torch.long)

        def device(emb=emb, mask=mask):
            tok, lp, lg, _ = eng.generate_sampling(emb, mask, n, nucleus_prob=NUCLEUS, keep_logits=True)
            tok.cpu(), lp.cpu(), lg.cpu()
            return n

        select_case(f"{args.geom} L{L_} T{T} nucleus rows {B}", emb, mask, 1, lambda: nucleus_host(emb, mask, n), device)
    sys.exit(0)


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
