"""Greedy and sampling generation with the EOS stop against the same call without it, ONE process, interleaved ABBA.

Synthetic ProCyon-Full decoder (32 layers, random weights), one prompt of T tokens, max_len generated ones.  A = `stop_on_eos=None` (the
parent behaviour: all max_len steps), B = `stop_on_eos=eos_id`.  Both sides are the whole driver call by the host clock (prefill included:
it is the same on both sides).  The EOS is taken from a run without a stop, as tests/test_gpu_stop_eos.py takes it:
  with a stop    the token of the step nearest to each --targets step that the run had not emitted before (so that the row's first EOS is
                 that step); random weights repeat themselves under greedy, so the step found may lie off the target -- it is printed
  its own cost   a token the run never emits: the stop-enabled loop (chunks of 8 steps, one look at `done` per chunk) over all max_len steps
                 against the plain loop; the ratio B / A per pair as min / median / max beside the spread max / min of the A runs alone.

  python tools/bench_stop_eos.py                        # greedy and sampling, T 512, 512 tokens, EOS near steps 64 and 256, 3 pairs
  python tools/bench_stop_eos.py --layers 2 --pairs 1   # a rehearsal"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from procyon_amd import synth
from procyon_amd.engine import Context, LlamaConfig, LlamaEngine

ap = argparse.ArgumentParser()
ap.add_argument("--prompt", type=int, default=512)
ap.add_argument("--max-len", type=int, default=512)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--targets", default="64,256")
ap.add_argument("--methods", default="greedy,sampling")
args = ap.parse_args()
kw = dict(vocab=128263, d=4096, n_layers=args.layers, n_heads=32, n_kv_heads=8, ffn=14336)
eng = LlamaEngine(synth.llama_state_dict(**kw, device="cuda"), LlamaConfig(**kw, max_pos=4096), free_source=True)
ctx = Context.get()
V, T, N = kw["vocab"], args.prompt, args.max_len
ids = torch.randint(0, 128000, (T,), generator=torch.Generator().manual_seed(1))
emb = eng.embed_tokens(ids[None])
u = torch.rand(N, generator=torch.Generator().manual_seed(2)).cuda()


def call(method, eos):
    stop = {} if eos is None else {"stop_on_eos": eos}
    if method == "greedy":
        return eng.generate_greedy(emb, None, N, **stop)
    return eng.generate_sampling(emb, None, N, temperature=1.0, uniforms=u, **stop)


def wall(fn):
    ctx.sync()
    t0 = time.perf_counter()
    out = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, out


def new_token_step(row, target):
    """the step >= 1 nearest to `target` whose token the row had not emitted before, or None"""
    seen, new = set(), []
    for k, t in enumerate(row):
        if t not in seen and k >= 1:
            new.append(k)
        seen.add(t)
    return min(new, key=lambda k: abs(k - target)) if new else None


print(f"stop_on_eos A/B: L{args.layers} T {T} max_len {N} pairs {args.pairs}", flush=True)
for method in args.methods.split(","):
    wall(lambda: call(method, None))                          # warm-up: code objects, the captured decode step
    row = call(method, None)[0][0].tolist()
    never = next(t for t in range(V) if t not in set(row))
    cases = [("never", never, None)]
    for target in (int(x) for x in args.targets.split(",")):
        k = new_token_step(row, target)
        if k is None:
            print(f"{method}: the run emits no new token behind step 0: no EOS to force near step {target}", flush=True)
        else:
            cases.append((f"eos@{k} (target {target})", row[k], k))
    for name, eos, k in cases:
        wall(lambda: call(method, eos))                       # (its own graph: a state with a stop never shares one)
        a_ms, b_ms, ratios, steps_run = [], [], [], None
        for _ in range(args.pairs):
            for side in "ABBA":
                ms, out = wall(lambda: call(method, None if side == "A" else eos))
                (a_ms if side == "A" else b_ms).append(ms)
                if side == "B":
                    steps_run = out[3][0].steps_run
            ratios.append((b_ms[-1] + b_ms[-2]) / (a_ms[-1] + a_ms[-2]))
        a, b = statistics.median(a_ms), statistics.median(b_ms)
        print(f"{method:8s} {name:24s} steps_run {steps_run:4d}  A {a:8.1f} ms  B {b:8.1f} ms  B/A per pair min {min(ratios):.4f} median "
              f"{statistics.median(ratios):.4f} max {max(ratios):.4f}  spread of A max/min {max(a_ms) / min(a_ms):.4f}", flush=True)
