"""QA batches whose rows share a prefix: the shared columns prefilled ONCE + one cache extension against the full prefill
`forward` runs today, ONE process, interleaved, the ProCyon-Full geometry (seeded random weights).  The shape is a configs[4] chunk
(workloads.config5_inputs): 64 rows of 439 tokens (bos, 437 words and slots, eos) that differ in the peptide of the last slot; the rows'
ends `<|protein|> ? [ANSWER]` are S = 3 tokens behind Tp = 435 shared ones, the closing eos is run by `forward` alone.

End to end (wall clock between two device synchronisations; tokenizer, protein encoder, projectors, splice, the host plan, the decoder):
  A  model.forward(inputs)                                        (the parent's path for this workload)
  B  model.forward(inputs, share_prefix=True, packed=False)
  C  model.forward(inputs, share_prefix=True)                     (packed=True)
The text decoder alone (device events), what the three calls above run on it:
  A  LlamaEngine.prefill of the [B, T] rows, logits at the answer rows
  B  prefill of the [1, Tp] prefix + LlamaEngine.extend of the [B, S] suffixes, no mask (the suffixes have one length)
  C  the same with the packed extension attention

`--pairs` rounds in ABC / CBA order, a block = `reps` back-to-back calls.  Prints one line per block, then ms per call of every side
(median), the per-round ratios B / A and C / B as min . median . max, the row arithmetic and the largest difference of the answer logits
between the sides.  Then the attention operator alone (pcy_attn_extend / pcy_attn_extend_packed on one layer: positions,
rope, K / V append and the attention launch -- the first three are the same launches on both sides), us per call at S in {3, 32} and
rows_per_prefix in {16, 64}, 64 rows, interleaved the same way.

`--groups G` measures something else and nothing of the above: the chunk of `--rows` rows spread over G receptors, rows / G each
(the receptor slots of group g read another protein; the rows of a group still differ in the peptide of the last slot; every call carries
only the proteins its own rows read), end to end:
  A  model.forward(inputs, share_prefix="groups")                 ONE prefill of the G prefixes + ONE grouped extension
  P  G calls of model.forward(inputs of one receptor, share_prefix=True)   (the parent's way for this batch: chunk by receptor)
  F  model.forward(inputs)                                        (the ordinary pass, for scale)
interleaved APF / FPA; prints ms per batch of every side (median) and the per-round ratio A / P as min . median . max.

  python tools/bench_qa_prefix.py
  python tools/bench_qa_prefix.py --pairs 1 --layers 4
  python tools/bench_qa_prefix.py --groups 4"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from procyon_amd import synthetic_model as SM
from procyon_amd import workloads
from procyon_amd.engine import BF16, KVCache, LlamaConfig, rope_tables
from procyon_amd.synthetic_model import GEOMETRIES

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=64)
ap.add_argument("--t", type=int, default=439, help="tokens per row (decoder-only part)")
ap.add_argument("--s", type=int, default=3, help="tokens per row behind the shared prefix, the answer token last")
ap.add_argument("--tail", type=int, default=1, help="tokens behind the answer token, which the full prefill alone runs (eos)")
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--block-ms", type=float, default=300.0)
ap.add_argument("--layers", type=int, default=0, help="decoder layers (0 = the geometry's 32)")
ap.add_argument("--attn-reps", type=int, default=200)
ap.add_argument("--groups", type=int, default=0, help="G > 0: the rows spread over G receptors, forward(share_prefix=\"groups\") against G calls of share_prefix=True")
args = ap.parse_args()

g = dict(GEOMETRIES["full"]["llama"])
if args.layers:
    g["n_layers"] = args.layers
cfg = LlamaConfig(**g, max_pos=4096)
model = SM.build("full", device="cuda", llama_layers=args.layers or None)
eng = model.text_encoder.engine
ctx = eng.ctx
B, T, S = args.rows, args.t, args.s
Tp = T - S - args.tail


def interleaved(sides, pairs, reps, unit, scale, tag, wall=False):
    ms = {k: [] for k in sides}
    order = list(sides)
    for p in range(pairs):
        for k in (order if p % 2 == 0 else order[::-1]):      # neither side always runs first
            fn = sides[k]
            ctx.sync()
            if wall:
                t0 = time.perf_counter()
                for _ in range(reps[k]):
                    fn()
                ctx.sync()
                ms[k].append((time.perf_counter() - t0) * 1e3 / reps[k] * scale)
            else:
                ctx.timer_start()
                for _ in range(reps[k]):
                    fn()
                ms[k].append(ctx.timer_stop() / reps[k] * scale)
            print(f"{tag} round {p} {k} {ms[k][-1]:.3f} {unit}/call ({reps[k]} calls)", flush=True)
    return ms


def ratio_line(ms, num, den):
    r = [a / b for a, b in zip(ms[num], ms[den])]
    return f"{num}/{den} per round min {min(r):.4f} med {statistics.median(r):.4f} max {max(r):.4f}"


# ---- end to end: UnifiedProCyon.forward on a chunk of the pair workload
make, _ = workloads.config5_inputs(256, B)

if args.groups:
    G = args.groups
    per = B // G
    assert per * G == B, f"--rows {B} is no multiple of --groups {G}"
    receptors = [0] + [3 + 200 + j for j in range(1, G)]        # group 0 keeps the 805-residue receptor, the others read another protein


    def part(lo, hi):
        inp = make(0)
        seq = [[receptors[i // per], 1, receptors[i // per], 2, receptors[i // per], 3 + i] for i in range(lo, hi)]
        used = sorted({j for row in seq for j in row})           # every call carries (and encodes) only the proteins its rows read
        new = {j: n for n, j in enumerate(used)}
        inp["data"]["seq"] = inp["data"]["seq"][used].clone()
        inp["data"]["seq_idx"] = torch.arange(len(used))
        seq = [[new[j] for j in row] for row in seq]
        inp["input"] = {"seq": seq, "text": [[] for _ in seq], "drug": None}
        inp["instructions"] = inp["instructions"][lo:hi]
        return inp


    def side_p():
        return torch.cat([model.forward(part(j * per, (j + 1) * per), retrieval=False, share_prefix=True)["outputs"].answer_logits[:, 0] for j in range(G)])


    e2e = {"A": lambda: model.forward(part(0, B), retrieval=False, share_prefix="groups")["outputs"].answer_logits[:, 0],
           "P": side_p,
           "F": lambda: model.forward(part(0, B), retrieval=False)["outputs"].answer_logits[:, 0]}
    plan = model.forward(part(0, B), retrieval=False, share_prefix="groups")["prefix_plan"]
    one = model.forward(part(0, per), retrieval=False, share_prefix=True)["prefix_plan"]
    reps, outs = {}, {}
    for k, fn in e2e.items():
        outs[k] = fn().float()
        ctx.sync()
        t0 = time.perf_counter(); fn(); ctx.sync()
        reps[k] = max(1, int(args.block_ms / max((time.perf_counter() - t0) * 1e3, 1e-3)))
    ms = interleaved(e2e, args.pairs, reps, "ms", 1.0, f"groups={G}", wall=True)
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(f"SUMMARY groups={G} rows={B} ({per} per receptor) group_len={plan['group_len']} S={plan['S']} (one receptor alone: Tp={one['Tp']} S={one['S']}) "
          f"layers={eng.cfg.n_layers}: A {med['A']:.3f} P {med['P']:.3f} F {med['F']:.3f} ms/batch wall (median of {args.pairs}); {ratio_line(ms, 'A', 'P')}; "
          f"{ratio_line(ms, 'A', 'F')}; token rows A = P {sum(plan['group_len']) + B * plan['S']} F {B * args.t}; "
          f"max |logits_A - logits_P| {float((outs['A'] - outs['P']).abs().max()):.3e} A and P bit-equal: {bool(torch.equal(outs['A'], outs['P']))}; "
          f"max |logits_A - logits_F| {float((outs['A'] - outs['F']).abs().max()):.3e} (max |logit| {float(outs['F'].abs().max()):.3e})", flush=True)
    sys.exit(0)

e2e = {"A": lambda: model.forward(make(0), retrieval=False),
       "B": lambda: model.forward(make(0), retrieval=False, share_prefix=True, packed=False),
       "C": lambda: model.forward(make(0), retrieval=False, share_prefix=True)}
reps, outs = {}, {}
for k, fn in e2e.items():
    out = fn()
    outs[k] = out["outputs"].answer_logits[:, 0].float()
    if k == "C":
        plan = out["prefix_plan"]
        real = int(out["outputs"].logits.shape[1])
    ctx.sync()
    t0 = time.perf_counter(); fn(); ctx.sync()
    reps[k] = max(1, int(args.block_ms / max((time.perf_counter() - t0) * 1e3, 1e-3)))
ms = interleaved(e2e, args.pairs, reps, "ms", 1.0, "forward", wall=True)
med = {k: statistics.median(v) for k, v in ms.items()}
print(f"SUMMARY forward rows={B} T={real} Tp={plan['Tp']} S={plan['S']} mask={'no' if bool(plan['suffix_mask'].all()) else 'yes'} layers={eng.cfg.n_layers}: "
      f"A {med['A']:.3f} B {med['B']:.3f} C {med['C']:.3f} ms/call wall (median of {args.pairs}); {ratio_line(ms, 'B', 'A')}; {ratio_line(ms, 'C', 'B')}; "
      f"token rows A {B * real} B = C {plan['Tp'] + B * plan['S']}; max |logits_A - logits_C| {float((outs['A'] - outs['C']).abs().max()):.3e} "
      f"(max |logit| {float(outs['A'].abs().max()):.3e}); B and C bit-equal: {bool(torch.equal(outs['B'], outs['C']))}", flush=True)

# ---- the text decoder alone
gen = torch.Generator().manual_seed(B)
pre_ids = torch.randint(0, 128000, (1, Tp), generator=gen)
suf_ids = torch.randint(0, 128000, (B, S + args.tail), generator=gen)
pre_emb, suf_emb = eng.embed_tokens(pre_ids), eng.embed_tokens(suf_ids[:, :S]).contiguous()
cat_emb = torch.cat([pre_emb.expand(B, -1, -1), eng.embed_tokens(suf_ids)], 1).contiguous()
rows_a = ((torch.arange(B) + 1) * T - 1 - args.tail).to(torch.int32)
cache_a = eng.new_cache(B, T)
prefix = eng.new_cache(1, Tp)
shared = eng.new_shared_cache(prefix, B, S)


def side_a():
    return eng.prefill(cat_emb, None, cache_a, rows_a)[0]


def side_bc(packed):
    def run():
        eng.prefill(pre_emb, None, prefix, logit_rows=None)
        return eng.extend(shared, suf_emb, Tp, logit_rows="last", packed=packed)[0]
    return run


sides = {"A": side_a, "B": side_bc(False), "C": side_bc(True)}
reps = {}
outs = {}
for k, fn in sides.items():          # warm-up + block size
    outs[k] = fn().float()
    ctx.sync()
    ctx.timer_start(); fn(); t1 = ctx.timer_stop()
    reps[k] = max(1, int(args.block_ms / max(t1, 1e-3)))
d_ab = float((outs["A"] - outs["B"]).abs().max())
bits_bc = bool(torch.equal(outs["B"], outs["C"]))
ms = interleaved(sides, args.pairs, reps, "ms", 1.0, "decoder")
med = {k: statistics.median(v) for k, v in ms.items()}
print(f"SUMMARY decoder rows={B} T={T} Tp={Tp} S={S} layers={g['n_layers']}: A {med['A']:.3f} B {med['B']:.3f} C {med['C']:.3f} ms/call (median of {args.pairs}); "
      f"{ratio_line(ms, 'B', 'A')}; {ratio_line(ms, 'C', 'B')}; token rows A {B * T} B = C {Tp + B * S} (x{B * T / (Tp + B * S):.1f}); "
      f"max |logits_A - logits_B| {d_ab:.3e} (max |logit| {float(outs['A'].abs().max()):.3e}); B and C bit-equal: {bits_bc}", flush=True)
del cache_a, prefix, shared, cat_emb
torch.cuda.empty_cache()

# ---- the attention operator alone, one layer
H, Hkv, dh = cfg.n_heads, cfg.n_kv_heads, cfg.d // cfg.n_heads
cfg1 = LlamaConfig(**dict(g, n_layers=1), max_pos=4096)
cos, sin = rope_tables(dh, 10000.0, 1024, "cuda")
for s_new in (3, 32):
    for rpp in (16, 64):
        gq = torch.Generator().manual_seed(s_new * 100 + rpp)
        pre = KVCache(cfg1, B // rpp, Tp, "cuda")
        pre.k.copy_(torch.randn(pre.k.shape, generator=gq).to(BF16))
        pre.v.copy_(torch.randn(pre.v.shape, generator=gq).to(BF16))
        cache = KVCache(cfg1, B, s_new, "cuda", prefix=pre, rows_per_prefix=rpp)
        qkv0 = torch.randn(B * s_new, (H + 2 * Hkv) * dh, generator=gq).to(BF16).cuda()
        qkv = qkv0.clone()

        def attn(packed):
            return lambda: ctx.attn_extend(qkv, cache, 0, Tp, cos, sin, H, Hkv, dh, packed=packed)

        o_b = ctx.attn_extend(qkv0.clone(), cache, 0, Tp, cos, sin, H, Hkv, dh, packed=False)
        o_c = ctx.attn_extend(qkv0.clone(), cache, 0, Tp, cos, sin, H, Hkv, dh, packed=True)
        sides = {"B": attn(False), "C": attn(True)}
        tag = f"attn S={s_new} rows_per_prefix={rpp}"
        ms = interleaved(sides, args.pairs, {k: args.attn_reps for k in sides}, "us", 1e3, tag)
        print(f"SUMMARY {tag} rows={B} Tp={Tp} H={H} Hkv={Hkv} dh={dh}: unpacked {statistics.median(ms['B']):.1f} packed {statistics.median(ms['C']):.1f} "
              f"us/call (median of {args.pairs}); {ratio_line(ms, 'C', 'B')}; bit-equal: {bool(torch.equal(o_b, o_c))}", flush=True)
