"""Plain references of the prefill attention operator (pcy_attention) and the input sets its tests share.

Three references, all over packed sequences as pcy_attention takes them (q [ntok, H*dh], k / v [ntok, Hkv*dh], `lens`):
  eager_bf16      the rounding-point oracle: HF eager attention in bf16, op for op (oracle/llama_ref.layer_forward, oracle/esm_ref.layer_forward)
  truth_f64       the same operation in float64 from the bf16 inputs, no intermediate rounding
  exact_key_sets  the expected output of the PROBE inputs by integer arithmetic: which keys each query attended, nothing else

The probe (probe_inputs): q = 0, so every score is 0 and every allowed key gets the weight bf16(1 / |A|); V[j][kvh*dh + d] = 2^(kvh % 4) where
j % dh == d and 0 elsewhere, so column d of the output counts the attended keys j with j % dh == d, scaled by a power of two that names the kv
head.  One wrongly attended or wrongly dropped key changes |A| and one count: the comparison is bit for bit.

Used by tests/test_attn_ref_cpu.py (what can be settled without a GPU) and tests/test_gpu_attn_prefill.py."""
import torch
import torch.nn.functional as F

BF = torch.bfloat16

# ---- input sets --------------------------------------------------------------------------------------------------------------------------
RAGGED = [500, 1, 127, 128, 129, 257, 64, 65, 33, 384, 385, 450, 31, 32, 200, 499]
LLAMA3 = [512, 450, 129, 1]
SHORT = [45] * 32
# name -> (H, Hkv, dh, lens).  Which kernel serves a set is NOT stated here: the GPU tests name the kernel they claim per set and the library's
# counter (pcy_debug_attn_route_count) is the evidence.
SETS = {
    "ragged16": (8, 2, 128, RAGGED),
    "llama3x4": (32, 8, 128, LLAMA3),
    "short32": (16, 16, 128, SHORT),
    "ragged3": (8, 2, 128, RAGGED[:3]),
    "llama3x2": (32, 8, 128, LLAMA3[:2]),
    "short3": (16, 16, 128, SHORT[:3]),
    "dh64": (4, 1, 64, [64, 65, 193, 300]),
    "dh32": (2, 2, 32, [50, 129]),
}
# the random-input cases: (set, causal, masked).  dh = 64: causal, and non-causal with keep (unmasked non-causal dh = 64 is the single-pass
# kernel's shape, tests/test_gpu_round3.py); everything else in all four combinations -- non-causal dh = 128 included.
RANDOM_CASES = [(s, c, m) for s in ("ragged16", "llama3x4", "short32", "ragged3", "llama3x2", "short3", "dh32") for c in (True, False) for m in (False, True)]
RANDOM_CASES += [("dh64", True, False), ("dh64", True, True), ("dh64", False, True)]
# Seeds of the random inputs (q, k, v = seed, seed + 1, seed + 2).  An input set must let the oracle's own twin (eager_bf16(alt=True)) pass
# the elementwise bar; tests/test_attn_ref_cpu.py holds every set to that.  Seed 1 does not for the Llama-3 heads: causal row 1 of head 19
# has P = 0.50195311507 against the bf16 rounding midpoint 0.501953125 -- 1.7e-8 relative, below fp32 resolution -- with |v| = 1.5, so two
# correct fp32 softmaxes round P to 0.5 and to 0.50390625 and five outputs move by 2^-8 |v|, past the bar's grant.  The input set changes,
# not the bar.
SEED = {name: 1 for name in SETS}
SEED.update(llama3x4=11, llama3x2=11)
LEFT_PADS = (0, 5, 33, 64, 130, -1)    # -1: n - 1 keys (one kept key, the last)


def rnd(*shape, seed=0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(BF)


def _seqs(lens):
    t0 = 0
    for n in lens:
        yield t0, n
        t0 += n


def mask_patterns(lens):
    """name -> keep (uint8 [ntok]) or None.  Every pattern is built per sequence from its own length."""
    ntok = sum(lens)

    def build(fn):
        keep = torch.ones(ntok, dtype=torch.uint8)
        for s, (t0, n) in enumerate(_seqs(lens)):
            fn(keep[t0:t0 + n], n, s)
        return keep

    def left(pad):
        def fn(kp, n, s):
            kp[:min(pad if pad >= 0 else n - 1, n - 1)] = 0
        return fn

    def full_seq(kp, n, s):          # sequences 0, 3, 6, ...: no kept key at all
        if s % 3 == 0:
            kp[:] = 0

    def every7(kp, n, s):
        kp[3::7] = 0

    def block(kp, n, s):             # one whole 32-key block: the second one, or the first of a short sequence (none of a one-block sequence)
        if n > 32:
            b0 = 32 if n > 64 else 0
            kp[b0:b0 + 32] = 0

    def diagonal(kp, n, s):          # holes across rows 64 and 128: the causal diagonal where a 64-row and a 128-row workgroup end
        kp[50:80] = 0
        kp[120:140] = 0

    def trailing(kp, n, s):
        kp[max(1, n - (1 + n // 3)):] = 0

    pats = {"none": None}
    for pad in LEFT_PADS:
        pats["left%s" % ("N-1" if pad < 0 else pad)] = build(left(pad))
    pats.update(full_seq=build(full_seq), every7=build(every7), block=build(block), diagonal=build(diagonal), trailing=build(trailing))
    return pats


def mixed_mask(lens):
    """the mask of the random-input cases: the patterns above, one per sequence in turn"""
    pats = [p for name, p in mask_patterns(lens).items() if name in ("left5", "left33", "left130", "every7", "block", "diagonal", "trailing")]
    keep = torch.ones(sum(lens), dtype=torch.uint8)
    for s, (t0, n) in enumerate(_seqs(lens)):
        keep[t0:t0 + n] = pats[s % len(pats)][t0:t0 + n]
    return keep


def random_inputs(name, causal, seed=None):
    """q, k, v, scale of a random-input case, as tests/test_gpu_kernels.py::test_attention_exact_rounding draws them: the Llama convention
    (scale = dh^-0.5) when causal, the ESM one (q pre-scaled, scale = 1) when not."""
    H, Hkv, dh, lens = SETS[name]
    n, sd = sum(lens), SEED[name] if seed is None else seed
    q, k, v = rnd(n, H * dh, seed=sd), rnd(n, Hkv * dh, seed=sd + 1), rnd(n, Hkv * dh, seed=sd + 2)
    if causal:
        return q, k, v, dh ** -0.5
    return (q.float() * dh ** -0.5).to(BF), k, v, 1.0


def probe_inputs(H, Hkv, dh, lens):
    ntok = sum(lens)
    q = torch.zeros(ntok, H * dh, dtype=BF)
    k = rnd(ntok, Hkv * dh, seed=5)
    v = torch.zeros(ntok, Hkv, dh)
    for t0, n in _seqs(lens):
        j = torch.arange(n)
        v[t0 + j, :, j % dh] = (2.0 ** (torch.arange(Hkv) % 4))[None, :].expand(n, Hkv)
    return q, k, v.view(ntok, Hkv * dh).to(BF)


# ---- references --------------------------------------------------------------------------------------------------------------------------
def allowed_keys(n, causal, keep_seq):
    """[n, n] bool: query i may attend key j.  Rows without any allowed key stay all-False here."""
    a = torch.ones(n, n, dtype=torch.bool)
    if causal:
        a = torch.tril(a)
    if keep_seq is not None:
        a = a & keep_seq.bool()[None, :]
    return a


MUTANTS = ("strict_causal_from_256", "pad_keys_v0", "pad_keys_v1", "keep_prev_sequence", "kv_head_modulo", "empty_rows_causal")


def eager_bf16(q, k, v, H, Hkv, dh, lens, causal, scale, keep=None, alt=False, mutant=None):
    """HF eager attention per packed sequence with the reference's rounding points:
        S = bf16(bf16(Q K^T) * scale) + additive finfo.min mask ; P = bf16(softmax_fp32(S)) ; O = bf16(P V)
    A row without an allowed key ends as S = finfo.min everywhere: uniform over all keys of its sequence.
    alt: the same rounding points through other fp32 arithmetic (the idea of conftest.alt_accumulation) -- both matmuls in fp32, rounded once,
        and the softmax as exp2(s log2e - max) x (1 / sum).  What the twin and the oracle disagree on is the reference's own noise.
    mutant: one of MUTANTS, a deliberately WRONG mask / head rule (tests/test_attn_ref_cpu.py shows that the probe sees each of them):
        strict_causal_from_256  j < i instead of j <= i for query rows at or above 256
        pad_keys_v0 / _v1       keys n .. roundup(n, 32) - 1 take part (K of the last key, V = 0 / 1) wherever causality allows
        keep_prev_sequence      keep read at the offset of the sequence before
        kv_head_modulo          kv head h % Hkv instead of h // (H / Hkv)
        empty_rows_causal       rows without an allowed key uniform over j <= i instead of over all keys"""
    assert mutant is None or mutant in MUTANTS, mutant
    G = H // Hkv

    def mm(a, b):
        return (a.float() @ b.float()).to(BF) if alt else torch.matmul(a, b)

    def heads(x, n):
        x = x.view(n, Hkv, dh).transpose(0, 1)
        return x[torch.arange(H) % Hkv] if mutant == "kv_head_modulo" else x.repeat_interleave(G, 0)

    outs, prev = [], (sum(lens) - lens[-1], lens[-1])
    for t0, n in _seqs(lens):
        qs, ks, vs = q[t0:t0 + n].view(n, H, dh).transpose(0, 1), heads(k[t0:t0 + n], n), heads(v[t0:t0 + n], n)
        kp = None if keep is None else keep[t0:t0 + n]
        if mutant == "keep_prev_sequence" and keep is not None:
            kp = torch.roll(keep, t0 - prev[0])[t0:t0 + n]
        allowed = allowed_keys(n, causal, kp)
        if mutant == "strict_causal_from_256" and causal:
            i = torch.arange(n)
            allowed = allowed & ~((i[:, None] == i[None, :]) & (i[:, None] >= 256))
        if mutant == "empty_rows_causal" and causal:
            allowed = torch.where(allowed.any(1, keepdim=True), allowed, torch.tril(torch.ones(n, n, dtype=torch.bool)))
        if mutant in ("pad_keys_v0", "pad_keys_v1"):
            npad = (n + 31) // 32 * 32 - n
            ks = torch.cat([ks, ks[:, -1:].expand(H, npad, dh)], 1)
            vs = torch.cat([vs, torch.full((H, npad, dh), 0.0 if mutant == "pad_keys_v0" else 1.0, dtype=BF)], 1)
            allowed = torch.cat([allowed, torch.full((n, npad), not causal, dtype=torch.bool)], 1)
        s = mm(qs, ks.transpose(1, 2)) * scale
        minv = torch.finfo(BF).min
        s = s + torch.where(allowed, torch.zeros((), dtype=BF), torch.full((), minv, dtype=BF))[None]
        if alt:      # exp(s - m) / l as exp2(s log2e - m log2e) x (1 / l): every step fp32, as a single-exponent-instruction softmax runs it
            t = torch.where(s == minv, s.float(), s.float() * torch.tensor(1.4426950408889634, dtype=torch.float32))   # (masked: finfo.min stays finite)
            e =torch.exp2(t - t.amax(-1, keepdim=True))
            p = (e * (1.0 / e.sum(-1, keepdim=True))).to(BF)
        else:
            p = F.softmax(s, dim=-1, dtype=torch.float32).to(BF)
        outs.append(mm(p, vs).transpose(0, 1).reshape(n, H * dh))
        prev = (t0, n)
    return torch.cat(outs)


def truth_f64(q, k, v, H, Hkv, dh, lens, causal, scale, keep=None):
    """the same operation in float64 from the bf16 inputs, no intermediate rounding; a row without a kept key: uniform over all keys"""
    G, outs = H // Hkv, []
    for t0, n in _seqs(lens):
        qs = q[t0:t0 + n].double().view(n, H, dh).transpose(0, 1)
        ks = k[t0:t0 + n].double().view(n, Hkv, dh).transpose(0, 1).repeat_interleave(G, 0)
        vs = v[t0:t0 + n].double().view(n, Hkv, dh).transpose(0, 1).repeat_interleave(G, 0)
        allowed = allowed_keys(n, causal, None if keep is None else keep[t0:t0 + n])
        s = torch.matmul(qs, ks.transpose(1, 2)) * float(scale)
        s = s.masked_fill(~allowed[None], float("-inf"))
        empty = ~allowed.any(1)
        s[:, empty] = 0.0
        outs.append(torch.matmul(torch.softmax(s, dim=-1), vs).transpose(0, 1).reshape(n, H * dh))
    return torch.cat(outs)


def exact_key_sets(H, Hkv, dh, lens, causal, keep=None):
    """Expected output of probe_inputs: O[i][h*dh + d] = bf16(bf16(1 / |A|) * 2^(kvh % 4) * #{j in A : j % dh == d}), kvh = h // (H / Hkv),
    A = {j < n : (not causal or j <= i) and keep[j]}, or all n keys when that set is empty.  Integer counts, one correctly rounded fp32
    division, an exact product (8 significant bits x a power of two x a small integer), one bf16 rounding.  No matmul, no softmax."""
    G, outs = H // Hkv, []
    for t0, n in _seqs(lens):
        allowed = allowed_keys(n, causal, None if keep is None else keep[t0:t0 + n])
        allowed = torch.where(allowed.any(1, keepdim=True), allowed, torch.ones(n, n, dtype=torch.bool))
        size = allowed.sum(1)                                                                # |A| per query
        cnt = torch.zeros(n, dh, dtype=torch.int64).index_add_(1, torch.arange(n) % dh, allowed.long())
        p = (torch.ones(n, dtype=torch.float32) / size.float()).to(BF).float()               # bf16(1 / |A|)
        head = 2.0 ** ((torch.arange(H) // G) % 4).float()                                   # 2^(kvh % 4)
        o = p[:, None, None] * head[None, :, None] * cnt.float()[:, None, :]                 # exact in fp32
        outs.append(o.to(BF).reshape(n, H * dh))
    return torch.cat(outs)
