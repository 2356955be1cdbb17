"""Plain torch restatements of the fp32 operator family (`pcy_f32_*`, include/pcy.h), written from the definitions in the header and
the oracle, never from the kernels.  Every function takes the operator's fp32 inputs, upcasts them to `dt` (float64: the reference
the GPU tests compare against; float32: the "plain torch fp32" evaluation tests/test_f32_ref_cpu.py holds to the same bar) and
returns a `dt` tensor.  The input sets of the GPU operator tests live here too (`*_case`), so that the CPU test sees the same numbers."""
import math

import torch

F64 = torch.float64
MASK_ID, PAD_ID = 32, 1
OP_BAR, OP_MAXABS = 2e-5, 2e-4          # single-operator bars of tests/test_gpu_fp32.py: norm-wise relative, max-abs / max|ref|


def rnd(*shape, seed=0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


def rel64(a, b):
    """norm-wise relative error of a against the reference b, in float64"""
    a, b = a.to(F64), b.to(F64)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def maxabs64(a, b):
    """max |a - b| / max |b|"""
    a, b = a.to(F64), b.to(F64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ references
def linear(A, W, bias=None, resid=None, act=0, dt=F64):
    """C = act(A . W^T + bias) (+ resid); act 1 = x * 0.5 * (1 + erf(x / sqrt 2))"""
    y = A.to(dt) @ W.to(dt).T
    if bias is not None:
        y = y + bias.to(dt)
    if act == 1:
        y = y * 0.5 * (1.0 + torch.erf(y / math.sqrt(2.0)))
    if resid is not None:
        y = y + resid.to(dt)
    return y


def layernorm(x, w, b, eps, dt=F64):
    x = x.to(dt)
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)
    return (x - mean) * torch.rsqrt(var + eps) * w.to(dt) + b.to(dt)


def rmsnorm(x, w, eps, dt=F64):
    x = x.to(dt)
    return w.to(dt) * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def rope(buf, col0, nh, dh, pos, cos, sin, prescale=0.0, dt=F64):
    """the whole buffer, heads [col0, col0 + nh*dh) of every row rotated: x' cos[pos] + rotate_half(x') sin[pos], x' = x * prescale"""
    out = buf.to(dt).clone()
    T = buf.shape[0]
    x = out[:, col0:col0 + nh * dh].reshape(T, nh, dh)
    if prescale != 0.0:
        x = x * torch.tensor(prescale, dtype=torch.float32).to(dt)      # the fp32 value of the factor, as the kernel receives it
    c, s = cos.to(dt)[pos.long()][:, None], sin.to(dt)[pos.long()][:, None]
    rot = torch.cat((-x[..., dh // 2:], x[..., :dh // 2]), -1)
    out[:, col0:col0 + nh * dh] = (x * c + rot * s).reshape(T, nh * dh)
    return out


def attention(q, k, v, cu, keep, H, Hkv, dh, causal, scale, dt=F64):
    """q [ntok, H*dh], k / v [ntok, Hkv*dh] packed by cu; keep [ntok] (0 = the key is masked) or None -> [ntok, H*dh].
    A query row with no allowed key takes the plain average of V over all keys of its sequence: the reference adds finfo.min to every
    masked score, in fp32 that sum IS finfo.min whatever the score, and the softmax of a constant row is uniform (include/pcy.h)."""
    out = torch.zeros(q.shape[0], H * dh, dtype=dt)
    g = H // Hkv
    for s_ in range(cu.numel() - 1):
        t0, t1 = int(cu[s_]), int(cu[s_ + 1])
        n = t1 - t0
        if n == 0:
            continue
        qq = q[t0:t1].to(dt).view(n, H, dh).transpose(0, 1)
        kk = k[t0:t1].to(dt).view(n, Hkv, dh).transpose(0, 1).repeat_interleave(g, 0)
        vv = v[t0:t1].to(dt).view(n, Hkv, dh).transpose(0, 1).repeat_interleave(g, 0)
        allowed = torch.ones(n, n, dtype=torch.bool)
        if keep is not None:
            allowed &= keep[t0:t1].bool()[None, :]
        if causal:
            allowed &= torch.tril(torch.ones(n, n, dtype=torch.bool))
        sc = (qq @ kk.transpose(1, 2)) * torch.tensor(scale, dtype=torch.float32).to(dt)
        sc = sc.masked_fill(~allowed[None], float("-inf"))
        keyless = ~allowed.any(-1)
        sc[:, keyless] = 0.0                                     # constant row -> uniform over all n keys
        out[t0:t1] = (sc.softmax(-1) @ vv).transpose(0, 1).reshape(n, H * dh)
    return out


def keyless_rows(cu, keep, causal):
    """bool [ntok]: query rows without any allowed key"""
    out = torch.zeros(int(cu[-1]), dtype=torch.bool)
    for s_ in range(cu.numel() - 1):
        t0, t1 = int(cu[s_]), int(cu[s_ + 1])
        kp = torch.ones(t1 - t0, dtype=torch.bool) if keep is None else keep[t0:t1].bool()
        out[t0:t1] = (kp.cumsum(0) == 0) if causal else ~kp.any().expand(t1 - t0)
    return out


def attn_decode(q, kc, vc, nkeys, H, Hkv, dh, scale, dt=F64):
    """q [B, H*dh] against slots [0, nkeys) of kc / vc [B, Tmax, Hkv*dh], no mask -> [B, H*dh]"""
    B = q.shape[0]
    g = H // Hkv
    qq = q.to(dt).reshape(B, H, 1, dh)
    kk = kc[:, :nkeys].to(dt).reshape(B, nkeys, Hkv, dh).permute(0, 2, 1, 3).repeat_interleave(g, 1)
    vv = vc[:, :nkeys].to(dt).reshape(B, nkeys, Hkv, dh).permute(0, 2, 1, 3).repeat_interleave(g, 1)
    sc = (qq @ kk.transpose(2, 3)) * torch.tensor(scale, dtype=torch.float32).to(dt)
    return (sc.softmax(-1) @ vv).reshape(B, H * dh)


def esm_embed(table, tokens, cu, mask_pads, dt=F64):
    """packed tokens [ntok] of sequences cu -> [ntok, d]: table[t] * (1 - 0.15 * 0.8) / (1 - n_mask / n), n = the sequence's non-pad
    tokens (mask_pads) or all of its tokens; <mask> rows zero; pad rows zero when mask_pads"""
    out = table.to(dt)[tokens.long()]
    for s_ in range(cu.numel() - 1):
        t0, t1 = int(cu[s_]), int(cu[s_ + 1])
        t = tokens[t0:t1]
        n = int((t != PAD_ID).sum()) if mask_pads else t1 - t0
        ratio = torch.tensor(float((t == MASK_ID).sum()), dtype=dt) / n
        out[t0:t1] = out[t0:t1] * (1 - 0.15 * 0.8) / (1 - ratio)
    zero = (tokens == MASK_ID) | ((tokens == PAD_ID) if mask_pads else torch.zeros_like(tokens, dtype=torch.bool))
    out[zero] = 0.0
    return out


def pool(h, seg, rng, mode, dt=F64):
    """h [ntok, d]; protein p owns ranges seg[p] .. seg[p+1]-1 of rng [(start, length)]: its rows are the ranges' rows in order.
    mode 0 nanmean over the rows, 1 nanmean over rows[1:-1], 2 max"""
    outs = []
    for p in range(len(seg) - 1):
        rows = torch.cat([h[st:st + ln] for st, ln in rng[seg[p]:seg[p + 1]]]).to(dt)
        if mode == 1:
            rows = rows[1:-1]
        outs.append(rows.max(0)[0] if mode == 2 else rows.nanmean(0))
    return torch.stack(outs)


def embed(table, ids, soft=None, soft_map=None):
    """out[r] = soft[soft_map[r]] if soft_map[r] >= 0 else table[ids[r]]  (a gather: exact, any dtype)"""
    out = table[ids.long()].clone()
    if soft_map is not None:
        m = soft_map >= 0
        out[m] = soft[soft_map[m].long()]
    return out


def acc_rows(dst, src, rows, d, dt=F64):
    """dst[r] + src[rows[r], :d]"""
    return dst.to(dt) + src.to(dt)[rows.long(), :d]


def silu_mul(g, u, dt=F64):
    g = g.to(dt)
    return g * torch.sigmoid(g) * u.to(dt)


# ------------------------------------------------------------------------------------------------ input sets of the operator tests
LINEAR_MODES = ("plain", "bias_gelu", "bias_resid")
# name -> (M, N, K); `window`: lda > K, ldc > N, ldr > N into a column window; `alias`: resid is C; `offset`: A starts one float late
LINEAR_CASES = {"window": (130, 200, 64), "alias": (130, 200, 64), "m1": (1, 200, 64), "k16": (130, 200, 16), "n130": (130, 130, 64),
                "offset": (130, 200, 64)}


def linear_case(name):
    M, N, K = LINEAR_CASES[name]
    return dict(A=rnd(M, K, seed=11), W=rnd(N, K, seed=12, std=0.05), bias=rnd(N, seed=13, std=0.1), resid=rnd(M, N, seed=14))


def linear_args(case, mode):
    """(bias, resid, act) of a mode"""
    return (None if mode == "plain" else case["bias"], case["resid"] if mode == "bias_resid" else None, 1 if mode == "bias_gelu" else 0)


NORM_DIMS = (1, 100, 256, 257, 4096)


def norm_case(d):
    return dict(x=8 + rnd(5, d, seed=21), w=1 + rnd(d, seed=22, std=0.1), b=rnd(d, seed=23, std=0.1), eps=1e-5)


ROPE_GEOMS = ((8, 128), (1, 16))
ROPE_NPOS, ROPE_COL0, ROPE_TAIL = 96, 8, 5


def rope_tables(dh, n_pos):
    """fp32 cos / sin [n_pos, dh], the formula of oracle.llama_ref.rope_tables"""
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, dh, 2, dtype=torch.float32) / dh))
    freqs = (inv_freq[:, None] @ torch.arange(n_pos, dtype=torch.float32)[None, :]).transpose(0, 1)
    emb = torch.cat((freqs, freqs), -1)
    return emb.cos(), emb.sin()


def rope_case(nh, dh):
    T = 11
    pos = torch.randint(0, ROPE_NPOS, (T,), generator=torch.Generator().manual_seed(31)).to(torch.int32)
    pos[0], pos[1] = 0, ROPE_NPOS - 1
    cos, sin = rope_tables(dh, ROPE_NPOS)
    return dict(buf=rnd(T, ROPE_COL0 + nh * dh + ROPE_TAIL, seed=32), pos=pos, cos=cos, sin=sin)


DECODE_NKEYS = (1, 63, 64, 65, 200)
DECODE_GEOMS = ((4, 4, 16), (8, 2, 64), (4, 1, 128))


def decode_case(nkeys, H, Hkv, dh):
    """qkv [B, (H + 2 Hkv) dh] (q is its first H*dh columns), caches [B, nkeys + 7, Hkv*dh] with NaN beyond slot nkeys"""
    B, Tmax = 3, nkeys + 7
    kc, vc = rnd(B, Tmax, Hkv * dh, seed=41), rnd(B, Tmax, Hkv * dh, seed=42)
    kc[:, nkeys:] = float("nan")
    vc[:, nkeys:] = float("nan")
    return dict(qkv=rnd(B, (H + 2 * Hkv) * dh, seed=43), kc=kc, vc=vc)


ATTN_GEOM = (4, 2, 64)
ATTN_LENS, ATTN_PADS = (12, 70, 1, 65), (5, 0, 0, 64)


def attn_case():
    H, Hkv, dh = ATTN_GEOM
    cu = torch.tensor([0] + list(torch.tensor(ATTN_LENS).cumsum(0)), dtype=torch.int32)
    keep = torch.ones(int(cu[-1]), dtype=torch.uint8)
    for s_, p in enumerate(ATTN_PADS):
        keep[int(cu[s_]):int(cu[s_]) + p] = 0
    return dict(qkv=rnd(int(cu[-1]), (H + 2 * Hkv) * dh, seed=51), cu=cu, keep=keep)


def attn_windows(qkv):
    H, Hkv, dh = ATTN_GEOM
    return qkv[:, :H * dh], qkv[:, H * dh:(H + Hkv) * dh], qkv[:, (H + Hkv) * dh:]


ESM_LENS, ESM_VOCAB = (1, 5, 64, 65, 300), 33
ESM_VARIANTS = ((1, False), (0, True), (1, True))       # (mask_pads, pad tokens inside the packed rows)


def esm_case(d, pads):
    """packed residues (ids 4..23) with <mask> at 0, 1, 3, 4 and 9 positions of the five sequences; `pads`: the tail of every row longer
    than one token is pad (id 1), as a row packed with its pads"""
    g = torch.Generator().manual_seed(61)
    toks, cu = [], [0]
    for n, nm in zip(ESM_LENS, (0, 1, 3, 4, 9)):
        t = torch.randint(4, 24, (n,), generator=g)
        npad = min(n - 1, 1 + n // 7) if pads else 0
        if npad:
            t[n - npad:] = PAD_ID
        t[torch.randperm(n - npad, generator=g)[:nm]] = MASK_ID
        assert int((t == MASK_ID).sum()) == nm and nm < max(n - npad, 1)       # never a whole sequence
        toks.append(t)
        cu.append(cu[-1] + n)
    return dict(table=rnd(ESM_VOCAB, d, seed=62), tokens=torch.cat(toks).to(torch.int32), cu=torch.tensor(cu, dtype=torch.int32))


POOL_DIMS = (320, 100, 257)
POOL_SEG = (0, 1, 3, 6, 7)                                          # proteins of 1, 2, 3 and 1 ranges
POOL_RNG = ((0, 9), (9, 1), (10, 6), (16, 5), (21, 1), (22, 4), (26, 3))   # the last protein: a single range of length 3


def pool_case(d, nan):
    h = rnd(29, d, seed=71)
    if nan:
        h[12, d - 1] = float("nan")            # protein 1, second range, not an end row; the last feature (the second slab when d > 256)
    return dict(h=h)


EMBED_DIMS = (100, 1280)


def embed_case(d):
    V = 50
    ids = torch.tensor([0, V - 1, 7, 7, 3, V - 1, 0, 21, 30], dtype=torch.int32)
    soft_map = torch.tensor([-1, -1, 2, -1, 0, -1, -1, 1, -1], dtype=torch.int32)
    return dict(table=rnd(V, d, seed=81), ids=ids, soft=rnd(3, d, seed=82), soft_map=soft_map)


def acc_case():
    d, ld = 100, 132
    return dict(src=rnd(9, ld, seed=91), rows=torch.tensor([4, 0, 4, 8], dtype=torch.int32), dst=rnd(4, d, seed=92), d=d,
                src2=rnd(9, ld, seed=93))


SILU_BIG = 65536 * 256 + 257
SILU_SPECIAL = (1e4, -1e4, 88.0, -88.0, 0.0)


def silu_case(n):
    g = rnd(n, seed=101, std=2.0)
    u = rnd(n, seed=102)
    if n >= 2 * len(SILU_SPECIAL):
        g[:len(SILU_SPECIAL)] = torch.tensor(SILU_SPECIAL)
        g[-len(SILU_SPECIAL):] = torch.tensor(SILU_SPECIAL)
    return dict(g=g, u=u)


# ------------------------------------------------------------------------------------------------ padded generation (fp32 Llama)
GEN_GEOM = dict(vocab=331, d=256, n_layers=3, n_heads=4, n_kv_heads=2, ffn=512)
GEN_B, GEN_T, GEN_PADS, GEN_STEPS = 3, 12, (0, 5, 1), 6


def gen_case():
    """prompt ids [3, 12] and the 0/1 mask with left pads {0, 5, 1}"""
    ids = torch.randint(0, GEN_GEOM["vocab"], (GEN_B, GEN_T), generator=torch.Generator().manual_seed(111))
    mask = torch.ones(GEN_B, GEN_T, dtype=torch.long)
    for b, p in enumerate(GEN_PADS):
        mask[b, :p] = 0
    return ids, mask
