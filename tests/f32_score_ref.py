"""Helpers of the fp32 scoring tests: float64 restatements of `pcy_f32_lm_head_xent` and `pcy_f32_attn_extend`, written from the contracts in
include/pcy.h (never from the kernels), and the input sets the GPU tests and tests/test_f32_score_ref_cpu.py share.  Style and bars as
tests/f32_ref.py: every reference upcasts its fp32 inputs to `dt` (float64 = the reference, float32 = "plain torch fp32")."""
import math

import torch

import f32_ref as R

F64 = torch.float64
TILE, MAX_BLOCKS, MCHUNK = 128, 512, 1024       # the operator's partition constants (include/pcy.h, procyon_amd/csrc/pcy_f32.hip)


# ------------------------------------------------------------------------------------------------ lm_head x cross-entropy
def col_blocks(V):
    """(tiles per column block, column blocks) of a vocabulary of V columns: at most MAX_BLOCKS blocks of consecutive 128-column tiles"""
    tiles = (V + TILE - 1) // TILE
    cb = (tiles + MAX_BLOCKS - 1) // MAX_BLOCKS
    return cb, (tiles + cb - 1) // cb


def ws_bytes(M, V):
    return min(M, MCHUNK) * (col_blocks(V)[1] * 8 + 4)


def lm_head_xent(L, targets, dt=F64):
    """L [M, V] logits, targets [M] -> (nll, lse, row_max, label_logit) [M] in dt; lse = max + log sum exp(l - max), nll = lse - l[target];
    a target outside [0, V) gives NaN in nll and label_logit of that row"""
    L = L.to(dt)
    M, V = L.shape
    mx = L.max(-1).values
    lse = mx + torch.log(torch.exp(L - mx[:, None]).sum(-1))
    t = targets.long()
    ok = (t >= 0) & (t < V)
    lab = torch.where(ok, L.gather(1, t.clamp(0, V - 1)[:, None])[:, 0], torch.full((), float("nan"), dtype=dt))
    return lse - lab, lse, mx, lab


def ulp32(v):
    """one fp32 ulp at |v| (float64 tensor in, float64 out)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 23)


def xent_bar(L, targets):
    """The project's bar for lse / nll on given fp32 logits L (on the host): 8 x max(torch's own fp32 cross_entropy / logsumexp error against
    float64 on the same logits, one fp32 ulp at max(|lse|, |row max|)) -> (bar [M] float64, torch's error, the float64 reference tuple)"""
    ref = lm_head_xent(L, targets)
    l32 = torch.logsumexp(L.float(), -1).double()
    ce32 = torch.nn.functional.cross_entropy(L.float(), targets.long(), reduction="none").double()
    err_a = max(float((l32 - ref[1]).abs().max()), float((ce32 - ref[0]).abs().max()))
    ulp = ulp32(torch.maximum(ref[1].abs(), ref[2].abs()))
    return 8 * torch.clamp(ulp, min=err_a), err_a, ref


XENT_SETS = ("random", "negative", "peaked")
XENT_M = 257


def planted_targets(V):
    """column 0, column V-1, the first and last column of a tile, the ragged tail"""
    last0 = (V - 1) // TILE * TILE                  # first column of the last (ragged) tile
    return [0, V - 1, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, last0, last0 - 1, V - 7]


def xent_case(V, d, kind):
    """x [257, d], W [V, d] fp32, targets int64 [257] (the first ones planted).  random: logits ~ N(0, 1); negative: every logit in
    [-22, -18], so a zero pad column that gets counted dominates the sum; peaked: 85-92 at tile edges and in the ragged tail, so that exp
    overflows without the max and a dropped tail costs several units"""
    g = torch.Generator().manual_seed(2000 + V % 977 + 7 * d + XENT_SETS.index(kind))
    M = XENT_M
    x0 = torch.randn(d, generator=g)
    x = x0[None] + 0.1 * torch.randn(M, d, generator=g)
    n2 = float(x0.pow(2).sum())
    if kind == "random":
        W = torch.randn(V, d, generator=g) / math.sqrt(d)
    elif kind == "negative":
        W = -(20 / n2) * x0[None] + (0.16 / math.sqrt(d)) * torch.randn(V, d, generator=g)
    else:
        W = torch.randn(V, d, generator=g) / math.sqrt(d)
        W[V - 1] = (90 / n2) * x0
        W[V - 7] = (88 / n2) * x0
        for k in (TILE - 1, TILE, 2 * TILE - 1, 2 * TILE):
            if k < V - 7:
                W[k] = (85 / n2) * x0
    tg = torch.randint(0, V, (M,), generator=g)
    pt = planted_targets(V)
    tg[:len(pt)] = torch.tensor(pt)
    return x.contiguous(), W.contiguous(), tg


def fault_costs(L):
    """What the two faults of a row reduction over a ragged vocabulary would move the LSE by, as float64 arithmetic on given logits [M, V]:
    (dropping the columns of the last, partly filled tile; counting its pad columns as logits of 0) -> two [M] tensors"""
    L = L.double()
    V = L.shape[1]
    last0 = (V - 1) // TILE * TILE
    npad = last0 + TILE - V
    lse = torch.logsumexp(L, -1)
    dropped = lse - torch.logsumexp(L[:, :last0], -1) if last0 > 0 else torch.full_like(lse, float("inf"))
    padded = torch.logsumexp(torch.cat([L, torch.zeros(L.shape[0], npad, dtype=F64)], 1), -1) - lse
    return dropped, padded


# ------------------------------------------------------------------------------------------------ cache extension
def attn_extend(qkv, kc, vc, t_past, S, H, Hkv, dh, scale, keep=None, cache_row=None, dt=F64):
    """qkv [B*S, (H + 2 Hkv) dh] roped (q | new K | new V); kc / vc [rows, Tmax, Hkv*dh]; query s of row b attends slots [0, t_past) of cache
    row cache_row[b] (None = b) and the new keys 0..s of its own row; keep [B, >= t_past + S] (0 = masked key) or None -> [B*S, H*dh].
    A query without any kept key takes the plain average of V over all t_past + S keys of its row (include/pcy.h)."""
    B = qkv.shape[0] // S
    g = H // Hkv
    n = t_past + S
    out = torch.zeros(B * S, H * dh, dtype=dt)
    causal = torch.arange(n)[None, :] <= (t_past + torch.arange(S))[:, None]                     # [S, n]
    for b in range(B):
        cr = b if cache_row is None else int(cache_row[b])
        rows = qkv[b * S:(b + 1) * S].to(dt)
        q = rows[:, :H * dh].view(S, H, dh).transpose(0, 1)                                     # [H, S, dh]
        k = torch.cat([kc[cr, :t_past].to(dt), rows[:, H * dh:(H + Hkv) * dh]], 0).view(n, Hkv, dh).transpose(0, 1).repeat_interleave(g, 0)
        v = torch.cat([vc[cr, :t_past].to(dt), rows[:, (H + Hkv) * dh:(H + 2 * Hkv) * dh]], 0).view(n, Hkv, dh).transpose(0, 1).repeat_interleave(g, 0)
        allowed = causal.clone()
        if keep is not None:
            allowed &= keep[b, :n].bool()[None, :]
        sc = (q @ k.transpose(1, 2)) * torch.tensor(scale, dtype=torch.float32).to(dt)
        sc = sc.masked_fill(~allowed[None], float("-inf"))
        sc[:, ~allowed.any(-1)] = 0.0                                                           # constant row -> uniform over all n keys
        out[b * S:(b + 1) * S] = (sc.softmax(-1) @ v).transpose(0, 1).reshape(S, H * dh)
    return out


def keyless_queries(keep, B, S, t_past):
    """bool [B*S]: queries without any kept key"""
    n = t_past + S
    causal = torch.arange(n)[None, :] <= (t_past + torch.arange(S))[:, None]
    kp = torch.ones(B, n, dtype=torch.bool) if keep is None else keep[:, :n].bool()
    return ~(causal[None] & kp[:, None]).any(-1).reshape(-1)


EXT_GEOMS = R.DECODE_GEOMS
EXT_TPAST, EXT_S = (0, 1, 63, 64, 200), (1, 5, 66)
EXT_B, EXT_P = 4, 2


def extend_case(t_past, S, H, Hkv, dh):
    """qkv [4*S, (H + 2 Hkv) dh]; caches [4, t_past + 7, Hkv*dh] with NaN in every slot >= t_past; keep [4, t_past + S]: row 1 loses every
    key up to and including its first new one (query 0 of row 1 has no key), the other rows one old and one new slot where they have
    them; cache_row maps the 4 rows onto the first 2 cache rows"""
    B, Tmax = EXT_B, t_past + 7
    kc, vc = R.rnd(B, Tmax, Hkv * dh, seed=141), R.rnd(B, Tmax, Hkv * dh, seed=142)
    kc[:, t_past:] = float("nan")
    vc[:, t_past:] = float("nan")
    keep = torch.ones(B, t_past + S, dtype=torch.uint8)
    for b in range(B):
        if b == 1:
            keep[b, :t_past + 1] = 0
            continue
        if t_past > 1:
            keep[b, (7 * b + 3) % t_past] = 0
        if S > 1:
            keep[b, t_past + (b + 1) % S] = 0
    return dict(qkv=R.rnd(B * S, (H + 2 * Hkv) * dh, seed=143), kc=kc, vc=vc, keep=keep,
                cache_row=torch.tensor([0, 0, 1, 1], dtype=torch.int32))
