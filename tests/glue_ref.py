"""Plain torch restatements of the bf16 glue operators (`pcy_layernorm`, `pcy_rmsnorm`, `pcy_rope`, `pcy_pool`, `pcy_embed_splice`;
include/pcy.h, procyon_amd/csrc/pcy_elem.hip) with the operators' rounding points, written from the header and the oracle, never from
the kernels: float64 arithmetic (the functions of tests/f32_ref.py) between the roundings, except the rotary, whose fp32 evaluation is
exact.  The input sets of tests/test_gpu_glue_ops.py live here too (`*_case`), so that tests/test_glue_ref_cpu.py sees the same numbers."""
import torch

import f32_ref as R

BF, F32, F64, I16, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int16, torch.int32
NORM_MAX_FRAC, POOL_MAX_FRAC = 0.005, 0.05          # assert_bf16_close(max_frac=...) of test_norms / test_pool_matches_reference_pooler
EPS = 1e-5


def bits(t):
    """the bit patterns of a bf16 tensor"""
    return t.contiguous().view(I16)


def rnd(*shape, seed, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std


# ------------------------------------------------------------------------------------------------ norms
def layernorm(x, w, b, eps=EPS):
    """float64 statistics, one rounding"""
    return R.layernorm(x, w, b, eps).to(BF)


def rmsnorm(x, w, eps=EPS, cast=0):
    """cast 0 (transformers 5.x): bf16(w * bf16(x rstd)); cast 1 (4.31): bf16(w * (x rstd))"""
    h = R.rmsnorm(x, torch.ones_like(w), eps)
    if cast == 0:
        h = h.to(BF)
    return (w.to(F64) * h.to(F64)).to(BF)


def tie_distance(y):
    """float64 y -> the distance of |y| to the nearest bf16 rounding boundary (the midpoint of two neighbouring bf16 values), relative to
    |y|; inf where y == 0"""
    m, _ = torch.frexp(y.abs())                       # |y| = m 2^e, m in [0.5, 1): the bf16 grid has 256 steps per unit of m
    t = m * 256.0
    return torch.where(y == 0, torch.full_like(t, float("inf")), ((t - t.floor()) - 0.5).abs() / t.clamp_min(1.0))


RMS_TIE_MARGIN = 2.0 ** -20


def settle_rms_ties(x, eps=EPS):
    """RMSNorm with cast 0 rounds x rstd before it multiplies by w.  Where x rstd lies closer to a bf16 rounding boundary than an fp32
    evaluation can resolve, a correct kernel and the float64 reference may round to different neighbours, and w times a one-ulp step is up
    to two ulps of the output: the one-ulp bar would then be a matter of luck (about 2e-5 of all elements, over the 3.3 M elements of
    the shapes below).  An fp32 evaluation of rstd carries at most ~4e-7 of relative error (the sum of squares, one division, one
    addition, a reciprocal square root of one ulp, one product), so every element within 2^-20 of a boundary is moved to the next bf16
    value, and again until none is left (a move changes rstd by ~2^-8 / d).  Returns the number of moves."""
    moved = 0
    for _ in range(64):
        y = R.rmsnorm(x, torch.ones(x.shape[-1]), eps)
        near = tie_distance(y) < RMS_TIE_MARGIN
        if not bool(near.any()):
            return moved
        moved += int(near.sum())
        bits(x)[near] += 1                            # the next bf16 value away from zero: finite inputs far below the top of the range
    raise AssertionError("settle_rms_ties did not converge")


NORM_ROWS, NORM_DIMS = (1, 63, 64, 65, 67), (8, 136, 1280, 1536, 1544, 2560, 2568)
NORM_SHAPES = tuple((r, d) for r in NORM_ROWS for d in NORM_DIMS) + tuple((r, d) for r in (1, 65) for d in (4096, 8192))
NORM_INPLACE = ((65, 4096), (3, 136))
ROW_ZERO, ROW_SPIKE, ROW_CONST = 1, 2, 3              # where the special rows stand (shapes of at least 4 rows)


def norm_case(rows, d, kind):
    """kind "ln" | "rms" -> x [rows, d], w, b (bf16).  Row r is N(0, 1) times 2^((r + 4) % 9 - 4) (1/16 .. 16; row 0 has scale 1),
    plus 3 for LayerNorm; with four rows or more: row 1 all zero, row 2 a single 64.0 among values of std 0.01 (plus 3 for LayerNorm),
    row 3 the constant 1.5 where d is a power of two (every fp32 sum of it is exact)"""
    seed = 1000 * rows + d + (500000 if kind == "ln" else 0)
    scale = torch.tensor([2.0 ** ((r + 4) % 9 - 4) for r in range(rows)])[:, None]
    off = 3.0 if kind == "ln" else 0.0
    x = rnd(rows, d, seed=seed) * scale + off
    if rows >= 4:
        x[ROW_ZERO] = 0.0
        x[ROW_SPIKE] = rnd(d, seed=seed + 1, std=0.01) + off
        x[ROW_SPIKE, d // 3] = 64.0
        if d & (d - 1) == 0:
            x[ROW_CONST] = 1.5
    x = x.to(BF)
    if kind == "rms":
        settle_rms_ties(x)
    return dict(x=x, w=(1 + rnd(d, seed=seed + 2, std=0.02)).to(BF), b=rnd(d, seed=seed + 3, std=0.02).to(BF))


# ------------------------------------------------------------------------------------------------ rotary
ROPE_GEOMS = ((2, 16, 32, 0), (3, 32, 96, 0), (6, 64, 1152, 384), (36, 128, 4608, 0), (40, 128, 6144, 0))    # (nh, dh, ld, col0)
ROPE_NPOS, ROPE_POS = 64, (0, 63, 5, 5, 62, 1, 17)
ROPE_VARIANTS = ((0, False), (1, False), (1, True))   # (mode, prescale by dh^-0.5)


def rope_tables(dh, n_pos=ROPE_NPOS):
    """bf16 cos / sin [n_pos, dh]: the fp32 tables of the oracle, rounded once"""
    cos, sin = R.rope_tables(dh, n_pos)
    return cos.to(BF), sin.to(BF)


def rope(buf, col0, nh, dh, pos, cos, sin, mode, prescale=0.0):
    """the whole bf16 buffer [ntok, ld] with heads [col0, col0 + nh*dh) of every row rotated.  mode 0: every product and the sum rounded
    to bf16; mode 1: fp32 products and sum, one rounding; prescale != 0: x' = bf16(fp32(x) * prescale) first.  All in float32: a product
    of two bf16 values is exact in fp32, so every sum is one IEEE rounding of an exact quantity, with or without FMA contraction."""
    out = buf.clone()
    T = buf.shape[0]
    x = buf[:, col0:col0 + nh * dh].reshape(T, nh, dh).to(F32)
    if prescale != 0.0:
        x = (x * torch.tensor(prescale, dtype=F32)).to(BF).to(F32)
    c, s = cos.to(F32)[pos.long()][:, None], sin.to(F32)[pos.long()][:, None]
    rot = torch.cat((-x[..., dh // 2:], x[..., :dh // 2]), -1)
    if mode == 0:
        y = ((x * c).to(BF).to(F32) + (rot * s).to(BF).to(F32)).to(BF)
    else:
        y = (x * c + rot * s).to(BF)
    out[:, col0:col0 + nh * dh] = y.reshape(T, nh * dh)
    return out


def rope_case(nh, dh, ld, col0):
    return dict(buf=rnd(len(ROPE_POS), ld, seed=7000 + ld + dh).to(BF), pos=torch.tensor(ROPE_POS, dtype=I32))


# ------------------------------------------------------------------------------------------------ pooler
POOL_DIMS = (8, 136, 520, 1280)
# the ranges of each protein, by length: 1, 2, 3, 4, 31, 32, 33, 34, 65 and 130 tokens over 1 to 3 ranges, first and last ranges of length 1
POOL_SPLIT = ((1,), (1, 1), (1, 2), (3, 1), (31,), (1, 30, 1), (16, 17), (34,), (1, 32, 32), (64, 65, 1))
POOL_TOKENS = tuple(sum(p) for p in POOL_SPLIT)
POOL_GAP = 1e30                                       # what every row outside the ranges holds
POOL_NAN_PROTEIN = 6                                  # NaN variant: the last feature of every row of this protein


def pool_layout():
    """-> (seg, rng, nrows): seg [nprot + 1], rng [(start, length)] in protein order.  The ranges lie in the hidden buffer in another
    order (the odd-numbered ranges first, then the even ones), one unused row before each and after the last: starts are not monotonic"""
    lens = [ln for p in POOL_SPLIT for ln in p]
    order = list(range(1, len(lens), 2)) + list(range(0, len(lens), 2))
    start, at = {}, 1
    for i in order:
        start[i] = at
        at += lens[i] + 1
    seg = [0]
    for p in POOL_SPLIT:
        seg.append(seg[-1] + len(p))
    return tuple(seg), tuple((start[i], lens[i]) for i in range(len(lens))), at


def pool_case(d, nan):
    """h [nrows, d] bf16: multiples of 1/32 below 8 in size, so that every partial sum of up to 130 rows is exact in fp32 in any order
    and the first of nanmean's two roundings cannot fall to the other side in a correct kernel (the quotient by a count that is no power
    of two would turn that one ulp into up to two, beyond the bar).  nan: about 2 % NaN elements in the proteins of 31 tokens and more,
    and the last feature of every row of protein 6."""
    seg, rng, nrows = pool_layout()
    h = (rnd(nrows, d, seed=9000 + d) * 32).round().clamp(-255, 255) / 32 + 0.0      # (+ 0.0: no -0, which a sum does not hand back)
    used = torch.zeros(nrows, dtype=torch.bool)
    for st, ln in rng:
        assert not bool(used[st:st + ln].any())
        used[st:st + ln] = True
    if nan:
        g = torch.Generator().manual_seed(9100 + d)
        for p in range(len(POOL_SPLIT)):
            for st, ln in rng[seg[p]:seg[p + 1]]:
                if POOL_TOKENS[p] >= 31:
                    h[st:st + ln][torch.rand(ln, d, generator=g) < 0.02] = float("nan")
                if p == POOL_NAN_PROTEIN:
                    h[st:st + ln, d - 1] = float("nan")
    h[~used] = POOL_GAP
    return dict(h=h.to(BF), seg=seg, rng=rng)


def pool(h, seg, rng, mode):
    """mode 0 nanmean over a protein's rows, 1 over rows[1:-1], 2 max.  The means with torch.nanmean's two roundings on a bf16 tensor:
    bf16(nansum) / count in fp32, rounded again; no row left gives 0 / 0 = NaN"""
    outs = []
    for p in range(len(seg) - 1):
        rows = torch.cat([h[st:st + ln] for st, ln in rng[seg[p]:seg[p + 1]]])
        if mode == 1:
            rows = rows[1:-1]
        if mode == 2:
            outs.append(rows.max(0)[0])
        else:
            s = rows.to(F64).nansum(0).to(BF)
            outs.append((s.to(F32) / (~rows.isnan()).sum(0).to(F32)).to(BF))
    return torch.stack(outs)


# ------------------------------------------------------------------------------------------------ splice
SPLICE_DIMS, SPLICE_ROWS, SPLICE_VOCAB, SPLICE_SOFT = (8, 2048, 2056, 4096), 70, 50, 5
SPLICE_MAPS = ("null", "none_soft", "mixed", "all_soft")
N_FINITE = 2 * 0x7F80                                 # finite bf16 bit patterns


def _patterns(first, n):
    """n consecutive finite bf16 bit patterns (mod their number) from index `first`: 0x0000 .. 0x7F7F, then 0x8000 .. 0xFF7F"""
    v = (torch.arange(first, first + n, dtype=torch.int64)) % N_FINITE
    v = torch.where(v < 0x7F80, v, v - 0x7F80 + 0x8000)
    return torch.where(v >= 0x8000, v - 0x10000, v).to(I16).view(BF)


def splice_case(d, which):
    """table [50, d] and soft [5, d]: element (r, k) of the two stacked holds finite pattern number r d + k -- distinct along every row,
    and no two of the 55 rows agree in any column (127 does not divide a row difference below 55).  ids [70] with 0, 49 and repeats"""
    both = _patterns(0, (SPLICE_VOCAB + SPLICE_SOFT) * d).view(-1, d)
    ids = (torch.arange(SPLICE_ROWS) * 37) % SPLICE_VOCAB
    ids[0], ids[1], ids[2], ids[-1] = 0, SPLICE_VOCAB - 1, SPLICE_VOCAB - 1, 0
    r = torch.arange(SPLICE_ROWS)
    soft_map = {"null": None, "none_soft": torch.full((SPLICE_ROWS,), -1),
                "mixed": torch.where(r % 4 == 1, (r * 3) % SPLICE_SOFT, torch.full_like(r, -1)),      # 3, 0, 2, 4, 1, 3, ... at rows 1, 5, 9, ...
                "all_soft": (SPLICE_ROWS - 1 - r) % SPLICE_SOFT}[which]
    return dict(table=both[:SPLICE_VOCAB].contiguous(), soft=both[SPLICE_VOCAB:].contiguous(), ids=ids.to(I32),
                soft_map=None if soft_map is None else soft_map.to(I32))


splice = R.embed                                      # a gather: exact in any dtype
