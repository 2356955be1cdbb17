"""GPU: the bf16 glue operators of procyon_amd/csrc/pcy_elem.hip through the C ABI (`pcy_layernorm`, `pcy_rmsnorm`, `pcy_rope`,
`pcy_pool`, `pcy_embed_splice`) against the references of tests/glue_ref.py, at the smallest shapes that reach each branch: the three
LayerNorm kernels on both sides of their thresholds with a partly filled last workgroup, 1 / 2 / 4 trips of the 2048-element loops,
rotary on column windows and with more chunks than threads, the pooler around its token stride and feature tile, the splice with and
without soft rows.  Bars: the project's own for single bf16 operators (`assert_bf16_close`, max_frac 0.005 for the norms, 0.05 for the
two means); bit equality for the rotary, the maximum, the gather and everything an operator must leave alone.
tests/test_glue_ref_cpu.py holds the references to torch's bf16 operators and the oracle on the same inputs at the same bars."""
import ctypes as C

import pytest
import torch

import glue_ref as G
from conftest import assert_bf16_close

pytestmark = pytest.mark.gpu
BF, I16, I32 = torch.bfloat16, torch.int16, torch.int32
SENTINEL = 0x5A5A                                      # guard rows: a finite bf16 pattern no operator here produces as a whole row


@pytest.fixture(scope="module")
def ctx():
    from procyon_amd.engine import Context
    return Context.get()


def _ptr(t, elem_off=0):
    return C.c_void_p(t.data_ptr() + 2 * elem_off)


def _call(ctx, name, *args):
    from procyon_amd import _lib as L
    L.check(getattr(ctx.lib, name)(ctx.h, *args), name)
    torch.cuda.synchronize()


def _guarded(rows, d):
    """[rows + 2, d] of the sentinel: the operator writes rows 1 .. rows, the first and the last row are guards"""
    return torch.full((rows + 2, d), SENTINEL, dtype=I16, device="cuda").view(BF)


def _guards_intact(buf):
    return bool((G.bits(buf[0]) == SENTINEL).all()) and bool((G.bits(buf[-1]) == SENTINEL).all())


def _refuses(call, entry):
    from procyon_amd._lib import PcyError
    with pytest.raises(PcyError, match=r"\(code 1\): " + entry + ":"):
        call()


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("rows,d", G.NORM_SHAPES)
def test_layernorm(ctx, rows, d):
    """rows 1 (the one-row-per-workgroup kernel), 63 | 64 (the threshold of the wave-per-row kernels), 65 and 67 (a last workgroup of 1
    and of 3 rows); d <= 1536 | <= 2560 | above (three, five 16-byte vectors per lane, or the workgroup kernel), d = 8 and 136 leave
    lanes without data; inputs around a mean of 3, an all-zero row (the output is the bias), a spike row, a constant row"""
    c = G.norm_case(rows, d, "ln")
    x, w, b, y = c["x"].cuda(), c["w"].cuda(), c["b"].cuda(), _guarded(rows, d)
    _call(ctx, "pcy_layernorm", _ptr(x), _ptr(w), _ptr(b), _ptr(y, d), rows, d, G.EPS)
    out = y[1:-1].cpu()
    assert _guards_intact(y)
    assert_bf16_close(out, G.layernorm(c["x"], c["w"], c["b"]), f"ln {rows}x{d}", max_frac=G.NORM_MAX_FRAC)
    if rows >= 4:
        assert torch.equal(G.bits(out[G.ROW_ZERO]), G.bits(c["b"]))


@pytest.mark.parametrize("cast", [0, 1])
@pytest.mark.parametrize("rows,d", G.NORM_SHAPES)
def test_rmsnorm(ctx, rows, d, cast):
    """the same shapes: d = 8 .. 2048 is one trip of the 2048-element loop, 2560 / 2568 two (the second partly filled), 8192 four;
    both rounding orders; an all-zero row gives zeros"""
    c = G.norm_case(rows, d, "rms")
    x, w, y = c["x"].cuda(), c["w"].cuda(), _guarded(rows, d)
    _call(ctx, "pcy_rmsnorm", _ptr(x), _ptr(w), _ptr(y, d), rows, d, G.EPS, cast)
    out = y[1:-1].cpu()
    assert _guards_intact(y)
    assert_bf16_close(out, G.rmsnorm(c["x"], c["w"], G.EPS, cast), f"rms cast {cast} {rows}x{d}", max_frac=G.NORM_MAX_FRAC)
    if rows >= 4:
        assert bool((out[G.ROW_ZERO] == 0).all())


@pytest.mark.parametrize("cast", [0, 1])
@pytest.mark.parametrize("rows,d", G.NORM_INPLACE)
def test_rmsnorm_in_place(ctx, rows, d, cast):
    """y == x, as the row-summing callers of the engine run it: the bits of the out-of-place call"""
    c = G.norm_case(rows, d, "rms")
    x, w = c["x"].cuda(), c["w"].cuda()
    out = ctx.rmsnorm(x, w, G.EPS, cast)
    assert_bf16_close(out.cpu(), G.rmsnorm(c["x"], c["w"], G.EPS, cast), f"rms cast {cast} {rows}x{d}", max_frac=G.NORM_MAX_FRAC)
    y = _guarded(rows, d)
    y[1:-1] = x
    _call(ctx, "pcy_rmsnorm", _ptr(y, d), _ptr(w), _ptr(y, d), rows, d, G.EPS, cast)
    assert _guards_intact(y) and torch.equal(G.bits(y[1:-1]), G.bits(out))


# ------------------------------------------------------------------------------------------------ rotary
def _rope(ctx, buf_ptr, ld, col0, nh, dh, pos, cos, sin, ntok, mode, prescale):
    _call(ctx, "pcy_rope", buf_ptr, ld, col0, nh, dh, _ptr(pos), _ptr(cos), _ptr(sin), ntok, mode, prescale)


@pytest.mark.parametrize("nh,dh,ld,col0", G.ROPE_GEOMS)
@pytest.mark.parametrize("mode,scaled", G.ROPE_VARIANTS)
def test_rope(ctx, nh, dh, ld, col0, mode, scaled):
    """head_dim 16 / 32 / 64 / 128; the ESM key window of a [ntok, 3d] buffer; 36 x 128 and the Llama-3 q + k heads of the fused qkv row:
    288 and 320 chunks per token, the second trip of the 256-thread loop; positions 0, the table's last row, a repeated one.  Every
    product of two bf16 values is exact in fp32: bit-equal to the reference, and the columns outside the window keep their bits"""
    c = G.rope_case(nh, dh, ld, col0)
    cos, sin = G.rope_tables(dh)
    prescale = dh ** -0.5 if scaled else 0.0
    T = len(G.ROPE_POS)
    buf, pos_d, cos_d, sin_d = _guarded(T, ld), c["pos"].cuda(), cos.cuda(), sin.cuda()
    buf[1:-1] = c["buf"].cuda()
    _rope(ctx, _ptr(buf, ld), ld, col0, nh, dh, pos_d, cos_d, sin_d, T, mode, prescale)
    ref = G.rope(c["buf"], col0, nh, dh, c["pos"], cos, sin, mode, prescale)
    out = buf[1:-1].cpu()
    w = slice(col0, col0 + nh * dh)
    assert _guards_intact(buf)
    assert torch.equal(G.bits(out[:, w]), G.bits(ref[:, w]))
    assert torch.equal(G.bits(out[:, :col0]), G.bits(c["buf"][:, :col0])) and torch.equal(G.bits(out[:, w.stop:]), G.bits(c["buf"][:, w.stop:]))


# (nh, dh, ld, col0) the entry must refuse before any launch; every window lies inside the buffer the test passes, whatever the entry does
ROPE_REFUSED = {"dh2": (2, 2, 8, 0), "dh8": (2, 8, 16, 0), "dh24": (2, 24, 48, 0), "dh40": (2, 40, 80, 0), "ld": (2, 16, 36, 0),
                "col0": (2, 16, 48, 4), "window": (3, 16, 40, 0)}


@pytest.mark.parametrize("name", list(ROPE_REFUSED))
def test_rope_refuses_what_the_kernel_cannot_rotate(ctx, name):
    """the kernel moves 8-element chunks of each half head with 16-byte accesses: head_dim 8 would rotate nothing, 24 and 40 would leave
    the tail of each half, a row stride or first column off the 8-element grid would misalign every access, and heads beyond ld would
    reach into the next row.  Code 1 naming the entry, the buffer as it was, and a valid call on the same context behind it"""
    nh, dh, ld, col0 = ROPE_REFUSED[name]
    T = len(G.ROPE_POS)
    cos, sin = G.rope_tables(dh)
    host = G.rnd(T + 2, ld + 16, seed=77).to(BF)                       # (more than T x ld elements)
    buf, pos, cos_d, sin_d = host.cuda(), torch.tensor(G.ROPE_POS, dtype=I32).cuda(), cos.cuda(), sin.cuda()
    for mode in (0, 1):
        _refuses(lambda: _rope(ctx, _ptr(buf), ld, col0, nh, dh, pos, cos_d, sin_d, T, mode, 0.0), "pcy_rope")
    torch.cuda.synchronize()
    assert torch.equal(G.bits(buf.cpu()), G.bits(host))
    nh, dh, ld, col0 = G.ROPE_GEOMS[0]
    c = G.rope_case(nh, dh, ld, col0)
    cos, sin = G.rope_tables(dh)
    out = ctx.rope_(c["buf"].cuda(), col0, nh, dh, c["pos"].cuda(), cos.cuda(), sin.cuda(), 0, 0.0).cpu()
    assert torch.equal(G.bits(out), G.bits(G.rope(c["buf"], col0, nh, dh, c["pos"], cos, sin, 0)))


# ------------------------------------------------------------------------------------------------ pooler
@pytest.fixture(scope="module")
def pool_refs():
    """(d, nan) -> the case and its three references, computed once"""
    cache = {}

    def get(d, nan):
        if (d, nan) not in cache:
            c = G.pool_case(d, nan)
            cache[(d, nan)] = (c, {m: G.pool(c["h"], c["seg"], c["rng"], m) for m in ((0, 1) if nan else (0, 1, 2))})
        return cache[(d, nan)]
    return get


@pytest.mark.parametrize("d", G.POOL_DIMS)
@pytest.mark.parametrize("mode,nan", [(0, False), (0, True), (1, False), (1, True), (2, False)])
def test_pool(ctx, pool_refs, d, mode, nan):
    """ten proteins of 1 .. 130 tokens in one call: below, at and above the 32-token stride of stage 1, two and four full strides; 1 to 3
    ranges each, ranges of length 1 first and last (mode 1 empties them), starts in no order, 1e30 in every row outside the ranges;
    d = 8 and 136 leave feature lanes idle, 520 and 1280 take a second and third 512-feature tile.  NaN: skipped by the two means and
    counted out; a feature that is NaN in every row of a protein is NaN there and nowhere else"""
    c, refs = pool_refs(d, nan)
    ref = refs[mode]
    nprot = len(c["seg"]) - 1
    out = ctx.pool(c["h"].cuda(), torch.tensor(c["seg"], dtype=I32).cuda(), torch.tensor(c["rng"], dtype=I32).reshape(-1).cuda(), nprot, mode)
    torch.cuda.synchronize()
    out = out.cpu()
    if mode == 2:
        assert torch.equal(G.bits(out), G.bits(ref))
        return
    want_nan = ref.isnan()
    assert torch.equal(out.isnan(), want_nan)
    assert bool(want_nan[:2].all()) == (mode == 1) and int(want_nan[2:].sum()) == int(nan)     # 1 and 2 tokens: mode 1 leaves no row
    assert_bf16_close(out[~want_nan], ref[~want_nan], f"pool {d} mode {mode} nan {nan}", max_frac=G.POOL_MAX_FRAC)
    if mode == 1:
        st = c["rng"][c["seg"][2] + 1][0]             # three tokens in ranges of 1 and 2: the middle one is the second range's first
        assert torch.equal(G.bits(out[2]), G.bits(c["h"][st]))


# ------------------------------------------------------------------------------------------------ splice
@pytest.mark.parametrize("d", G.SPLICE_DIMS)
@pytest.mark.parametrize("which", G.SPLICE_MAPS)
def test_embed_splice(ctx, d, which):
    """d = 8 (one lane), 2048 (exactly one trip of the copy loop), 2056 and 4096 (a second trip, partly and wholly filled); no soft_map,
    none soft, soft rows out of order and repeated, all soft; table rows 0 and 49: bit-equal"""
    c = G.splice_case(d, which)
    sm = c["soft_map"]
    out = ctx.embed_splice(c["table"].cuda(), c["ids"].cuda(), None if sm is None else c["soft"].cuda(), None if sm is None else sm.cuda())
    torch.cuda.synchronize()
    assert torch.equal(G.bits(out.cpu()), G.bits(G.splice(c["table"], c["ids"], c["soft"], sm)))


# ------------------------------------------------------------------------------------------------ refusals that were there before
def test_d_off_the_vector_grid_is_refused(ctx):
    """d = 100 (no multiple of 8) on the norms, the pooler and the splice: code 1 naming the entry, and the context goes on working"""
    x, w = torch.zeros(3, 100, dtype=BF, device="cuda"), torch.ones(100, dtype=BF, device="cuda")
    ids, rng = torch.zeros(3, dtype=I32, device="cuda"), torch.tensor([0, 3], dtype=I32, device="cuda")
    seg, y = torch.tensor([0, 1], dtype=I32, device="cuda"), torch.zeros(3, 100, dtype=BF, device="cuda")
    for cast in (0, 1):
        _refuses(lambda: _call(ctx, "pcy_rmsnorm", _ptr(x), _ptr(w), _ptr(y), 3, 100, G.EPS, cast), "pcy_rmsnorm")
    _refuses(lambda: _call(ctx, "pcy_layernorm", _ptr(x), _ptr(w), _ptr(w), _ptr(y), 3, 100, G.EPS), "pcy_layernorm")
    _refuses(lambda: _call(ctx, "pcy_embed_splice", _ptr(x), _ptr(ids), C.c_void_p(0), C.c_void_p(0), _ptr(y), 3, 100), "pcy_embed_splice")
    for mode in (0, 1, 2):
        _refuses(lambda: _call(ctx, "pcy_pool", _ptr(x), 100, _ptr(seg), _ptr(rng), 1, mode, _ptr(y)), "pcy_pool")
    c = G.norm_case(3, 136, "rms")
    assert_bf16_close(ctx.rmsnorm(c["x"].cuda(), c["w"].cuda(), G.EPS, 0).cpu(), G.rmsnorm(c["x"], c["w"], G.EPS, 0), "rms after refusals",
                      max_frac=G.NORM_MAX_FRAC)
