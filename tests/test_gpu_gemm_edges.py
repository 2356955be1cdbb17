"""GPU: `pcy_gemm`, `pcy_gemv` and `pcy_gemm_fp8` through the C ABI at their edges, against tests/gemm_ref.py.

Inputs are exactly summable (gemm_ref.py says why), so the bar of every case is EQUALITY OF BITS with the float64 reference rounded at the
rounding points of include/pcy.h -- ragged tiles, the 8-element tail of K, vector-store tails and exact bf16 ties included -- and every case
asserts by dispatch / GEMV route counter that exactly the kernel it names ran.  Operands sit in larger buffers: outputs are pre-filled with
a sentinel pattern and everything outside rows [0, M) x columns [c0, c0 + N) must keep it; A / x / W carry NaN in their padding columns and
in two rows below the matrix, the residual NaN around its window.  Placements per kernel: contiguous; column windows of wider buffers; row
strides that are multiples of 4 or 2 but not of 8 and bases 8 (4, 6) bytes off a 16-byte boundary (the element-wise forms of the epilogues);
the residual in place; with and without bias.  Only placements that include/pcy.h promises are run; what it refuses is asserted to be refused
(code 1, output untouched, no counter moved) by `test_refusals`.  tests/test_gemm_ref_cpu.py checks references and inputs without a GPU."""
import contextlib
import ctypes as C
import os

import pytest
import torch

import gemm_ref as R
from conftest import record_parity

pytestmark = pytest.mark.gpu
BF, F32, I16 = R.BF, R.F32, R.I16
NAN = float("nan")
K_DISPATCH = dict(k128=0, k64=1, k64_nomid=1, big=2, persist=3, fp8=5, mid=8)
ROUTE = dict(stream2=0, stream4=1, chunked4=2, chunked1=2, mfma2=3, mfma3=4, mfma4=5, mfma4_passes=5)


@pytest.fixture(scope="module")
def ctx():
    from procyon_amd.engine import Context
    return Context.get()


def _counts(lib):
    return [int(lib.pcy_debug_dispatch_count(k)) for k in range(20)] + [int(lib.pcy_debug_gemv_route_count(k)) for k in range(6)]


def _delta(lib, before):
    """{counter index: increase}; GEMV routes at 20 + route"""
    return {i: a - b for i, (a, b) in enumerate(zip(_counts(lib), before)) if a != b}


@contextlib.contextmanager
def _env(**kw):
    """environment switches that the launchers read on every call"""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _vp(t, byte_off=0):
    return C.c_void_p(0 if t is None else t.data_ptr() + byte_off)


def _up8(n):
    return (n + 7) // 8 * 8


def _padded(t, ld, c0, extra_rows=2):
    """bf16 [rows, cols] -> device [rows + extra, ld] with NaN everywhere but the window at column c0; returns (buffer, window view)"""
    rows, cols = t.shape
    buf = torch.full((rows + extra_rows, ld), NAN, dtype=BF, device="cuda")
    buf[:rows, c0:c0 + cols] = t.cuda()
    return buf, buf[:rows, c0:c0 + cols]


def _sentinel(rows, ld):
    return torch.full((rows + 2, ld), R.SENTINEL, dtype=I16, device="cuda").view(BF)


def _check_window(buf, rows, c0, cols, ref_dev, tag):
    """the window holds the reference's bits, everything else its sentinel"""
    win = buf[:rows, c0:c0 + cols]
    bad = int((win.contiguous().view(I16) != ref_dev.view(I16)).sum())
    rest = buf.clone().view(I16)
    rest[:rows, c0:c0 + cols] = R.SENTINEL
    spilled = int((rest != R.SENTINEL).sum())
    if bad or spilled:
        print(f"{tag}: {bad} of {rows * cols} elements differ, {spilled} outside the window changed")
    assert spilled == 0, (tag, "wrote outside the window", spilled)
    assert bad == 0, (tag, "bits differ", bad)


# ------------------------------------------------------------------------------------------------ GEMM placements
def _gemm_variants(epi, N, Nout):
    """name -> (lda pad, a0, ldc, c0, ldr, r0, alias, bias shift in elements)"""
    w = _up8(Nout)
    v = {"contig": (0, 0, Nout, 0, N, 0, False, 0),
         "window": (16, 8, w + 24, 8, _up8(N) + 32, 16, False, 0),
         "narrow4": (0, 0, Nout + 4, 0, N + 12, 0, False, 0),
         "shifted": (0, 0, w + 8, 4, _up8(N) + 8, 4, False, 4)}
    if epi != R.EPI_SWIGLU:                       # (SwiGLU: ldc % 4 == 0 is part of the contract)
        v["narrow2"] = (0, 0, Nout + 2, 0, N + 2, 0, False, 0)
        v["odd"] = (0, 0, Nout + 3, 1, N + 5, 3, False, 1)
    if epi == R.EPI_RESID:
        v["alias"] = (0, 0, w + 8, 0, w + 8, 0, True, 0)
        v["alias_shifted"] = (0, 0, Nout + 4, 4, Nout + 4, 4, True, 0)
    return v


def _run_gemm(ctx, key, kind, variants=None, tag=""):
    lib = ctx.lib
    M, N, K, epi, bias = key
    c = R.gemm_case(*key)
    Nout = c["Nout"]
    ref_dev = R.reference("gemm", *key).cuda()
    W, _ = _padded(c["W"], K, 0)
    A_bufs, calls = {}, 0
    for name, (apad, a0, ldc, c0, ldr, r0, alias, bshift) in _gemm_variants(epi, N, Nout).items():
        if variants is not None and name not in variants:
            continue
        if (apad, a0) not in A_bufs:
            A_bufs[(apad, a0)] = _padded(c["A"], K + apad, a0)
        Abuf, _ = A_bufs[(apad, a0)]
        Cbuf = _sentinel(M, ldc)
        rbuf = None
        if epi == R.EPI_RESID and alias:
            Cbuf[:M, c0:c0 + N] = c["resid"].cuda()
            rbuf, rptr, ldr = Cbuf, _vp(Cbuf, 2 * c0), ldc
        elif epi == R.EPI_RESID:
            rbuf, _ = _padded(c["resid"], ldr, r0)
            rptr = _vp(rbuf, 2 * r0)
        else:
            rptr, ldr = _vp(None), 0
        bbuf = None
        if c["bias"] is not None:
            bbuf = torch.full((N + 16,), NAN, dtype=BF, device="cuda")
            bbuf[bshift:bshift + N] = c["bias"].cuda()
        n0 = _counts(lib)
        rc = lib.pcy_gemm(ctx.h, _vp(Abuf, 2 * a0), K + apad, _vp(W), _vp(bbuf, 2 * bshift), rptr, ldr, _vp(Cbuf, 2 * c0), ldc, M, N, K, epi)
        torch.cuda.synchronize()
        assert rc == 0, (key, name, lib.pcy_last_error())
        assert _delta(lib, n0) == {K_DISPATCH[kind]: 1}, (key, name, kind, _delta(lib, n0))
        _check_window(Cbuf, M, c0, Nout, ref_dev, f"gemm{tag} {kind} {key} {name}")
        calls += 1
    return calls


def _record(key, calls):
    """one line of the parity report per test: how many calls it compared, every one bit for bit"""
    assert calls > 0, key
    print(f"gemm_edges/{key}: {calls} calls, bits equal")
    record_parity(f"gemm_edges/{key}", calls=calls, bits_equal=1)


def _gemm_params(*groups):
    out = []
    for g in groups:
        for M, N, Ks, epis in R.GEMM_SHAPES[g]:
            for epi in epis:
                out.append(pytest.param(g, M, N, Ks, epi, id=f"{g}-{M}x{N}-e{epi}"))
    return out


def _keys(M, N, Ks, epi):
    for K in Ks:
        for bias in ((True, False) if epi in (R.EPI_STORE, R.EPI_RESID) else (epi != R.EPI_SWIGLU,)):
            yield (M, N, K, epi, bias)


@pytest.mark.parametrize("group,M,N,Ks,epi", _gemm_params("k64", "mid"))
def test_gemm_small_and_mid_tiles(ctx, group, M, N, Ks, epi):
    """64 x 64 tiles (M < 128: 70 x 130 is 2 x 3 ragged tiles, 1 x 132 one row) and the launcher's own mid-tile choice (130 x 1290 / 1312:
    two row tiles, the second with 2 rows; 513 x 6144: the 128 x 96 shape); K = 64 is one k-step, 192 three"""
    with _env(PCY_GEMM_MID=None, PCY_GEMM_PERM=None):
        n = sum(_run_gemm(ctx, key, group) for key in _keys(M, N, Ks, epi))
    _record(f"{group}/{M}x{N}-e{epi}", n)


@pytest.mark.parametrize("group,M,N,Ks,epi", _gemm_params("k64_nomid", "k128"))
def test_gemm_without_mid_tiles(ctx, group, M, N, Ks, epi):
    """PCY_GEMM_MID=-1 (the launcher's choice before the mid tiles): 130 x 260 is six 128 x 128 tiles, which the launcher still cuts into
    64 x 64 ones for every epilogue that has that form; the 128 x 128 kernel itself runs SwiGLU at 70 x 288 (no 64 x 64 form) and the
    other epilogues at 130 x 24580 (2 x 193 tiles, the last 4 columns wide)"""
    with _env(PCY_GEMM_MID=-1, PCY_GEMM_PERM=None):
        n = sum(_run_gemm(ctx, key, group, variants=None if M * N < 1 << 20 else ("contig", "window", "narrow2", "alias"))
                for key in _keys(M, N, Ks, epi))
    _record(f"{group}/{M}x{N}-e{epi}", n)


@pytest.mark.parametrize("perm", [None, 0])
@pytest.mark.parametrize("group,M,N,Ks,epi", _gemm_params("big"))
def test_gemm_256_tiles(ctx, group, M, N, Ks, epi, perm):
    """M >= 2048, N >= 1280: the 256 x 256 kernels (the persistent ESM-GELU one for epilogue 3), 9 x 6 tiles with 2 rows in the last row
    tile and 8 / 10 / 32 columns in the last column tile.  N = 1288 can take the 16-byte epilogue, 1290 never; PCY_GEMM_PERM default
    (permuted W rows, 16-byte pieces) and 0 (natural order, 8-byte pieces).  K = 4160: the pipelined loop over an odd number (65) of k-steps"""
    with _env(PCY_GEMM_MID=None, PCY_GEMM_PERM=perm):
        n = sum(_run_gemm(ctx, key, "persist" if epi == R.EPI_GELU_ESM else "big", tag=f"[perm={perm}]",
                          variants=("contig", "shifted") if key[2] >= 4096 else None) for key in _keys(M, N, Ks, epi))
    _record(f"{'persist' if epi == R.EPI_GELU_ESM else 'big'}[perm={perm}]/{M}x{N}-e{epi}", n)


def test_gemm_gelu_erf_placements(ctx):
    """epilogue 2 has no bit-exact CPU twin: a window, the narrow strides and the shifted bases must give the bits of the contiguous call
    on random data (it has the 64 x 64 and the 128 x 128 kernel only; 2050 x 1288 is 17 x 11 = 187 tiles: still 64 x 64)"""
    lib = ctx.lib
    for kind, M, N, K in (("k64", 70, 130, 192), ("k128", 130, 24580, 64), ("k64", 2050, 1288, 64)):
        g = torch.Generator().manual_seed(M + N)
        A = torch.randn(M, K, generator=g).to(BF)
        W = (torch.randn(N, K, generator=g) * 0.1).to(BF)
        b = torch.randn(N, generator=g).to(BF)
        Wd, _ = _padded(W, K, 0)
        first = None
        for name, (apad, a0, ldc, c0, _, _, _, bshift) in _gemm_variants(R.EPI_GELU_ERF, N, N).items():
            Abuf, _ = _padded(A, K + apad, a0)
            Cbuf = _sentinel(M, ldc)
            bbuf = torch.full((N + 16,), NAN, dtype=BF, device="cuda")
            bbuf[bshift:bshift + N] = b.cuda()
            n0 = _counts(lib)
            rc = lib.pcy_gemm(ctx.h, _vp(Abuf, 2 * a0), K + apad, _vp(Wd), _vp(bbuf, 2 * bshift), _vp(None), 0, _vp(Cbuf, 2 * c0), ldc, M, N, K, 2)
            torch.cuda.synchronize()
            assert rc == 0 and _delta(lib, n0) == {K_DISPATCH[kind]: 1}, (kind, name, _delta(lib, n0))
            out = Cbuf[:M, c0:c0 + N].contiguous()
            assert bool(out.float().isfinite().all()), name
            first = out if first is None else first
            _check_window(Cbuf, M, c0, N, first, f"gelu_erf {M}x{N}x{K} {name}")


# ------------------------------------------------------------------------------------------------ fp8 GEMM
@pytest.mark.parametrize("perm", [7, 23])
@pytest.mark.parametrize("M,N,Ks,epis", [pytest.param(*s, id=f"{s[0]}x{s[1]}") for s in R.FP8_SHAPES])
def test_gemm_fp8(ctx, M, N, Ks, epis, perm):
    """exact codes through the 256 x 256 fp8 kernel: 5 rows, 257 rows (a second row tile of one row), ragged N = 264 / 1290, SwiGLU at
    288 / 1312 packed rows; natural (PCY_GEMM_PERM 7: the default) and permuted (23) W rows; sw 16-byte aligned and 4 bytes past; C and
    resid contiguous, as windows and in place (300 x 512).  K = 128 is one k-step, 384 three"""
    lib, calls = ctx.lib, 0
    for key in [(M, N, K, epi) for K in Ks for epi in epis]:
        c = R.fp8_case(*key)
        K, epi, Nout = key[2], key[3], c["Nout"]
        a8, sa = ctx.quant_rows_fp8(c["A"].cuda())
        w8, sw = ctx.quant_rows_fp8(c["W"].cuda())
        assert torch.equal(sa.cpu(), c["sa"]) and torch.equal(sw.cpu(), c["sw"]), key                  # the quantiser is exact on these rows
        assert torch.equal(a8.cpu().view(torch.float8_e4m3fn).float(), c["a_val"]) and torch.equal(w8.cpu().view(torch.float8_e4m3fn).float(), c["w_val"])
        ref_dev = R.fp8_reference(*key).cuda()
        sw_off = torch.full((N + 5,), NAN, dtype=F32, device="cuda")
        sw_off[1:N + 1] = sw
        in_place = (M, N) == (300, 512)
        w = _up8(Nout)
        for name, (ldc, c0, ldr, r0, sw_shift) in {"contig": (Nout, 0, N, 0, 0), "window": (w + 24, 8, _up8(N) + 32, 16, 1),
                                                   "narrow4": (Nout + 4, 0, N + 12, 0, 0), "shifted": (w + 8, 4, _up8(N) + 8, 4, 1)}.items():
            Cbuf = _sentinel(M, ldc)
            if epi == R.EPI_RESID and in_place:
                Cbuf[:M, c0:c0 + N] = c["resid"].cuda()
                rptr, ldr = _vp(Cbuf, 2 * c0), ldc
            elif epi == R.EPI_RESID:
                rbuf, _ = _padded(c["resid"], ldr, r0)
                rptr = _vp(rbuf, 2 * r0)
            else:
                rptr, ldr = _vp(None), 0
            n0 = _counts(lib)
            with _env(PCY_GEMM_PERM=perm):
                rc = lib.pcy_gemm_fp8(ctx.h, _vp(a8), _vp(sa), _vp(w8), _vp(sw_off, 4) if sw_shift else _vp(sw), rptr, ldr, _vp(Cbuf, 2 * c0), ldc,
                                      M, N, K, epi)
            torch.cuda.synchronize()
            assert rc == 0, (key, name, lib.pcy_last_error())
            assert _delta(lib, n0) == {K_DISPATCH["fp8"]: 1}, (key, name, _delta(lib, n0))
            _check_window(Cbuf, M, c0, Nout, ref_dev, f"gemm_fp8[perm={perm}] {key} {name}")
            calls += 1
    _record(f"fp8[perm={perm}]/{M}x{N}", calls)


# ------------------------------------------------------------------------------------------------ GEMV
def _gemv_variants(epi, N):
    """name -> (ldx pad, ldy, c0, resid in place)"""
    if epi == R.EPI_SWIGLU:                       # (y 8-byte aligned and ldy % 4 == 0 are part of the contract)
        return {"contig": (0, N, 0, False), "window": (8, N + 8, 4, False)}
    v = {"contig": (0, N, 0, False), "window": (8, N + 6, 3, False), "half": (0, N + 4, 2, False)}
    if epi == R.EPI_RESID:
        v["alias"] = (0, N, 0, True)
        v["alias_window"] = (8, N + 6, 3, True)
    return v


def _call_gemv(ctx, xbuf, ldx, W, bias, rptr, ybuf, c0, ldy, N, K, B, epi, rms_w=None, cast=0):
    rc = ctx.lib.pcy_gemv(ctx.h, _vp(W), _vp(xbuf), ldx, _vp(bias), rptr, _vp(ybuf, 2 * c0), ldy, _vp(rms_w), 1e-5, cast, N, K, B, epi)
    torch.cuda.synchronize()
    assert rc == 0, ctx.lib.pcy_last_error()


def _run_gemv(ctx, key, route):
    lib = ctx.lib
    B, N, K, epi, bias = key
    c = R.gemv_case(*key)
    ref_dev = R.reference("gemv", *key).cuda()
    W, _ = _padded(c["W"], K, 0)
    bbuf = None
    if c["bias"] is not None:
        bbuf = torch.full((N + 8,), NAN, dtype=BF, device="cuda")
        bbuf[:N] = c["bias"].cuda()
    passes, calls = -(-B // (32 if route.startswith("mfma") else 4)), 0
    for name, (xpad, ldy, c0, alias) in _gemv_variants(epi, N).items():
        xbuf, _ = _padded(c["A"], K + xpad, 0)
        ybuf = _sentinel(B, ldy)
        if epi == R.EPI_RESID and alias:
            ybuf[:B, c0:c0 + N] = c["resid"].cuda()
            rptr = _vp(ybuf, 2 * c0)
        elif epi == R.EPI_RESID:                  # its own buffer at the stride of y, NaN around the window
            rbuf, _ = _padded(c["resid"], ldy, 0)
            rptr = _vp(rbuf)
        else:
            rptr = _vp(None)
        n0 = _counts(lib)
        _call_gemv(ctx, xbuf, K + xpad, W, bbuf, rptr, ybuf, c0, ldy, N, K, B, epi)
        assert _delta(lib, n0) == {20 + ROUTE[route]: passes}, (route, key, name, _delta(lib, n0))
        _check_window(ybuf, B, c0, N, ref_dev, f"gemv {route} {key} {name}")
        calls += 1
    return calls


GEMV_DISABLE = dict(mfma3="gemv_mfma4", mfma2="gemv_lds")


@pytest.mark.parametrize("epi", [0, 1, 3, 4])
@pytest.mark.parametrize("route", sorted(R.GEMV_SHAPES))
def test_gemv(ctx, route, epi):
    """every kernel pcy_launch_gemv can choose without a workspace (R.GEMV_SHAPES): the streaming kernel with 2-row units (1 .. 4 rows of x;
    N = 1, 5: lanes and waves without a row; K = 8: one lane with data, 136 / 520: a partly filled 512-element step) and with 4-row units
    (N = 8190: the last unit has 2 rows); the chunked kernel with a last chunk of 8 elements; the MFMA kernels with one 16-row batch tile and
    two (B = 17: one row in the second), a partly filled 16-row weight tile (N = 70), several workgroups (N = 1040), K in units of 128 (384:
    mfma4 only) and of 512; B = 33 / 64: a second pass of one row / of 32.  SwiGLU in the 16-row interleave at 16 and 1040 features"""
    with _env(PCY_DISABLE=GEMV_DISABLE.get(route)):
        n = sum(_run_gemv(ctx, key, route) for key in R.gemv_keys(route) if key[3] == epi)
    _record(f"gemv_{route}/e{epi}", n)


@pytest.mark.parametrize("B", [2, 4, 5, 33])
def test_gemv_row_invariance(ctx, B):
    """row b of a B-row call has the bits of the same row alone.  On random data where both calls take the streaming kernel (K = 136: passes
    of 4 rows, B = 5 ends with a pass of one, 33 likewise); on exactly summable data across kernels (K = 128: B >= 4 is an MFMA call, the
    single row a streaming one)"""
    N = 70
    for K, exact in ((136, False), (128, True)):
        if exact:
            c = R.gemv_case(B, N, K, 0, True)
            x, W, b = c["A"], c["W"], c["bias"]
        else:
            g = torch.Generator().manual_seed(B)
            x, W, b = torch.randn(B, K, generator=g).to(BF), (torch.randn(N, K, generator=g) * 0.2).to(BF), torch.randn(N, generator=g).to(BF)
        xd, Wd, bd = x.cuda(), W.cuda(), b.cuda()
        y = _sentinel(B, N)
        _call_gemv(ctx, xd, K, Wd, bd, _vp(None), y, 0, N, N, K, B, 0)
        if exact:
            assert R.compare(y[:B].cpu(), R.reference("gemv", B, N, K, 0, True)) == 0
        for r in range(B):
            y1 = _sentinel(1, N)
            _call_gemv(ctx, xd[r:r + 1], K, Wd, bd, _vp(None), y1, 0, N, N, K, 1, 0)
            assert torch.equal(y1[0].view(I16), y[r].view(I16)), (B, K, r)


@pytest.mark.parametrize("cast", [0, 1])
@pytest.mark.parametrize("B", [1, 4])
def test_gemv_fused_rmsnorm_window(ctx, B, cast):
    """the fused RMSNorm prologue is not exactly summable: a windowed x (ldx = K + 8, NaN behind every row) gives the bits of the contiguous
    call, for the store and the SwiGLU epilogue, both rounding orders, on the streaming kernel"""
    lib = ctx.lib
    K = 520
    for epi, N in ((0, 130), (4, 16)):
        g = torch.Generator().manual_seed(B + 10 * cast + epi)
        x = torch.randn(B, K, generator=g).to(BF)
        W = (torch.randn(N * (2 if epi == 4 else 1), K, generator=g) * 0.2).to(BF).cuda()
        w = (1.0 + 0.1 * torch.randn(K, generator=g)).to(BF).cuda()
        outs = []
        for xpad in (0, 8):
            xbuf, _ = _padded(x, K + xpad, 0)
            y = _sentinel(B, N)
            n0 = _counts(lib)
            _call_gemv(ctx, xbuf, K + xpad, W, None, _vp(None), y, 0, N, N, K, B, epi, rms_w=w, cast=cast)
            assert _delta(lib, n0) == {20 + ROUTE["stream2"]: 1}
            outs.append(y.clone())
        assert bool(outs[0][:B].float().isfinite().all())
        assert torch.equal(outs[0].view(I16), outs[1].view(I16)), (B, cast, epi)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(ctx):
    """everything include/pcy.h says the three entries refuse: code 1 with a text that names the entry, the sentinel-filled output untouched,
    no dispatch or route counter moved"""
    lib = ctx.lib
    M, N, K = 8, 64, 64
    A = torch.zeros(M + 2, K + 16, dtype=BF, device="cuda")
    W = torch.zeros(2 * N + 2, 256, dtype=BF, device="cuda")
    r = torch.zeros(M + 2, N + 16, dtype=BF, device="cuda")
    b = torch.zeros(N + 16, dtype=BF, device="cuda")
    a8 = torch.zeros(2 * N + 2, 256, dtype=torch.uint8, device="cuda")
    s = torch.ones(2 * N + 8, dtype=F32, device="cuda")
    out = _sentinel(M, N + 16)
    null = _vp(None)

    def d(v, default):                            # (a NULL c_void_p is falsy: `v or default` would replace it)
        return _vp(default) if v is None else v

    def gemm(A_=None, lda=K, W_=None, bias=null, resid=null, ldr=0, C_=None, ldc=N, M_=M, N_=N, K_=K, epi=0):
        return lib.pcy_gemm(ctx.h, d(A_, A), lda, d(W_, W), bias, resid, ldr, d(C_, out), ldc, M_, N_, K_, epi)

    def gemv(W_=None, x=None, ldx=K, bias=null, resid=null, y=None, ldy=N, rms=null, N_=N, K_=K, B=4, epi=0):
        return lib.pcy_gemv(ctx.h, d(W_, W), d(x, A), ldx, bias, resid, d(y, out), ldy, rms, 1e-5, 0, N_, K_, B, epi)

    def fp8(A_=None, sa=None, W_=None, sw=None, resid=null, ldr=0, C_=None, ldc=N, M_=M, N_=N, K_=128, epi=0):
        return lib.pcy_gemm_fp8(ctx.h, d(A_, a8), d(sa, s), d(W_, a8), d(sw, s), resid, ldr, d(C_, out), ldc, M_, N_, K_, epi)

    cases = {
        "pcy_gemm": [dict(K_=96), dict(K_=0), dict(lda=K + 4), dict(lda=K - 8), dict(A_=_vp(A, 8)), dict(W_=_vp(W, 8)), dict(A_=null), dict(C_=null),
                     dict(ldc=N - 1), dict(epi=1, resid=_vp(r), ldr=N - 1), dict(epi=1), dict(epi=5), dict(epi=-1), dict(C_=_vp(out, 1)),
                     dict(bias=_vp(b, 1)), dict(epi=1, resid=_vp(r, 1), ldr=N), dict(epi=1, resid=_vp(out), ldr=N + 8, ldc=N), dict(M_=-1), dict(N_=-1),
                     dict(epi=4, N_=48), dict(epi=4, ldc=N // 2 + 2), dict(epi=4, C_=_vp(out, 4)), dict(epi=4, ldc=N // 2 - 4)],
        "pcy_gemv": [dict(K_=12), dict(K_=0), dict(ldx=K + 4), dict(ldx=K - 8), dict(x=_vp(A, 8)), dict(W_=_vp(W, 8)), dict(x=null), dict(y=null),
                     dict(ldy=N - 1), dict(epi=7), dict(epi=1), dict(y=_vp(out, 1)), dict(bias=_vp(b, 1)), dict(epi=1, resid=_vp(r, 1)), dict(B=-1),
                     dict(N_=-1), dict(epi=4, N_=20, ldy=24), dict(epi=4, ldy=N + 6), dict(epi=4, y=_vp(out, 4)), dict(epi=1, resid=_vp(r), rms=_vp(b)),
                     dict(rms=_vp(b, 8))],
        "pcy_gemm_fp8": [dict(K_=64), dict(K_=0), dict(epi=3), dict(epi=2), dict(A_=_vp(a8, 8)), dict(W_=_vp(a8, 4)), dict(ldc=N - 1), dict(epi=1),
                         dict(epi=1, resid=_vp(r), ldr=N - 1), dict(sa=_vp(s, 2)), dict(sw=_vp(s, 2)), dict(sa=null), dict(sw=null), dict(C_=_vp(out, 1)), dict(epi=4, N_=48),
                         dict(epi=4, ldc=N // 2 + 2), dict(epi=4, C_=_vp(out, 4)), dict(M_=-1)],
    }
    n0 = _counts(lib)
    for entry, call in (("pcy_gemm", gemm), ("pcy_gemv", gemv), ("pcy_gemm_fp8", fp8)):
        for kw in cases[entry]:
            rc = call(**kw)
            assert rc == 1, (entry, kw, rc)
            assert lib.pcy_last_error().decode().startswith(entry + ":"), (entry, kw, lib.pcy_last_error())
    torch.cuda.synchronize()
    assert _counts(lib) == n0
    assert bool((out.view(I16) == R.SENTINEL).all())
    # the empty problem is no refusal and no launch
    assert gemm(M_=0) == 0 and gemm(N_=0) == 0 and gemv(B=0) == 0 and gemv(N_=0) == 0 and fp8(M_=0) == 0
    assert _counts(lib) == n0
    # ... and the same arguments without the violation run
    assert gemm() == 0 and gemv() == 0 and fp8() == 0
    torch.cuda.synchronize()
    assert _delta(lib, n0) == {K_DISPATCH["k64"]: 1, 20 + ROUTE["stream2"]: 1, K_DISPATCH["fp8"]: 1}
