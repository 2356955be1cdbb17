"""CPU: the references and the inputs of tests/gemm_ref.py, on EVERY case that tests/test_gpu_gemm_edges.py runs on the device.

a. exactly summable: the float64 accumulator equals torch's float32 matmul of the same bf16 values (a different summation order), and every
   value in front of a rounding point is an fp32 number (`exact32` inside the reference) -- so bit equality is the right bar, and the two
   long-K GEMM cases may take the float32 matmul;
b. the reference equals `ref_linear` of tests/test_gpu_kernels.py (torch's bf16 `F.linear` chain) where that chain rounds at the same points:
   no bias (F.linear's own bias handling is not stated anywhere), epilogues store / residual / ESM-GELU;
c. every case has an exact bf16 tie in front of a rounding point (K >= 64: a sum needs nine significant bits, 257 or more), outputs on both
   sides of zero (two or more outputs) and non-zero values in its last row and last column;
d. the comparison helper fails when one element of A[:, K-8:], of the last row of W, bias[N-1] or resid[M-1, N-1] changes, or two rows of W
   trade places: the bar cannot pass a lost tail.  An output that no single change can move -- a saturated activation -- would be reported
   here, not hidden."""
import pytest
import torch

import gemm_ref as R

BF, F32, F64 = R.BF, R.F32, R.F64


def _other(v, small):
    """a different value of the same input family: integers in [-3, 3] (sixteenths when small)"""
    unit = 1.0 / 16 if small else 1.0
    return v - 4 * unit if v > 0 else v + 4 * unit if v < 0 else 3 * unit


def _check_case(c, ref, tag, fast_ok=True):
    A, W, b, r, epi = c["A"], c["W"], c["bias"], c["resid"], c["epi"]
    M, K = A.shape
    N = W.shape[0]
    small = epi in (R.EPI_GELU_ESM, R.EPI_SWIGLU)
    # a
    acc64 = R.accumulate(A, W)
    assert torch.equal(R.accumulate(A, W, fast=True), acc64), tag
    assert float(acc64.abs().max()) < 2 ** 19 and bool((acc64 * 16 == (acc64 * 16).round()).all()), tag
    st = {}
    out = R.epilogue(acc64, b, r, epi, st)
    assert R.compare(out, ref) == 0, tag
    # c
    if K >= 64:
        assert st["ties"] >= 1, tag
    o = out.to(F32)
    if o.numel() >= 2:
        assert float(o.min()) < 0 < float(o.max()), tag
    assert bool((o[-1] != 0).any()) and bool((o[:, -1] != 0).any()), tag
    # d
    def differs(**kw):
        d = dict(A=A, W=W, bias=b, resid=r)
        d.update(kw)
        return R.compare(R.linear(d["A"], d["W"], d["bias"], d["resid"], epi), out) > 0
    tail = [k for k in range(K - 8, K) if float(W[N - 1, k]) != 0 and float(A[M - 1, k]) != 0]
    k = tail[0] if tail else K - 1
    A2 = A.clone()
    A2[M - 1, k] = _other(float(A[M - 1, k]), False)
    assert differs(A=A2), (tag, "A tail")
    W2 = W.clone()
    W2[N - 1, k] = _other(float(W[N - 1, k]), small)
    assert differs(W=W2), (tag, "W last row")
    if b is not None:
        b2 = b.clone()
        b2[N - 1] = float(b[N - 1]) + (8.0 if float(b[N - 1]) <= 0 else -8.0)
        assert differs(bias=b2), (tag, "bias")
    if r is not None:
        r2 = r.clone()
        r2[M - 1, N - 1] = -float(r[M - 1, N - 1]) if float(r[M - 1, N - 1]) != 0 else 64.0
        assert differs(resid=r2), (tag, "resid")
    if N >= 2:
        W3 = W.clone()
        W3[[N - 1, N - 2]] = W[[N - 2, N - 1]]
        assert differs(W=W3), (tag, "W rows swapped")
    return out


def _vs_ref_linear(c, out, tag):
    """b: torch's bf16 chain on the same tensors"""
    from test_gpu_kernels import ref_linear
    if c["epi"] not in (0, 1, 3) or c["bias"] is not None or c["M"] * c["N"] * c["K"] > 1 << 28:
        return 0
    assert R.compare(ref_linear(c["A"], c["W"], None, c["resid"], c["epi"]), out) == 0, tag
    return 1


@pytest.mark.parametrize("group", sorted(R.GEMM_SHAPES))
def test_gemm_cases(group):
    n = 0
    for key in R.gemm_keys(group):
        c = R.gemm_case(*key)
        out = _check_case(c, R.reference("gemm", *key), ("gemm", group) + key)
        n += _vs_ref_linear(c, out, key)
    assert n >= 1 or all(k[3] == R.EPI_SWIGLU for k in R.gemm_keys(group)), group


@pytest.mark.parametrize("route", sorted(R.GEMV_SHAPES))
def test_gemv_cases(route):
    n = 0
    for key in R.gemv_keys(route):
        c = R.gemv_case(*key)
        out = _check_case(c, R.reference("gemv", *key), ("gemv", route) + key)
        n += _vs_ref_linear(c, out, key)
    assert n >= 1, route


def test_swiglu_matches_torch_on_unpacked_weights():
    """the reference reads the 16-row interleave as include/pcy.h states it: equal to silu(A g^T) * (A u^T) of the unpacked halves in torch's
    bf16 chain, and `pack_gate_up` is the inverse of `split_gate_up`"""
    import torch.nn.functional as F
    for key in [(70, 288, 64, 4, False), (130, 1312, 192, 4, False)]:
        c = R.gemm_case(*key)
        g, u = R.split_gate_up(c["W"])
        assert torch.equal(R.pack_gate_up(g, u), c["W"])
        assert R.compare(F.silu(F.linear(c["A"], g)) * F.linear(c["A"], u), R.reference("gemm", *key)) == 0
        try:
            from procyon_amd.engine import interleave_gate_up
        except Exception:      # (the engine module needs the built library)
            continue
        assert torch.equal(interleave_gate_up(g, u), c["W"])


def test_fp8_cases():
    """exact codes: the oracle's row quantiser gives power-of-two scales and the integers times 64 as e4m3 values, the accumulator is an fp32
    number whatever the order, ties and both signs occur, and a changed tail element or swapped rows of W fail the comparison"""
    from oracle import fp8_ref as F8
    for key in R.fp8_keys():
        c = R.fp8_case(*key)
        for x, val, sc in ((c["A"], c["a_val"], c["sa"]), (c["W"], c["w_val"], c["sw"])):
            q, s = F8.quant_rows(x)
            assert torch.equal(s, sc), key
            assert torch.equal(q.view(torch.uint8).view(torch.float8_e4m3fn).to(F32), val), key
        acc = c["a_val"].to(F64) @ c["w_val"].to(F64).T
        assert torch.equal((c["a_val"] @ c["w_val"].T).to(F64), acc) and float(acc.abs().max()) < 2 ** 31, key
        st = {}
        out = R.linear_fp8(c["a_val"], c["sa"], c["w_val"], c["sw"], c["resid"], c["epi"], st)
        assert R.compare(out, R.fp8_reference(*key)) == 0
        o = out.to(F32)
        assert st["ties"] >= 1 and float(o.min()) < 0 < float(o.max()) and bool((o[-1] != 0).any()) and bool((o[:, -1] != 0).any()), key
        M, N, K = c["M"], c["N"], c["K"]
        a2, w2, w3 = c["a_val"].clone(), c["w_val"].clone(), c["w_val"].clone()
        a2[M - 1, K - 1] = -a2[M - 1, K - 1] if a2[M - 1, K - 1] != 0 else 64.0
        w2[N - 1, K - 1] = -w2[N - 1, K - 1] if w2[N - 1, K - 1] != 0 else 64.0
        w3[[N - 1, N - 2]] = c["w_val"][[N - 2, N - 1]]
        for a_, w_ in ((a2, c["w_val"]), (c["a_val"], w2), (c["a_val"], w3)):
            assert R.compare(R.linear_fp8(a_, c["sa"], w_, c["sw"], c["resid"], c["epi"]), out) > 0, key


def test_compare_sees_one_bit():
    ref = R.reference("gemm", 70, 130, 64, 0, True)
    out = ref.clone()
    assert R.compare(out, ref) == 0
    out.view(torch.int16)[-1, -1] ^= 1
    assert R.compare(out, ref) == 1
    z = torch.zeros(2, 2, dtype=BF)
    assert R.compare(-z, z) == 4          # -0 is not +0 here


def test_gemv_route_counter_is_bound_and_bounded():
    """pcy_debug_gemv_route_count: six words (procyon_amd._lib.GEMV_ROUTE_*), anything else reads 0; nothing has run without a GPU"""
    import __graft_entry__ as g
    g.build()
    from procyon_amd import _lib
    lib = _lib.load()
    assert (_lib.GEMV_ROUTE_STREAM2, _lib.GEMV_ROUTE_STREAM4, _lib.GEMV_ROUTE_CHUNKED, _lib.GEMV_ROUTE_MFMA2, _lib.GEMV_ROUTE_MFMA3,
            _lib.GEMV_ROUTE_MFMA4) == tuple(range(6))
    for which in (-1, 6, 100):
        assert lib.pcy_debug_gemv_route_count(which) == 0, which
    if not torch.cuda.is_available():
        assert [lib.pcy_debug_gemv_route_count(k) for k in range(6)] == [0] * 6
