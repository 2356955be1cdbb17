"""References and inputs for the edge tests of `pcy_gemm`, `pcy_gemv` and `pcy_gemm_fp8` (tests/test_gpu_gemm_edges.py on the device,
tests/test_gemm_ref_cpu.py for the references themselves).  Written from include/pcy.h -- `C = epi(A . W^T + bias)`, rounding points
`bf16(acc + bias)`, then `bf16(. + resid)`, SwiGLU `bf16(bf16(silu(bf16 g)) * bf16 u)` over W in the 16-row gate/up interleave -- with
float64 between the rounding points, never from the kernels.

Every input is EXACTLY SUMMABLE: A and x hold integers in [-3, 3], W integers in [-3, 3] (sixteenths of them for the epilogues that want
small pre-activations: ESM-GELU and SwiGLU), bias multiples of 0.5 in [-8, 8], the residual integers with |r| <= 512.  For K <= 32776
every partial sum of products is a multiple of 2^-4 below 9 * 32776 / 1 < 2^19 in magnitude: 23 bits, so ANY order of fp32 additions
(MFMA, dot products, wave trees, K chunks) gives the same accumulator, `acc + bias` and `. + resid` are exact in fp32 as well (`exact32`
asserts all three), and the operator's output is ONE bit pattern: the comparison is equality of bits, no tolerance.  Planted rows give
every case sums of +-257 and +-259 (bf16 ties: 257 -> 256, 259 -> 260), which pins round-to-nearest-even in every epilogue.

The ESM-GELU and SiLU epilogues are functions bf16 -> bf16 that tests/test_gpu_kernels.py / test_gpu_round3.py prove equal to torch's CPU
bf16 chain on every bit pattern; that chain is their reference here."""
import functools
import math

import torch
import torch.nn.functional as F

BF, F32, F64, I16, I32 = torch.bfloat16, torch.float32, torch.float64, torch.int16, torch.int32
EPI_STORE, EPI_RESID, EPI_GELU_ERF, EPI_GELU_ESM, EPI_SWIGLU = range(5)
SENTINEL = 0x5A5A          # bf16 3.8e16: no output of an exactly summable case comes near it
TIES = (257, -259)         # planted sums of (row 0 of A) x (rows 0, 1 of W)


def bits(t):
    return t.contiguous().view(I16)


def exact32(x64):
    """float64 -> float32, asserting that nothing is lost: the claim that makes every summation order agree"""
    x32 = x64.to(F32)
    assert torch.equal(x32.to(F64), x64), "an intermediate is not an fp32 number: the case is not exactly summable"
    return x32


def is_tie(x32):
    """fp32 values that lie exactly half way between two bf16 neighbours"""
    return (x32.contiguous().view(I32) & 0xFFFF) == 0x8000


def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).to(F32)


def _plant_a(a_row):
    """row 0 of A / x: 3 with eight 1s behind position 28, so that a row of W can hit any target up to 28 x 9 + 8 x 3 within the first 36
    positions; behind them +3 on the first half and -3 on the second, which a row of W cancels by repeating its values"""
    K = a_row.numel()
    a_row.fill_(3.0)
    a_row[28:36] = 1.0
    a_row[36 + (K - 36) // 2:] = -3.0


def _plant_w(a_row, w_row, target, gen):
    """rewrite a row of W (integers in [-3, 3]) so that its dot product with the planted row of A is `target`: the target from the first 36
    positions, the rest random, non-zero and cancelling HALF A ROW apart -- so a lost or doubled 8-element piece at the end of K still
    moves the sum"""
    K = a_row.numel()
    h = (K - 36) // 2
    tail = _ints((h,), 1, 3, gen) * (_ints((h,), 0, 1, gen) * 2 - 1)
    w_row[36:36 + h] = tail
    w_row[36 + h:] = tail
    rest = float(target)
    for k in range(36):
        w = float(int(max(-3.0, min(3.0, rest / float(a_row[k])))))
        w_row[k] = w
        rest -= w * float(a_row[k])
    assert rest == 0 and float(a_row @ w_row) == target, target


def esm_gelu(x):
    """the oracle's ESM GELU on a bf16 tensor: every operation rounds to bf16 (tests/test_gpu_kernels.py `esm_gelu`)"""
    return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))


def split_gate_up(W):
    """[2F, K] in the 16-row interleave (rows 32j .. 32j+15: gate of features 16j .., rows 32j+16 .. 32j+31: their up rows) -> gate, up [F, K]"""
    N, K = W.shape
    v = W.view(N // 32, 2, 16, K)
    return v[:, 0].reshape(N // 2, K), v[:, 1].reshape(N // 2, K)


def pack_gate_up(g, u):
    F_, K = g.shape
    assert F_ % 16 == 0
    return torch.stack([g.view(F_ // 16, 16, K), u.view(F_ // 16, 16, K)], dim=1).reshape(2 * F_, K).contiguous()


def accumulate(A, W, fast=False):
    """A . W^T in float64 (exact: products of small integers and sixteenths); fast: torch's float32 matmul, which tests/test_gemm_ref_cpu.py
    shows equal on every case before the two long-K cases rely on it"""
    if fast:
        return (A.to(F32) @ W.to(F32).T).to(F64)
    return A.to(F64) @ W.to(F64).T


def epilogue(acc, bias, resid, epi, stats=None):
    """the rounding points of include/pcy.h on a float64 accumulator [M, N]; stats: dict that receives the number of exact ties met"""
    def rb(x64):
        x32 = exact32(x64)
        if stats is not None:
            stats["ties"] = stats.get("ties", 0) + int(is_tie(x32).sum())
        return x32.to(BF)
    if epi == EPI_SWIGLU:
        N = acc.shape[1]
        v = acc.view(-1, N // 32, 2, 16)
        g, u = rb(v[:, :, 0].reshape(-1, N // 2)), rb(v[:, :, 1].reshape(-1, N // 2))
        return F.silu(g) * u
    y = rb(acc + (bias.to(F64) if bias is not None else 0.0))
    if epi == EPI_RESID:
        return rb(y.to(F64) + resid.to(F64))
    if epi == EPI_GELU_ESM:
        return esm_gelu(y)
    assert epi == EPI_STORE, epi
    return y


def linear(A, W, bias, resid, epi, fast=False, stats=None):
    """C[M, N] (N/2 for SwiGLU) = epi(A . W^T + bias) for epi 0, 1, 3, 4: bf16 in, bf16 out"""
    return epilogue(accumulate(A, W, fast), bias, resid, epi, stats)


def linear_fp8(a_val, sa, w_val, sw, resid, epi, stats=None):
    """pcy_gemm_fp8 on exact codes: a_val / w_val = the e4m3 VALUES of the codes (integers in [-7, 7] times 64), sa [M] / sw [N] the
    power-of-two scales; C = epi(((A8 . W8^T) * sa[m]) * sw[n]), every product exact"""
    acc = (a_val.to(F64) @ w_val.to(F64).T) * sa.to(F64)[:, None] * sw.to(F64)[None, :]
    return epilogue(acc, None, resid, epi, stats)


# ------------------------------------------------------------------------------------------------ cases
def _case(rows, N, K, epi, bias, seed):
    """inputs of one (A | x)[rows, K] x W[N, K] problem; N = packed rows for SwiGLU.  The few outputs of a one-row or one-column problem can all fall on one
    side of zero, or its last element on a zero of the activation, by chance: such a draw is thrown away and the next one taken (decided here, on the reference, before any kernel sees the case)"""
    for draw in range(64):
        c = _draw(rows, N, K, epi, bias, seed + 7717 * draw)
        if min(rows, N) > 4:
            return c
        o = linear(c["A"], c["W"], c["bias"], c["resid"], epi).to(F32)
        if (o.numel() < 2 or float(o.min()) < 0 < float(o.max())) and bool((o[-1] != 0).any()) and bool((o[:, -1] != 0).any()):
            return c
    raise AssertionError((rows, N, K, epi))


def _draw(rows, N, K, epi, bias, seed):
    gen = torch.Generator().manual_seed(seed * 1000003 + rows * 7919 + N * 31 + K + epi)
    small = epi in (EPI_GELU_ESM, EPI_SWIGLU)
    A, W = _ints((rows, K), -3, 3, gen), _ints((N, K), -3, 3, gen)
    if K >= 64:                                   # (K = 8 cannot hold a tie: 9 significant bits need a sum of 257 or more)
        _plant_a(A[0])
        for n, t in zip(range(min(N, 2)), TIES):
            _plant_w(A[0], W[n], t, gen)
    if small:
        W = W / 16.0
    Nout = N // 2 if epi == EPI_SWIGLU else N
    b = None
    if bias and epi != EPI_SWIGLU:
        b = _ints((N,), -4, 4, gen) * 0.5 if small else _ints((N,), -16, 16, gen) * 0.5   # (|b| <= 2 in front of the GELU: -8 saturates a whole column to -0)
        b[:2] = 0.0                               # the planted ties stay ties
    r = _ints((rows, Nout), -512, 512, gen).to(BF).to(F32) if epi == EPI_RESID else None   # (rounded to bf16: still integers)
    c = {"A": A.to(BF), "W": W.to(BF), "bias": None if b is None else b.to(BF), "resid": None if r is None else r.to(BF),
         "epi": epi, "M": rows, "N": N, "K": K, "Nout": Nout}
    for k in ("A", "W", "bias", "resid"):         # every input is a bf16 number as generated
        if c[k] is not None:
            assert torch.equal(c[k].to(F32), {"A": A, "W": W, "bias": b, "resid": r}[k]), k
    return c


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, epi, bias=True, seed=0):
    assert epi != EPI_SWIGLU or (N % 32 == 0 and not bias)   # (rows 0 / 1 of the packed W are gate rows of features 0 / 1)
    return _case(M, N, K, epi, bias, seed)


@functools.lru_cache(maxsize=None)
def gemv_case(B, N, K, epi, bias=True, seed=1):
    """pcy_gemv: N = output columns (features for SwiGLU: W has 2N packed rows); x is key "A" """
    if epi == EPI_SWIGLU:
        assert N % 16 == 0
        c = dict(gemm_case(B, 2 * N, K, epi, False, seed))
    else:
        c = dict(_case(B, N, K, epi, bias, seed))
    c.update(B=B, N=N, Nout=N)
    return c


@functools.lru_cache(maxsize=None)
def reference(kind, *key):
    """the expected output of gemm_case(*key) / gemv_case(*key), computed once and shared; long K through the float32 matmul"""
    c = gemm_case(*key) if kind == "gemm" else gemv_case(*key)
    return linear(c["A"], c["W"], c["bias"], c["resid"], c["epi"], fast=c["K"] >= 4096 and kind == "gemm")


@functools.lru_cache(maxsize=None)
def fp8_case(M, N, K, epi, seed=2):
    """bf16 matrices whose per-row e4m3 quantisation is exact: integers in [-7, 7] with every row reaching 7, row r of A times 2^(r % 3),
    row n of W times 2^-(4 + n % 2) -- scale = amax / 448 = 2^e / 64 exactly, codes = the integers times 64"""
    gen = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 31 + K + epi)
    ai, wi = _ints((M, K), -7, 7, gen), _ints((N, K), -7, 7, gen)
    ai[:, 0] = 7.0
    wi[:, 1] = -7.0
    ea, ew = torch.arange(M) % 3, -(4 + torch.arange(N) % 2)
    Nout = N // 2 if epi == EPI_SWIGLU else N
    r = _ints((M, Nout), -512, 512, gen).to(BF) if epi == EPI_RESID else None
    return {"A": (ai * 2.0 ** ea[:, None]).to(BF), "W": (wi * 2.0 ** ew[:, None]).to(BF), "a_val": ai * 64.0, "w_val": wi * 64.0,
            "sa": (2.0 ** ea.to(F32)) / 64.0, "sw": (2.0 ** ew.to(F32)) / 64.0, "resid": r, "epi": epi, "M": M, "N": N, "K": K, "Nout": Nout}


@functools.lru_cache(maxsize=None)
def fp8_reference(*key):
    c = fp8_case(*key)
    return linear_fp8(c["a_val"], c["sa"], c["w_val"], c["sw"], c["resid"], c["epi"])


# The shapes of tests/test_gpu_gemm_edges.py, by the kernel each reaches (the GPU file asserts the route; the CPU file checks every case).
# (M, N, K list, epilogues); N = packed rows for SwiGLU.
GEMM_SHAPES = {
    "k64":  [(70, 130, (64, 192), (0, 1, 3)), (1, 132, (64, 192), (0, 1, 3))],
    # PCY_GEMM_MID=-1.  130 x 260 is six 128 x 128 tiles: below 192 tiles the launcher still prefers 64 x 64 tiles for every epilogue that has
    # that form, so of the issue's shapes only SwiGLU reaches the 128 x 128 kernel; 130 x 24580 (2 x 193 tiles) reaches it for the others
    "k64_nomid": [(130, 260, (64, 192), (0, 1, 3))],
    "k128": [(70, 288, (64, 192), (4,)), (130, 24580, (64,), (0, 1, 3))],
    "mid":  [(130, 1290, (64, 192), (0, 1, 3)), (130, 1312, (64, 192), (4,)), (513, 6144, (64, 192), (0, 1, 3, 4))],
    "big":  [(2050, 1288, (64, 192, 4160), (0, 1, 3)), (2050, 1290, (64, 192), (0, 1, 3)), (2050, 1312, (64, 192), (4,))],
}
FP8_SHAPES = [(5, 264, (128, 384), (0, 1)), (5, 288, (128, 384), (4,)), (257, 1290, (128, 384), (0, 1)), (257, 1312, (128, 384), (4,)),
              (300, 512, (128, 384), (1,))]
# route -> (B list, N list, K list, epilogues); SwiGLU runs at the feature counts GEMV_SWIGLU_N of a route (N % 16 == 0)
GEMV_SHAPES = {
    "stream2": ((1, 2, 3, 4), (1, 5, 130), (8, 136, 520), (0, 1, 3, 4)),
    "stream4": ((1, 3), (8190,), (72,), (0, 1, 3, 4)),
    "chunked4": ((4,), (20,), (8200,), (0, 1, 3, 4)),
    "chunked1": ((1,), (20,), (32776,), (0, 1, 3, 4)),
    "mfma4": ((4, 16, 17, 32), (16, 70, 1040), (128, 384, 512, 1536), (0, 1, 3, 4)),
    "mfma4_passes": ((33, 64), (70,), (128, 512), (0, 1, 3, 4)),
    "mfma3": ((4, 16, 17, 32), (16, 70, 1040), (512, 1536), (0, 1, 3, 4)),
    "mfma2": ((4, 16, 17, 32), (16, 70, 1040), (512, 1536), (0, 1, 3, 4)),
}
GEMV_SWIGLU_N = {"stream2": (16, 1040), "stream4": (8192,), "chunked4": (16,), "chunked1": (16,), "mfma4": (16, 1040), "mfma4_passes": (16,),
                 "mfma3": (16, 1040), "mfma2": (16, 1040)}


def gemv_keys(route):
    """every (B, N, K, epi, bias) of a route: bias on and off for epilogues 0 and 1, on for ESM-GELU, none for SwiGLU"""
    Bs, Ns, Ks, epis = GEMV_SHAPES[route]
    for epi in epis:
        for N in (GEMV_SWIGLU_N[route] if epi == EPI_SWIGLU else Ns):
            for K in Ks:
                for B in Bs:
                    for bias in ((True, False) if epi in (EPI_STORE, EPI_RESID) else (epi != EPI_SWIGLU,)):
                        yield (B, N, K, epi, bias)


def gemm_keys(group):
    for M, N, Ks, epis in GEMM_SHAPES[group]:
        for K in Ks:
            for epi in epis:
                for bias in ((True, False) if epi in (EPI_STORE, EPI_RESID) else (epi != EPI_SWIGLU,)):
                    yield (M, N, K, epi, bias)


def fp8_keys():
    for M, N, Ks, epis in FP8_SHAPES:
        for K in Ks:
            for epi in epis:
                yield (M, N, K, epi)


def compare(out, ref):
    """the bar of every case: the same bits everywhere.  Returns the number of differing elements (0 = pass)"""
    assert out.shape == ref.shape and out.dtype == BF and ref.dtype == BF, (out.shape, ref.shape)
    return int((bits(out) != bits(ref)).sum())
