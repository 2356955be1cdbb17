"""GPU: every operator of the fp32 family (`pcy_f32_*`, procyon_amd/csrc/pcy_f32.hip) against the float64 references of
tests/f32_ref.py, at the smallest shapes that reach each loop edge of the kernels: the second pass of every strided loop, partly
empty tiles and slabs, strided windows of wider buffers, unaligned operands.  Bars as tests/test_gpu_fp32.py states them for single
operators: norm-wise relative error <= 2e-5, max-abs <= 2e-4 of the largest reference value; exact equality for pure gathers and
for everything the operator must leave alone.  tests/test_f32_ref_cpu.py holds the references to the oracle and shows that plain
torch fp32 meets the same bars on the same inputs."""
import ctypes as C

import pytest
import torch

import f32_ref as R
from conftest import record_parity

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture(scope="module")
def ops():
    from procyon_amd.engine_f32 import F32Ops
    return F32Ops()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _call(ops, name, *args):
    from procyon_amd import _lib as L
    L.check(getattr(ops.lib, name)(ops.h, *args), name)
    torch.cuda.synchronize()


def check(key, out, ref, maxabs=True):
    e, m = R.rel64(out.cpu(), ref), R.maxabs64(out.cpu(), ref)
    record_parity(f"fp32_ops/{key}", rel_err=f"{e:.3e}", max_abs_over_max=f"{m:.3e}")      # (as text: the report rounds floats to 1e-6)
    print(f"fp32_ops/{key}: rel {e:.3e} maxabs {m:.3e}")
    assert bool(out.isfinite().all()), key
    assert e <= R.OP_BAR, (key, e)
    if maxabs:
        assert m < R.OP_MAXABS, (key, m)


# ------------------------------------------------------------------------------------------------ decode attention
@pytest.mark.parametrize("H,Hkv,dh", R.DECODE_GEOMS)
@pytest.mark.parametrize("nkeys", R.DECODE_NKEYS)
def test_attn_decode(ops, nkeys, H, Hkv, dh):
    """one query per row against slots [0, nkeys) of its cache: the 64-lane key stride below, at and above one pass, the e += 64 loop at
    dh = 128, grouped heads; q is the strided view of the fused qkv rows; NaN in every slot >= nkeys must not reach the output"""
    c = R.decode_case(nkeys, H, Hkv, dh)
    qkv = c["qkv"].cuda()
    q = qkv[:, :H * dh]
    assert q.stride(0) == (H + 2 * Hkv) * dh and not q.is_contiguous()
    out = ops.attn_decode(q, c["kc"].cuda(), c["vc"].cuda(), nkeys, H, Hkv, dh, dh ** -0.5)
    ref = R.attn_decode(c["qkv"][:, :H * dh], c["kc"], c["vc"], nkeys, H, Hkv, dh, dh ** -0.5)
    check(f"attn_decode[{nkeys}-{H}x{Hkv}x{dh}]", out, ref)
    for b in range(out.shape[0]):                     # per row and head: a swapped row or KV head is a large error on that slice
        for h in range(H):
            assert R.rel64(out[b, h * dh:(h + 1) * dh].cpu(), ref[b, h * dh:(h + 1) * dh]) <= R.OP_BAR, (b, h)


def test_attn_decode_checks_q(ops):
    """F32Ops.attn_decode refuses a q the kernel cannot read: wrong dtype, host memory, a strided inner dimension, an unaligned row stride"""
    kc = torch.zeros(2, 4, 32, device="cuda")
    good = torch.zeros(2, 64, device="cuda")
    ops.attn_decode(good, kc, kc, 4, 2, 1, 32, 1.0)
    for bad in (good.double(), good.cpu(), torch.zeros(2, 128, device="cuda")[:, ::2], torch.zeros(2, 65, device="cuda")[:, :64]):
        with pytest.raises(TypeError):
            ops.attn_decode(bad, kc, kc, 4, 2, 1, 32, 1.0)


# ------------------------------------------------------------------------------------------------ prefill attention
@pytest.mark.parametrize("causal", [True, False])
def test_attention_keep_and_keyless_rows(ops, causal):
    """packed lengths [12, 70, 1, 65] with 5 / 0 / 0 / 64 left pads (the last sequence keeps a single token), GQA 4/2, dh 64.  Causal:
    the left-pad query rows have no kept key and must hold the plain average of V over ALL keys of their sequence (include/pcy.h)."""
    c = R.attn_case()
    H, Hkv, dh = R.ATTN_GEOM
    qkv = c["qkv"].cuda()
    out = ops.attention(qkv, 0, qkv, H * dh, qkv, (H + Hkv) * dh, c["cu"].cuda(), c["keep"].cuda(), len(R.ATTN_LENS), max(R.ATTN_LENS),
                        H, Hkv, dh, causal, dh ** -0.5)
    q, k, v = R.attn_windows(c["qkv"])
    ref = R.attention(q, k, v, c["cu"], c["keep"], H, Hkv, dh, causal, dh ** -0.5)
    dead = R.keyless_rows(c["cu"], c["keep"], causal)
    check(f"attention[causal={int(causal)}]", out, ref)
    for s_ in range(len(R.ATTN_LENS)):
        t0, t1 = int(c["cu"][s_]), int(c["cu"][s_ + 1])
        assert R.rel64(out[t0:t1].cpu(), ref[t0:t1]) <= R.OP_BAR, s_
    if causal:
        assert int(dead.sum()) == sum(R.ATTN_PADS)
        check("attention[keyless_rows]", out[dead.cuda()], ref[dead])
        check("attention[keyed_rows]", out[(~dead).cuda()], ref[~dead])
    else:
        assert int(dead.sum()) == 0


# ------------------------------------------------------------------------------------------------ ESM embedding
@pytest.mark.parametrize("d", [320, 100])
@pytest.mark.parametrize("mask_pads,pads", R.ESM_VARIANTS)
def test_esm_embed(ops, d, mask_pads, pads):
    """lengths [1, 5, 64, 65, 300] in one call: the gridDim.y token loop (over 64 tokens) and the 256-thread counting loop (300) take a
    second pass; <mask> at 0, 1 and several positions: the observed mask ratio rescales the rest; with mask_pads the pads are zero"""
    c = R.esm_case(d, pads)
    out = torch.full((c["tokens"].numel(), d), float("nan"), device="cuda")
    table, tokens, cu = c["table"].cuda(), c["tokens"].cuda(), c["cu"].cuda()
    _call(ops, "pcy_f32_esm_embed", _p(table), _p(tokens), _p(cu), len(R.ESM_LENS), max(R.ESM_LENS), _p(out), d, mask_pads)
    ref = R.esm_embed(c["table"], c["tokens"], c["cu"], mask_pads)
    check(f"esm_embed[d={d}-mask_pads={mask_pads}-pads={int(pads)}]", out, ref)
    zero = (c["tokens"] == R.MASK_ID) | ((c["tokens"] == R.PAD_ID) if mask_pads else torch.zeros_like(c["tokens"], dtype=torch.bool))
    assert int(zero.sum()) > 0 and bool((out.cpu()[zero] == 0).all())
    for s_ in range(len(R.ESM_LENS)):                 # per sequence: each has its own ratio
        t0, t1 = int(c["cu"][s_]), int(c["cu"][s_ + 1])
        if bool(ref[t0:t1].any()):
            assert R.rel64(out[t0:t1].cpu(), ref[t0:t1]) <= R.OP_BAR, s_


# ------------------------------------------------------------------------------------------------ pooling
@pytest.mark.parametrize("d", R.POOL_DIMS)
@pytest.mark.parametrize("mode,nan", [(0, False), (0, True), (1, False), (1, True), (2, False)])
def test_pool(ops, d, mode, nan):
    """proteins of 1, 2, 3 and 1 ranges, range lengths 1 .. 9, the corrected mean of a single range of length 3 (one row left), a partly
    empty second 256-feature slab (d = 257, 320); the two means skip a NaN element as nanmean does"""
    c = R.pool_case(d, nan)
    nprot = len(R.POOL_SEG) - 1
    seg = torch.tensor(R.POOL_SEG, dtype=torch.int32).cuda()
    rng = torch.tensor(R.POOL_RNG, dtype=torch.int32).reshape(-1).cuda()
    out = torch.full((nprot, d), float("nan"), device="cuda")
    h = c["h"].cuda()
    _call(ops, "pcy_f32_pool", _p(h), d, _p(seg), _p(rng), nprot, mode, _p(out))
    ref = R.pool(c["h"], R.POOL_SEG, R.POOL_RNG, mode)
    check(f"pool[d={d}-mode={mode}-nan={int(nan)}]", out, ref)
    for p in range(nprot):
        assert R.rel64(out[p].cpu(), ref[p]) <= R.OP_BAR, p
    if mode == 2:
        assert torch.equal(out.cpu().double(), ref)          # a maximum is one of its inputs


# ------------------------------------------------------------------------------------------------ linear
def _run_linear(ops, A, lda, W, bias, resid, ldr, Cp, ldc, M, N, K, act):
    _call(ops, "pcy_f32_linear", _p(A), lda, _p(W), _p(bias), _p(resid), ldr, _p(Cp), ldc, M, N, K, act)


@pytest.mark.parametrize("name", list(R.LINEAR_CASES))
@pytest.mark.parametrize("mode", R.LINEAR_MODES)
def test_linear_edges(ops, name, mode):
    """window: A, C and resid are column windows of wider buffers (lda > K, ldc > N, ldr > N), the columns left and right of C keep
    their sentinel; alias: resid is C; m1: one row; k16: a single k-tile; n130: N % 4 != 0, the scalar store path; offset: A starts one
    float late, which must take the plain kernel and still be right"""
    c = R.linear_case(name)
    M, N, K = R.LINEAR_CASES[name]
    bias, resid, act = R.linear_args(c, mode)
    ref = R.linear(c["A"], c["W"], bias, resid, act)
    W, bias_d = c["W"].cuda(), None if bias is None else bias.cuda()
    A, resid_d = c["A"].cuda(), None if resid is None else c["resid"].cuda()
    if name == "window":
        SENT = 777.0
        Aw = torch.full((M, K + 8), SENT, device="cuda")
        Aw[:, 4:4 + K] = A
        Cw = torch.full((M, N + 16), SENT, device="cuda")
        Rw = torch.full((M, N + 12), SENT, device="cuda")
        Rw[:, 4:4 + N] = c["resid"].cuda()
        _run_linear(ops, Aw[:, 4:], K + 8, W, bias_d, None if resid is None else Rw[:, 4:], N + 12, Cw[:, 8:], N + 16, M, N, K, act)
        out = Cw[:, 8:8 + N]
        assert bool((Cw[:, :8] == SENT).all()) and bool((Cw[:, 8 + N:] == SENT).all())
        assert bool((Rw[:, :4] == SENT).all()) and bool((Rw[:, 4 + N:] == SENT).all()) and torch.equal(Rw[:, 4:4 + N].cpu(), c["resid"])
    elif name == "alias":
        out = c["resid"].cuda().contiguous()               # C holds the residual going in
        _run_linear(ops, A, K, W, bias_d, None if resid is None else out, N, out, N, M, N, K, act)
    elif name == "offset":
        flat = torch.zeros(M * K + 1, device="cuda")
        flat[1:] = A.reshape(-1)
        A1 = flat[1:].view(M, K)
        assert A1.data_ptr() % 16 == 4
        out = torch.full((M, N), float("nan"), device="cuda")
        _run_linear(ops, A1, K, W, bias_d, resid_d, N, out, N, M, N, K, act)
    else:
        out = torch.full((M, N), float("nan"), device="cuda")
        _run_linear(ops, A, K, W, bias_d, resid_d, N, out, N, M, N, K, act)
    check(f"linear[{name}-{mode}]", out, ref)


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("d", R.NORM_DIMS)
def test_norms(ops, d):
    """rows of 1, 100, 256, 257 and 4096 features around a mean of 8: one element, a partly filled pass, exactly one pass, one element
    into the second, sixteen passes; the variance is taken around the mean, which a sum of squares minus mean^2 would lose here"""
    c = R.norm_case(d)
    x, w, b = c["x"].cuda(), c["w"].cuda(), c["b"].cuda()
    check(f"layernorm[d={d}]", ops.layernorm(x, w, b, c["eps"]), R.layernorm(c["x"], c["w"], c["b"], c["eps"]))
    check(f"rmsnorm[d={d}]", ops.rmsnorm(x, w, c["eps"]), R.rmsnorm(c["x"], c["w"], c["eps"]))


# ------------------------------------------------------------------------------------------------ rotary
@pytest.mark.parametrize("nh,dh", R.ROPE_GEOMS)
@pytest.mark.parametrize("prescale", [0.0, 0.125])
def test_rope(ops, nh, dh, prescale):
    """a window at col0 = 8 of a wider buffer; 8 x 128 gives 512 pairs per row, a second pass of the 256-thread loop; positions include 0
    and the table's last row; the columns outside the window keep their bits"""
    c = R.rope_case(nh, dh)
    c0 = R.ROPE_COL0
    buf = c["buf"].cuda().contiguous()
    ops.rope(buf, c0, nh, dh, c["pos"].cuda(), c["cos"].cuda(), c["sin"].cuda(), prescale=prescale)
    torch.cuda.synchronize()
    ref = R.rope(c["buf"], c0, nh, dh, c["pos"], c["cos"], c["sin"], prescale)
    check(f"rope[{nh}x{dh}-prescale={prescale}]", buf[:, c0:c0 + nh * dh], ref[:, c0:c0 + nh * dh])
    for t in (0, 1):                                    # position 0 and the last table row
        assert R.rel64(buf[t, c0:c0 + nh * dh].cpu(), ref[t, c0:c0 + nh * dh]) <= R.OP_BAR, t
    assert torch.equal(buf[:, :c0].cpu(), c["buf"][:, :c0]) and torch.equal(buf[:, c0 + nh * dh:].cpu(), c["buf"][:, c0 + nh * dh:])


# ------------------------------------------------------------------------------------------------ gathers
@pytest.mark.parametrize("d", R.EMBED_DIMS)
def test_embed(ops, d):
    """table rows (first and last included) mixed with soft rows, a partly filled pass (d = 100) and five passes (1280): exact"""
    c = R.embed_case(d)
    out = ops.embed(c["table"].cuda(), c["ids"].cuda(), c["soft"].cuda(), c["soft_map"].cuda())
    assert torch.equal(out.cpu(), R.embed(c["table"], c["ids"], c["soft"], c["soft_map"]))
    assert torch.equal(ops.embed(c["table"].cuda(), c["ids"].cuda()).cpu(), R.embed(c["table"], c["ids"]))


def test_acc_rows(ops):
    """dst[r] += src[rows[r]] with ld > d, a repeated source row, two accumulating calls into the same dst"""
    c = R.acc_case()
    d, ld = c["d"], c["src"].shape[1]
    dst, rows = c["dst"].cuda().contiguous(), c["rows"].cuda()
    for src in (c["src"].cuda(), c["src2"].cuda()):
        _call(ops, "pcy_f32_acc_rows", _p(src), ld, _p(rows), _p(dst), rows.numel(), d)
    ref = R.acc_rows(R.acc_rows(c["dst"], c["src"], c["rows"], d), c["src2"], c["rows"], d)
    check("acc_rows", dst, ref)
    assert torch.equal(dst.cpu(), (c["dst"] + c["src"][c["rows"].long(), :d]) + c["src2"][c["rows"].long(), :d])     # two fp32 additions: exact


# ------------------------------------------------------------------------------------------------ SiLU-mul
@pytest.mark.parametrize("n", [1, R.SILU_BIG])
def test_silu_mul(ops, n):
    """n = 65536 * 256 + 257 runs the grid-stride loop (the grid is capped at 65536 workgroups); gates +-1e4, +-88 and 0 at both ends:
    finite, and every element within the bar of float64 silu(g) * u"""
    c = R.silu_case(n)
    out = ops.silu_mul(c["g"].cuda(), c["u"].cuda()).cpu()
    ref = R.silu_mul(c["g"], c["u"])
    check(f"silu_mul[n={n}]", out, ref)
    assert bool(((out.double() - ref).abs() <= R.OP_BAR * ref.abs() + 1e-30).all())
    k = len(R.SILU_SPECIAL)
    if n > 2 * k:
        assert torch.equal(c["g"][-k:], torch.tensor(R.SILU_SPECIAL))
        check(f"silu_mul[n={n}-tail]", out[-300:], ref[-300:])         # the elements only the second pass of the loop reaches
