"""GPU: every two-pass prefill attention kernel behind pcy_attention, at operator level, with the kernel that ran PROVEN by the library's own
counter (pcy_debug_attn_route_count): each call below asserts that exactly the kernel its input set claims ran once, and that the
single-pass ESM kernel (dispatch kind 6) did not.

a. exact key sets   the probe of tests/attn_ref.py (q = 0, V = a power of two per kv head on the column j % dh): the output says which keys
                    each query attended, and must equal the integer model bit for bit -- every mask pattern, causal and not, every kernel.
                    One wrongly attended or dropped key fails it; tests/test_attn_ref_cpu.py ties the integer model to the oracle and shows
                    the wrong mask rules that the random-input bar lets through.
b. random inputs    the bars of test_gpu_kernels.py::test_attention_exact_rounding unchanged, plus no further from float64 than the bf16
                    oracle is (conftest.assert_no_further_from_truth at its defaults), with and without masks, non-causal dh = 128 included.
c. route independence  a sequence gives the same bits prefilled alone (one query tile per wave) and beside 15 others (two tiles per wave).
d. prefill layout   q, k, v as column windows of one [ntok, (H + 2 Hkv) dh] buffer, as pcy_llama_prefill calls the launcher: same bits."""
import pytest
import torch

import attn_ref as R
from conftest import assert_bf16_close, assert_no_further_from_truth, record_parity, rel_err
from procyon_amd import _lib

pytestmark = pytest.mark.gpu

# the kernel each input set claims to reach; `routed` holds every call to it
CLAIM = {"ragged16": _lib.ATTN_ROUTE_LDS128_2, "llama3x4": _lib.ATTN_ROUTE_LDS128_2, "short32": _lib.ATTN_ROUTE_LDS128_2,
         "ragged3": _lib.ATTN_ROUTE_LDS128_1, "llama3x2": _lib.ATTN_ROUTE_LDS128_1, "short3": _lib.ATTN_ROUTE_LDS128_1,
         "dh64": _lib.ATTN_ROUTE_DH64, "dh32": _lib.ATTN_ROUTE_DH32}
ROUTE_NAME = {_lib.ATTN_ROUTE_DH32: "attn_kernel<32,2>", _lib.ATTN_ROUTE_DH64: "attn_kernel<64,3>",
              _lib.ATTN_ROUTE_LDS128_1: "attn_lds_kernel<128,1>", _lib.ATTN_ROUTE_LDS128_2: "attn_lds_kernel<128,2>"}


@pytest.fixture(scope="module")
def ctx():
    from procyon_amd.engine import Context
    return Context.get()


@pytest.fixture(autouse=True)
def exact_kernels(monkeypatch):
    monkeypatch.setenv("PCY_ESM_ATTN", "exact")     # the single-pass kernel would otherwise take dh = 64, non-causal, unmasked calls


def routed(ctx, route, *args, **kw):
    """ctx.attention(...) -> CPU tensor, asserting that exactly kernel `route` was launched once and the single-pass kernel not at all"""
    lib = ctx.lib
    before = [lib.pcy_debug_attn_route_count(i) for i in range(4)]
    fast = lib.pcy_debug_dispatch_count(_lib.DISPATCH_ATTN_FAST)
    out = ctx.attention(*args, **kw).cpu()
    delta = [lib.pcy_debug_attn_route_count(i) - before[i] for i in range(4)]
    assert delta == [int(i == route) for i in range(4)], (ROUTE_NAME[route], delta)
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_ATTN_FAST) == fast
    return out


def _dev(t):
    return None if t is None else t.cuda()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("name", list(R.SETS))
def test_exact_key_sets(ctx, name, causal):
    H, Hkv, dh, lens = R.SETS[name]
    q, k, v = (t.cuda() for t in R.probe_inputs(H, Hkv, dh, lens))
    for pat, keep in R.mask_patterns(lens).items():
        out = routed(ctx, CLAIM[name], q, k, v, lens, H, Hkv, dh, causal, dh ** -0.5, _dev(keep))
        exp = R.exact_key_sets(H, Hkv, dh, lens, causal, keep)
        if not torch.equal(out, exp):
            bad = (out != exp).any(1).nonzero()[:, 0]
            raise AssertionError(f"{name} causal={causal} mask={pat}: {bad.numel()} token rows differ from the attended-key model, "
                                 f"first packed rows {bad[:8].tolist()}")


@pytest.mark.parametrize("name,causal,masked", R.RANDOM_CASES)
def test_oracle_and_truth_on_random_inputs(ctx, name, causal, masked):
    H, Hkv, dh, lens = R.SETS[name]
    q, k, v, scale = R.random_inputs(name, causal)
    keep = R.mixed_mask(lens) if masked else None
    ref = R.eager_bf16(q, k, v, H, Hkv, dh, lens, causal, scale, keep)
    truth = R.truth_f64(q, k, v, H, Hkv, dh, lens, causal, scale, keep)
    out = routed(ctx, CLAIM[name], q.cuda(), k.cuda(), v.cuda(), lens, H, Hkv, dh, causal, scale, _dev(keep))
    what = f"{ROUTE_NAME[CLAIM[name]]} {name} causal={causal} masked={masked}"
    print(f"{what}: rel_err(HIP, oracle) {rel_err(out, ref):.3e}, {float((out != ref).float().mean()):.4f} of elements differ")
    e_hip, e_ref = assert_no_further_from_truth(out, ref, truth, what)
    record_parity(f"attn_prefill/{name}/{'causal' if causal else 'full'}/{'masked' if masked else 'unmasked'}", kernel=ROUTE_NAME[CLAIM[name]],
                  err_hip_f64=e_hip, err_oracle_f64=e_ref, err_hip_oracle=rel_err(out, ref))
    assert rel_err(out, ref) < 1e-3
    assert_bf16_close(out, ref, what, max_frac=0.03, inter=torch.full_like(ref, 0.5))


@pytest.mark.parametrize("pattern", ["none", "left33", "left130"])
@pytest.mark.parametrize("causal", [True, False])
def test_route_independence(ctx, causal, pattern):
    """sequences of 129, 257 and 500 tokens: their rows of the 16-sequence call (two query tiles per wave) equal bit for bit what the same
    sequence gives alone (one tile per wave).  Same key-block order and rounding points in both; a left-pad mask adds the workgroup-wide
    retry over the full key range, which the two kernels decide over 128 and over 64 query rows."""
    name = "ragged16"
    H, Hkv, dh, lens = R.SETS[name]
    q, k, v, scale = R.random_inputs(name, causal)
    keep = R.mask_patterns(lens)[pattern]
    both = routed(ctx, _lib.ATTN_ROUTE_LDS128_2, q.cuda(), k.cuda(), v.cuda(), lens, H, Hkv, dh, causal, scale, _dev(keep))
    starts = dict((n, t0) for t0, n in R._seqs(lens))
    for n in (129, 257, 500):
        t0 = starts[n]
        sl = slice(t0, t0 + n)
        alone = routed(ctx, _lib.ATTN_ROUTE_LDS128_1, q[sl].cuda(), k[sl].cuda(), v[sl].cuda(), [n], H, Hkv, dh, causal, scale,
                       None if keep is None else keep[sl].cuda())
        diff = int((alone != both[sl]).sum())
        assert diff == 0, f"sequence of {n} tokens, causal={causal}, mask={pattern}: {diff} elements differ between the two kernels"


@pytest.mark.parametrize("name", ["ragged16", "ragged3"])
def test_prefill_layout(ctx, name):
    H, Hkv, dh, lens = R.SETS[name]
    q, k, v, scale = R.random_inputs(name, True)
    keep = R.mixed_mask(lens).cuda()
    plain = routed(ctx, CLAIM[name], q.cuda(), k.cuda(), v.cuda(), lens, H, Hkv, dh, True, scale, keep)
    qkv = torch.cat([q, k, v], 1).contiguous().cuda()
    W = (H + 2 * Hkv) * dh
    assert tuple(qkv.shape) == (sum(lens), W)
    fused = routed(ctx, CLAIM[name], qkv, qkv, qkv, lens, H, Hkv, dh, True, scale, keep, ld=W, col0=(0, H * dh, (H + Hkv) * dh))
    assert torch.equal(fused, plain)
    with pytest.raises(ValueError):        # a window past the row is refused on the host, not read on the device
        ctx.attention(qkv, qkv, qkv, lens, H, Hkv, dh, True, scale, keep, ld=W, col0=(0, H * dh, (H + Hkv) * dh + 8))
