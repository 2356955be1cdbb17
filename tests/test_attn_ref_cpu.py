"""CPU: what the prefill attention tests (tests/test_gpu_attn_prefill.py) rest on, settled without a GPU.

1. The integer model of the probe (attn_ref.exact_key_sets) equals the rounding-point oracle (attn_ref.eager_bf16) bit for bit on every probe
   input: the GPU test compares the kernels with the integer model, and this ties the model to the oracle.
2. The oracle against its other-accumulation-order twin and against float64 on every random input set of the GPU test: the reference alone
   stays inside the caps that the GPU test applies to the kernels.
3. Six deliberately wrong mask / head rules: each must fail the exact probe.  Whether the random-input bar would have seen it is measured and
   reported (`PARITY attn_mutant/...` lines of the terminal summary), not asserted.
4. The route counter reads 0 outside its four words, and the pinned kinds of pcy_debug_dispatch_count did not grow."""
import pytest
import torch

import attn_ref as R
from conftest import assert_bf16_close, assert_no_further_from_truth, record_parity, rel_err


@pytest.fixture(scope="module")
def probe_oracle():
    """eager_bf16 of every probe input: (set, causal, pattern) -> output.  Computed once, read by the tests below."""
    cache = {}

    def get(name, causal, pat, keep):
        key = (name, causal, pat)
        if key not in cache:
            H, Hkv, dh, lens = R.SETS[name]
            q, k, v = R.probe_inputs(H, Hkv, dh, lens)
            cache[key] = R.eager_bf16(q, k, v, H, Hkv, dh, lens, causal, dh ** -0.5, keep)
        return cache[key]
    return get


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("name", list(R.SETS))
def test_integer_model_equals_the_oracle_on_every_probe(probe_oracle, name, causal):
    H, Hkv, dh, lens = R.SETS[name]
    for pat, keep in R.mask_patterns(lens).items():
        ref = probe_oracle(name, causal, pat, keep)
        exp = R.exact_key_sets(H, Hkv, dh, lens, causal, keep)
        assert torch.equal(exp, ref), (name, causal, pat, int((exp != ref).sum()))


def test_probe_patterns_are_what_they_claim():
    """the masks hold the cases their names promise: every left pad, a sequence without a kept key, holes across rows 64 and 128"""
    lens = R.RAGGED
    pats = R.mask_patterns(lens)
    assert pats["none"] is None and bool(pats["left0"].all())
    assert [int((pats["left%s" % p][:500] == 0).sum()) for p in (5, 33, 64, 130, "N-1")] == [5, 33, 64, 130, 499]
    assert int(pats["full_seq"][:500].sum()) == 0 and int(pats["full_seq"][500:501].sum()) == 1
    d = pats["diagonal"][:500]
    assert d[63] == 0 and d[64] == 0 and d[127] == 0 and d[128] == 0 and d[49] == 1 and d[140] == 1
    assert int(pats["block"][32:64].sum()) == 0 and int(pats["block"][:32].sum()) == 32
    assert pats["trailing"][499] == 0 and pats["trailing"][0] == 1
    for kp in pats.values():        # every non-empty sequence of every pattern but full_seq keeps at least one key
        if kp is not None and kp is not pats["full_seq"]:
            assert all(int(kp[t0:t0 + n].sum()) >= 1 for t0, n in R._seqs(lens))


@pytest.mark.parametrize("name,causal,masked", R.RANDOM_CASES)
def test_oracle_alone_stays_inside_the_caps(name, causal, masked):
    """eager_bf16 vs its fp32-matmul twin under the elementwise bar of test_attention_exact_rounding, and vs float64 under
    assert_no_further_from_truth at its defaults"""
    H, Hkv, dh, lens = R.SETS[name]
    q, k, v, scale = R.random_inputs(name, causal)
    keep = R.mixed_mask(lens) if masked else None
    ref = R.eager_bf16(q, k, v, H, Hkv, dh, lens, causal, scale, keep)
    twin = R.eager_bf16(q, k, v, H, Hkv, dh, lens, causal, scale, keep, alt=True)
    truth = R.truth_f64(q, k, v, H, Hkv, dh, lens, causal, scale, keep)
    what = f"attention twin {name} causal={causal} masked={masked}"
    assert rel_err(twin, ref) < 1e-3, (what, rel_err(twin, ref))
    assert_bf16_close(twin, ref, what, max_frac=0.03, inter=torch.full_like(ref, 0.5))
    assert_no_further_from_truth(twin, ref, truth, what)


def _passes_random_bar(out, ref):
    try:
        assert rel_err(out, ref) < 1e-3
        assert_bf16_close(out, ref, "mutant", max_frac=0.03, inter=torch.full_like(ref, 0.5))
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_probe_catches_every_mask_mutant(probe_oracle, mutant):
    """each wrong rule changes at least one probe output (required); whether the random-input bar of test_attention_exact_rounding would
    have failed on the ragged 16-sequence set with the mixed mask is recorded next to it"""
    name = "ragged16"
    H, Hkv, dh, lens = R.SETS[name]
    q, k, v = R.probe_inputs(H, Hkv, dh, lens)
    caught_by = []
    for causal in (True, False):
        for pat, keep in R.mask_patterns(lens).items():
            out = R.eager_bf16(q, k, v, H, Hkv, dh, lens, causal, dh ** -0.5, keep, mutant=mutant)
            if not torch.equal(out, probe_oracle(name, causal, pat, keep)):
                caught_by.append(f"{'causal' if causal else 'full'}/{pat}")
    random_bar = {}
    for causal in (True, False):
        qr, kr, vr, scale = R.random_inputs(name, causal)
        keep = R.mixed_mask(lens)
        ref = R.eager_bf16(qr, kr, vr, H, Hkv, dh, lens, causal, scale, keep)
        out = R.eager_bf16(qr, kr, vr, H, Hkv, dh, lens, causal, scale, keep, mutant=mutant)
        random_bar["causal" if causal else "full"] = "bits equal" if torch.equal(out, ref) else ("passes" if _passes_random_bar(out, ref) else "fails")
    print(f"mutant {mutant}: exact probe catches it in {len(caught_by)} of {2 * len(R.mask_patterns(lens))} probe cases "
          f"(first: {caught_by[:3]}); random-input bar: {random_bar}")
    record_parity(f"attn_mutant/{mutant}", caught_by_exact_probe="yes" if caught_by else "NO", probe_cases_differing=len(caught_by),
                  random_bar_causal=random_bar["causal"], random_bar_full=random_bar["full"])
    assert caught_by, mutant


def test_route_counter_words_and_pinned_kinds():
    import __graft_entry__ as g
    g.build()
    from procyon_amd import _lib
    lib = _lib.load()
    for which in (-1, 4, 5, 6, 20, 1 << 20, -(1 << 31)):
        assert lib.pcy_debug_attn_route_count(which) == 0, which
    assert [_lib.ATTN_ROUTE_DH32, _lib.ATTN_ROUTE_DH64, _lib.ATTN_ROUTE_LDS128_1, _lib.ATTN_ROUTE_LDS128_2] == [0, 1, 2, 3]
    for which in range(4):
        assert lib.pcy_debug_attn_route_count(which) >= 0
    assert lib.pcy_debug_dispatch_count(20) == 0 and _lib.ABI_VERSION == 13 and lib.pcy_abi_version() == 13
