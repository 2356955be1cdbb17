"""CPU: the references and fixtures of the fp32 stream step (tests/f32_stream_ref.py) hold what the GPU tests demand of the kernels --
plain torch fp32 meets the single-operator bars on every case (the bars are reachable by the reference alone), the greedy fixture's
top-2 margins and the beam fixture's selection gaps are wide enough for token equality to be a fair demand, and the ABI binds the new
entries."""
import pytest
import torch

import f32_ref as R
import f32_stream_ref as S

F32 = torch.float32


@pytest.mark.parametrize("epi", list(S.EPIS))
def test_plain_fp32_meets_the_gemv_bars(epi):
    for name in S.gemv_cases(epi):
        c = S.gemv_case(epi, name)
        ref = S.gemv(c["x"], c["W"], c["W2"], c["resid"], S.EPIS[epi])
        got = S.gemv(c["x"], c["W"], c["W2"], c["resid"], S.EPIS[epi], dt=F32)
        assert got.dtype == F32 and ref.dtype == torch.float64
        assert R.rel64(got, ref) < R.OP_BAR and R.maxabs64(got, ref) < R.OP_MAXABS, (epi, name, R.rel64(got, ref), R.maxabs64(got, ref))


def test_gemv_cases_reach_the_loop_edges():
    for epi in S.EPIS:
        P, cs = S.GEMV_PASS[epi], S.gemv_cases(epi)
        ks = {k for _, _, k in cs.values()}
        assert {S.GEMV_KSTEP, P, P + S.GEMV_KSTEP} <= ks and any(k % 16 for k in ks) and any(k >= 4 * P for k in ks)
        ns = {n for _, n, _ in cs.values()}
        assert {S.GEMV_ROWS - 1, S.GEMV_ROWS + 1} <= ns and any(n % 4 for n in ns)
        assert {1, S.GEMV_WIDEST, S.GEMV_WIDEST + 1, 32, 33, 16, 17} <= {b for b, _, _ in cs.values()}
        assert all(k % 4 == 0 for k in ks)


@pytest.mark.parametrize("H,Hkv,dh", R.DECODE_GEOMS)
def test_plain_fp32_meets_the_attention_bars(H, Hkv, dh):
    for t in S.ATTN_POS + ((S.ATTN_POS_LONG,) if dh == 64 else ()):
        c = S.attn_pos_case(t, H, Hkv, dh)
        args = (c["qkv"], c["kc"], c["vc"], t, c["cos"], c["sin"], H, Hkv, dh, dh ** -0.5)
        o64, k64, v64 = S.attn_decode_pos(*args)
        o32, k32, v32 = S.attn_decode_pos(*args, dt=F32)
        assert not torch.isnan(o64).any() and torch.isnan(k64[:, t + 1:]).all()        # slot t was written, the NaN above it never read
        assert R.rel64(o32, o64) < R.OP_BAR and R.maxabs64(o32, o64) < R.OP_MAXABS, (t, R.rel64(o32, o64))
        assert R.rel64(k32[:, t], k64[:, t]) < R.OP_BAR and torch.equal(v32[:, t].double(), v64[:, t])
        # S == 1 restated through the family's own references: rope + the cache write + attn_decode over t + 1 slots
        pos = torch.full((3,), t, dtype=torch.int32)
        r = R.rope(c["qkv"], 0, H, dh, pos, c["cos"], c["sin"])
        r = R.rope(r, H * dh, Hkv, dh, pos, c["cos"], c["sin"])
        assert torch.equal(r[:, H * dh:(H + Hkv) * dh], k64[:, t])


@pytest.fixture(scope="module")
def gen():
    return S.gen_fixture()


def test_greedy_fixture_margins_allow_token_equality(gen):
    """the oracle's smallest top-2 margin on the padded greedy fixture, over the row's norm: >= 1e-3, ten times the 1e-4 logits bar"""
    m = S.top2_margins(gen["logits"])
    print("top-2 margins / norm per row and step:\n", m)
    assert tuple(m.shape) == (R.GEN_B, R.GEN_STEPS) and float(m.min()) >= S.TOKEN_MARGIN, float(m.min())
    assert torch.equal(gen["logits"].argmax(-1), gen["toks"])
    # the summed fp32 log-softmax the device loop is compared with
    lp = gen["logits"].log_softmax(-1).gather(2, gen["toks"][..., None])[..., 0].sum(1)
    assert torch.allclose(lp, gen["logprob"], atol=1e-5)


def test_beam_fixture_gaps_allow_token_equality(gen):
    """diverse beam search over two prompts on the fixture's model (one left-padded), the engine-level beam case of the GPU test: the
    oracle's smallest gap between the last selected and the first rejected candidate per group and step exceeds 2e-4 x the row norm.
    (The model-level case needs the synthetic model, which is built on a GPU: tests/test_gpu_f32_stream.py asserts the same condition on
    the oracle's run, on the CPU, before it compares.)"""
    emb, mask = S.beam_fixture(gen)
    t, s, lg, rel = S.beam_oracle(gen["sd"], gen["geom"], emb, mask, eos_id=2, **S.BEAM_KW)
    print("smallest selection gap / row norm:", rel)
    assert rel > S.BEAM_GAP, rel
    assert tuple(t.shape) == (2, S.BEAM_KW["beam_size"], S.BEAM_KW["max_len"])


def test_abi_binds_the_stream_entries():
    import os
    import re
    import __graft_entry__ as g
    g.build()
    from procyon_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcy.h")).read()
    for n in ("pcy_f32_gemv", "pcy_f32_attn_decode_pos", "pcy_f32_llama_decode", "pcy_f32_llama_decode_graph", "pcy_f32_greedy_pick",
              "pcy_f32_llama_greedy", "pcy_debug_f32_stream_count"):
        assert n in _lib.SIGNATURES and hasattr(lib, n) and re.search(rf"\b{n}\(", header), n
    assert lib.pcy_debug_f32_stream_count() >= 0
    # host arithmetic only: the descriptor structs have the header's field order
    assert [f for f, _ in _lib.LlamaLayerF32._fields_] == ["wqkv", "wo", "wg", "wu", "wd", "ln1", "ln2"]
    assert [f for f, _ in _lib.KvCacheF32._fields_] == ["k", "v", "B", "Tmax"]
    from procyon_amd.model.model_unified import UnifiedProCyon
    from procyon_amd import pipelines
    import inspect
    for fn in (UnifiedProCyon.generate, pipelines.caption_bulk):
        assert inspect.signature(fn).parameters["decode_f32"].default == "ops"
