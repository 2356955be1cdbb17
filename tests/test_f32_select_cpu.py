"""CPU: the float64 helpers and fixtures of the fp32 selection kernels (tests/f32_select_ref.py) -- the helpers agree with the oracle's
own restatements on inputs without near-ties, the fixtures the GPU tests run on are decidable from the float64 reference alone (nucleus
rows hold at most BAND_CAP tokens within DELTA of the threshold; every beam selection is an exact tie or a clear gap), and the ABI binds
the new entries with every default unchanged."""
import inspect
import os
import re

import pytest
import torch

import f32_select_ref as Q
from select_oracle import softmax64

F32 = torch.float32
NEW = {"pcy_f32_beam_step": 8, "pcy_f32_kv_reorder_range": 7, "pcy_f32_kv_copy_rows": 7, "pcy_f32_llama_beam_steps": 12, "pcy_f32_sample_pick": 10,
       "pcy_f32_llama_sample": 10, "pcy_debug_f32_select_count": 1}


def test_abi_binds_the_select_entries_and_defaults_stay():
    import __graft_entry__ as g
    g.build()
    from procyon_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pcy.h")).read()
    for n, nargs in NEW.items():
        assert n in _lib.SIGNATURES and hasattr(lib, n) and re.search(rf"\b{n}\(", header), n
        assert len(_lib.SIGNATURES[n][1]) == nargs, n
    # header, binding and library agree on the ABI number (it stays where the suite's older files pin it: the entries are additions)
    m = re.search(r"#define PCY_ABI_VERSION (\d+)\b", header)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == lib.pcy_abi_version()
    assert lib.pcy_debug_f32_select_count(0) >= 0 and lib.pcy_debug_f32_select_count(1) >= 0 and lib.pcy_debug_f32_select_count(2) == 0
    from procyon_amd import pipelines
    from procyon_amd.engine_f32 import GenStateF32, LlamaEngineF32
    from procyon_amd.model.model_unified import UnifiedProCyon
    for fn in (UnifiedProCyon.generate, pipelines.caption_bulk, UnifiedProCyon._generate_beam_search_f32, UnifiedProCyon._generate_sampling_f32):
        assert inspect.signature(fn).parameters["decode_f32"].default == "ops"
    assert {"pos", "next_tok"} <= set(inspect.signature(GenStateF32.__init__).parameters)
    for name in ("beam_step", "kv_reorder", "kv_copy_rows", "beam_steps", "sample_pick", "sample_steps", "generate_beam", "generate_sampling"):
        assert callable(getattr(LlamaEngineF32, name)), name
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "caption_bulk.py")).read()
    assert "--fp32_device" in src and "--fp32_stream" in src


@pytest.mark.parametrize("mode", list(Q.SAMPLE_MODES))
def test_sampling_helpers_agree_with_the_oracle(mode):
    """random fp32 rows (no equal probabilities, thresholds far from a cumulative mass): the float64 vector within fp32 rounding of the
    oracle's fp32 one, the same nucleus mask, the same token for every variate"""
    from oracle import llama_ref as LR
    temperature, nucleus = Q.SAMPLE_MODES[mode]
    rows = torch.randn(4, 97, generator=torch.Generator().manual_seed(5)) * 2.0
    p64, keep = Q.sampling_probs64(rows, temperature, nucleus)
    p32 = LR.sampling_probs(rows, temperature, nucleus)
    assert p32.dtype == F32 and torch.allclose(p32.double(), p64, rtol=1e-5, atol=1e-12)
    if nucleus is not None:
        assert int(Q.band_count(softmax64(rows), nucleus, 1e-4).max()) == 0
        assert torch.equal(LR.nucleus_mask(rows.softmax(-1), nucleus).bool(), keep)
        assert bool(keep.any(-1).all()) and not bool(keep.all())
    for u in Q.SAMPLE_US:
        uv = torch.full((4,), u, dtype=F32)
        cdf = p64.cumsum(-1)
        target = uv.double() * cdf[:, -1]
        if float((cdf - target[:, None]).abs().min()) > 1e-6:       # (the fp32 vector's CDF can only differ where a step lies this close)
            assert torch.equal(Q.sample_token64(p64, uv), LR.sample_token(p32, uv)), u


def test_nucleus_keep_is_stable_and_keeps_all_when_nothing_reaches():
    p = torch.tensor([[0.25, 0.25, 0.25, 0.25]], dtype=torch.float64)
    assert Q.nucleus_keep64(p, 0.5).tolist() == [[False, True, True, True]]       # cum 0.25, 0.5, ...: the second reaches 1 - 0.5
    assert Q.nucleus_keep64(p, 0.4).tolist() == [[False, False, True, True]]
    assert Q.nucleus_keep64(p * 0.1, 0.5).tolist() == [[True, True, True, True]]  # total mass 0.1 never reaches 0.5
    assert Q.nucleus_cum64(torch.tensor([[0.3, 0.1, 0.3, 0.3]], dtype=torch.float64)).tolist() == [[0.4, 0.1, 0.7, 1.0]]


def test_beam_helper_agrees_with_the_oracle():
    """oracle.llama_ref.beam_search on random fp32 tables (no ties): the same tokens, scores within fp32 rounding of the float64 ones"""
    from oracle import llama_ref as LR
    B, beam, g, V, steps, M = 2, 4, 2, 53, 5, Q.BEAM_M
    tab = torch.randn(steps, M, V, generator=torch.Generator().manual_seed(9)) * 2.0
    ref = Q.beam_search64(lambda i, nt: Q.table_step(tab, i, nt, B * beam), B, beam, g, V, steps, 0.8, eos_id=V - 1)
    assert min(gap for sel in ref["gaps"] for gap, _ in sel) > 1e-4
    state = {"i": 0}

    def enc(input_embeds=None, input_ids=None, attn_masks=None, past_key_values=None):
        i = state["i"]
        state["i"] += 1
        lg = Q.table_step(tab, i, None if input_ids is None else input_ids.view(-1), B * beam)
        past = [[torch.zeros(B * beam, 1, 1, 1), torch.zeros(B * beam, 1, 1, 1)]] if past_key_values is None else past_key_values
        return lg[:, None, :].clone(), past

    t, s, _ = LR.beam_search(enc, torch.zeros(B, 3, 8), torch.ones(B, 3), vocab_size=V, eos_id=V - 1, max_len=steps, beam_size=beam,
                             beam_group_size=g, diversity_penalty=0.8)
    assert torch.equal(t.view(B * beam, -1)[:, :ref["n"]], ref["tokens"])
    assert torch.allclose(s.view(-1).double(), ref["scores"], atol=1e-4)
    assert ref["pos"] == Q.BEAM_PROMPT + ref["n"] - 1 and tuple(ref["src"].shape) == (ref["n"], B * beam)


@pytest.mark.parametrize("V", Q.SAMPLE_V)
def test_nucleus_rows_hold_few_tokens_at_the_threshold(V):
    """every nucleus row of the GPU test: at most BAND_CAP tokens whose float64 ascending cumulative mass lies within DELTA of 1 - p"""
    p = softmax64(Q.sample_rows(V))
    for mode, (_, nucleus) in Q.SAMPLE_MODES.items():
        if nucleus is not None:
            n = Q.band_count(p, nucleus)
            print(V, mode, "tokens within DELTA of the threshold per row:", n.tolist())
            assert int(n.max()) <= Q.BAND_CAP, (V, mode, n.tolist())
    # the dominated row holds a token of probability > 0.999; every row a finite logit
    assert float(p[Q.SAMPLE_KINDS.index("dominated")].max()) > 0.999 and bool(torch.isfinite(Q.sample_rows(V)).any(-1).all())


@pytest.mark.parametrize("case", [c + (False, None) for c in Q.BEAM_CASES] + [Q.BEAM_MASKED + (True, None), Q.BEAM_DONE + (False, 2)],
                         ids=lambda c: "-".join(str(x) for x in c))
def test_beam_fixture_selections_are_decidable(case):
    """every beam case of the GPU test: the float64 gap between adjacent candidates among the first g + 1 of every selection is an exact
    tie (the index rule decides) or exceeds 4 x logprob_slack -- so tokens and parents are a fair demand"""
    c = Q.beam_case(*case)
    ref = c["ref"]
    assert Q.gaps_are_decidable(ref["gaps"])
    ties = sum(gap == 0.0 for sel in ref["gaps"] for gap, _ in sel)
    print("selections", len(ref["gaps"]), "pairs tied exactly", ties, "seeds tried", c["seeds"], "steps", ref["n"], "done", ref["done"])
    assert ties > 0 and bool(torch.isfinite(ref["scores"]).all())
    if case[-1] is not None:
        assert ref["done"] and ref["n"] == case[-1] + 1 < case[4]
