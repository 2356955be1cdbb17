"""CPU: the host side of `UnifiedProCyon.forward(share_prefix=True)` -- `shared_prefix_plan` on the synthetic tokenizer -- and the ABI
numbers of the packed extension (pcy_attn_extend_packed / pcy_llama_extend_packed, dispatch kind 19).  No device is touched."""
import os
from types import SimpleNamespace

import pytest
import torch


@pytest.fixture(scope="module")
def host():
    """the tokenizer-side slice of UnifiedProCyon (no engine, no device)"""
    from procyon_amd.model import model_unified as MU
    from procyon_amd.tokenizer import SyntheticTokenizer
    tok = SyntheticTokenizer(n_text=2000, base_vocab=2048, bos_token_id=2040, eos_token_id=2041)
    ids = MU.special_token_ids(tok, "llama-3-8b")
    me = SimpleNamespace(tokenizer=tok, config=SimpleNamespace(max_text_len=64), use_llama_tokenizer=False, train_qa_full_lm=False, **ids)
    tokenize = lambda texts: MU.UnifiedProCyon._prepare_text_inputs_and_tokenize(me, list(texts), [[] for _ in texts], crop_off=True)
    return SimpleNamespace(MU=MU, tok=tok, me=me, tokenize=tokenize)


HEAD = "w1 w2 <|protein|> binds <|protein|> ? [ANSWER] yes w3 w4 <|protein|> binds"
ROWS = [HEAD + " <|protein|> ? [ANSWER]",
        HEAD + " <|protein|> w5 ? [ANSWER]",
        HEAD + " <|protein|> w5 w6 ? [ANSWER]",
        HEAD + " <|protein|> ? [ANSWER]"]
SRC = [[0, 1, 0, 2], [0, 1, 0, 3], [0, 1, 0, 4], [0, 1, 0, 5]]      # the receptor thrice, the peptide of the last slot differs


def _plan(host, rows=ROWS, src=SRC, ids_mask=None):
    ids, mask = host.tokenize(rows) if ids_mask is None else ids_mask
    me = host.me
    p = host.MU.shared_prefix_plan(ids, mask, src, me.answer_idx, (me.prot_replacement_idx, me.drug_idx), host.tok.pad_token_id)
    return p, ids, mask


def _check_reassembly(p, ids, mask):
    """prefix || suffix gives back every row up to its answer position; answer_rows address the answer token of the suffix batch"""
    Tp, S, B = p["Tp"], p["S"], p["B"]
    assert p["suffix_ids"].shape == p["suffix_mask"].shape == (B, S) and S >= 1
    for r in range(B):
        ap = int(p["answer_pos"][r])
        n = int(p["suffix_mask"][r].sum())
        assert p["suffix_mask"][r].tolist() == [1] * n + [0] * (S - n)                       # right-padded
        assert ids[0, :Tp].tolist() + p["suffix_ids"][r, :n].tolist() == ids[r, :ap + 1].tolist()
        assert ids[r, :Tp].tolist() == ids[0, :Tp].tolist() and bool(mask[r, :Tp].all())
        assert int(p["answer_rows"][r]) == r * S + ap - Tp and ap - Tp == n - 1
    assert p["answer_rows"].dtype == torch.int32
    assert S == int(p["suffix_mask"].sum(1).max())


def test_cut_at_a_differing_slot_source(host):
    """the ids of the rows agree far beyond the cut: the last <|protein|> slot holds another peptide in every row"""
    p, ids, mask = _plan(host)
    me = host.me
    slots = (ids[0] == me.prot_replacement_idx).nonzero()[:, 0].tolist()
    assert len(slots) == 4 and p["Tp"] == slots[3]
    assert bool((ids[:, :slots[3] + 1] == ids[0, :slots[3] + 1]).all())                      # ... the ids alone would have cut later
    assert p["S"] == 5 and p["suffix_mask"].sum(1).tolist() == [3, 4, 5, 3]                   # ragged: right pads in the suffixes
    assert [int(x) for x in p["answer_pos"]] == [int((ids[r] == me.answer_idx).nonzero().max()) for r in range(4)]
    _check_reassembly(p, ids, mask)


def test_cut_at_the_first_differing_token(host):
    """equal sources everywhere: the cut is the first column whose token differs"""
    p, ids, mask = _plan(host, src=[[0, 1, 0, 2]] * 4)
    first = next(t for t in range(ids.shape[1]) if not bool((ids[:, t] == ids[0, t]).all()))
    assert p["Tp"] == first and first > int((ids[0] == host.me.prot_replacement_idx).nonzero()[3, 0])
    _check_reassembly(p, ids, mask)
    # an earlier slot that differs wins over the later token
    p2, _, _ = _plan(host, src=[[0, 1, 0, 2], [0, 1, 0, 2], [0, 9, 0, 2], [0, 1, 0, 2]])
    assert p2["Tp"] == int((ids[0] == host.me.prot_replacement_idx).nonzero()[1, 0])
    _check_reassembly(p2, ids, mask)


def test_cut_is_clamped_to_the_earliest_answer(host):
    """rows that agree up to and beyond an [ANSWER]: every answer row must lie in the suffix, so the cut stops at the earliest one"""
    rows = ["w1 w2 w3 [ANSWER]", "w1 w2 w3 [ANSWER]", "w1 w2 w3 [ANSWER]"]
    p, ids, mask = _plan(host, rows=rows, src=[[], [], []])                                  # an identical batch
    ap = int((ids[0] == host.me.answer_idx).nonzero().max())
    assert p["Tp"] == ap and p["S"] == 1 and p["answer_rows"].tolist() == [0, 1, 2]
    assert p["suffix_ids"].tolist() == [[host.me.answer_idx]] * 3
    _check_reassembly(p, ids, mask)
    # the LAST [ANSWER] of a row counts, and the minimum over the rows
    rows = ["w1 [ANSWER] yes w2 [ANSWER]", "w1 [ANSWER] yes w2 [ANSWER] no w2 [ANSWER]"]
    p, ids, mask = _plan(host, rows=rows, src=[[], []])
    a0 = int((ids[0] == host.me.answer_idx).nonzero().max())
    assert p["Tp"] == a0 and p["S"] == int((ids[1] == host.me.answer_idx).nonzero().max()) - a0 + 1
    _check_reassembly(p, ids, mask)


def test_one_row(host):
    p, ids, mask = _plan(host, rows=ROWS[2:3], src=SRC[2:3])
    ap = int((ids[0] == host.me.answer_idx).nonzero().max())
    assert (p["B"], p["Tp"], p["S"]) == (1, ap, 1) and p["answer_rows"].tolist() == [0]
    _check_reassembly(p, ids, mask)


def test_nothing_shared(host):
    """Tp = 0: the first column already differs (no bos in common), or the rows' first slot differs under a leading slot"""
    ids, mask = host.tokenize(["w1 w2 [ANSWER]", "w1 w2 w3 [ANSWER]"])
    ids = ids.clone()
    ids[1, 0] = 7
    p, _, _ = _plan(host, src=[[], []], ids_mask=(ids, mask))
    assert p["Tp"] == 0 and p["S"] == int(p["answer_pos"].max()) + 1
    _check_reassembly(p, ids, mask)
    ids, mask = host.tokenize(["<|protein|> w2 [ANSWER]", "<|protein|> w2 [ANSWER]"])
    p, _, _ = _plan(host, src=[[0], [1]], ids_mask=(ids[:, 1:], mask[:, 1:]))                 # (the bos column dropped)
    assert p["Tp"] == 0
    _check_reassembly(p, ids[:, 1:], mask[:, 1:])


def test_errors(host):
    me, tok = host.me, host.tok
    with pytest.raises(ValueError, match=r"no \[ANSWER\]"):
        _plan(host, rows=["w1 w2 [ANSWER]", "w1 w2"], src=[[], []])
    ids, mask = host.tokenize(["w1 w2 [ANSWER]", "w1 w2 w3 w4 [ANSWER]"])
    bad = mask.clone()
    bad[0, 1] = 0                                                                            # a hole: not right-padded
    with pytest.raises(ValueError, match="right-padded"):
        _plan(host, src=[[], []], ids_mask=(ids, bad))
    # an [ANSWER] that only stands among the pads does not count
    ids2 = ids.clone()
    ids2[0, int((ids[0] == me.answer_idx).nonzero().max())] = 5
    ids2[0, -1] = me.answer_idx
    assert not bool(mask[0, -1])
    with pytest.raises(ValueError, match=r"row 0: no \[ANSWER\]"):
        _plan(host, src=[[], []], ids_mask=(ids2, mask))
    with pytest.raises(ValueError, match="sources"):
        _plan(host, src=[[0, 1, 0], [0, 1, 0, 3], [0, 1, 0, 4], [0, 1, 0, 5]])
    with pytest.raises(ValueError, match="slot source lists"):
        _plan(host, src=SRC[:3])


def test_pair_workload_chunk_cuts_in_front_of_the_peptide():
    """a configs[4] chunk (`workloads.config5_inputs`) on the full-size synthetic tokenizer: 64 rows that share everything but the peptide of the
    last slot -> the cut lies at that slot, three tokens per row remain, no suffix mask is needed; and the token rows through the layers that
    DESIGN.md section 4.7 quotes: B T for `forward` against Tp + B S"""
    from procyon_amd import workloads
    from procyon_amd.model import model_unified as MU
    from procyon_amd.tokenizer import SyntheticTokenizer
    tok = SyntheticTokenizer()
    sp = MU.special_token_ids(tok, "llama-3-8b")
    me = SimpleNamespace(tokenizer=tok, config=SimpleNamespace(max_text_len=2048), **sp)
    make, n_words = workloads.config5_inputs(256, 64)
    inp = make(64)                                                                           # the second chunk
    B = len(inp["instructions"])
    ids, mask = MU.UnifiedProCyon._prepare_text_inputs_and_tokenize(me, list(inp["instructions"]), [[] for _ in range(B)])
    T = int(mask.sum(1).max())
    assert B == 64 and T == n_words + 2 and bool((mask.sum(1) == T).all())                   # bos + the words + eos
    src = MU.UnifiedProCyon._slot_sources(me, inp, ids[:, :T])
    assert src[5] == [("seq", 0), ("seq", 1), ("seq", 0), ("seq", 2), ("seq", 0), ("seq", 3 + 64 + 5)]
    p = MU.shared_prefix_plan(ids[:, :T], mask[:, :T], src, me.answer_idx, (me.prot_replacement_idx, me.drug_idx), tok.pad_token_id)
    last_slot = int((ids[0] == me.prot_replacement_idx).nonzero()[-1, 0])
    assert p["Tp"] == last_slot == T - 4 and p["S"] == 3                                     # <|protein|> ? [ANSWER], then eos
    assert p["suffix_ids"][:, 0].tolist() == [me.prot_replacement_idx] * B and p["suffix_ids"][:, 2].tolist() == [me.answer_idx] * B
    assert bool(p["suffix_mask"].all()) and p["answer_rows"].tolist() == [3 * b + 2 for b in range(B)]
    assert (T, p["Tp"]) == (439, 435)
    assert (B * T, p["Tp"] + B * p["S"]) == (28096, 627)
    _check_reassembly(p, ids[:, :T], mask[:, :T])
    # the same receptor under another index is another source: the cut moves to the first slot that differs
    src2 = [list(s) for s in src]
    src2[7][2] = ("seq", 9)
    p2 = MU.shared_prefix_plan(ids[:, :T], mask[:, :T], src2, me.answer_idx, (me.prot_replacement_idx, me.drug_idx), tok.pad_token_id)
    assert p2["Tp"] == int((ids[0] == me.prot_replacement_idx).nonzero()[2, 0])


def test_abi_symbols_and_dispatch_index():
    from procyon_amd import _lib
    lib = _lib.load()
    assert _lib.DISPATCH_EXTEND_PACKED == 19 and _lib.DISPATCH_EXTEND == 18
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND_PACKED) >= 0      # a valid index (its count depends on what ran in this process)
    assert lib.pcy_debug_dispatch_count(20) == 0                               # ... and the first invalid one: always 0
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "pcy_internal.h")).read()
    assert "PCY_DISPATCH_EXTEND_PACKED = 19" in src and "PCY_DISPATCH_N = 20" in src
    for name, twin in (("pcy_attn_extend_packed", "pcy_attn_extend"), ("pcy_llama_extend_packed", "pcy_llama_extend")):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[twin]                  # the arguments of the unpacked entry
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "pcy.h")).read()
    assert "int pcy_attn_extend_packed(" in hdr and "int pcy_llama_extend_packed(" in hdr


def test_public_signatures_default_to_the_existing_paths():
    import inspect
    from procyon_amd.engine import Context, LlamaEngine
    from procyon_amd.model.model_unified import UnifiedProCyon
    from procyon_amd import workloads
    dflt = lambda f, n: inspect.signature(f).parameters[n].default
    assert dflt(Context.attn_extend, "packed") is False and dflt(LlamaEngine.extend, "packed") is False
    assert dflt(UnifiedProCyon.score_candidates, "packed") is False
    assert dflt(UnifiedProCyon.forward, "share_prefix") is False and dflt(UnifiedProCyon.forward, "packed") is True
    assert dflt(workloads.score_pairs, "share_prefix") is False
