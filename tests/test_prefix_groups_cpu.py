"""CPU: the host side of the grouped shared-prefix extension -- `shared_prefix_groups` (forward(share_prefix="groups")) and
`candidate_plan_groups` (score_candidates(ragged=True)) on the synthetic tokenizer, the host-side refusals of `KVCache.grouped`, and the
symbols of the grouped entries.  No device is touched."""
import inspect
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
    label_rule = lambda x: MU.UnifiedProCyon._full_labels(me, x)
    return SimpleNamespace(MU=MU, tok=tok, me=me, tokenize=tokenize, label_rule=label_rule)


HEAD_A = "w1 w2 <|protein|> binds <|protein|> ? [ANSWER] yes w3 w4 <|protein|> binds"       # receptor A: three slots in front of the peptide's
HEAD_B = "w9 <|protein|> binds"                                                             # receptor B: a shorter prefix
TAILS = ["", "w5 ", "w5 w6 "]
A = [HEAD_A + " <|protein|> " + t + "? [ANSWER]" for t in TAILS]
B_ = [HEAD_B + " <|protein|> " + t + "? [ANSWER]" for t in TAILS[:2]]
ONE = "w7 w8 w9 w10 w11 [ANSWER]"                                                           # a singleton without any slot
# interleaved in row order: A0 B0 ONE A1 B1 A2
ROWS = [A[0], B_[0], ONE, A[1], B_[1], A[2]]
SRC = [[0, 1, 0, 2], [5, 10], [], [0, 1, 0, 3], [5, 11], [0, 1, 0, 4]]
MEMBERS = [[0, 3, 5], [1, 4], [2]]


def _args(host):
    me = host.me
    return me.answer_idx, (me.prot_replacement_idx, me.drug_idx), host.tok.pad_token_id


def _groups(host, rows=ROWS, src=SRC, ids_mask=None):
    ids, mask = host.tokenize(rows) if ids_mask is None else ids_mask
    return host.MU.shared_prefix_groups(ids, mask, src, *_args(host)), ids, mask


def test_interleaved_receptors_and_a_singleton(host):
    g, ids, mask = _groups(host)
    MU = host.MU
    # groups in first-appearance order, the rows sorted by group (stable), order / inverse permutations of each other
    assert g["n_groups"] == 3 and g["B"] == 6 and g["group_rows"] == [3, 2, 1] and g["prefix_rows"] == [0, 1, 2]
    assert g["order"].tolist() == [0, 3, 5, 1, 4, 2]
    assert sorted(g["order"].tolist()) == list(range(6)) and g["inverse"][g["order"]].tolist() == list(range(6))
    assert g["order"][g["inverse"]].tolist() == list(range(6))
    # the cut of a group = shared_prefix_plan of the group's rows
    subs = [MU.shared_prefix_plan(ids[m], mask[m], [SRC[r] for r in m], *_args(host)) for m in MEMBERS]
    assert g["group_len"] == [p["Tp"] for p in subs]
    slots_a = (ids[0] == host.me.prot_replacement_idx).nonzero()[:, 0].tolist()
    slots_b = (ids[1] == host.me.prot_replacement_idx).nonzero()[:, 0].tolist()
    ans = lambda r: int((ids[r] == host.me.answer_idx).nonzero().max())
    assert g["group_len"] == [slots_a[3], slots_b[1], ans(2)] and len(set(g["group_len"])) == 3
    assert g["prefix_T"] == slots_a[3]
    # the singleton shares everything in front of its [ANSWER] with itself: one suffix token
    assert subs[2]["S"] == 1 and g["suffix_mask"][5].tolist() == [1, 0, 0, 0, 0]
    assert g["S"] == max(p["S"] for p in subs) == 5
    # ragged suffix masks, in sorted order; prefix || suffix gives every row back up to its answer
    assert g["suffix_mask"].sum(1).tolist() == [3, 4, 5, 3, 4, 1]
    assert g["answer_rows"].dtype == torch.int32
    i = 0
    for gi, m in enumerate(MEMBERS):
        for r in m:
            n, L = int(g["suffix_mask"][i].sum()), g["group_len"][gi]
            assert g["order"][i] == r and g["suffix_mask"][i].tolist() == [1] * n + [0] * (g["S"] - n)
            assert ids[m[0], :L].tolist() + g["suffix_ids"][i, :n].tolist() == ids[r, :ans(r) + 1].tolist()
            assert int(g["answer_rows"][i]) == i * g["S"] + ans(r) - L and ans(r) - L == n - 1
            assert g["suffix_ids"][i, n:].tolist() == [host.tok.pad_token_id] * (g["S"] - n)
            i += 1
    assert g["answer_pos"].tolist() == [ans(r) for r in range(6)]                           # caller order


def test_one_group_reproduces_shared_prefix_plan(host):
    rows, src = [A[0], A[1], A[2], A[0]], [[0, 1, 0, 2], [0, 1, 0, 3], [0, 1, 0, 4], [0, 1, 0, 5]]
    g, ids, mask = _groups(host, rows=rows, src=src)
    p = host.MU.shared_prefix_plan(ids, mask, src, *_args(host))
    assert g["n_groups"] == 1 and g["group_rows"] == [4] and g["group_len"] == [p["Tp"]] and g["prefix_T"] == p["Tp"] and g["prefix_rows"] == [0]
    assert g["order"].tolist() == g["inverse"].tolist() == [0, 1, 2, 3]
    assert (g["S"], g["B"]) == (p["S"], p["B"])
    for k in ("suffix_ids", "suffix_mask", "answer_pos", "answer_rows"):
        assert torch.equal(g[k], p[k]) and g[k].dtype == p[k].dtype, k


def test_rows_that_differ_only_in_a_slot_source_split(host):
    """the same text four times; the receptor slot (third) reads another protein in rows 1 and 3"""
    rows = [A[0]] * 4
    src = [[0, 1, 0, 2], [0, 1, 7, 3], [0, 1, 0, 4], [0, 1, 7, 5]]
    g, ids, _ = _groups(host, rows=rows, src=src)
    slot3 = int((ids[0] == host.me.prot_replacement_idx).nonzero()[3, 0])
    assert g["n_groups"] == 2 and g["order"].tolist() == [0, 2, 1, 3] and g["group_rows"] == [2, 2] and g["prefix_rows"] == [0, 1]
    assert g["group_len"] == [slot3, slot3]
    # ... while another source in the LAST slot in front of [ANSWER] (the peptide) does not: that slot lies behind the key
    g1, _, _ = _groups(host, rows=rows, src=[[0, 1, 0, 2 + i] for i in range(4)])
    assert g1["n_groups"] == 1
    # a group whose rows share nothing: group_len 0 is reported, not hidden (forward then takes the ordinary path)
    ids2, mask2 = host.tokenize(["<|protein|> w2 [ANSWER]", "<|protein|> w2 [ANSWER]"])
    g2, _, _ = _groups(host, src=[[0], [1]], ids_mask=(ids2[:, 1:], mask2[:, 1:]))
    assert g2["n_groups"] == 1 and g2["group_len"] == [0]


def test_errors_are_those_of_shared_prefix_plan(host):
    me = host.me
    with pytest.raises(ValueError, match=r"no \[ANSWER\]"):
        _groups(host, rows=["w1 w2 [ANSWER]", "w1 w2"], src=[[], []])
    ids, mask = host.tokenize(["w1 w2 [ANSWER]", "w1 w2 w3 w4 [ANSWER]"])
    bad = mask.clone()
    bad[0, 1] = 0
    with pytest.raises(ValueError, match="right-padded"):
        _groups(host, src=[[], []], ids_mask=(ids, bad))
    ids2 = ids.clone()
    ids2[0, int((ids[0] == me.answer_idx).nonzero().max())] = 5
    ids2[0, -1] = me.answer_idx                                                            # an [ANSWER] among the pads does not count
    with pytest.raises(ValueError, match=r"row 0: no \[ANSWER\]"):
        _groups(host, src=[[], []], ids_mask=(ids2, mask))
    with pytest.raises(ValueError, match="sources"):
        _groups(host, src=[[0, 1, 0]] + SRC[1:])
    with pytest.raises(ValueError, match="slot source lists"):
        _groups(host, src=SRC[:5])


# ---- candidate_plan_groups --------------------------------------------------------------------------------------------------------------
INSTR = ["w1 <|protein|> is w2 ? [ANSWER]", "describe w8 <|protein|> and <|protein|> now please [ANSWER]", "w4 [ANSWER]"]
CANDS = [["yes w3 w4 w5"], ["beta gamma", "yes", "w3 w4 w5 w6 w7 w8"], ["alpha", "q r"]]


def _cplan(host, instr=INSTR, cands=CANDS):
    return host.MU.candidate_plan_groups(host.tokenize, host.label_rule, instr, cands, host.me.answer_idx, host.tok.pad_token_id)


def test_candidate_plan_groups_ragged_lists(host):
    tok, me = host.tok, host.me
    p = _cplan(host)
    enc = lambda s: tok.encode(s, add_special_tokens=False)
    pre = [[tok.bos_token_id] + enc(i)[:-1] for i in INSTR]
    assert (p["P"], p["Nmax"], p["R"]) == (3, 3, 6) and p["group_rows"] == [1, 3, 2] and p["n_candidates"].tolist() == [1, 3, 2]
    assert p["group_len"] == [len(x) for x in pre] and len(set(p["group_len"])) == 3 and p["Tp"] == max(p["group_len"])
    for i in range(3):                                                                      # RIGHT-padded: the prompt starts at position 0
        pad = p["Tp"] - len(pre[i])
        assert p["prefix_ids"][i].tolist() == pre[i] + [tok.pad_token_id] * pad
        assert p["prefix_mask"][i].tolist() == [1] * len(pre[i]) + [0] * pad
    assert p["row_of"].tolist() == [[0, -1, -1], [1, 2, 3], [4, 5, -1]]
    r = 0
    for i in range(3):
        for n, c in enumerate(CANDS[i]):
            suf = [me.answer_idx] + enc(" " + c) + [tok.eos_token_id]
            assert int(p["cut"][r]) == len(pre[i])
            assert p["suffix_ids"][r].tolist() == suf + [tok.pad_token_id] * (p["S"] - len(suf))
            assert p["suffix_mask"][r].tolist() == [1] * len(suf) + [0] * (p["S"] - len(suf))
            assert p["suffix_labels"][r].tolist() == [-100] + suf[1:] + [-100] * (p["S"] - len(suf))
            r += 1
    # n_tokens: what candidate_plan gives for every prompt run alone with its own list; 0 in the padding
    for i in range(3):
        alone = host.MU.candidate_plan(host.tokenize, host.label_rule, [INSTR[i]], [CANDS[i]], me.answer_idx, tok.pad_token_id)
        n = len(CANDS[i])
        assert p["n_tokens"][i, :n].tolist() == alone["n_tokens"][0].tolist() and p["n_tokens"][i, n:].tolist() == [0] * (3 - n)
        rows = p["row_of"][i, :n]
        assert torch.equal(p["suffix_ids"][rows][:, :alone["S"]], alone["suffix_ids"]) and torch.equal(p["suffix_labels"][rows][:, :alone["S"]], alone["suffix_labels"])
        assert bool((p["suffix_mask"][rows][:, alone["S"]:] == 0).all())


def test_candidate_plan_groups_rejects(host):
    with pytest.raises(ValueError, match="at least one candidate"):
        _cplan(host, cands=[["a"], [], ["b"]])
    with pytest.raises(ValueError, match="candidate lists"):
        _cplan(host, cands=[["a", "b"]])
    with pytest.raises(ValueError, match="share its prefix"):
        _cplan(host, cands=[["yes"], ["a", "w9 [ANSWER] no", "x"], ["b", "c"]])
    with pytest.raises(ValueError, match=r"no \[ANSWER\]"):
        _cplan(host, instr=["w1 w2", INSTR[1], INSTR[2]])
    # the uniform planner keeps its own refusal of ragged lists
    with pytest.raises(ValueError, match="same number of candidates"):
        host.MU.candidate_plan(host.tokenize, host.label_rule, INSTR, CANDS, host.me.answer_idx, host.tok.pad_token_id)


# ---- the grouped cache's host checks, the symbols, the defaults --------------------------------------------------------------------------
def test_grouped_cache_host_checks():
    from procyon_amd.engine import KVCache, LlamaConfig
    cfg = LlamaConfig(vocab=16, d=128, n_layers=1, n_heads=2, n_kv_heads=1, ffn=64)
    prefix = KVCache(cfg, 2, 10, "cpu")
    ok = KVCache.grouped(cfg, "cpu", prefix, [3, 1], [10, 4], 5)
    assert ok.is_grouped and ok.B == 4 and ok.rows_per_prefix == 0 and ok.c.rows_per_prefix == 0 and ok.capacity == 15
    assert ok.row_group == [0, 0, 0, 1] and ok.row_len().tolist() == [10, 10, 10, 4]
    assert ok.d_row0.tolist() == [0, 3, 4] and ok.d_len.tolist() == [10, 4] and ok.d_row_grp.tolist() == [0, 0, 0, 1]
    ga = ok.groups_arg(2)
    assert (ga.n_groups, ga.t_own) == (2, 2) and [ga.rows[i] for i in range(2)] == [3, 1] and [ga.len[i] for i in range(2)] == [10, 4]
    assert not prefix.is_grouped
    k, v = ok.layer(0, 2)                                                                   # the logical rows, per row
    assert [tuple(x.shape) for x in k] == [(1, 12, 64)] * 3 + [(1, 6, 64)] and len(v) == 4
    for rows, lens, slots, match in [([3, 1, 1], [10, 4, 4], 5, "groups on a prefix cache"), ([3, 0], [10, 4], 5, "at least one row"),
                                     ([3, 1], [10, 11], 5, "outside"), ([3, 1], [0, 4], 5, "outside"), ([3, 1], [10], 5, "group_rows for"),
                                     ([], [], 5, "at least one group"), ([3, 1], [10, 4], 0, "suffix_slots")]:
        with pytest.raises(ValueError, match=match):
            KVCache.grouped(cfg, "cpu", prefix, rows, lens, slots)
    with pytest.raises(ValueError, match="plain cache"):
        KVCache.grouped(cfg, "cpu", ok, [1], [4], 5)


def test_symbols_and_defaults():
    from procyon_amd import _lib, workloads
    from procyon_amd.engine import Context, LlamaEngine
    from procyon_amd.model.model_unified import UnifiedProCyon
    lib = _lib.load()
    for name in ("pcy_attn_extend_grouped", "pcy_llama_extend_grouped", "pcy_debug_extend_grouped_count"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.pcy_debug_extend_grouped_count() >= 0
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "pcy.h")).read()
    assert "} pcy_prefix_groups;" in hdr and "int pcy_attn_extend_grouped(" in hdr and "int pcy_llama_extend_grouped(" in hdr
    dflt = lambda f, n: inspect.signature(f).parameters[n].default
    assert dflt(Context.attn_extend, "groups") is None and dflt(LlamaEngine.extend, "own_past") is None and dflt(LlamaEngine.extend, "t_past") is None
    assert dflt(UnifiedProCyon.score_candidates, "ragged") is False and dflt(UnifiedProCyon.forward, "share_prefix") is False
    assert dflt(workloads.score_pairs, "share_prefix") is False
