"""CPU: the host side of the cache extension (pcy_llama_extend / LlamaEngine.extend / UnifiedProCyon.score_candidates) -- the workspace
arithmetic, the ABI numbers and `candidate_plan` on the synthetic tokenizer.  No device is touched."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

FULL = dict(vocab=128263, d=4096, n_layers=32, n_heads=32, n_kv_heads=8, ffn=14336)


def _desc(max_pos=4096, **over):
    from procyon_amd import _lib
    g = dict(FULL, **over)
    d = _lib.LlamaDesc()
    d.vocab, d.d, d.n_layers, d.n_heads, d.n_kv_heads, d.ffn = g["vocab"], g["d"], g["n_layers"], g["n_heads"], g["n_kv_heads"], g["ffn"]
    d.head_dim, d.max_pos, d.rms_eps = g["d"] // g["n_heads"], max_pos, 1e-5
    return d


def test_abi_version_and_dispatch_index():
    from procyon_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 13 and lib.pcy_abi_version() == 13
    assert _lib.DISPATCH_EXTEND == 18
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND) == 0        # a valid index (nothing has run)
    assert lib.pcy_debug_dispatch_count(19) == 0                          # ... and the first invalid one
    for name in ("pcy_attn_extend", "pcy_llama_extend", "pcy_llama_extend_ws_bytes"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_workspace_depends_on_the_row_counts_only():
    """pcy_llama_extend_ws_bytes takes no past length, no cache: its arguments are (desc, B, S, logit rows, scored rows), and of the desc only
    the layer geometry counts -- not the rope table length, which bounds t_past + S."""
    from procyon_amd import _lib
    lib = _lib.load()
    assert _lib.SIGNATURES["pcy_llama_extend_ws_bytes"][1] == [C.POINTER(_lib.LlamaDesc), C.c_int, C.c_int, C.c_int, C.c_int]
    ws = lambda d, *a: int(lib.pcy_llama_extend_ws_bytes(C.byref(d), *a))
    base = ws(_desc(), 2, 32, 64, 62)
    assert base > 0
    assert ws(_desc(max_pos=512), 2, 32, 64, 62) == base == ws(_desc(max_pos=131072), 2, 32, 64, 62)
    assert ws(_desc(n_layers=2), 2, 32, 64, 62) == base                   # no per-layer buffer either
    # monotone in each count, zero for an empty call
    assert ws(_desc(), 4, 32, 64, 62) > base and ws(_desc(), 2, 32, 128, 62) > base and ws(_desc(), 2, 32, 64, 0) < base
    assert ws(_desc(), 0, 32, 0, 0) == 0 and ws(_desc(), 2, 0, 0, 0) == 0


def test_workspace_bytes_stay_within_the_slack_of_the_formula_they_replace():
    """The reported bytes are where the engine's own carve of the workspace ends (+ its 4096 bytes of slack); the values below are what the
    closed formula that carve replaced reported for the same calls.  The two may differ by alignment padding only, which the slack covers."""
    from procyon_amd import _lib
    lib = _lib.load()
    formula = {(2, 32, 64, 62): 18095872, (4, 32, 64, 62): 34873344, (2, 32, 128, 62): 18620160, (2, 32, 64, 0): 17338624,
               (1, 64, 64, 64): 18120192, (16, 4, 64, 64): 18120192}
    for args, was in formula.items():
        now = int(lib.pcy_llama_extend_ws_bytes(C.byref(_desc()), *args))
        assert abs(now - was) <= 4096, (args, now, was)


@pytest.mark.parametrize("B,S", [(1, 64), (2, 32), (16, 4)])
def test_workspace_is_below_one_copy_of_the_prefix(B, S):
    """B*S = 64 rows, logits and scores for all of them: the workspace stays below what ONE per-row copy of a 512-slot prefix (K and V,
    all layers) would take for the B rows -- the copy a transposed or un-shared prefix would need."""
    from procyon_amd import _lib
    lib = _lib.load()
    ws = int(lib.pcy_llama_extend_ws_bytes(C.byref(_desc()), B, S, B * S, B * S))
    g = FULL
    dh = g["d"] // g["n_heads"]
    copy = 2 * g["n_layers"] * g["n_kv_heads"] * 512 * dh * 2 * B
    assert 0 < ws < copy, f"extend workspace {ws} bytes at B={B} S={S} vs {copy} bytes for one row-copy of a 512-slot prefix K/V x {B} rows"


def test_rows_saved_arithmetic():
    """token rows through the layers: N (Tp + S) for the concatenated rows against Tp + N S with the prompt prefilled once"""
    rows = lambda P, N, Tp, S: (P * N * (Tp + S), P * Tp + P * N * S)
    assert rows(1, 16, 512, 32) == (8704, 1024)
    for P, N in [(1, 4), (1, 16), (1, 64), (4, 16)]:
        a, b = rows(P, N, 512, 32)
        assert a > b and abs(a / b - N * 544 / (512 + N * 32)) < 1e-12


# ---- candidate_plan on the synthetic tokenizer -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    """the tokenizer-side slice of UnifiedProCyon (no engine, no device): `_prepare_text_inputs_and_tokenize` and the label rule of `forward`"""
    from procyon_amd.model import model_unified as MU
    from procyon_amd.tokenizer import SyntheticTokenizer
    tok = SyntheticTokenizer(n_text=2000, base_vocab=2048, bos_token_id=2040, eos_token_id=2041)
    ids = MU.special_token_ids(tok, "llama-3-8b")
    me = SimpleNamespace(tokenizer=tok, config=SimpleNamespace(max_text_len=48), use_llama_tokenizer=False, train_qa_full_lm=False, **ids)
    tokenize = lambda texts: MU.UnifiedProCyon._prepare_text_inputs_and_tokenize(me, list(texts), [[] for _ in texts], crop_off=True)
    label_rule = lambda x: MU.UnifiedProCyon._full_labels(me, x)
    return SimpleNamespace(MU=MU, tok=tok, me=me, tokenize=tokenize, label_rule=label_rule)


INSTR = ["w1 <|protein|> is w2 ? [ANSWER]", "describe w8 <|protein|> and <|protein|> now please [ANSWER]"]
CANDS = [["yes w3 w4 w5", "alpha", "q r s t u v"], ["beta gamma", "yes", "w3 w4 w5 w6"]]


def _plan(host, instr=INSTR, cands=CANDS):
    return host.MU.candidate_plan(host.tokenize, host.label_rule, instr, cands, host.me.answer_idx, host.tok.pad_token_id)


def test_candidate_plan_cut_suffix_and_padding(host):
    tok, me = host.tok, host.me
    p = _plan(host)
    P, N = 2, 3
    assert (p["P"], p["N"]) == (P, N)
    enc = lambda s: tok.encode(s, add_special_tokens=False)
    pre = [[tok.bos_token_id] + enc(i)[:-1] for i in INSTR]                # bos + the instruction without its closing [ANSWER]
    assert p["Tp"] == max(len(x) for x in pre) and len(pre[0]) != len(pre[1])
    for i in range(P):
        pad = p["Tp"] - len(pre[i])
        assert p["prefix_ids"][i].tolist() == [tok.pad_token_id] * pad + pre[i]                    # LEFT-padded
        assert p["prefix_mask"][i].tolist() == [0] * pad + [1] * len(pre[i])
        for n in range(N):
            r = i * N + n
            assert int(p["cut"][r]) == len(pre[i])                                                # in front of [ANSWER]
            suf = [me.answer_idx] + enc(" " + CANDS[i][n]) + [tok.eos_token_id]                   # [ANSWER] + tokens + eos
            assert p["suffix_ids"][r].tolist() == suf + [tok.pad_token_id] * (p["S"] - len(suf))   # RIGHT-padded
            assert p["suffix_mask"][r].tolist() == [1] * len(suf) + [0] * (p["S"] - len(suf))
            assert p["suffix_labels"][r].tolist() == [-100] + suf[1:] + [-100] * (p["S"] - len(suf))
    assert p["S"] == max(len(enc(" " + c)) for cs in CANDS for c in cs) + 2
    assert bool((p["suffix_mask"].sum(1) < p["S"]).any())                  # the case has suffix pads at all


def test_candidate_plan_labels_equal_forwards_rule_on_the_concatenated_rows(host):
    """labels and n_tokens: what `forward` / `score_text` derive for the rows instruction + " " + candidate, restated from the whole row"""
    from procyon_amd.engine import score_plan
    p = _plan(host)
    texts = [INSTR[i] + " " + c for i in range(2) for c in CANDS[i]]
    ids, mask = host.tokenize(texts)
    full = host.label_rule(ids)
    real = int(mask.sum(1).max())
    n_ref = (full[:, 1:real] != -100).sum(1)                               # score_text's n_tokens
    assert p["n_tokens"].reshape(-1).tolist() == n_ref.tolist()
    rows, targets, bt = score_plan(full[:, :real], real, 4096)             # the rows the one-shot pass scores ...
    rows_e, targets_e, bt_e = score_plan(p["suffix_labels"], p["S"], 4096)  # ... and the rows of the extension
    assert targets.tolist() == targets_e.tolist()
    assert (bt[:, 0]).tolist() == (bt_e[:, 0]).tolist()
    assert (bt[:, 1] - p["cut"][bt[:, 0]]).tolist() == bt_e[:, 1].tolist()  # the same token positions, counted from the cut
    for r in range(6):                                                      # prefix + suffix is the row again
        n_pre, n_suf = int(p["prefix_mask"][r // 3].sum()), int(p["suffix_mask"][r].sum())
        row = p["prefix_ids"][r // 3][p["Tp"] - n_pre:].tolist() + p["suffix_ids"][r][:n_suf].tolist()
        assert row == ids[r][:int(mask[r].sum())].tolist()


def test_candidate_plan_rejects(host):
    MU = host.MU
    with pytest.raises(ValueError, match="same number of candidates"):
        _plan(host, cands=[["a", "b"], ["c"]])
    with pytest.raises(ValueError, match="candidate lists"):
        _plan(host, cands=[["a", "b"]])
    with pytest.raises(ValueError, match="same number of candidates"):
        _plan(host, cands=[[], []])
    # a "candidate" that brings its own [ANSWER] moves the cut: the prompts of the rows then differ
    with pytest.raises(ValueError, match="share its prefix"):
        _plan(host, cands=[["yes", "w9 [ANSWER] no", "x"], ["a", "b", "c"]])
    with pytest.raises(ValueError, match=r"no \[ANSWER\]"):
        _plan(host, instr=["w1 w2", INSTR[1]])
    # labels in front of the cut (train_qa_full_lm) cannot be scored by the extension
    me2 = SimpleNamespace(**{**vars(host.me), "train_qa_full_lm": True})
    with pytest.raises(ValueError, match="in front of the last"):
        MU.candidate_plan(host.tokenize, lambda x: MU.UnifiedProCyon._full_labels(me2, x), INSTR, CANDS, host.me.answer_idx, host.tok.pad_token_id)


def test_forward_label_rule_is_unchanged(host):
    """`qa_full_labels` restates the rule `forward` has always applied (pads, soft-token slots, everything up to the last [ANSWER])"""
    me, tok = host.me, host.tok
    ids, _ = host.tokenize(["w1 <|protein|> [ANSWER] a [ANSWER] b c", "[PROT] w2 [ANSWER] d"])
    lab = host.label_rule(ids)
    for r in range(2):
        last = int((ids[r] == me.answer_idx).nonzero().max())
        assert bool((lab[r, :last + 1] == -100).all())
        tail = ids[r, last + 1:]
        assert lab[r, last + 1:].tolist() == [(-100 if int(t) == tok.pad_token_id else int(t)) for t in tail]
