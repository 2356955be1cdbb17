"""Teacher-forced scoring, host side (no GPU): the row plan against HF's definition, the definition itself against transformers, and the
workspace arithmetic of the fused lm_head x cross-entropy operator."""
import math

import pytest
import torch
import torch.nn.functional as F


def hf_loss(logits, labels):
    """The pinned definition the GPU tests use: HF's causal-LM loss (shift, fp32 upcast, ignore_index -100, mean)."""
    V = logits.shape[-1]
    return F.cross_entropy(logits.float()[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100)


def _labels():
    T = 12
    lab = torch.full((5, T), -100, dtype=torch.long)
    lab[0, 3:9] = torch.tensor([5, 0, 63, 7, 7, 1])          # ragged: ends early
    lab[1, 6:] = torch.arange(6) + 10                          # a leading run of -100, labelled up to the LAST column
    lab[2, 1:11] = torch.arange(10) + 20                       # -100 in the last column (and column 0 never counts)
    lab[2, 0] = 9
    # row 3: no label at all
    lab[4, 0] = 3                                              # only column 0: never a target
    lab[4, 5] = 63
    return lab, T


def _brute(lab, T_real):
    rows, tg, bt = [], [], []
    for b in range(lab.shape[0]):
        for t in range(lab.shape[1]):
            if t + 1 < T_real and t + 1 < lab.shape[1] and int(lab[b, t + 1]) != -100:
                rows.append(b * T_real + t)
                tg.append(int(lab[b, t + 1]))
                bt.append((b, t))
    return rows, tg, bt


@pytest.mark.parametrize("T_real", [12, 9, 2, 1])
def test_score_plan_matches_hf_shift(T_real):
    from procyon_amd.engine import score_plan
    lab, T = _labels()
    rows, tg, bt = score_plan(lab, T_real, 64)
    r0, t0, b0 = _brute(lab, T_real)
    assert rows.dtype == torch.int32 and tg.dtype == torch.int32
    assert rows.tolist() == r0 and tg.tolist() == t0 and [tuple(x) for x in bt.tolist()] == b0
    if T_real == 12:
        # the scored pairs are exactly the terms of HF's loss: the mean of the picked -log_softmax equals it
        g = torch.Generator().manual_seed(0)
        logits = torch.randn(5, T, 64, generator=g).to(torch.bfloat16)
        lsm = torch.log_softmax(logits.float(), -1)
        picked = -lsm[bt[:, 0], bt[:, 1], tg.long()]
        assert len(r0) == int((lab[:, 1:] != -100).sum())
        assert abs(float(picked.mean()) - float(hf_loss(logits, lab))) < 1e-6


def test_score_plan_rejects_labels_outside_the_vocabulary():
    from procyon_amd.engine import score_plan
    lab, T = _labels()
    for bad in (64, 1000, -1, -99):
        l2 = lab.clone()
        l2[1, 7] = bad
        with pytest.raises(ValueError):
            score_plan(l2, T, 64)
    l2 = lab.clone()
    l2[1, 0] = 64          # column 0 is never a target, and a column that is not run is not looked at
    l2[1, 11] = 64
    score_plan(l2, 11, 64)


def test_pinned_definition_is_hf_causal_lm_loss():
    tr = pytest.importorskip("transformers")
    try:
        from transformers.loss.loss_utils import ForCausalLMLoss
    except ImportError:
        pytest.skip("transformers without loss_utils.ForCausalLMLoss")
    del tr
    g = torch.Generator().manual_seed(1)
    V = 97
    logits = (3 * torch.randn(3, 9, V, generator=g)).to(torch.bfloat16)
    labels = torch.randint(0, V, (3, 9), generator=g)
    labels[0, :4] = -100
    labels[2, 7:] = -100
    a, b = ForCausalLMLoss(logits, labels, V), hf_loss(logits, labels)
    assert a.dtype == torch.float32 and torch.equal(a, b), (a, b)
    none = torch.full_like(labels, -100)
    assert math.isnan(float(ForCausalLMLoss(logits, none, V))) and math.isnan(float(hf_loss(logits, none)))


def test_operator_workspace_is_a_thousandth_of_the_logits():
    from procyon_amd import _lib
    lib = _lib.load()
    M, V = 32768, 128263
    ws = lib.pcy_lm_head_xent_ws_bytes(M, V)
    assert 0 < ws * 1000 <= M * V * 2, (ws, M * V * 2)
    # M x n_col_blocks x 8 + O(M) up to the row chunk, constant beyond it; the column partition depends on V alone
    per_row = [lib.pcy_lm_head_xent_ws_bytes(m, V) / m for m in (64, 256, 1024)]
    assert max(per_row) <= 8 * 512 + 4 + 512 / 64 and lib.pcy_lm_head_xent_ws_bytes(2048, V) == lib.pcy_lm_head_xent_ws_bytes(1024, V)
    assert lib.pcy_lm_head_xent_ws_bytes(0, V) == 0
