"""The references of tests/select_oracle.py tested on their own, without a GPU: a selection kernel is only held to its documented tie rule and
rounding point if these helpers implement exactly that rule and that point."""
import pytest
import torch

from select_oracle import (BF, assert_rounded_from, bf16_half_ulp_towards, first_argmax, log_softmax64, logprob_preload, logprob_slack, lsm_rounded_once,
                           nucleus_keep_stable, softmax64, stable_topk)


def test_stable_topk_equals_topk_without_ties():
    g = torch.Generator().manual_seed(0)
    x = torch.randperm(5000, generator=g).float().view(5, 1000) - 2500.0
    for t, k, kw in [(x, 7, {}), (x, 1000, {}), (x, 3, dict(dim=0)), (x.ravel(), 11, {}), (x, 9, dict(largest=False))]:
        got, ref = stable_topk(t, k, **kw), torch.topk(t, k, **kw)
        assert isinstance(got, torch.return_types.topk)
        assert torch.equal(got.values, ref.values) and torch.equal(got.indices, ref.indices)
    v, i = stable_topk(x.ravel(), 4)                      # unpacks like torch's
    assert torch.equal(v, x.ravel()[i])


def test_stable_topk_lowest_index_first_inside_a_tie():
    x = torch.tensor([1.0, 3.0, 3.0, 2.0, 3.0, 0.0, 3.0])
    assert stable_topk(x, 2).indices.tolist() == [1, 2]
    assert stable_topk(x, 3).indices.tolist() == [1, 2, 4]
    assert stable_topk(x, 5).indices.tolist() == [1, 2, 4, 6, 3]
    # the beam step's flat index r * V + v: a tie between (row 0, token 5) and (row 1, token 2) goes to row 0
    lp = torch.full((2, 8), -9.0)
    lp[0, 5] = lp[1, 2] = lp[1, 7] = -1.0
    assert stable_topk(lp.ravel(), 2).indices.tolist() == [5, 10]
    # a constant tensor: the first k indices in order, in bf16 as well
    assert stable_topk(torch.zeros(300, dtype=BF), 6).indices.tolist() == list(range(6))


def test_first_argmax():
    x = torch.tensor([[0.0, 2.0, 2.0, 1.0], [5.0, 5.0, 5.0, 5.0], [-1.0, -3.0, -2.0, -1.0]]).to(BF)
    assert first_argmax(x).tolist() == [1, 0, 0]
    assert first_argmax(torch.tensor([float("-inf"), 1.0, float("-inf"), 1.0])).tolist() == 1
    assert first_argmax(x, dim=0).tolist() == [1, 1, 1, 1]


@pytest.mark.parametrize("b", [0.30078125, -2.265625, 5.75, -11.3125, 9.765625e-4, 1.0, -64.0, 3.0517578125e-05])
def test_assert_rounded_from_accepts_the_rounding_and_rejects_the_neighbours(b):
    got = torch.tensor([b])
    assert float(got.to(BF)) == b                                   # the cases are bf16 values
    ulp = 2 * float(bf16_half_ulp_towards(got, torch.tensor([2.0 * b], dtype=torch.float64)))   # spacing on the far side
    slack = 2.0 ** -18 * abs(b)
    for frac in (0.0, 0.25, -0.25 if abs(b) not in (1.0, 64.0) else -0.12):   # truth inside the interval that rounds to b
        truth = torch.tensor([b + frac * ulp * (1 if b > 0 else -1)], dtype=torch.float64)
        assert float(truth.float().to(BF)) == b
        assert assert_rounded_from(got, truth, slack) <= 1.0
        for nb in (b + ulp, b - ulp):                               # one ulp away (the far-side spacing: at least one ulp on the near side)
            with pytest.raises(AssertionError):
                assert_rounded_from(torch.tensor([nb]), truth, slack)


def test_assert_rounded_from_half_ulp_below_a_power_of_two():
    one = torch.tensor([1.0])
    # below 1.0 the bf16 spacing is 2^-8: 1 - 0.9 * 2^-9 rounds to 1.0, 1 - 1.5 * 2^-9 rounds to 1 - 2^-8
    assert assert_rounded_from(one, torch.tensor([1 - 0.9 * 2.0 ** -9], dtype=torch.float64), 0.0) <= 1.0
    with pytest.raises(AssertionError):
        assert_rounded_from(one, torch.tensor([1 - 1.5 * 2.0 ** -9], dtype=torch.float64), 0.0)
    assert assert_rounded_from(torch.tensor([1 - 2.0 ** -8]), torch.tensor([1 - 1.5 * 2.0 ** -9], dtype=torch.float64), 0.0) <= 1.0
    # above it the spacing is 2^-7
    assert assert_rounded_from(one, torch.tensor([1 + 0.9 * 2.0 ** -8], dtype=torch.float64), 0.0) <= 1.0


def test_assert_rounded_from_rejects_non_bf16_nan_and_wrong_infinities():
    t = torch.tensor([0.5], dtype=torch.float64)
    with pytest.raises(AssertionError, match="not a bf16 value"):
        assert_rounded_from(torch.tensor([0.5 + 2.0 ** -12]), t, 1.0)
    with pytest.raises(AssertionError, match="NaN"):
        assert_rounded_from(torch.tensor([float("nan")]), t, 1.0)
    with pytest.raises(AssertionError, match="infinite"):
        assert_rounded_from(torch.tensor([float("-inf")]), t, 1.0)
    ninf = torch.tensor([float("-inf")], dtype=torch.float64)
    with pytest.raises(AssertionError, match="infinite"):
        assert_rounded_from(torch.tensor([-300.0]), ninf, 1.0)
    assert assert_rounded_from(torch.tensor([float("-inf"), 0.0]), torch.tensor([float("-inf"), 0.0], dtype=torch.float64), 0.0) == 0.0
    # a broken reference must not turn into a silent pass: NaN truth, NaN slack, an infinity of the other sign
    with pytest.raises(AssertionError, match="reference itself"):
        assert_rounded_from(torch.tensor([0.5]), torch.tensor([float("nan")], dtype=torch.float64), 1.0)
    with pytest.raises(AssertionError, match="reference itself"):
        assert_rounded_from(torch.tensor([0.5]), t, float("nan"))
    with pytest.raises(AssertionError, match="wrong sign"):
        assert_rounded_from(torch.tensor([float("-inf")]), torch.tensor([float("inf")], dtype=torch.float64), 1.0)
    # an exact zero is only the rounding of (next to) nothing
    with pytest.raises(AssertionError):
        assert_rounded_from(torch.tensor([0.0]), torch.tensor([1e-30], dtype=torch.float64), 2.0 ** -18 * 1e-30)


def test_assert_rounded_from_rejects_log_sum_rounded_first():
    """The example of the beam bookkeeping test: the exact log-probability -2.2587 rounds to -2.2656; rounding log(sum) to bf16 before the
    subtraction gives -2.2500 instead.  x - max = -1, log(sum) = 1.2587: bf16(1.2587) = 1.2578125 and -1 - 1.2578125 = -2.2578125 is
    the midpoint of -2.25 and -2.265625, which rounds to the even -2.25."""
    d, lse = torch.tensor([-1.0], dtype=torch.float64), torch.tensor([1.2587], dtype=torch.float64)
    truth = d - lse
    once = truth.float().to(BF).float()
    first = (d.float() - lse.float().to(BF).float()).to(BF).float()
    assert float(once) == -2.265625 and float(first) == -2.25
    slack = 2.0 ** -18 * 1.2587
    assert assert_rounded_from(once, truth, slack) <= 1.0
    with pytest.raises(AssertionError):
        assert_rounded_from(first, truth, slack)


def test_rounding_log_sum_first_is_caught_on_random_rows():
    """On random rows: every entry at which bf16(d - bf16(lse)) differs from the once-rounded value is rejected, unless the truth lies within
    the slack of a rounding midpoint (where both neighbours are legitimate)."""
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(6, 1500, generator=g) * 3.0).to(BF)
    xd = x.double()
    d = xd - xd.max(-1, keepdim=True).values
    lse = torch.log(torch.exp(d).sum(-1, keepdim=True))
    truth, slack = log_softmax64(x), logprob_slack(x)
    once = lsm_rounded_once(x)
    assert assert_rounded_from(once, truth, slack) <= 1.0
    first = (d.float() - lse.float().to(BF).float()).to(BF)
    differ = (first != once).nonzero()
    assert len(differ) > 100
    n_rej = 0
    for r, c in differ.tolist():
        mid = (first[r, c].double() + once[r, c].double()) / 2
        if abs(float(truth[r, c] - mid)) <= 2 * float(slack[r, c]):
            continue
        with pytest.raises(AssertionError):
            assert_rounded_from(first[r, c], truth[r, c], slack[r, c])
        n_rej += 1
    assert n_rej > 100


def test_lsm_rounded_once_and_softmax_with_banned_tokens():
    x = torch.tensor([[1.0, float("-inf"), 0.5, float("-inf")], [float("-inf"), float("-inf"), -3.0, -3.0]]).to(BF)
    y, p = lsm_rounded_once(x), softmax64(x)
    assert y.dtype == BF and not bool(torch.isnan(y.float()).any()) and not bool(torch.isnan(p).any())
    assert torch.equal(torch.isinf(y.float()), torch.isinf(x.float())) and bool((p[torch.isinf(x.float())] == 0).all())
    assert float(y[1, 2]) == float(torch.tensor(-0.6931471805599453).to(BF)) and torch.allclose(p.sum(-1), torch.ones(2, dtype=torch.float64))
    # without -inf: the float64 log-softmax, rounded
    g = torch.Generator().manual_seed(1)
    z = (torch.randn(3, 700, generator=g) * 4).to(BF)
    assert torch.equal(lsm_rounded_once(z), torch.log_softmax(z.double(), -1).float().to(BF))


@pytest.mark.parametrize("nucleus_prob", [0.5, 0.9])
def test_nucleus_keep_stable_agrees_with_the_oracle_without_ties(nucleus_prob):
    from oracle import llama_ref as LR
    logits = (torch.arange(40).float() * 0.25).flip(0)[None].to(BF).repeat(2, 1)
    logits[1] = logits[1].flip(0)
    p = logits.softmax(-1)
    assert all(len(torch.unique(p[r])) == 40 for r in range(2))      # tie-free: the sort order is defined without the stable flag
    ref = LR.sampling_probs(logits, nucleus_prob=nucleus_prob)
    keep = nucleus_keep_stable(p, nucleus_prob)
    assert torch.equal(keep, ref > 0) and 0 < int(keep[0].sum()) < 40


def test_nucleus_keep_stable_keeps_the_higher_indices_of_a_tie_run():
    p = torch.full((1, 64), 1.0 / 64, dtype=BF)
    # ascending cumulative sums j / 64 (exact): >= 0.5 from the 32nd element on, i.e. indices 31..63
    assert nucleus_keep_stable(p, 0.5)[0].nonzero().view(-1).tolist() == list(range(31, 64))
    assert nucleus_keep_stable(p, 0.9)[0].nonzero().view(-1).tolist() == list(range(6, 64))


def test_logprob_preload_keeps_the_gain_exact():
    """-8.0 + y - (-8.0) == y in fp32 for every bf16 log-probability of a row that gets the preload; a row with a token of probability
    next to 1 gets 0."""
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(4, 3000, generator=g) * torch.tensor([1.0, 4.0, 12.0, 12.0])[:, None]).to(BF)
    x[3, 7] = 60.0                                                   # log-probability of token 7: about -e^-20
    pre = logprob_preload(x)
    assert pre.tolist() == [-8.0, -8.0, -8.0, 0.0]
    y = lsm_rounded_once(x).float()
    assert torch.equal((pre[:, None] + y) - pre[:, None], y)
    # the smallest magnitude that still gets the preload, and a large one
    for v in (-2.0 ** -12, -(2.0 ** -12) * (1 + 127 / 128), -7.96875, -8.0, -100.5, -126.0):
        t = torch.tensor([v])
        assert float(t.to(BF)) == v and float((torch.tensor([-8.0]) + t) - torch.tensor([-8.0])) == v
