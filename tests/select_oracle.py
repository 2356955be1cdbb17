"""CPU references for the kernels that turn a row of logits into a decision (greedy pick, sampling pick, beam step, QA read-out), all in
float64 from the bf16 inputs, with the tie rules the kernels document: shared by test_select_cpu.py (which tests these helpers) and
test_gpu_select.py / test_gpu_kernels.py (which hold the kernels to them)."""
import torch

BF = torch.bfloat16


def log_softmax64(x, dim=-1):
    """(x - max) - log(sum exp(x - max)) in float64; exp(-inf) counts as 0, so a -inf logit gives -inf and never a NaN."""
    xd = x.double()
    d = xd - xd.max(dim, keepdim=True).values
    return d - torch.log(torch.exp(d).sum(dim, keepdim=True))


def softmax64(x, dim=-1):
    xd = x.double()
    e = torch.exp(xd - xd.max(dim, keepdim=True).values)
    return e / e.sum(dim, keepdim=True)


def lsm_rounded_once(x, dim=-1):
    """log_softmax of a bf16 tensor with ONE rounding: the float64 value rounded to the input's dtype -- what a kernel with fp32 statistics
    and a single final rounding gives (torch's CPU kernel for bf16 rounds log(sum) to bf16 first).  Drop-in for F.log_softmax."""
    return log_softmax64(x, dim).float().to(x.dtype)


def logprob_slack(x, tok=None, dim=-1):
    """The fp32 error budget of a kernel's (x - max) - logf(sum): 2^-18 * max(1, |lse|, |x - max|), lse = log(sum exp(x - max)); per row
    at token `tok` [rows], or for every entry when tok is None."""
    xd = x.double()
    d = xd - xd.max(dim, keepdim=True).values
    lse = torch.log(torch.exp(d).sum(dim, keepdim=True))
    if tok is not None:
        d = d.gather(dim, tok.long().unsqueeze(dim))
    s = 2.0 ** -18 * torch.maximum(torch.maximum(d.abs(), lse.abs()), torch.ones_like(lse))
    return s.squeeze(dim) if tok is not None else s


PRELOAD = -8.0


def logprob_preload(x, dim=-1):
    """What to put into a row's logprob accumulator before a pick so that the kernel's `logprob +=` is under test and the step's gain can
    still be read back exactly as after - before: -8.0 wherever every log-probability of the row is at least 2^-12 in magnitude, else 0.
    The gain y is a bf16 value (8 significant bits, lowest bit >= 2^-19 for |y| >= 2^-12); for |y| < 8 the sum -8 + y lies in (-16, -8],
    whose fp32 spacing is 2^-20 or finer, and for |y| >= 8 both terms are multiples of 2^-4 below 2^24 of them: the fp32 sum and the
    difference after - before are exact.  A row with a log-probability nearer to 0 (a token of probability > 0.9997) keeps 0."""
    big_enough = log_softmax64(x, dim).abs().amin(dim) >= 2.0 ** -12
    return torch.where(big_enough, torch.tensor(PRELOAD), torch.tensor(0.0)).float()


def bf16_half_ulp_towards(got, truth):
    """Half the distance from the bf16 value `got` to its bf16 neighbour on the side of `truth` (float64): 2^(e-8) in the binade
    [2^e, 2^(e+1)) of |got|, half of that below a power of two, 2^-134 for zero and the subnormals."""
    g = got.double()
    m, ex = torch.frexp(g.abs())                                  # |g| = m * 2^ex, m in [0.5, 1): binade exponent e = ex - 1
    e = torch.where(g == 0, torch.full_like(g, -126.0), torch.clamp(ex.double() - 1.0, min=-126.0))
    half = torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 8.0)
    inward = (m == 0.5) & (truth.double().abs() < g.abs()) & (e > -126.0)
    return torch.where(inward, half / 2, half)


def assert_rounded_from(got_bf16_valued, truth64, slack, what=""):
    """`got` must be what rounding to bf16 makes of an fp32 evaluation of `truth`: a bf16 value with
        |got - truth| <= half a bf16 ulp of got + slack.
    slack is the fp32 error budget of the kernel's arithmetic before that one rounding: 2^-18 * max(1, |lse|, |x - max|) for a
    log-probability (logprob_slack), 2^-18 * p for a probability.  Derivation: a tree sum of up to 2^17 fp32 terms (17 levels, 2^-24
    each, on positive terms), logf (1 ulp) and two subtractions have a worst-case bound of about 1.5 * 2^-20 relative to the larger of the
    operands; 2^-18 gives roughly three times that.  For a log-probability y = (x - max) - lse with |y| in [2^e, 2^(e+1)), e >= 0, both
    operands are at most |y|, so the slack is below 2^-18 * 2^(e+1) against a half-ulp of 2^(e-8): it widens the acceptance window by
    less than 2^-9 < 0.4 % and cannot hide a wrong rounding point, which moves the result by a whole ulp for about as many truths as
    the misplaced rounding is ulps wide.
    Returns the worst |got - truth| / (half ulp + slack) for the parity report; -inf == -inf and 0 == 0 count as exact."""
    got = torch.as_tensor(got_bf16_valued).detach().cpu()
    truth = torch.as_tensor(truth64).detach().cpu().double()
    slack = torch.as_tensor(slack, dtype=torch.float64).expand_as(truth)
    assert got.shape == truth.shape, (what, got.shape, truth.shape)
    g32 = got.float()
    assert not bool(torch.isnan(g32).any()), f"{what}: NaN"
    assert torch.equal(g32.to(BF).float(), g32), f"{what}: not a bf16 value"
    assert not bool(torch.isnan(truth).any()) and not bool(torch.isnan(slack).any()), f"{what}: the reference itself holds a NaN"
    g = g32.double()
    same_inf = torch.isinf(g) & (g == truth)
    assert not bool((torch.isinf(g) != torch.isinf(truth)).any()), f"{what}: infinite where the truth is finite (or the reverse)"
    assert bool((torch.isinf(g) == same_inf).all()), f"{what}: infinite with the wrong sign"
    bound = bf16_half_ulp_towards(g32, truth) + slack
    err = torch.where(same_inf, torch.zeros_like(g), (g - truth).abs())
    ratio = torch.where(same_inf, torch.zeros_like(g), err / bound)
    bad = ratio > 1.0
    if bool(bad.any()):
        i = int(ratio.view(-1).argmax())
        raise AssertionError(f"{what}: {int(bad.sum())} values are not the bf16 rounding of the truth; worst: got {float(g.view(-1)[i])!r}, "
                             f"truth {float(truth.view(-1)[i])!r}, |diff| {float(err.view(-1)[i]):.3e} > half ulp + slack {float(bound.view(-1)[i]):.3e}")
    return float(ratio.max()) if ratio.numel() else 0.0


def stable_topk(self, k, dim=-1, largest=True, sorted=True):
    """torch.Tensor.topk with a defined order of equal values: the lower index first (torch.topk leaves it open).  On a flattened
    [rows, V] tensor that is the beam step's rule, the lowest flat index r * V + v."""
    v, i = torch.sort(self, dim=dim, descending=largest, stable=True)
    return torch.return_types.topk((v.narrow(dim, 0, k), i.narrow(dim, 0, k)))


def nucleus_keep_stable(p_bf16, nucleus_prob):
    """The reference's nucleus mask (`_get_nucleus_mask` as restated in oracle.llama_ref.nucleus_mask: ascending sort, cumsum on the bf16
    tensor, keep where >= 1 - p) with a STABLE ascending sort: inside a run of equal probabilities the lower indices count as the smaller
    ones, so a threshold inside the run keeps its higher indices.  -> bool mask of p's shape."""
    remove_prob = 1 - nucleus_prob
    sorted_vals, indices = torch.sort(p_bf16, dim=-1, descending=False, stable=True)
    keep_vals = sorted_vals.cumsum(dim=-1) >= remove_prob
    return torch.zeros_like(keep_vals).scatter_(-1, indices, keep_vals)


def first_argmax(x, dim=-1):
    """lowest index of the maximum along dim (int64)"""
    n = x.shape[dim]
    idx = torch.arange(n).view([-1 if d == (dim % x.dim()) else 1 for d in range(x.dim())])
    is_max = x == x.max(dim, keepdim=True).values
    return torch.where(is_max, idx, torch.full_like(idx, n)).min(dim).values
