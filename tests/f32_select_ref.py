"""Float64 restatements and fixtures of the fp32 selection kernels (include/pcy.h: pcy_f32_beam_step, pcy_f32_sample_pick), written from the
header and the oracle, never from the kernels; built on tests/select_oracle.py.  tests/test_f32_select_cpu.py holds the helpers to the
oracle and asserts the fixture conditions; tests/test_gpu_f32_select.py holds the kernels to the helpers on the same rows."""
import functools

import torch

from select_oracle import first_argmax, log_softmax64, logprob_slack, softmax64, stable_topk

F32, F64 = torch.float32, torch.float64
NINF = float("-inf")
DELTA = 2.0 ** -18              # the project's fp32 budget (select_oracle.py): masses and CDF points within DELTA of a threshold may go either way
BAND_CAP = 4                    # tokens a nucleus row may hold within DELTA of 1 - p


# ------------------------------------------------------------------------------------------------ sampling
def scaled_logits(logits, temperature):
    """logits / temperature as the kernel and the reference form it: the correctly rounded fp32 quotient by the fp32 temperature"""
    x = logits.to(F32)
    return x if temperature == 1.0 else x / torch.tensor(temperature, dtype=F32)


def nucleus_cum64(p64):
    """ascending cumulative mass at every token under a STABLE ascending sort (equal probabilities: the lower index is the smaller) -> [.., V]"""
    vals, idx = torch.sort(p64, dim=-1, descending=False, stable=True)
    return torch.zeros_like(p64).scatter_(-1, idx, vals.cumsum(-1))


def nucleus_keep64(p64, nucleus_prob):
    """the reference's mask in float64: keep where the ascending cumulative mass has reached 1 - p; nothing reaches it: keep everything"""
    keep = nucleus_cum64(p64) >= 1.0 - nucleus_prob
    none = ~keep.any(-1, keepdim=True)
    return keep | none


def sampling_probs64(logits, temperature=1.0, nucleus_prob=None):
    """-> (masked probability vector, keep mask) in float64: softmax(logits / T), or softmax(logits) times the un-renormalised nucleus mask"""
    if nucleus_prob is not None:
        p = softmax64(logits.to(F32))
        keep = nucleus_keep64(p, nucleus_prob)
        return p * keep, keep
    p = softmax64(scaled_logits(logits, temperature))
    return p, torch.ones_like(p, dtype=torch.bool)


def sample_token64(p_masked, u):
    """first index in vocabulary order whose cumulative probability exceeds u * total"""
    cdf = p_masked.to(F64).cumsum(-1)
    target = u.to(F64)[:, None] * cdf[:, -1:]
    return first_argmax((cdf > target).to(torch.uint8))


def band_count(p64, nucleus_prob, delta=DELTA):
    """tokens whose ascending cumulative mass lies within delta of 1 - p (they may legitimately fall on either side of the mask) -> [rows]"""
    return ((nucleus_cum64(p64) - (1.0 - nucleus_prob)).abs() <= delta).sum(-1)


SAMPLE_V = (64, 193, 4096, 16385, 128263)
SAMPLE_MODES = {"temp1.0": (1.0, None), "temp0.7": (0.7, None), "nucleus0.5": (1.0, 0.5), "nucleus0.9": (1.0, 0.9)}
SAMPLE_US = (0.0, 0.1, 0.37, 0.5, 0.73, 1.0 - 2.0 ** -24)
SAMPLE_KINDS = ("rand1", "rand3", "uniform", "dominated", "masked", "one_left")


@functools.lru_cache(maxsize=None)
def sample_rows(V):
    """[6, V] fp32, one row per kind: randn x {1, 3}; all logits equal; one token of probability > 0.999; a third of the row (and its whole
    first 32nd) -inf; all but one token -inf"""
    g = torch.Generator().manual_seed(4000 + V)
    rows = torch.empty(len(SAMPLE_KINDS), V, dtype=F32)
    rows[0] = torch.randn(V, generator=g)
    rows[1] = torch.randn(V, generator=g) * 3.0
    rows[2] = 0.75
    rows[3] = 0.0
    rows[3, V // 3] = 21.0        # (the others hold V * e^-21 < 1e-4 together; |x - max| / 0.7 stays below 32, where fp32 still resolves 2^-20)
    rows[4] = torch.randn(V, generator=g) * 2.0
    rows[4, torch.rand(V, generator=g) < 0.3] = NINF
    rows[4, :(V + 31) // 32] = NINF
    rows[5] = NINF
    rows[5, (2 * V) // 3] = 1.5
    return rows


# ------------------------------------------------------------------------------------------------ beam step
BEAM_CASES = ((1, 4, 2, 300, 6), (2, 6, 2, 481, 5), (1, 10, 2, 4099, 4), (2, 8, 4, 37, 5), (1, 10, 2, 128263, 3))
BEAM_MASKED = (2, 6, 2, 481, 5)
BEAM_M = 13                     # table rows per step
BEAM_PENALTY = 0.8              # (not a multiple of the level spacing: a penalised candidate never lands on another level)
BEAM_PROMPT = 3
BEAM_NCH = 16


BEAM_DONE = (2, 4, 2, 37, 5)    # with eos_at = 2: every beam takes the EOS at step 2 and the search stops after 3 of its 5 steps


def beam_tables(B, beam, g, V, steps, masked, seed, eos_at=None):
    """[steps, M, V] fp32 tables of integer levels -3 .. 0-3 (row m holds 4 + m % 4 levels, so rows of different classes sit far apart and
    every row is full of exact ties); masked: a fifth of every row -inf and a whole 16th of every other row; eos_at: the step at which
    the EOS token (V - 1) stands far above every other logit in every row"""
    gen = torch.Generator().manual_seed(1000 * seed + B * 100 + beam + 17 * masked + V)
    tab = torch.stack([torch.stack([torch.randint(-3, 1 + m % 4, (V,), generator=gen) for m in range(BEAM_M)]) for _ in range(steps)]).to(F32)
    if masked:
        sl = (V + BEAM_NCH - 1) // BEAM_NCH
        tab[torch.rand(steps, BEAM_M, V, generator=gen) < 0.2] = NINF
        for s_ in range(steps):
            for m in range(BEAM_M):
                if (s_ + m) % 2 == 0:
                    c = (3 * s_ + m) % ((V + sl - 1) // sl)
                    tab[s_, m, c * sl:(c + 1) * sl] = NINF
        assert int(torch.isfinite(tab).sum(-1).min()) > beam * BEAM_NCH
    if eos_at is not None:
        tab[eos_at, :, V - 1] = 9.0
    return tab


def table_step(tab, i, next_tok, BB):
    """the logits of step i: identical rows after the prompt, then the table row the previous token names"""
    if i == 0:
        return tab[0, 0][None].expand(BB, -1).contiguous()
    return tab[i][(next_tok.long() * 7 + 3) % BEAM_M].contiguous()


def beam_search64(step_logits, B, beam, g, V, steps, penalty, eos_id, prompt_len=BEAM_PROMPT):
    """The diverse beam search of `_generate_beam_search` (oracle.llama_ref.beam_search) with the device step's documented rules, in
    float64: candidate (log_softmax64(x) + cur) - penalty * (earlier picks of this step == v), top-g with ties to the lowest flat index
    (stable_topk), step 0 on beam 0 of a group, the penalty inside the running score, EOS-anywhere stop on zero-initialised rows.
    step_logits(i, next_tok | None) -> fp32 [BB, V].  Returns a dict: tokens [BB, n], scores [BB] float64, src [n, BB] parents per step,
    has_eos [BB], done, n, pos, slack [BB] (the accumulated logprob_slack along each slot's history), gaps: per selection the list of
    (gap to the next candidate, slack of the pair) over the first g candidates."""
    BB, groups = B * beam, beam // g
    cur = torch.zeros(BB, dtype=F64)
    acc = torch.zeros(BB, dtype=F64)
    out = torch.zeros(BB, steps, dtype=torch.int64)
    has_eos = torch.zeros(BB, dtype=torch.bool)
    srcs, gaps, next_tok, n, done = [], [], None, 0, False
    pen = float(torch.tensor(penalty, dtype=F32))
    for i in range(steps):
        x = step_logits(i, next_tok)
        lsm, slack = log_softmax64(x), logprob_slack(x)
        lp = lsm + cur[:, None]
        n_out, n_cur, n_acc, n_eos, src = out.clone(), cur.clone(), acc.clone(), has_eos.clone(), torch.arange(BB)
        for b in range(B):
            b0 = b * beam
            for k in range(groups):
                gs, inc = b0 + k * g, (1 if i == 0 else g)
                cand = lp[gs:gs + inc].clone()
                if k:
                    cand -= pen * torch.bincount(n_out[b0:gs, i], minlength=V).to(F64)
                flat = cand.ravel()
                top = stable_topk(flat, min(g + 1, flat.numel()))
                sl = slack[gs:gs + inc].reshape(-1)[top.indices]
                gaps.append([(float(top.values[j] - top.values[j + 1]), float(torch.maximum(sl[j], sl[j + 1]))) for j in range(len(top.values) - 1)])
                idx = top.indices[:g]
                parents, toks = idx // V + gs, idx % V
                n_out[gs:gs + g] = out[parents]
                n_out[torch.arange(gs, gs + g), i] = toks
                n_cur[gs:gs + g] = top.values[:g]
                n_acc[gs:gs + g] = acc[parents] + sl[:g]
                n_eos[gs:gs + g] = (has_eos[parents] if i > 0 else torch.zeros(g, dtype=torch.bool)) | (toks == eos_id)
                src[gs:gs + g] = parents
        out, cur, acc, has_eos = n_out, n_cur, n_acc, n_eos
        srcs.append(src)
        next_tok, n = out[:, i], i + 1
        if bool((out == eos_id).any(dim=1).all()):
            done = True
            break
    return dict(tokens=out[:, :n], scores=cur, src=torch.stack(srcs), has_eos=has_eos, done=done, n=n, pos=prompt_len + n - 1, slack=acc, gaps=gaps)


def gaps_are_decidable(gaps):
    """every adjacent pair among a selection's first g + 1 candidates is an exact tie (equal rows and scores, or equal logits of one row:
    the index rule decides) or further apart than 4 x the pair's logprob_slack (a banned candidate, -inf, is infinitely far)"""
    return all(gap == 0.0 or gap == float("inf") or gap > 4.0 * sl for sel in gaps for gap, sl in sel)


@functools.lru_cache(maxsize=None)
def beam_case(B, beam, g, V, steps, masked=False, eos_at=None):
    """the first seed (of 16) whose float64 run is decidable everywhere -> dict(tab, eos, ref = beam_search64's result, seeds tried)"""
    eos = V - 1
    for seed in range(16):
        tab = beam_tables(B, beam, g, V, steps, masked, seed, eos_at)
        ref = beam_search64(lambda i, nt: table_step(tab, i, nt, B * beam), B, beam, g, V, steps, BEAM_PENALTY, eos)
        if gaps_are_decidable(ref["gaps"]) and bool(torch.isfinite(ref["scores"]).all()):
            return dict(tab=tab, eos=eos, ref=ref, seeds=seed + 1)
    raise AssertionError("no table with decidable selections in 16 seeds: a fixture error, reseed")
