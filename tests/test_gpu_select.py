"""The kernels that turn a row of logits into a decision -- greedy pick, sampling pick, beam step, QA read-out -- on constructed rows: exact
ties across every boundary of their reductions, maxima at the edges of the chunks, banned (-inf) tokens, and every log-probability /
probability held to ONE bf16 rounding of the float64 value (tests/select_oracle.py).  The end-to-end tests forgive a token that differs at
a near-tie of the oracle; these do not: the tie rule (lowest index) and the rounding point are part of the kernels' contract."""
import functools
import math
from fractions import Fraction

import pytest
import torch

from conftest import record_parity
from select_oracle import (BF, assert_rounded_from, bf16_half_ulp_towards, first_argmax, log_softmax64, logprob_preload, logprob_slack, lsm_rounded_once, nucleus_keep_stable, softmax64,
                           stable_topk)

pytestmark = pytest.mark.gpu

NINF = float("-inf")
PICK_NB = 64        # chunks per row of the greedy / sampling statistics (pcy_elem.hip)
BEAM_NCH = 16       # slices per row of the beam step


@functools.lru_cache(maxsize=None)
def _engine(V):
    """the tiny engine of the sampling test: the selection kernels read only its vocabulary size"""
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    kw = dict(vocab=V, d=64, n_layers=1, n_heads=2, n_kv_heads=1, ffn=128)
    return LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, max_pos=64))


def _background(V, g, top):
    """random bf16 logits strictly below `top`"""
    return torch.randn(V, generator=g).clamp(max=top - 2.0).to(BF)


def _ban(row, g, V, chunk, kinds):
    """-inf entries: 'scatter' (about a third of the entries), or whole chunks by number (negative: from the last non-empty one)"""
    nch = (V + chunk - 1) // chunk
    for k in kinds:
        if k == "scatter":
            row[torch.rand(V, generator=g) < 0.3] = NINF
        else:
            c = k % nch
            row[c * chunk:(c + 1) * chunk] = NINF
    return row


# ------------------------------------------------------------------------------------------------ greedy pick
GREEDY_V = [37, 193, 16385, 128256]


@functools.lru_cache(maxsize=None)
def _greedy_case(V, masked):
    """-> rows [R, V] bf16, the expected token per row (lowest index of the maximum), the float64 log-probability at it, its fp32 slack; computed
    once per vocabulary and shared by the batch sizes.  Constructed rows also state the token they were built for."""
    g = torch.Generator().manual_seed(V + 7 * masked)
    chunk = (V + PICK_NB - 1) // PICK_NB
    nch = (V + chunk - 1) // chunk                    # non-empty chunks (V = 37: 37 of one entry, 27 empty; V = 193: the 49th holds one entry)
    c = nch // 2
    lo = c * chunk
    TOP = 5.0
    rows, built_for = [], []

    def add(row, tok=None):
        rows.append(row)
        built_for.append(-1 if tok is None else tok)

    if not masked:
        add(torch.full((V,), 1.5, dtype=BF), 0)                                             # a constant row
        for i in (0, V - 1, lo - 1, lo):                                                    # a unique maximum at the edges of the row and of a chunk
            r = _background(V, g, TOP)
            r[i] = TOP
            add(r, i)
        # the maximum twice: neighbouring lanes / waves (63 | 64 of the chunk), the same lane of two waves, the same thread's next
        # element, the last entry of a chunk and the first of the next, the two ends of the row
        for i, j in ((lo + 63, lo + 64), (lo + 5, lo + 6), (lo + 5, lo + 69), (lo, lo + 256), (lo + chunk - 1, lo + chunk), (0, V - 1)):
            if j < V:
                r = _background(V, g, TOP)
                r[i] = r[j] = TOP
                add(r, i)
        for scale in (1.0, 4.0, 12.0):
            add((torch.randn(V, generator=g) * scale).to(BF))
    else:
        for scale, kinds in ((1.0, ["scatter"]), (4.0, ["scatter"]), (1.0, [c]), (4.0, [0]), (1.0, [-1, "scatter"]), (4.0, [c, c + 1, 0, -1])):
            add(_ban((torch.randn(V, generator=g) * scale).to(BF), g, V, chunk, kinds))
        # the maximum right behind a banned chunk, and twice around one
        r = _ban(_background(V, g, TOP), g, V, chunk, [c])
        r[lo + chunk] = TOP
        add(r, lo + chunk)
        r = _ban(_background(V, g, TOP), g, V, chunk, [c])
        r[lo - 1] = r[lo + chunk] = TOP
        add(r, lo - 1)
    rows = torch.stack(rows)
    tok = first_argmax(rows.float())
    built_for = torch.tensor(built_for)
    assert torch.equal(tok[built_for >= 0], built_for[built_for >= 0])                      # the rows are what they were built to be
    finite = torch.isfinite(rows.float()).sum(-1)
    assert bool((finite >= min(V, 20)).all())
    ar = torch.arange(len(rows))
    return rows, tok, log_softmax64(rows)[ar, tok], logprob_slack(rows, tok)


def _check_greedy(V, B, masked):
    from procyon_amd.engine import GenState
    rows, tok_ref, lp_ref, slack = _greedy_case(V, masked)
    eng = _engine(V)
    R = len(rows)
    pre = logprob_preload(rows)                            # -8.0 in the accumulator (0 where a gain could not be read back exactly)
    assert bool((pre[:3] == -8.0).all())
    calls = (R + B - 1) // B
    calls += calls < 2                                     # both values of advance_pos
    st, cache = GenState(B, V, calls, "cuda"), eng.new_cache(B, 16)
    worst = 0.0
    for call in range(calls):
        idx = torch.tensor([(call * B + r) % R for r in range(B)])
        st.logits.copy_(rows[idx])
        st.logprob.copy_(pre[idx])                         # the kernel ADDS one step's value to what the accumulator holds
        adv = call % 2
        step0, pos0 = int(st.step), int(st.pos)
        eng.pick(cache, st, B, bool(adv))
        tok = st.next_tok.cpu().long()
        assert torch.equal(tok, tok_ref[idx]), (call, idx.tolist(), tok.tolist(), tok_ref[idx].tolist())
        assert torch.equal(st.tokens_out[:, step0].cpu().long(), tok)
        assert int(st.step) == step0 + 1 and int(st.pos) == pos0 + adv, (call, adv)
        assert bool(torch.isfinite(rows[idx, tok].float()).all())                           # a banned token is never chosen
        worst = max(worst, assert_rounded_from(st.logprob.cpu() - pre[idx], lp_ref[idx], slack[idx], f"greedy logprob V={V} B={B} call {call}"))
    assert int(eng.ctx.lib.pcy_ctx_sync(eng.ctx.h)) == 0
    return worst


@pytest.mark.parametrize("B", [1, 5, 9])
@pytest.mark.parametrize("V", GREEDY_V)
def test_greedy_pick_ties_edges_and_logprob(V, B):
    """pcy_greedy_pick on constructed rows: the token is the LOWEST index of the maximum -- across lanes, waves, a thread's successive
    elements, the 64 chunks (V = 37: chunks of one entry and 27 empty ones; V = 193: a last chunk of one entry; V = 16385: chunks longer
    than the workgroup) and the rows a wave of stage 2 walks (B = 5, 9) -- and logprob gains the float64 log-softmax at it, rounded to
    bf16 once.  step / pos advance as advance_pos says.
    (At the greedy token x == max, so the value is -log(sum) and rounding log(sum) to bf16 before the subtraction gives the same bits:
    this test pins the statistics -- a lost chunk, a wrong merge -- and not the rounding POINT, which the sampling pick's logprob at an
    arbitrary token and the beam step's scores pin.)"""
    worst = _check_greedy(V, B, masked=False)
    record_parity(f"select_greedy_V{V}_B{B}", worst_logprob_err_over_bound=worst)


@pytest.mark.parametrize("V", GREEDY_V)
def test_greedy_pick_masked_logits(V):
    """-inf logits mean "never chosen": scattered ones and whole chunks of them (ceil(V / 64) entries: such a chunk's partial must be
    (max = -inf, sum = 0), not exp(-inf + inf)).  Same checks as on finite rows; a NaN logprob fails them."""
    worst = _check_greedy(V, 5, masked=True)
    record_parity(f"select_greedy_masked_V{V}", worst_logprob_err_over_bound=worst)


# ------------------------------------------------------------------------------------------------ QA read-out
def _adjacent_below(x):
    """the next value below x > 0 in x's dtype"""
    if x.dtype == BF:
        return (x.view(torch.int16) - 1).view(BF)
    return torch.nextafter(x, torch.zeros_like(x))


@functools.lru_cache(maxsize=None)
def _qa_case(V, dtype, masked):
    g = torch.Generator().manual_seed(V + (dtype == torch.float32) + 11 * masked)
    TOP = torch.tensor(5.0, dtype=dtype)
    bg = lambda: torch.randn(V, generator=g).clamp(max=3.0).to(BF).to(dtype)
    rows = []
    if not masked:
        for i, j in ((5, 5 + 1024), (63, 64), (1023, 1024), (0, V - 1)):     # the same thread's next element, lanes 63 | 0, threads 1023 | 0, the ends
            if i < j < V:
                r = bg()
                r[i] = r[j] = TOP
                rows.append(r)
        # the two top logits adjacent values of the dtype, the larger one LAST: the stored probabilities may or may not tie
        r = bg()
        r[V - 1], r[0] = TOP, _adjacent_below(TOP)
        rows.append(r)
        r = bg()
        r[V // 2], r[V // 3] = TOP + 4, _adjacent_below(TOP + 4)
        rows.append(r)
        for scale in (1.0, 3.0):
            rows.append((torch.randn(V, generator=g) * scale).to(BF).to(dtype))
        if dtype == torch.float32:
            rows.append(torch.randn(V, generator=g) * 3.0)                   # not bf16 values
    else:
        blk = max(1, V // 16)
        for scale, kinds in ((1.0, ["scatter"]), (3.0, [0, "scatter"]), (3.0, [3, -1])):
            rows.append(_ban((torch.randn(V, generator=g) * scale).to(BF).to(dtype), g, V, blk, kinds))
        r = _ban(bg(), g, V, blk, [1])
        r[blk - 1] = r[min(2 * blk, V - 1)] = TOP                             # the maximum twice around a banned block
        rows.append(r)
    rows = torch.stack(rows)
    assert bool((torch.isfinite(rows).sum(-1) >= 1).all())
    return rows, softmax64(rows)


def _check_qa(V, nrows, dtype, masked):
    from procyon_amd.engine import Context
    ctx = Context.get()
    rows, p_ref = _qa_case(V, dtype, masked)
    R = len(rows)
    worst = 0.0
    pairs = [(0, V - 1), (V - 1, 0), (V // 2, V // 2), (0, 0), (V - 1, V - 1)]
    for call in range((R + nrows - 1) // nrows):
        idx = torch.tensor([(call * nrows + r) % R for r in range(nrows)])
        x = rows[idx].cuda()
        first = None
        for yes, no in pairs:
            probs, yn, am = ctx.qa_probs(x, yes, no, want_probs=True, want_argmax=True)
            _, yn2, am2 = ctx.qa_probs(x, yes, no, want_probs=False, want_argmax=True)      # probs_out NULL: the other outputs are unchanged
            p, yn, am = probs.cpu(), yn.cpu(), am.cpu()
            assert p.dtype == dtype and not bool(torch.isnan(p.float()).any())
            assert torch.equal(am, first_argmax(p.float())), (call, am.tolist(), first_argmax(p.float()).tolist())
            assert torch.equal(yn.view(torch.int32), torch.stack([p[:, yes], p[:, no]], -1).float().view(torch.int32)), (call, yes, no)
            assert torch.equal(yn2.cpu().view(torch.int32), yn.view(torch.int32)) and torch.equal(am2.cpu(), am)
            if first is None:
                first = p
            assert torch.equal(p, first)                                                    # the yes / no ids do not touch the vector
        ref = p_ref[idx]
        banned = torch.isinf(rows[idx]) & (rows[idx] < 0)
        assert bool((first[banned] == 0).all())                                             # a banned token's stored probability is exactly 0
        assert not bool(banned[torch.arange(nrows), am].any())
        if dtype == BF:
            worst = max(worst, assert_rounded_from(first, ref, 2.0 ** -18 * ref, f"qa probs V={V} call {call}"))
        else:
            rel = ((first.double() - ref).abs() / ref.clamp_min(1e-300))[~banned]
            assert bool((rel <= 2.0 ** -18).all()), (call, float(rel.max()))
            worst = max(worst, float(rel.max()) / 2.0 ** -18)
    assert int(ctx.lib.pcy_ctx_sync(ctx.h)) == 0
    return worst


@pytest.mark.parametrize("nrows", [1, 3])
@pytest.mark.parametrize("V", [2, 1000, 1025, 128256])
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_qa_probs_ties_and_rounding(dtype, V, nrows):
    """pcy_qa_probs: the argmax is the lowest index of the maximum of the STORED probabilities (equal logits in one thread, in
    neighbouring lanes, waves and at the two ends of the row; two top logits one ulp apart, whose probabilities may round to the same
    value), yes / no are bit-equal to the stored vector (equal ids, 0 and V - 1 included), nothing depends on probs_out being wanted, and
    the probabilities are the float64 softmax rounded once (bf16) or within 2^-18 relative (fp32).  V below, at and above the 1024
    threads of the workgroup."""
    worst = _check_qa(V, nrows, dtype, masked=False)
    record_parity(f"select_qa_{'bf16' if dtype == BF else 'fp32'}_V{V}_rows{nrows}", worst_prob_err_over_bound=worst)


@pytest.mark.parametrize("V", [1000, 128256])
@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32"])
def test_qa_probs_masked_logits(dtype, V):
    worst = _check_qa(V, 3, dtype, masked=True)
    record_parity(f"select_qa_masked_{'bf16' if dtype == BF else 'fp32'}_V{V}", worst_prob_err_over_bound=worst)


# ------------------------------------------------------------------------------------------------ sampling pick
def _uniform_us(V):
    """uniform variates at the boundaries of the inverse CDF of a uniform row: first / last token, lane, 64-token and wave boundaries"""
    us = [Fraction(0), Fraction(1, V), Fraction(63, V), Fraction(64, V), Fraction(V // 16 - 1, V), Fraction(V // 16, V), Fraction(1, 2),
          1 - Fraction(1, 2 ** 24)]
    return [u for u in us if u < 1]                        # 64 / V is no variate of [0, 1) at V = 64


def _sample_once(eng, st, cache, logits, u, temperature=1.0, nucleus=None):
    """one pcy_sample_pick on `logits` [B, V] with the variates u [B] -> tokens, logprob gain, probs_out (all on the CPU).  The
    accumulator holds logprob_preload's -8.0 beforehand: the kernel must ADD the step's value, and the gain is read back exactly."""
    B, V = logits.shape
    st.logits.copy_(logits)
    pre = logprob_preload(logits)
    st.logprob.copy_(pre)
    st.step.zero_()
    pos0 = int(st.pos)
    probs = torch.empty(B, V, dtype=BF, device="cuda")
    eng.sample_pick(cache, st, B, True, u.cuda(), temperature, nucleus, probs)
    tok = st.next_tok.cpu().long()
    assert torch.equal(st.tokens_out[:, 0].cpu().long(), tok) and int(st.step) == 1 and int(st.pos) == pos0 + 1
    return tok, st.logprob.cpu() - pre, probs.cpu()


@pytest.mark.parametrize("nucleus", [None, 0.5, 0.9])
@pytest.mark.parametrize("V", [64, 2048, 4096])
def test_sample_pick_uniform_rows_exact(V, nucleus):
    """All logits equal: p = 1 / V and every partial sum are exact in fp32, so nothing needs a tolerance.  Without the nucleus mask the
    token is floor(u * V); with it the kept set is the stable-sort mask of the reference (a suffix of the indices: inside the tie run the
    lower indices count as the smaller probabilities) and the token is the exact inverse CDF over that set."""
    from procyon_amd.engine import GenState
    eng = _engine(V)
    us = _uniform_us(V)
    B = len(us)
    st, cache = GenState(B, V, 1, "cuda"), eng.new_cache(B, 16)
    logits = torch.full((B, V), 0.75, dtype=BF)
    u = torch.tensor([float(x) for x in us], dtype=torch.float32)
    assert [Fraction(float(x)) for x in u] == us           # the variates are exact in fp32
    tok, lp, p = _sample_once(eng, st, cache, logits, u, nucleus=nucleus)
    full = torch.full((V,), 1.0 / V, dtype=BF)
    keep = torch.ones(V, dtype=torch.bool) if nucleus is None else nucleus_keep_stable(full[None], nucleus)[0]
    kept = keep.nonzero().view(-1)
    n = len(kept)
    assert 0 < n <= V and torch.equal(kept, torch.arange(V - n, V))
    for b in range(B):
        assert torch.equal(p[b], torch.where(keep, full, torch.zeros_like(full))), (b, int((p[b] > 0).sum()), n)
    expect = torch.tensor([int(kept[min(math.floor(x * n), n - 1)]) for x in us])
    assert torch.equal(tok, expect), (tok.tolist(), expect.tolist())
    worst = assert_rounded_from(lp, torch.full((B,), -math.log(V), dtype=torch.float64), 2.0 ** -18 * max(1.0, math.log(V)), "uniform logprob")
    record_parity(f"select_sample_uniform_V{V}_nucleus{nucleus}", worst_logprob_err_over_bound=worst, kept=n)


@pytest.mark.parametrize("nucleus", [None, 0.9])
@pytest.mark.parametrize("V", [4096, 128256])
def test_sample_pick_dominated_row(V, nucleus):
    """One logit 40, the rest -30: whatever the variate, the dominant token is drawn (wherever it sits in the row)."""
    from procyon_amd.engine import GenState
    eng = _engine(V)
    where = [0, V // 3, V - 1]
    us = [0.3, 0.999]
    B = len(where) * len(us)
    st, cache = GenState(B, V, 1, "cuda"), eng.new_cache(B, 16)
    logits = torch.full((B, V), -30.0, dtype=BF)
    expect = torch.tensor([w for w in where for _ in us])
    logits[torch.arange(B), expect] = 40.0
    tok, lp, p = _sample_once(eng, st, cache, logits, torch.tensor(us * len(where), dtype=torch.float32), nucleus=nucleus)
    assert torch.equal(tok, expect), (tok.tolist(), expect.tolist())
    assert bool((p[torch.arange(B), expect] == 1.0).all())
    worst = assert_rounded_from(lp, log_softmax64(logits)[torch.arange(B), tok], logprob_slack(logits, tok), "dominated logprob")
    record_parity(f"select_sample_dominated_V{V}_nucleus{nucleus}", worst_logprob_err_over_bound=worst)


@functools.lru_cache(maxsize=None)
def _sample_rows(V, masked):
    g = torch.Generator().manual_seed(3 * V + masked)
    chunk = (V + PICK_NB - 1) // PICK_NB
    nch = (V + chunk - 1) // chunk
    rows = torch.stack([(torch.randn(V, generator=g) * s).to(BF) for s in (1.0, 2.0, 4.0, 1.0, 3.0, 2.0)])
    if masked:
        for r, kinds in enumerate((["scatter"], [0], [-1], [nch // 2, "scatter"], [0, 1, -1, -2], [nch // 3])):
            _ban(rows[r], g, V, chunk, kinds)
    assert bool((torch.isfinite(rows.float()).sum(-1) >= 16).all())
    u = torch.rand(len(rows), generator=g)
    u[1], u[2] = 0.0, 1 - 2.0 ** -24            # masked: the first chunk banned with u = 0, the last one with u next to 1
    return rows, u


def _check_sample_random(V, masked, temperature, nucleus):
    from oracle import llama_ref as LR
    from procyon_amd.engine import GenState
    eng = _engine(V)
    rows, u = _sample_rows(V, masked)
    B = len(rows)
    st, cache = GenState(B, V, 1, "cuda"), eng.new_cache(B, 16)
    tok, lp, p = _sample_once(eng, st, cache, rows, u, temperature, nucleus)
    banned = torch.isinf(rows.float())
    assert not bool(torch.isnan(p.float()).any()) and bool((p[banned] == 0).all())
    ar = torch.arange(B)
    assert not bool(banned[ar, tok].any()) and bool((p[ar, tok] > 0).all())
    w_lp = assert_rounded_from(lp, log_softmax64(rows)[ar, tok], logprob_slack(rows, tok), f"sampling logprob V={V}")
    # the probability vector: the float64 softmax of the (bf16) scaled logits rounded once, wherever the nucleus mask kept it
    scaled = rows if (nucleus is not None or temperature == 1.0) else rows / temperature
    ref = softmax64(scaled)
    kept = p > 0
    if nucleus is None:
        w_p = assert_rounded_from(p, ref, 2.0 ** -18 * ref, f"sampling probs V={V}")
    else:
        w_p = assert_rounded_from(p[kept], ref[kept], 2.0 ** -18 * ref[kept], f"sampling probs V={V}")
    # the draw: the inverse CDF over the engine's own vector, unless u * total lies within fp32 rounding of a CDF step
    t_ref = LR.sample_token(p.float(), u)
    cdf = p.double().cumsum(-1)
    for b in range(B):
        if tok[b] != t_ref[b]:
            target = float(u[b]) * float(cdf[b, -1])
            near = min(abs(float(cdf[b, tok[b]]) - target), abs(float(cdf[b, t_ref[b]]) - target))
            assert near < 1e-5 * float(cdf[b, -1]), (b, int(tok[b]), int(t_ref[b]))
    assert int(eng.ctx.lib.pcy_ctx_sync(eng.ctx.h)) == 0
    return w_lp, w_p


@pytest.mark.parametrize("mode", ["temp1.0", "temp0.7", "nucleus0.9"])
@pytest.mark.parametrize("V", [193, 128256])
def test_sample_pick_random_rows_rounded_once(V, mode):
    nuc = float(mode[7:]) if mode.startswith("nucleus") else None
    temp = float(mode[4:]) if mode.startswith("temp") else 1.0
    w_lp, w_p = _check_sample_random(V, False, temp, nuc)
    record_parity(f"select_sample_random_V{V}_{mode}", worst_logprob_err_over_bound=w_lp, worst_prob_err_over_bound=w_p)


@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("V", [193, 16385, 128256])
def test_sample_pick_masked_logits(V, temperature):
    """Nucleus off, -inf logits scattered and in whole chunks of both chunked statistics (raw and temperature-scaled): probability exactly
    0 and never drawn -- with u = 0 behind a banned first chunk and u next to 1 in front of a banned last one --, no NaN anywhere."""
    w_lp, w_p = _check_sample_random(V, True, temperature, None)
    record_parity(f"select_sample_masked_V{V}_temp{temperature}", worst_logprob_err_over_bound=w_lp, worst_prob_err_over_bound=w_p)


# ------------------------------------------------------------------------------------------------ beam step
def _away_from_midpoints(tab):
    """every log-softmax value of every table row lies further than the kernel's fp32 error budget from a bf16 rounding midpoint, so the
    once-rounded float64 value is THE value a correct fp32 kernel stores and scores can be compared bit for bit"""
    truth, slack = log_softmax64(tab), logprob_slack(tab)
    fin = torch.isfinite(truth)
    r = truth.float().to(BF).double()
    room = bf16_half_ulp_towards(r.float(), truth) - (r - truth).abs()
    return bool((room[fin] > slack.expand_as(truth)[fin]).all())


@functools.lru_cache(maxsize=None)
def _beam_reference(B, beam, g, V, steps, masked):
    """The CPU side: the tables, the penalty and the oracle's run under the kernel's tie rule (no GPU involved)."""
    from unittest import mock
    from oracle import llama_ref as LR
    BB, M, eos = B * beam, 13, V - 1
    slice_ = (V + BEAM_NCH - 1) // BEAM_NCH
    for seed in range(8):
        gen = torch.Generator().manual_seed(1000 * seed + B * 100 + beam + 17 * masked)
        tab = torch.randint(-3, 4, (steps, M, V), generator=gen).to(BF)                    # [steps, M, V]: seven levels, ties everywhere
        if masked:
            tab[torch.rand(steps, M, V, generator=gen) < 0.2] = NINF
            for s_ in range(steps):
                for m in range(M):
                    if (s_ + m) % 2 == 0:                                                  # a whole slice of every other row, the step-0 row included
                        c = (3 * s_ + m) % ((V + slice_ - 1) // slice_)
                        tab[s_, m, c * slice_:(c + 1) * slice_] = NINF
            assert int(torch.isfinite(tab.float()).sum(-1).min()) > beam * BEAM_NCH
        if _away_from_midpoints(tab):
            break
    else:
        pytest.fail("no table whose log-softmax levels all stay clear of the bf16 rounding midpoints in 8 seeds")
    # a penalised token ties with an unpenalised one: the penalty is the exact distance of the two highest levels of the step-0 row
    lv = torch.unique(lsm_rounded_once(tab[0, 0]).float())
    penalty = float(lv[-1] - lv[-2])
    assert penalty > 0 and math.isfinite(penalty)
    state = {"i": 0}

    def enc(input_embeds=None, input_ids=None, attn_masks=None, past_key_values=None):
        i = state["i"]
        state["i"] += 1
        if input_ids is None:
            lg = tab[0, 0][None].expand(BB, V)                   # identical rows after the prompt, as in the real model
            past = [[torch.zeros(BB, 1, 1, 1), torch.zeros(BB, 1, 1, 1)]]
        else:
            lg = tab[i][(input_ids.view(-1) * 7 + 3) % M]
            past = past_key_values
        return lg[:, None, :].clone(), past

    trace = []
    # Selections in which a PENALISED candidate (a token an earlier group of the step picked) ties with an unpenalised one exactly at the
    # cut between rank g and g + 1 -- what the exact penalty is for.  The oracle calls bincount for the penalty of every group but the
    # first and then topk(g) on the penalised scores: the two spies pair them up.
    pen = {"count": None, "ties": 0}
    orig_bincount = torch.bincount

    def bincount_spy(*a, **kw):
        pen["count"] = orig_bincount(*a, **kw)
        return pen["count"]

    def topk_spy(self, k, *a, **kw):
        if k == g and pen["count"] is not None:
            flat = self.float()
            v = stable_topk(flat, g + 1).values
            penalised = (pen["count"] > 0).repeat(flat.numel() // V)
            at_cut = flat == v[g]
            if float(v[g - 1]) == float(v[g]) and bool((at_cut & penalised).any()) and bool((at_cut & ~penalised).any()):
                pen["ties"] += 1
            pen["count"] = None
        return stable_topk(self, k, *a, **kw)

    # the kernel's documented rules: ties go to the lowest flat index r * V + v (a stable sort), log-softmax rounded once
    with mock.patch.object(LR.F, "log_softmax", lsm_rounded_once), mock.patch.object(torch.Tensor, "topk", topk_spy), \
            mock.patch.object(torch, "bincount", bincount_spy):
        t_ref, s_ref, lg_ref = LR.beam_search(enc, torch.zeros(B, 3, 8), torch.ones(B, 3), vocab_size=V, eos_id=eos, max_len=steps,
                                              beam_size=beam, beam_group_size=g, diversity_penalty=penalty, trace=trace)
    n_ref = state["i"]
    ties = [(i, b, k) for (i, b, k, top) in trace if float(top[g - 1]) == float(top[g])]
    return dict(tab=tab, penalty=penalty, eos=eos, t_ref=t_ref, s_ref=s_ref, lg_ref=lg_ref, n_ref=n_ref, ties=ties, n_sel=len(trace), seeds=seed + 1, penalised_ties=pen["ties"])


def _run_beam_case(B, beam, g, V, steps, masked):
    from procyon_amd.engine import BeamState, Context, LlamaEngine
    ref = _beam_reference(B, beam, g, V, steps, masked)
    tab, penalty, eos, t_ref, s_ref, lg_ref, n_ref, ties = (ref[k] for k in ("tab", "penalty", "eos", "t_ref", "s_ref", "lg_ref", "n_ref", "ties"))
    BB, M = B * beam, 13
    # the run is about ties: every step holds a selection whose rank-g and rank-(g+1) candidates are equal
    assert {i for i, _, _ in ties} == set(range(n_ref)), (sorted({i for i, _, _ in ties}), n_ref)
    assert bool(torch.isfinite(s_ref).all())
    # With fewer top-level tokens in the step-0 row than beams (V / 7 < beam), the second group of step 0 has to choose among the first
    # group's picks, which the exact penalty has moved onto the second level, and the unpenalised tokens of that level: a penalised
    # candidate ties with an unpenalised one at the cut.  (At the larger vocabularies the cut stays inside the top level.)
    if V < 7 * beam:
        assert ref["penalised_ties"] >= 1, ref["penalised_ties"]
    # ---- the kernel, driven the same way
    ctx = Context.get()
    bs = BeamState(B, beam, steps, eos, prompt_len=3, device="cuda")
    tabd = tab.cuda()
    beam_step = LlamaEngine.beam_step.__get__(type("E", (), {"ctx": ctx})())   # the wrapper needs only .ctx
    rec = torch.zeros(steps, BB, V, dtype=BF, device="cuda")
    for i in range(steps):
        lg = tabd[0, 0][None].expand(BB, V).contiguous() if i == 0 else tabd[i][(bs.next_tok.long() * 7 + 3) % M].contiguous()
        rec[i] = lg
        beam_step(lg, bs, g, penalty)
    tok, n = bs.tokens()
    assert n == n_ref, (n, n_ref)
    assert not bool(torch.isnan(bs.cur).any())
    assert torch.equal(tok.cpu().view(B, beam, n), t_ref[:, :, :n])
    assert torch.equal(bs.cur.cpu().view(B, beam), s_ref)
    assert int(bs.pos) == 3 + (n - 1)
    # logits record: per-slot rows + the parent chain == the reference's record (re-indexed by every step's parents)
    anc = bs.anc[:n].cpu().long()
    slot = torch.arange(BB)
    for s_ in range(n - 1, -1, -1):
        slot = anc[s_][slot]
        assert torch.equal(rec[s_].cpu()[slot], lg_ref.view(BB, -1, V)[:, s_]), s_
    # no chosen token was banned in the row it was chosen from
    assert bool(torch.isfinite(lg_ref.view(BB, -1, V)[:, :n].float().gather(-1, t_ref.view(BB, -1)[:, :n, None])).all())
    assert int(ctx.lib.pcy_ctx_sync(ctx.h)) == 0
    return len(ties), ref["n_sel"], ref["seeds"], penalty, ref["penalised_ties"]


@pytest.mark.parametrize("B,beam,g,V,steps", [(1, 4, 2, 300, 6), (2, 6, 2, 481, 5), (1, 10, 2, 4099, 4), (2, 8, 4, 37, 5)])
def test_beam_step_under_ties(B, beam, g, V, steps):
    """pcy_beam_step against oracle.llama_ref.beam_search on tables of seven integer levels, where nearly every selection has an exact
    tie at the cut between rank g and g + 1 and the diversity penalty makes penalised tokens tie with unpenalised ones: the oracle takes
    the kernel's documented rule (stable sort = lowest flat index r * V + v) and the once-rounded log-softmax, and tokens, running scores,
    step count, position and the parent chain of the logits record must be equal.  This exercises the rule in all three places it is
    implemented, and the claim that a group's picks lie among the `beam` best entries of each of the 16 slices of a row when far more than
    `beam` entries of a slice are equal.  (2, 8, 4, 37, 5): slices shorter than `beam` and three empty ones, and the shape at which
    penalised tokens tie with unpenalised ones AT the cut (asserted from the oracle's run)."""
    n_ties, n_sel, seeds, penalty, n_pen = _run_beam_case(B, beam, g, V, steps, masked=False)
    record_parity(f"select_beam_ties_B{B}_beam{beam}_g{g}_V{V}", selections_with_tie_at_cut=n_ties, selections=n_sel, seeds_tried=seeds, penalty=penalty,
                  penalised_ties_at_cut=n_pen)


def test_beam_step_masked_logits():
    """The same run with banned tokens: a fifth of every row -inf, and a whole slice (ceil(V / 16) entries) of every other row -- whose
    partial must be (max = -inf, sum = 0) for the row's log-sum-exp to stay a number.  No NaN score, no banned token chosen."""
    n_ties, n_sel, seeds, penalty, n_pen = _run_beam_case(2, 6, 2, 481, 5, masked=True)
    record_parity("select_beam_masked_B2_beam6_g2_V481", selections_with_tie_at_cut=n_ties, selections=n_sel, seeds_tried=seeds, penalty=penalty,
                  penalised_ties_at_cut=n_pen)
