"""GPU: beam search and sampling selection of an fp32 generation on the device (procyon_amd/csrc/pcy_f32_select.hip, the fp32 instantiation
of the beam step in pcy_elem.hip, include/pcy.h).  Single steps are held to the float64 restatements of
tests/f32_select_ref.py on fixtures that tests/test_f32_select_cpu.py shows to be decidable: tokens, parents and kept sets exactly, running
scores and log-probabilities within the project's 2^-18 budget (select_oracle.logprob_slack), probabilities within 2^-18 p + 2^-149, masses
and CDF points within DELTA = 2^-18.  Chains and the model are held to the oracle at the bars of tests/test_gpu_f32_stream.py (tokens equal,
scores atol 1e-3, logits < 1e-4) and to their own separate calls bit for bit."""
import functools
import os

import pytest
import torch

import f32_ref as R
import f32_select_ref as Q
import f32_stream_ref as S
from conftest import record_parity, rel_err
from select_oracle import log_softmax64, logprob_slack, softmax64

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the beam step against float64
def _beam_engine():
    """the wrapper needs only .ops"""
    from procyon_amd.engine_f32 import F32Ops, LlamaEngineF32
    return type("E", (), {"ops": F32Ops(), "beam_step": LlamaEngineF32.beam_step})()


def _beam_arrays(bs):
    return {k: getattr(bs, k).clone() for k in ("out", "cur", "cur_new", "next_tok", "src", "anc", "has_eos", "blk_eos", "ticket", "pos", "step", "done")}


def _run_beam_case(case):
    from procyon_amd.engine import BeamState
    B, beam, g, V, steps = case[:5]
    c = Q.beam_case(*case)
    ref, tab = c["ref"], c["tab"].cuda()
    BB, n = B * beam, c["ref"]["n"]
    eng = _beam_engine()
    bs = BeamState(B, beam, steps, c["eos"], prompt_len=Q.BEAM_PROMPT, device="cuda")
    srcs = []
    for i in range(n):
        eng.beam_step(Q.table_step(tab, i, None if i == 0 else bs.next_tok, BB), bs, g, Q.BEAM_PENALTY)
        srcs.append(bs.src.clone())
    tok, n_got = bs.tokens()
    assert n_got == n, (n_got, n)
    assert torch.equal(tok.cpu(), ref["tokens"]), (tok.cpu(), ref["tokens"])
    assert torch.equal(torch.stack(srcs).cpu().long(), ref["src"]) and torch.equal(bs.anc[:n].cpu().long(), ref["src"])
    assert torch.equal(bs.next_tok.cpu().long(), ref["tokens"][:, n - 1])
    assert torch.equal(bs.has_eos[n & 1].cpu().bool(), ref["has_eos"])
    assert int(bs.done) == int(ref["done"]) and int(bs.pos) == ref["pos"] and int(bs.ticket) == 0
    # running scores: the sum over the steps of logprob_slack along the slot's history + one fp32 ulp of the score per step
    cur, truth = bs.cur.cpu().double(), ref["scores"]
    assert not bool(torch.isnan(cur).any())
    ulp = torch.pow(torch.tensor(2.0, dtype=F64), torch.floor(torch.log2(truth.abs().clamp_min(2.0 ** -126))) - 23.0)
    bound = ref["slack"] + n * ulp
    err = (cur - truth).abs()
    print(f"beam {case}: worst |cur - truth| {float(err.max()):.3e}, bound there {float(bound[err.argmax()]):.3e}, seeds tried {c['seeds']}")
    assert bool((err <= bound).all()), (err, bound)
    ties = sum(gap == 0.0 for sel in ref["gaps"] for gap, _ in sel)
    record_parity("f32_select_beam_" + "_".join(str(x) for x in case), worst_score_err_over_bound=float((err / bound).max()), exact_ties=ties, steps=n)
    return eng, bs, tab, BB, g


@pytest.mark.parametrize("case", Q.BEAM_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_beam_step_under_ties(case):
    """pcy_f32_beam_step against the float64 beam search on tables of integer levels: nearly every selection is decided by the tie rule
    (lowest flat index r * V + v), among them ties between identical rows with identical scores; tokens, parents (src, anc), histories,
    EOS flags, done / step / pos equal, running scores within the 2^-18 budget"""
    _run_beam_case(case + (False, None))


def test_beam_step_masked_logits():
    """a fifth of every row -inf and a whole slice (ceil(V / 16) entries) of every other row: its partial must be (max = -inf, sum = 0);
    no NaN score, no banned token chosen"""
    _, bs, _, _, _ = _run_beam_case(Q.BEAM_MASKED + (True, None))
    assert bool(torch.isfinite(bs.cur).all())              # (a banned token would have brought -inf into its slot's score)


def test_beam_step_after_done_changes_nothing():
    """every beam takes the EOS at step 2 of 5: done is raised there, and a further launch leaves every array bit-identical -- but src, which
    it sets to the identity so that the reorder behind it moves nothing (the bf16 step's rule)"""
    eng, bs, tab, BB, g = _run_beam_case(Q.BEAM_DONE + (False, 2))
    assert int(bs.done) == 1 and int(bs.step) == 3
    before = _beam_arrays(bs)
    eng.beam_step(Q.table_step(tab, 3, bs.next_tok, BB), bs, g, Q.BEAM_PENALTY)
    after = _beam_arrays(bs)
    for k in before:
        if k == "src":
            assert torch.equal(after[k].cpu(), torch.arange(BB, dtype=torch.int32)), k
        elif before[k].dtype == F32:
            assert torch.equal(_bits(before[k]), _bits(after[k])), k
        else:
            assert torch.equal(before[k], after[k]), k


def test_beam_step_refusals():
    from procyon_amd import _lib as L
    from procyon_amd.engine import BeamState
    eng = _beam_engine()
    lg = torch.zeros(33, 50, device="cuda")
    n0 = eng.ops.lib.pcy_debug_f32_select_count(0)
    with pytest.raises(L.PcyError, match="beam"):
        eng.beam_step(lg, BeamState(1, 33, 4, 2, 3, "cuda"), 3, 0.8)
    with pytest.raises(L.PcyError, match="group_size"):
        eng.beam_step(lg[:4], BeamState(1, 4, 4, 2, 3, "cuda"), 3, 0.8)
    assert eng.ops.lib.pcy_debug_f32_select_count(0) == n0


# ------------------------------------------------------------------------------------------------ 2. the sampling step against float64
@functools.lru_cache(maxsize=None)
def _engine(V):
    """a one-layer engine: the selection kernels read only its vocabulary size"""
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig
    from procyon_amd.engine_f32 import LlamaEngineF32
    kw = dict(vocab=V, d=64, n_layers=1, n_heads=2, n_kv_heads=1, ffn=128)
    return LlamaEngineF32(synth.llama_state_dict(**kw, dtype=F32), LlamaConfig(**kw, max_pos=64))


def _sample_once(eng, rows, u, temperature, nucleus):
    """one pcy_f32_sample_pick at step 1 of 3 (the variates of step 0 are poison) -> tokens, logprob gain, probs_out on the CPU"""
    B, V = rows.shape
    st, cache = eng.new_gen_state(B, 3), eng.new_cache(B, 8)
    st.logits.copy_(rows)
    st.set(pos=2, step=1)
    probs = torch.full((B, V), -1.0, dtype=F32, device="cuda")
    uv = torch.cat([torch.full((B,), 0.999), u.to(F32), torch.full((B,), 0.999)]).cuda()
    eng.sample_pick(cache, st, B, True, uv, temperature, nucleus, probs)
    tok = st.next_tok.cpu().long()
    assert torch.equal(st.tokens_out[:, 1].cpu().long(), tok) and bool((st.tokens_out[:, [0, 2]] == 0).all())
    assert int(st.step) == 2 and int(st.pos) == 3
    return tok, st.logprob.cpu(), probs.cpu()


def _check_sample(rows, kinds, u, tok, lp, p_out, temperature, nucleus):
    """the step's rules per row, from float64 alone: probabilities, kept set, the drawn token's CDF interval, the log-probability"""
    B, V = rows.shape
    p64, keep64 = Q.sampling_probs64(rows, temperature, nucleus)
    full64 = softmax64(Q.scaled_logits(rows, 1.0 if nucleus is not None else temperature))
    banned = torch.isinf(rows)
    assert not bool(torch.isnan(p_out).any()) and bool((p_out >= 0).all()) and bool((p_out[banned] == 0).all())
    kept = p_out > 0
    tol = 2.0 ** -18 * full64 + 2.0 ** -149
    err = (p_out.double() - full64).abs()
    where = kept if nucleus is not None else torch.ones_like(kept)
    assert bool((err[where] <= tol[where]).all()), float((err[where] / tol[where]).max())
    if nucleus is not None:
        cum, thr = Q.nucleus_cum64(full64), 1.0 - nucleus
        assert bool(kept[cum >= thr + Q.DELTA].all()), "a token whose cumulative mass is clearly past the threshold was dropped"
        assert not bool(kept[cum < thr - Q.DELTA].any()), "a token whose cumulative mass is clearly short of the threshold was kept"
        for b, kind in enumerate(kinds):
            if kind == "uniform":              # ties decide everything: the kept indices are exact (the suffix of the stable sort)
                assert torch.equal(kept[b], keep64[b]), (int(kept[b].sum()), int(keep64[b].sum()))
                n = int(kept[b].sum())
                assert torch.equal(kept[b].nonzero().view(-1), torch.arange(V - n, V))
    ar = torch.arange(B)
    assert bool(kept[ar, tok].all()) and not bool(banned[ar, tok].any())
    cdf = (full64 * kept).cumsum(-1)
    total = cdf[:, -1]
    target = u.to(F32).double() * total
    hi = cdf[ar, tok]
    lo = torch.where(tok > 0, cdf[ar, (tok - 1).clamp_min(0)], torch.zeros_like(hi))
    assert bool((lo - Q.DELTA * total <= target).all()) and bool((target <= hi + Q.DELTA * total).all()), (tok, lo, target, hi)
    lp_err = (lp.double() - log_softmax64(rows)[ar, tok]).abs()
    assert bool((lp_err <= logprob_slack(rows, tok)).all()), (lp_err, logprob_slack(rows, tok))
    for b, kind in enumerate(kinds):
        if kind == "one_left":
            assert int(tok[b]) == int(rows[b].argmax()), (kind, int(tok[b]))
    return float((err[where] / tol[where]).max()), float((lp_err / logprob_slack(rows, tok)).max())


@pytest.mark.parametrize("mode", list(Q.SAMPLE_MODES))
@pytest.mark.parametrize("V", Q.SAMPLE_V)
def test_sample_pick_vs_float64(V, mode):
    """pcy_f32_sample_pick on uniform, dominated, random and masked rows, 5 rows at a time and the all-but-one-masked row alone, for every
    variate of SAMPLE_US: probabilities, kept set, drawn token and log-probability by the float64 rules; two runs bit-equal"""
    temperature, nucleus = Q.SAMPLE_MODES[mode]
    eng, all_rows = _engine(V), Q.sample_rows(V)
    worst_p = worst_lp = 0.0
    for sel in (slice(0, 5), slice(5, 6)):
        rows, kinds = all_rows[sel].contiguous(), Q.SAMPLE_KINDS[sel]
        for u_ in Q.SAMPLE_US:
            u = torch.full((rows.shape[0],), u_, dtype=F64)
            tok, lp, p = _sample_once(eng, rows, u, temperature, nucleus)
            wp, wl = _check_sample(rows, kinds, u, tok, lp, p, temperature, nucleus)
            worst_p, worst_lp = max(worst_p, wp), max(worst_lp, wl)
        tok2, lp2, p2 = _sample_once(eng, rows, u, temperature, nucleus)
        assert torch.equal(tok, tok2) and torch.equal(_bits(lp), _bits(lp2)) and torch.equal(_bits(p), _bits(p2))
    assert int(eng.ops.lib.pcy_ctx_sync(eng.ops.h)) == 0
    record_parity(f"f32_select_sample_V{V}_{mode}", worst_prob_err_over_bound=worst_p, worst_logprob_err_over_bound=worst_lp)


def test_sample_pick_refusals():
    from procyon_amd import _lib as L
    eng = _engine(64)
    st, cache = eng.new_gen_state(2, 2), eng.new_cache(2, 8)
    u = torch.zeros(4, device="cuda")
    n0 = eng.select_count(1)
    for kw, what in ((dict(temperature=0.0), "temperature"), (dict(nucleus_prob=1.0), "nucleus_prob")):
        with pytest.raises(L.PcyError, match=what):
            eng.sample_pick(cache, st, 2, True, u, **kw)
    with pytest.raises(L.PcyError, match="B=3"):
        eng.sample_pick(cache, st, 3, True, u)
    assert eng.select_count(1) == n0 and int(st.step) == 0


# ------------------------------------------------------------------------------------------------ 3. reorder and copy
KV_MAPS = {"identity": [0, 1, 2, 3, 4, 5], "all_from_0": [0, 0, 0, 0, 0, 0], "two_cycle": [1, 0, 2, 3, 4, 5], "three_cycle": [1, 2, 0, 3, 4, 5],
           "r_div_3": [0, 0, 0, 1, 1, 1]}


@functools.lru_cache(maxsize=None)
def _kv_engine():
    """L = 2, Hkv * dh = 2 * 16"""
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig
    from procyon_amd.engine_f32 import LlamaEngineF32
    kw = dict(vocab=64, d=32, n_layers=2, n_heads=2, n_kv_heads=2, ffn=64)
    return LlamaEngineF32(synth.llama_state_dict(**kw, dtype=F32), LlamaConfig(**kw, max_pos=64))


def _filled_cache(eng, rows, Tmax, seed):
    c = eng.new_cache(rows, Tmax)
    g = torch.Generator().manual_seed(seed)
    c.k.copy_(torch.randn(c.k.shape, generator=g))
    c.v.copy_(torch.randn(c.v.shape, generator=g))
    return c


@pytest.mark.parametrize("t0,t", [(0, 4), (3, 10), (5, 5)])
@pytest.mark.parametrize("name", list(KV_MAPS))
def test_kv_reorder_range(name, t0, t):
    """rows [0, 6) of an 8-row cache of 10 slots: the moved slots equal the gathered source bitwise (any map: cycles, one source for many
    rows); slots outside [t0, t) and rows >= 6 are intact"""
    eng = _kv_engine()
    cache = _filled_cache(eng, 8, 10, 7)
    k0, v0 = cache.k.clone(), cache.v.clone()
    m = torch.tensor(KV_MAPS[name])
    eng.kv_reorder(cache, m, t, t0=t0)
    for got, orig in ((cache.k, k0), (cache.v, v0)):
        want = orig.clone()
        want[:, :6, t0:t] = orig[:, m.cuda(), t0:t]
        assert torch.equal(_bits(got), _bits(want)), name


def test_kv_copy_rows_and_refusals():
    """a 2-row cache of 7 slots into rows [0, 6) of an 8-row cache of 10: slots [0, 4) equal the source rows r // 3, everything else intact"""
    from procyon_amd import _lib as L
    eng = _kv_engine()
    src, dst = _filled_cache(eng, 2, 7, 8), _filled_cache(eng, 8, 10, 9)
    k0, v0 = dst.k.clone(), dst.v.clone()
    m = torch.arange(6) // 3
    eng.kv_copy_rows(dst, src, m, 4)
    for got, orig, s in ((dst.k, k0, src.k), (dst.v, v0, src.v)):
        want = orig.clone()
        want[:, :6, :4] = s[:, m.cuda(), :4]
        assert torch.equal(_bits(got), _bits(want))
    with pytest.raises(L.PcyError, match="slots"):
        eng.kv_copy_rows(dst, src, m, 8)                       # the source holds 7
    with pytest.raises(L.PcyError, match="out of place"):
        eng.kv_copy_rows(dst, dst, m, 4)
    with pytest.raises(L.PcyError, match="B=9"):
        eng.kv_reorder(dst, torch.arange(9), 4)
    with pytest.raises(L.PcyError, match="slots"):
        eng.kv_reorder(dst, torch.arange(6), 11)
    assert torch.equal(_bits(dst.k[:, :6, :4]), _bits(src.k[:, m.cuda(), :4]))     # the refusals wrote nothing


# ------------------------------------------------------------------------------------------------ 4. the chain
@pytest.fixture(scope="module")
def gen():
    from procyon_amd.engine import LlamaConfig
    from procyon_amd.engine_f32 import LlamaEngineF32
    g = S.gen_fixture()
    g["eng"] = LlamaEngineF32(g["sd"], LlamaConfig(**R.GEN_GEOM, max_pos=256))
    return g


def test_generate_beam_matches_the_oracle(gen):
    """LlamaEngineF32.generate_beam on two prompts (one left-padded), beam 4, groups of 2, 5 steps: the oracle's tokens (its smallest
    selection gap asserted first, on the CPU), scores atol 1e-3, logits < 1e-4; the select counter moves by the steps; a cache with room
    for 3 tokens raises before any step"""
    eng = gen["eng"]
    emb, mask = S.beam_fixture(gen)
    kw = S.BEAM_KW
    t_ref, s_ref, l_ref, rel = S.beam_oracle(gen["sd"], gen["geom"], emb, mask, eos_id=2, **kw)
    assert rel > S.BEAM_GAP, rel
    n0 = eng.select_count(0)
    tok, sc, lg = eng.generate_beam(emb, mask, kw["max_len"], kw["beam_size"], kw["beam_group_size"], kw["diversity_penalty"], eos_id=2, max_new=8)
    steps = lg.shape[1]
    assert eng.select_count(0) - n0 >= steps and lg.dtype == F32 and lg.is_pinned() and tok.dtype == torch.int64
    assert tuple(tok.shape) == (2 * kw["beam_size"], kw["max_len"]) and steps == l_ref.shape[2]
    e_rows = [rel_err(lg.view(2, kw["beam_size"], steps, -1)[b], l_ref[b]) for b in range(2)]
    print(f"beam logits error per prompt {e_rows}; scores {sc.tolist()} oracle {s_ref.view(-1).tolist()}")
    record_parity("f32_select_generate_beam", err_logits=max(e_rows), tokens_equal=bool(torch.equal(tok.view_as(t_ref), t_ref)))
    assert torch.equal(tok.view_as(t_ref), t_ref), (tok, t_ref)
    assert torch.allclose(sc.view_as(s_ref), s_ref, atol=1e-3), (sc, s_ref)
    assert max(e_rows) < 1e-4, e_rows
    lib = eng.ops.lib
    n1, s1 = eng.select_count(0), lib.pcy_debug_f32_stream_count()
    with pytest.raises(ValueError, match="capacity"):
        eng.generate_beam(emb, mask, kw["max_len"], kw["beam_size"], kw["beam_group_size"], kw["diversity_penalty"], eos_id=2, max_new=3)
    assert eng.select_count(0) == n1 and lib.pcy_debug_f32_stream_count() == s1
    with pytest.raises(ValueError, match="beam_size"):
        eng.generate_beam(emb, mask, 3, 33, 3, 0.8, eos_id=2, max_new=8)


def _beam_run(gen, chain):
    """generate_beam's opening, then the 4 cached steps as ONE beam_steps call (chain) or as the four separate calls per step"""
    from procyon_amd.engine import BeamState
    from procyon_amd.engine_f32 import GenStateF32
    eng, kw = gen["eng"], S.BEAM_KW
    emb, mask = S.beam_fixture(gen)
    B, T, _ = emb.shape
    beam, g, pen, n = kw["beam_size"], kw["beam_group_size"], kw["diversity_penalty"], kw["max_len"]
    BB, V = B * beam, R.GEN_GEOM["vocab"]
    small = eng.new_cache(B, T)
    lg_b, _ = eng.prefill(emb, mask, "last", cache=small)
    cache = eng.new_cache(BB, T + n)
    eng.kv_copy_rows(cache, small, torch.arange(BB) // beam, T)
    bs = BeamState(B, beam, n, 2, prompt_len=T, device="cuda")
    st = GenStateF32(BB, V, 1, "cuda", pos=bs.pos, next_tok=bs.next_tok)
    rec = torch.zeros(n, BB, V, dtype=F32, device="cuda")
    logits = lg_b.repeat_interleave(beam, dim=0).contiguous()
    rec[0].copy_(logits)
    eng.beam_step(logits, bs, g, pen)
    if chain:
        eng.beam_steps(cache, st, bs, g, pen, rec, n - 1, kv_t0=T)
    else:
        for i in range(1, n):
            eng.decode_stream(cache, st, BB, graph=True)
            rec[i].copy_(st.logits)
            eng.beam_step(st.logits, bs, g, pen)
            eng.kv_reorder(cache, bs.src, T + i, t0=T)         # (host arithmetic: the beam step has advanced *pos to T + i)
    torch.cuda.synchronize()
    assert int(bs.step) == n and int(bs.pos) == T + n - 1
    return bs.out.clone(), bs.cur.clone(), rec, cache.k.clone(), cache.v.clone(), bs.anc.clone()


def test_beam_chain_equals_the_separate_calls(gen):
    """pcy_f32_llama_beam_steps (4 steps enqueued by one call: nothing is read back in between) and decode_stream + copy + beam_step +
    kv_reorder per step: bit-equal histories, scores, record, parents and K / V"""
    a, b = _beam_run(gen, chain=True), _beam_run(gen, chain=False)
    for x, y, what in zip(a, b, ("tokens", "scores", "record", "K", "V", "parents")):
        assert torch.equal(_bits(x.float()) if x.dtype == F32 else x, _bits(y.float()) if y.dtype == F32 else y), what
    assert bool((a[0] != 0).any())


# ------------------------------------------------------------------------------------------------ 5. the sampling loop
def _oracle_logits(gen, toks):
    """the oracle's logits [B, steps, V] for the prefix actually generated (teacher-forced on toks [B, steps])"""
    from oracle import llama_ref as LR
    out, past = [], None
    for i in range(toks.shape[1]):
        r = LR.llama_forward(gen["sd"], gen["geom"], inputs_embeds=gen["emb"], attn_mask=gen["mask"], logits_rows="last") if i == 0 else \
            LR.llama_forward(gen["sd"], gen["geom"], input_ids=toks[:, i - 1:i], attn_mask=None, past_kv=past, logits_rows="last")
        past = r["past_kv"]
        out.append(r["logits"][:, -1, :])
    return torch.stack(out, 1)


@pytest.mark.parametrize("mode", ["temp1.0", "nucleus0.9"])
def test_sampling_loop(gen, mode):
    """generate_sampling with injected variates, 3 rows (left pads 0 / 5 / 1), 6 steps.  Every step's token is held to the ORACLE's float64
    probabilities for the prefix actually generated: the kept set obeys the band rule on the oracle's ascending cumulative masses
    (everything at or past 1 - p + DELTA kept, everything short of 1 - p - DELTA dropped), and the token's CDF interval over the kept
    tokens, widened by DELTA x total on both sides, contains u x total.  The kernel's kept set of a step comes from one more pick on the
    step's recorded logits with the same variate: the pick is a function of (logits, variate), so it must return the loop's token, and it
    writes probs_out.  Eager and replayed runs bit-equal; the recorded logits < 1e-4 from the oracle's; logprob = the sum of the record's
    fp32 log-softmax at the tokens"""
    eng = gen["eng"]
    temperature, nucleus = Q.SAMPLE_MODES[mode]
    B, n = R.GEN_B, R.GEN_STEPS
    u = torch.rand(n * B, generator=torch.Generator().manual_seed(77))
    n0 = eng.select_count(1)
    runs = {}
    for graph in (False, True):
        tok, lp, lg, _ = eng.generate_sampling(gen["emb"], gen["mask"], n, temperature=temperature, nucleus_prob=nucleus, keep_logits=True,
                                               uniforms=u, graph=graph)
        runs[graph] = (tok.cpu(), lp.cpu(), lg.cpu().contiguous())
    assert eng.select_count(1) - n0 == 2 * n
    tok, lp, lg = runs[True]
    assert torch.equal(tok, runs[False][0]) and torch.equal(_bits(lp), _bits(runs[False][1])) and torch.equal(_bits(lg), _bits(runs[False][2]))
    assert tuple(tok.shape) == (B, n) and tok.dtype == torch.int64 and tuple(lg.shape) == (B, n, R.GEN_GEOM["vocab"])
    ora = _oracle_logits(gen, tok)
    e = max(rel_err(lg[b, i], ora[b, i]) for b in range(B) for i in range(n))
    assert e < 1e-4, e
    ar, worst, worst_band = torch.arange(B), 0.0, 0
    for i in range(n):
        ui = u[i * B:(i + 1) * B]
        tok_i, _, p_out = _sample_once(eng, lg[:, i].contiguous(), ui, temperature, nucleus)
        assert torch.equal(tok_i, tok[:, i]), (i, tok_i, tok[:, i])
        kept = p_out > 0
        full_o = softmax64(Q.scaled_logits(ora[:, i], temperature if nucleus is None else 1.0))
        if nucleus is not None:
            cum, thr = Q.nucleus_cum64(full_o), 1.0 - nucleus
            worst_band = max(worst_band, int(Q.band_count(full_o, nucleus).max()))
            assert bool(kept[cum >= thr + Q.DELTA].all()) and not bool(kept[cum < thr - Q.DELTA].any()), i
        else:
            assert bool(kept[full_o > 2.0 ** -126].all()), i
        cdf = (full_o * kept).cumsum(-1)
        total = cdf[:, -1]
        target = ui.to(F32).double() * total
        hi = cdf[ar, tok[:, i]]
        lo = torch.where(tok[:, i] > 0, cdf[ar, (tok[:, i] - 1).clamp_min(0)], torch.zeros_like(hi))
        dist = torch.maximum(torch.maximum(lo - target, target - hi), torch.zeros_like(hi)) / total
        print(f"sampling loop {mode} step {i}: tokens {tok[:, i].tolist()} distance of u x total from the oracle's CDF interval / total {dist.tolist()} (DELTA {Q.DELTA:.3e})")
        worst = max(worst, float(dist.max()))
        assert bool(kept[ar, tok[:, i]].all()) and bool((dist <= Q.DELTA).all()), (i, tok[:, i], lo, target, hi)
    print(f"sampling loop {mode}: all {B * n} draws inside the oracle's CDF interval, worst distance / total {worst:.3e}; most band tokens in a row {worst_band}; logits error {e:.3e}")
    assert worst_band <= Q.BAND_CAP
    want = lg.log_softmax(-1).gather(2, tok[..., None])[..., 0].sum(1)
    assert torch.allclose(lp, want, atol=1e-3), (lp, want)
    record_parity(f"f32_select_sampling_loop_{mode}", err_logits=e, draws_held_to_the_oracle=B * n, worst_cdf_distance=worst)
    with pytest.raises(ValueError, match="capacity"):
        eng.generate_sampling(gen["emb"], gen["mask"], 256, keep_logits=False, uniforms=torch.zeros(256 * B))


# ------------------------------------------------------------------------------------------------ 6. model level
def test_model_generates_with_device_side_selection():
    """UnifiedProCyon.generate(decode_f32="device") on the tiny fp32 model and the inputs of test_model_generates_on_the_stream_step: beam
    search gives the oracle's tokens, scores (atol 1e-3) and logits < 1e-4; nucleus and sampling return the shapes and dtypes of "ops" and
    move the select counter; greedy is bit-equal to "stream"; a bf16 model and beam_size = 33 are ValueErrors"""
    from oracle import esm_ref as ER
    from oracle import llama_ref as LR
    from oracle import procyon_ref as PR
    from procyon_amd import synth
    from procyon_amd import synthetic_model as SM
    m, w = SM.build("small", device="cuda", return_weights=True, max_new_tokens=8, dtype=F32, as_loaded=True)
    m.eval()
    lgeom, egeom = LR.LlamaGeom(**w["geom"]["llama"]), ER.EsmGeom(**w["geom"]["esm"])
    prot = synth.protein_tokens([90, 41], seed=3)
    mk = lambda instr, seq, slots: {
        "data": {"seq": seq, "seq_idx": torch.arange(seq.shape[0]), "text": [], "drug": None},
        "input": {"seq": slots, "text": [[] for _ in instr], "drug": None},
        "target": {"seq": None, "text": None, "drug": None}, "instructions": list(instr)}
    ginstr = ["w4 <|protein|> w5 [ANSWER]", "w1 w2 w3 w6 <|protein|> is w7 w8 ? [ANSWER]"]        # row 0 is left-padded
    gslots = [[1], [0]]
    gids, gmask = m._prepare_text_inputs_and_tokenize(list(ginstr), [[], []], crop_off=True, no_pad=True, left_pad=True)
    z = PR.esm_plm_forward(w["esm"], egeom, prot, pooling="mean")
    gsoft = PR.mlp_forward(z[[1, 0]], w["projs"]["aaseq"])
    gemb, _ = PR.prepare_input_embeddings(w["llama"]["model.embed_tokens.weight"], gids.long(), m.prot_replacement_idx, gsoft, ret_idx=m.prot_retrieval_idx)
    eng = m.text_encoder.engine_f32
    # beam: the oracle's smallest selection gap first (on the CPU, from the oracle alone)
    kw = dict(max_len=5, beam_size=4, beam_group_size=2, diversity_penalty=0.8)
    tb_ref, sb_ref, lb_ref, rel = S.beam_oracle(w["llama"], lgeom, gemb, gmask, eos_id=m.tokenizer.eos_token_id, **kw)
    print("beam selection gap / row norm:", rel)
    assert rel > S.BEAM_GAP, rel
    n0 = eng.select_count(0)
    tb, sb, lb, _ = m.generate(mk(ginstr, prot, gslots), method="beam", decode_f32="device", **kw)
    assert eng.select_count(0) > n0
    eb_rows = [rel_err(lb[b].float(), lb_ref[b]) for b in range(2)]
    print(f"beam logits error per prompt {eb_rows}")
    record_parity("f32_select_model_small_beam", err_beam_logits=max(eb_rows), beam_tokens_equal=bool(torch.equal(tb, tb_ref)))
    assert lb.dtype == F32 and lb.device.type == "cpu" and tb.dtype == torch.int64
    assert torch.equal(tb, tb_ref) and torch.allclose(sb, sb_ref, atol=1e-3), (tb, tb_ref, sb, sb_ref)
    assert max(eb_rows) < 1e-4, eb_rows
    # sampling methods: the shapes and dtypes of the default path; the selection ran on the device
    for method in ("nucleus", "sampling"):
        n1 = eng.select_count(1)
        ts, ls, gs, _ = m.generate(mk(ginstr, prot, gslots), max_len=4, method=method, decode_f32="device")
        assert eng.select_count(1) - n1 == 4
        to, lo, go, _ = m.generate(mk(ginstr, prot, gslots), max_len=4, method=method)
        assert ts.shape == to.shape and ls.shape == lo.shape and gs.shape == go.shape
        assert ts.dtype == to.dtype and ls.dtype == lo.dtype and gs.dtype == go.dtype and gs.device == go.device
        assert rel_err(gs[:, 0, 0].float(), go[:, 0, 0].float()) == 0.0          # step 0 is the prefill's logits on both paths
    # greedy is the stream path
    a = m.generate(mk(ginstr, prot, gslots), max_len=6, method="greedy", decode_f32="device")
    b = m.generate(mk(ginstr, prot, gslots), max_len=6, method="greedy", decode_f32="stream")
    assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(_bits(a[2]), _bits(b[2]))
    # refusals
    with pytest.raises(ValueError, match="beam_size"):
        m.generate(mk(ginstr, prot, gslots), method="beam", decode_f32="device", max_len=3, beam_size=33, beam_group_size=3)
    with pytest.raises(ValueError, match="decode_f32"):
        m.generate(mk(ginstr, prot, gslots), max_len=3, method="greedy", decode_f32="fast")
    m.bfloat16()
    with pytest.raises(ValueError, match="bf16"):
        m.generate(mk(ginstr, prot, gslots), max_len=3, method="beam", decode_f32="device")


from test_gpu_round3 import instruct_env  # noqa: E402,F401  (the fixture that builds the instruction-tuning data tree)


def test_caption_bulk_on_the_device(instruct_env):
    """pipelines.caption_bulk(decode_f32="device") on two proteins of an fp32 embedding-table checkpoint: the model stays fp32, the beam
    search runs on the device (the select counter moves), the table has the script's columns"""
    from procyon.training.training_args_IT import DataArgs, ModelArgs
    from procyon_amd import synth
    from procyon_amd.checkpoint import from_pretrained
    from procyon_amd.pipelines import caption_bulk
    from procyon_amd.tokenizer import SyntheticTokenizer
    tok = SyntheticTokenizer(n_text=2000, base_vocab=2048, bos_token_id=2040, eos_token_id=2041)
    root, D = str(instruct_env / "ckpt32"), 128
    kw = dict(vocab=len(tok) - 1, d=256, n_layers=2, n_heads=2, n_kv_heads=1, ffn=512)
    sd = {"text_encoder.model." + k: v for k, v in synth.llama_state_dict(**kw, dtype=F32).items()}
    for name, (i, o), off in (("token_projectors.aaseq", (D, 256), 0), ("aaseq_shared_projector", (D, D), 20), ("aaseq_lm_projector", (256, D), 40)):
        for j, (wt, b) in zip((0, 3, 6), synth.mlp_layers(3, i, o, 128, off, dtype=F32)):
            sd[f"{name}.{j}.weight"], sd[f"{name}.{j}.bias"] = wt, b
    sd["protein_seq_embeddings.weight"] = torch.randn(20000, D, generator=torch.Generator().manual_seed(77)) * 0.5
    os.makedirs(root, exist_ok=True)
    torch.save(ModelArgs(use_aaseq_embeddings=True, ret_token_access="last", protein_pooling_opt="mean", max_text_len=160), os.path.join(root, "model_args.pt"))
    torch.save(DataArgs(data_dir="/x"), os.path.join(root, "data_args.pt"))
    torch.save(sd, os.path.join(root, "txllm_model_ckpt.pt"))
    model, margs = from_pretrained(checkpoint_dir=root, tokenizer=tok, max_new_tokens=16, max_pos=512)
    assert model._f32
    lib = model.text_encoder.engine_f32.ops.lib
    n0 = lib.pcy_debug_f32_select_count(0)
    ids = ["P00530", "P00007"]
    df = caption_bulk(model, margs, DataArgs(), ids, "uniprot", "all", max_len=4, beam_size=4, diversity_penalty=0.8, batch_size=2, decode_f32="device")
    assert model._f32 and lib.pcy_debug_f32_select_count(0) - n0 >= 1
    assert list(df.columns) == ["uniprot_id", "response0", "response1"] and df["uniprot_id"].tolist() == ids
    with pytest.raises(ValueError, match="decode_f32"):
        caption_bulk(model, margs, DataArgs(), ids, decode_f32="fast")
