"""GPU: the EOS stop of greedy and sampling generation (include/pcy.h, the trailing fields of pcy_gen_state).

Pick level: the four pick kernels (bf16 / fp32, greedy / sampling, the sampling ones with and without the nucleus mask) run tables of logits
written straight into st.logits, once without a stop and once with; the run with a stop is held to tests/stop_eos_ref.py applied to the
tokens of the run without -- tokens, finished, done, the counters -- and its logprob to the partial sums of the run without, bit for bit.
Chains, engines, model: every decode path runs with the option off, takes a token that row 0 emitted at some step >= 1 as the EOS, and runs
again with the stop."""
import functools

import pytest
import torch

import stop_eos_ref as R

pytestmark = pytest.mark.gpu
F32, BF16 = torch.float32, torch.bfloat16
V_PICK = 193          # odd, no multiple of the 64 chunks of the bf16 pick nor of the 32 of the fp32 sampling pick
E = 77                # the EOS of the pick-level tables
HOT = 40.0            # a logit that makes its token the argmax and gives it all but exp(-39) of the probability


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == BF16 else t.view(torch.int32) if t.dtype == F32 else t


def _same(a, b):
    return torch.equal(_bits(a).cpu(), _bits(b).cpu())


# ------------------------------------------------------------------------------------------------ the four picks behind one face
KINDS = ["bf16_greedy", "bf16_sample", "bf16_nucleus", "f32_greedy", "f32_sample", "f32_nucleus"]
TINY = dict(d=128, n_layers=1, n_heads=2, n_kv_heads=1, ffn=256)


@functools.lru_cache(maxsize=None)
def _pick_engine(f32, V):
    """a one-layer engine: the picks read only its vocabulary size"""
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    from procyon_amd.engine_f32 import LlamaEngineF32
    kw = dict(vocab=V, **TINY)
    if f32:
        return LlamaEngineF32(synth.llama_state_dict(**kw, dtype=F32), LlamaConfig(**kw, max_pos=64))
    return LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, max_pos=64))


class Pick:
    def __init__(self, kind, V=V_PICK):
        self.kind, self.f32, self.V = kind, kind.startswith("f32"), V
        self.greedy = kind.endswith("greedy")
        self.nucleus = 0.5 if kind.endswith("nucleus") else None
        self.eng = _pick_engine(self.f32, V)
        self.dtype = F32 if self.f32 else BF16

    def state(self, B, S, eos=None, keep_logits=False):
        from procyon_amd.engine import GenState
        if self.f32:
            st = self.eng.new_gen_state(B, S, keep_logits, eos_id=eos)
            st.set(pos=2, step=0)
        else:
            st = GenState(B, self.V, S, "cuda", keep_logits, eos_id=eos)
            st.pos.fill_(2)
        return st, self.eng.new_cache(B, 8)

    def pick(self, st, cache, B, advance, u, probs=None):
        if self.greedy:
            (self.eng.greedy_pick if self.f32 else self.eng.pick)(cache, st, B, advance)
        else:
            self.eng.sample_pick(cache, st, B, advance, u, 1.0, self.nucleus, probs)


def _table(script, B, S, V, seed):
    """[S, B, V] logits: noise in [-1, 1] on a 1/64 grid (exact in bf16), HOT at the token(s) the script names for (step, row) -- a pair is a
    tie -- and at the filler token 3 + b where it names none"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-64, 65, (S, B, V), generator=g).float() / 64
    for s in range(S):
        for b in range(B):
            want = script.get((s, b), 3 + b)
            for tok in (want if isinstance(want, tuple) else (want,)):
                t[s, b, tok] = HOT
    return t


ARRAYS = ("tokens_out", "next_tok", "logprob", "step", "pos", "finished", "done", "n_steps_run", "logits_all")


def _snapshot(st, probs):
    torch.cuda.synchronize()
    snap = {k: getattr(st, k).clone() for k in ARRAYS if getattr(st, k, None) is not None}
    if probs is not None:
        snap["probs_out"] = probs.clone()
    return snap


def _run(P, table, u, eos=None, first_advance=False, poison=None, fin_before=None, keep_logits=False, want_probs=False, snap_at=None):
    """the table step by step through one state -> (state, logprob after every step [S][B], probs rows per step, snapshot behind step snap_at)"""
    S, B, V = table.shape
    st, cache = P.state(B, S, eos, keep_logits)
    probs = torch.full((B, V), -1.0, dtype=P.dtype, device="cuda") if want_probs and not P.greedy else None
    lps, prs, snap = [], [], None
    for s in range(S):
        rows = table[s].clone()
        if poison is not None:
            for b in range(B):
                if fin_before[s][b]:
                    rows[b] = poison
        st.logits.copy_(rows.to(P.dtype))
        P.pick(st, cache, B, s > 0 or first_advance, u, probs)
        lps.append(st.logprob.clone())
        if probs is not None:
            prs.append(probs.clone())
        if snap_at == s:
            snap = _snapshot(st, probs)
    torch.cuda.synchronize()
    return st, lps, prs, snap, probs


def _check_case(kind, script, B, S, expect_done_step, first_advance=False, poison=None, seed=0, tie=False):
    P = Pick(kind)
    table = _table(script, B, S, P.V, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    u = torch.rand(S * B, generator=g).mul(0.998).cuda()      # one variate per (step, row), all different, none at the far end of the CDF
    base, lps0, _, _, _ = _run(P, table, u, first_advance=first_advance)
    toks0 = base.tokens_out.cpu().T.tolist()                  # [S][B]
    ref = R.stop_eos(toks0, E)
    if not tie or P.greedy:                                   # (a tie is decided by the variate in a sampling pick: the table of the run without is the judge)
        assert ref["done_step"] == expect_done_step, (ref["done_step"], expect_done_step, toks0)
    n = ref["steps_run"]
    cols = [[toks0[s][b] for s in range(S)] for b in range(B)]
    firsts = [R.first_eos(c, E) for c in cols]
    fin_before = [[firsts[b] is not None and firsts[b] < s for b in range(B)] for s in range(S)]
    st, _, _, snap, _ = _run(P, table, u, eos=E, first_advance=first_advance, poison=poison, fin_before=fin_before, keep_logits=True,
                             snap_at=ref["done_step"])
    got = st.tokens_out.cpu()
    assert got[:, :n].T.tolist() == ref["tokens"], (got, ref["tokens"])
    assert bool((got[:, n:] == 0).all())                      # nothing behind the step that raised done
    assert int(st.step) == n and int(st.pos) == 2 + n - (0 if first_advance else 1)
    assert int(st.done) == int(ref["done"]) and int(st.n_steps_run) == (n if ref["done"] else 0)
    assert st.finished.cpu().bool().tolist() == ref["finished"]
    assert st.next_tok.cpu().tolist() == ref["tokens"][n - 1]
    for b in range(B):                                        # the partial sum of the run without a stop, up to and including the row's EOS
        e = firsts[b] if firsts[b] is not None and firsts[b] < n else n - 1
        assert _same(st.logprob[b], lps0[e][b]), (kind, b, e, float(st.logprob[b]), float(lps0[e][b]))
    # the record rows of every step run are written as without a stop -- a finished row's too, whatever it holds
    rec = st.logits_all[:n].cpu() if st.logits_all is not None else None
    for s in range(n):
        want = table[s].clone()
        if poison is not None:
            for b in range(B):
                if fin_before[s][b]:
                    want[b] = poison
        assert _same(rec[s], want.to(P.dtype)), (kind, s)
    if ref["done"] and ref["done_step"] < S - 1:              # launches behind done changed nothing at all
        after = _snapshot(st, None)
        for k in snap:
            assert _same(snap[k], after[k]), (kind, k)
    if not P.greedy:                                          # the scratch of the sampling picks is as a run without a stop left it
        again, lps1, _, _, _ = _run(P, table, u, first_advance=first_advance)
        assert torch.equal(again.tokens_out, base.tokens_out) and _same(lps1[-1], lps0[-1])
    return ref


CASES = {
    # name: (script, B, S, the step that raises done, first_advance)
    "eos_at_step0_on_prefill_logits": ({(0, 0): E, (1, 1): E}, 2, 3, 1, False),
    "one_of_three_then_the_others": ({(1, 1): E, (2, 0): E, (3, 2): E}, 3, 5, 3, True),
    "all_rows_in_one_launch": ({(1, 0): E, (1, 1): E, (1, 2): E}, 3, 3, 1, True),
    "one_row": ({(2, 0): E}, 1, 4, 2, False),
    "one_row_at_once": ({(0, 0): E}, 1, 3, 0, False),
    "six_rows_two_waves_deep": ({(0, 5): E, (1, 0): E, (1, 1): E, (1, 2): E, (2, 3): E, (2, 4): E}, 6, 4, 2, True),
    "never": ({}, 2, 3, None, False),
    "last_step": ({(2, 0): E, (2, 1): E}, 2, 3, 2, True),
}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(CASES))
def test_pick_follows_the_stop_rule(kind, case):
    script, B, S, done_step, first_advance = CASES[case]
    _check_case(kind, script, B, S, done_step, first_advance=first_advance, seed=len(case))


@pytest.mark.parametrize("kind", KINDS)
def test_pick_eos_tied_with_a_lower_and_a_higher_index(kind):
    """row 0: the EOS ties with a LOWER index -- the argmax is the lower one, the row goes on; row 1: it ties with a HIGHER index -- the argmax
    is the EOS.  (A sampling pick draws between the two by its variate: the run without a stop says which.)"""
    script = {(0, 0): (E - 5, E), (0, 1): (E, E + 5), (1, 0): E, (1, 2): E, (2, 1): (E - 70, E)}
    ref = _check_case(kind, script, 3, 4, 1, first_advance=True, seed=5, tie=True)
    if kind.endswith("greedy"):
        assert ref["tokens"][0] == [E - 5, E, 5] and ref["tokens"][1] == [E, E, E]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("poison", [float("nan"), float("-inf")], ids=["nan", "neginf"])
def test_finished_row_of_poison_disturbs_nothing(kind, poison):
    """from the step behind its EOS on a finished row's logits are all NaN / all -inf: its tokens stay the EOS, its logprob frozen, the other
    rows as without a stop, done where the reference says"""
    script, B, S, done_step, first_advance = CASES["one_of_three_then_the_others"]
    _check_case(kind, script, B, S, done_step, first_advance=first_advance, poison=poison, seed=9)


@pytest.mark.parametrize("kind", [k for k in KINDS if not k.endswith("greedy")])
def test_sampling_finished_row_moves_no_variate_and_keeps_its_probs_record(kind):
    """every unfinished pick is a draw between two equally likely tokens, decided by the row's own variate uniforms[step * B + b]: with row 1
    finished from step 1 on, rows 0 and 2 draw what they draw without a stop; with probs_out the finished row's probability row is still
    written, as without a stop, and nothing of it behind done"""
    P = Pick(kind)
    B, S = 3, 6
    script = {(s, b): (10 + b, 100 + b) for s in range(S) for b in range(B)}
    script[(0, 1)] = E
    script[(4, 0)] = script[(4, 2)] = E
    table = _table(script, B, S, P.V, 3)
    u = torch.rand(S * B, generator=torch.Generator().manual_seed(8)).mul(0.998).cuda()
    base, lps0, prs0, _, _ = _run(P, table, u, first_advance=True, want_probs=True)
    toks0 = base.tokens_out.cpu().T.tolist()
    assert len({toks0[s][0] for s in range(4)} | {toks0[s][2] for s in range(4)}) >= 3      # both sides of the coin came up
    ref = R.stop_eos(toks0, E)
    assert ref["done_step"] == 4
    st, _, prs1, _, probs = _run(P, table, u, eos=E, first_advance=True, want_probs=True)
    assert st.tokens_out.cpu()[:, :5].T.tolist() == ref["tokens"] and int(st.done) == 1 and int(st.step) == 5
    for s in range(5):
        assert _same(prs1[s], prs0[s]), (kind, s)              # row 1 included
    assert _same(prs1[5], prs1[4])                             # the launch behind done wrote no probabilities
    for b, e in ((0, 4), (1, 0), (2, 4)):
        assert _same(st.logprob[b], lps0[e][b])


def test_refusals_launch_nothing():
    """finished without done; an eos_id outside the vocabulary: code 1 from each of the four picks, state untouched"""
    from procyon_amd import _lib as L
    for kind in ("bf16_greedy", "bf16_sample", "f32_greedy", "f32_sample"):
        P = Pick(kind)
        u = torch.rand(6).cuda()
        for breakage in ("no_done", "eos_high", "eos_negative"):
            st, cache = P.state(2, 3, E)
            if breakage == "no_done":
                st.c.done = None
            else:
                st.c.eos_id = P.V if breakage == "eos_high" else -1
            st.logits.fill_(0.0)
            with pytest.raises(L.PcyError, match="done|eos_id"):
                P.pick(st, cache, 2, False, u)
            torch.cuda.synchronize()
            assert int(st.step) == 0 and not bool(st.tokens_out.any()) and not bool(st.finished.any()) and int(st.done) == 0


# ------------------------------------------------------------------------------------------------ chains and engines
GEOM = dict(vocab=320, d=256, n_layers=2, n_heads=4, n_kv_heads=2, ffn=512)
T_PROMPT, MAXLEN = 12, 40


@functools.lru_cache(maxsize=None)
def _engine(f32):
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    from procyon_amd.engine_f32 import LlamaEngineF32
    if f32:
        return LlamaEngineF32(synth.llama_state_dict(**GEOM, dtype=F32), LlamaConfig(**GEOM, max_pos=128))
    return LlamaEngine(synth.llama_state_dict(**GEOM), LlamaConfig(**GEOM, max_pos=128))


def _prompts(B, same):
    ids = torch.randint(0, 300, (3, T_PROMPT), generator=torch.Generator().manual_seed(11))
    return ids[[0 if same else b % 3 for b in range(B)]]


def _pick_eos(tok_row):
    """the token of the first step k >= 1 that the row had not emitted before (so that its first EOS is step k); a row that repeats one token
    gives that token, whose first occurrence is step 0"""
    row = tok_row.tolist()
    for k in range(1, len(row)):
        if row[k] not in row[:k]:
            return row[k]
    return row[1]


def _decode_steps(eng, path):
    lib = eng.ops.lib if hasattr(eng, "ops") else eng.ctx.lib
    if path == "gemm":
        return int(lib.pcy_debug_decode_gemm_count())
    if path == "w8":
        return int(lib.pcy_debug_decode_w8_count())
    if path == "f32":
        return int(lib.pcy_debug_f32_stream_count())
    if path in ("extend", "window"):
        return int(lib.pcy_debug_look_count(1))
    from procyon_amd import _lib as L
    return sum(int(lib.pcy_debug_dispatch_count(k)) for k in L.DISPATCH_DECODE.values())


def _record_same(lg1, lg0, tok0, eos, n):
    """the record of a run with a stop against the run without: rows [0, steps_run) exist, and every row of the batch holds the bits of the
    run without up to and including the step of its EOS (behind it the row is fed the EOS, not what it went on to emit: other logits)"""
    ok = tuple(lg1.shape) == (lg0.shape[0], n, lg0.shape[2])
    for b in range(lg0.shape[0]):
        e = R.first_eos(tok0[b].tolist(), eos)
        e = e if e is not None and e < n else n - 1
        ok = ok and _same(lg1[b, :e + 1], lg0[b, :e + 1])
    return ok


def _partial_sums(kind, lg, u, B):
    """the log-probability after every step as the pick WITHOUT a stop forms it, from the logits record of the run without a stop (row s of
    the record is what the pick of step s read): the same kernel on the same rows in the same order -> [S][B]"""
    P = Pick(kind, lg.shape[-1])
    table = lg.transpose(0, 1).float()                         # [S, B, V]
    _, lps, _, _, _ = _run(P, table, u)
    return lps


def _check_run(off, on, st_on, eos, kind, u, B, eager_steps=None, bound_chunk=None):
    from procyon_amd.engine import STOP_CHUNK
    tok0, lp0, lg0 = off
    tok1, lp1, lg1 = on
    ref = R.stop_eos(tok0.T.tolist(), eos)
    n = ref["steps_run"]
    assert st_on.steps_run == n and (not ref["done"] or int(st_on.n_steps_run) == n)
    assert tok1.tolist() == R.padded_tokens(ref, eos, MAXLEN)
    assert _record_same(lg1, lg0, tok0, eos, n)
    lps = _partial_sums(kind, lg0.cuda() if not lg0.is_cuda else lg0, u, B)
    assert _same(lps[-1], lp0)                                 # (the replay IS the chain's sum)
    for b in range(B):
        e = R.first_eos(tok0[b].tolist(), eos)
        e = e if e is not None and e < n else n - 1
        assert _same(lp1[b], lps[e][b]), (b, e)
    if eager_steps is not None and ref["done"]:
        chunk = STOP_CHUNK if bound_chunk is None else bound_chunk
        assert eager_steps <= min(MAXLEN - 1, R.enqueued_bound(ref["done_step"], chunk)), (eager_steps, ref["done_step"])
        if ref["done_step"] + 2 * chunk - 1 < MAXLEN - 1:
            assert eager_steps < MAXLEN - 1
    return ref


BF16_PATHS = [("default", 1, True), ("default", 3, False), ("default", 3, True), ("default", 9, False), ("default", 9, True),
              ("gemm", 3, True), ("gemm", 3, False), ("w8", 1, True), ("w8", 3, False)]


@pytest.mark.parametrize("path,B,same", BF16_PATHS, ids=[f"{p}-{b}{'same' if s else 'rows'}" for p, b, s in BF16_PATHS])
def test_bf16_greedy_stops(path, B, same):
    eng = _engine(False)
    emb, mask = eng.embed_tokens(_prompts(B, same)), torch.ones(B, T_PROMPT)
    kw = {"gemm": dict(decode_gemm=True), "w8": dict(decode_w8=True)}.get(path, {})
    run = lambda **x: eng.generate_greedy(emb, mask, MAXLEN, keep_logits=True, **kw, **x)
    tok0, lp0, lg0, _ = run()
    off = (tok0.cpu(), lp0.clone(), lg0.clone())
    eos = _pick_eos(off[0][0])
    n0 = _decode_steps(eng, path)
    tok1, lp1, lg1, (st, _) = run(stop_on_eos=eos, use_graph=False)
    steps = _decode_steps(eng, path) - n0
    ref = _check_run(off, (tok1.cpu(), lp1, lg1), st, eos, "bf16_greedy", None, B, eager_steps=steps)
    assert ref["finished"][0] and (ref["done"] or not same)
    if same or B == 1:
        assert ref["done"] and steps < MAXLEN - 1
    if path != "gemm":                                         # the replayed chain: the eager one bit for bit
        tok2, lp2, lg2, (st2, _) = run(stop_on_eos=eos, use_graph=True)
        assert torch.equal(tok2, tok1) and _same(lp2, lp1) and _same(lg2, lg1) and st2.steps_run == st.steps_run
    # an EOS that never occurs: the run without a stop, exactly
    never = next(t for t in range(GEOM["vocab"]) if not bool((off[0] == t).any()))
    tok3, lp3, lg3, (st3, _) = run(stop_on_eos=never)
    assert torch.equal(tok3.cpu(), off[0]) and _same(lp3, off[1]) and _same(lg3, off[2]) and st3.steps_run == MAXLEN and int(st3.done) == 0


def _variates(B, shared, seed):
    """uniforms[step * B + b]: every (step, row) its own, or -- shared -- one per step for all rows, so that rows with equal prompts draw
    equal tokens and the whole batch finishes (and raises done) in one step"""
    g = torch.Generator().manual_seed(seed)
    if shared:
        return torch.rand(MAXLEN, generator=g).repeat_interleave(B).cuda()
    return torch.rand(MAXLEN * B, generator=g).cuda()


def _check_sampling(eng, path, B, shared, run, replay_state, u):
    """a sampling driver with the option off, with a token row 0 drew at a step >= 1 as the EOS (eagerly, the decode steps counted), and with
    an EOS that never occurs; `run(**kw)` -> the driver's tuple, `replay_state()` -> (state, cache) for the pick without a stop"""
    from procyon_amd.engine import STOP_CHUNK
    tok0, lp0, lg0, _ = run()
    off = (tok0.cpu(), lp0.clone(), lg0.clone())
    eos = _pick_eos(off[0][0])
    n0 = _decode_steps(eng, path)
    out = run(stop_on_eos=eos, **({"graph": False} if path == "f32" else {}))
    steps = _decode_steps(eng, path) - n0
    tok1, lp1, lg1, st = out[0], out[1], out[2], out[3][0]
    ref = R.stop_eos(off[0].T.tolist(), eos)
    n = ref["steps_run"]
    assert st.steps_run == n and tok1.cpu().tolist() == R.padded_tokens(ref, eos, MAXLEN)
    assert int(st.done) == int(ref["done"]) and (not ref["done"] or int(st.n_steps_run) == n)
    assert _record_same(lg1, off[2], off[0], eos, n)
    # partial sums: the sampling pick without a stop replayed over the record with the same variates (temperature 0.7)
    st_r, cache_r = replay_state()
    lps = []
    for s in range(MAXLEN):
        st_r.logits.copy_(off[2][:, s])
        eng.sample_pick(cache_r, st_r, B, s > 0, u, 0.7, None)
        lps.append(st_r.logprob.clone())
    assert torch.equal(st_r.tokens_out.cpu(), off[0].int()) and _same(lps[-1], off[1])
    for b in range(B):
        e = R.first_eos(off[0][b].tolist(), eos)
        e = e if e is not None and e < n else n - 1
        assert _same(lp1[b], lps[e][b]), (b, e)
    assert ref["finished"][0]
    # the decode steps that were enqueued: within the documented bound of the step that raised done, and fewer than max_len - 1
    assert steps <= MAXLEN - 1
    if B == 1 or shared:
        assert ref["done"], ref
    if ref["done"]:
        assert steps <= min(MAXLEN - 1, R.enqueued_bound(ref["done_step"], STOP_CHUNK)), (steps, ref["done_step"])
        if ref["done_step"] + 2 * STOP_CHUNK - 1 < MAXLEN - 1:
            assert steps < MAXLEN - 1, (steps, ref["done_step"])
    else:
        assert steps == MAXLEN - 1
    if B == 1 or shared:
        assert steps < MAXLEN - 1, (steps, ref["done_step"])
    # an EOS that never occurs: the run without a stop, exactly, every step run, done never raised
    never = next(t for t in range(GEOM["vocab"]) if not bool((off[0] == t).any()))
    n0 = _decode_steps(eng, path)
    out = run(stop_on_eos=never, **({"graph": False} if path == "f32" else {}))
    assert _decode_steps(eng, path) - n0 == MAXLEN - 1
    st3 = out[3][0]
    assert torch.equal(out[0].cpu(), off[0]) and _same(out[1], off[1]) and _same(out[2], off[2])
    assert st3.steps_run == MAXLEN and int(st3.done) == 0 and not bool(st3.finished.any())
    return eos, (tok1, lp1, lg1, st)


SAMPLING_PATHS = [("default", 1, False), ("default", 3, False), ("default", 3, True), ("gemm", 3, False), ("gemm", 3, True), ("w8", 2, False),
                  ("w8", 2, True)]


@pytest.mark.parametrize("path,B,shared", SAMPLING_PATHS, ids=[f"{p}-{b}{'shared' if s else 'own'}" for p, b, s in SAMPLING_PATHS])
def test_bf16_sampling_stops(path, B, shared):
    from procyon_amd.engine import GenState
    eng = _engine(False)
    emb, mask = eng.embed_tokens(_prompts(B, True)), torch.ones(B, T_PROMPT)
    u = _variates(B, shared, 21)
    kw = {"gemm": dict(decode_gemm=True), "w8": dict(decode_w8=True)}.get(path, {})
    run = lambda **x: eng.generate_sampling(emb, mask, MAXLEN, temperature=0.7, keep_logits=True, uniforms=u, **kw, **x)

    def replay_state():
        st_r = GenState(B, GEOM["vocab"], MAXLEN, "cuda")
        st_r.pos.fill_(2)
        return st_r, eng.new_cache(B, 8)
    _check_sampling(eng, path, B, shared, run, replay_state, u)


def test_bf16_sampling_refuses_too_few_variates(monkeypatch):
    """the pick of step s reads uniforms[s * B + b]: fewer than max_len * B variates are refused before the prefill (as the fp32 family
    refuses them); exactly as many, and more, are the same call"""
    from procyon_amd.engine import LlamaEngine
    eng = _engine(False)
    B, max_len = 2, 4
    emb, mask = eng.embed_tokens(_prompts(B, False)), torch.ones(B, T_PROMPT)
    u = torch.rand(12, generator=torch.Generator().manual_seed(5)).cuda()
    prefills, prefill = [], LlamaEngine.prefill
    monkeypatch.setattr(LlamaEngine, "prefill", lambda self, *a, **k: (prefills.append(1), prefill(self, *a, **k))[1])
    with pytest.raises(ValueError, match="7 uniform variates"):
        eng.generate_sampling(emb, mask, max_len, temperature=0.7, uniforms=u[:7])
    assert prefills == []
    tok8 = eng.generate_sampling(emb, mask, max_len, temperature=0.7, uniforms=u[:8])[0]
    tok12 = eng.generate_sampling(emb, mask, max_len, temperature=0.7, uniforms=u)[0]
    assert len(prefills) == 2 and tok8.shape == (B, max_len) and torch.equal(tok8, tok12)


@pytest.mark.parametrize("step", ["extend", "window"])
def test_lookahead_stops(step):
    """the commit of the pass that holds the EOS ends with it (tokens, logprob and record of the run without a stop up to there), and no
    pass runs behind it"""
    eng = _engine(False)
    ids = _prompts(1, True)[0]
    emb = eng.embed_tokens(ids[None])
    run = lambda **x: eng.generate_lookahead(emb, ids, MAXLEN, 4, keep_logits=True, step=step, **x)
    tok0, lp0, lg0, (_, _, look0) = run()
    off = (tok0.cpu(), lp0.clone(), lg0.clone())
    eos = _pick_eos(off[0][0])
    n0 = _decode_steps(eng, step)
    tok1, lp1, lg1, (st, _, look) = run(stop_on_eos=eos)
    passes = _decode_steps(eng, step) - n0
    ref = _check_run(off, (tok1.cpu(), lp1, lg1), st, eos, "bf16_greedy", None, 1)
    assert ref["done"] and int(st.done) == 1 and int(st.finished) == 1
    assert passes == look.stats()["passes"] <= ref["done_step"] and passes < look0.stats()["passes"]
    never = next(t for t in range(GEOM["vocab"]) if not bool((off[0] == t).any()))
    tok3, lp3, lg3, (st3, _, look3) = run(stop_on_eos=never)
    assert torch.equal(tok3.cpu(), off[0]) and _same(lp3, off[1]) and _same(lg3, off[2]) and look3.stats() == look0.stats()


F32_PATHS = [(1, True), (3, False), (3, True)]


@pytest.mark.parametrize("B,same", F32_PATHS, ids=[f"{b}{'same' if s else 'rows'}" for b, s in F32_PATHS])
def test_f32_greedy_stops(B, same):
    eng = _engine(True)
    emb, mask = eng.embed_tokens(_prompts(B, same)), torch.ones(B, T_PROMPT)
    run = lambda **x: eng.generate_greedy(emb, mask, MAXLEN, keep_logits=True, **x)
    tok0, lp0, lg0, _ = run()
    off = (tok0.cpu(), lp0.clone(), lg0.clone())
    eos = _pick_eos(off[0][0])
    n0 = _decode_steps(eng, "f32")
    tok1, lp1, lg1, (st, _) = run(stop_on_eos=eos, graph=False)
    steps = _decode_steps(eng, "f32") - n0
    ref = _check_run(off, (tok1.cpu(), lp1, lg1), st, eos, "f32_greedy", None, B, eager_steps=steps)
    assert ref["finished"][0] and (ref["done"] or not same)
    if same or B == 1:
        assert ref["done"] and steps < MAXLEN - 1
    tok2, lp2, lg2, (st2, _) = run(stop_on_eos=eos, graph=True)
    assert torch.equal(tok2, tok1) and _same(lp2, lp1) and _same(lg2, lg1) and st2.steps_run == st.steps_run
    never = next(t for t in range(GEOM["vocab"]) if not bool((off[0] == t).any()))
    tok3, lp3, lg3, (st3, _) = run(stop_on_eos=never)
    assert torch.equal(tok3.cpu(), off[0]) and _same(lp3, off[1]) and _same(lg3, off[2]) and st3.steps_run == MAXLEN


F32_SAMPLING = [(1, False), (3, False), (3, True)]


@pytest.mark.parametrize("B,shared", F32_SAMPLING, ids=[f"{b}{'shared' if s else 'own'}" for b, s in F32_SAMPLING])
def test_f32_sampling_stops(B, shared):
    eng = _engine(True)
    emb, mask = eng.embed_tokens(_prompts(B, True)), torch.ones(B, T_PROMPT)
    u = _variates(B, shared, 22)
    run = lambda **x: eng.generate_sampling(emb, mask, MAXLEN, temperature=0.7, keep_logits=True, uniforms=u, **x)

    def replay_state():
        st_r = eng.new_gen_state(B, MAXLEN)
        st_r.set(pos=2, step=0)
        return st_r, eng.new_cache(B, 8)
    n_sel = eng.select_count(1)
    eos, (tok1, lp1, lg1, st) = _check_sampling(eng, "f32", B, shared, run, replay_state, u)
    assert eng.select_count(1) > n_sel
    # the replayed chain: the eager one bit for bit, and its enqueued steps (counted by the sampling entry, replayed or not) inside the bound
    n_sel = eng.select_count(1)
    tok2, lp2, lg2, (st2, _, _) = run(stop_on_eos=eos, graph=True)
    enq = eng.select_count(1) - n_sel - 1                      # (one count is the pick on the prefill's logits)
    assert torch.equal(tok2, tok1) and _same(lp2, lp1) and _same(lg2, lg1) and st2.steps_run == st.steps_run
    if int(st2.done):
        assert enq <= min(MAXLEN - 1, R.enqueued_bound(st2.steps_run - 1, 8)), (enq, st2.steps_run)


def test_stop_and_no_stop_never_share_a_graph():
    """the same engine, prompts and cache geometry, alternately with and without a stop and with two different EOS ids: every replayed run
    gives what its own eager run gives"""
    eng = _engine(False)
    emb, mask = eng.embed_tokens(_prompts(1, True)), torch.ones(1, T_PROMPT)
    tok0, lp0, _, _ = eng.generate_greedy(emb, mask, MAXLEN, use_graph=False)
    eos_a = _pick_eos(tok0.cpu()[0])
    eos_b = next(t for t in tok0.cpu()[0].tolist()[::-1] if t != eos_a)
    want = {e: eng.generate_greedy(emb, mask, MAXLEN, use_graph=False, stop_on_eos=e)[0].clone() for e in (eos_a, eos_b)}
    for e in (eos_a, None, eos_b, None, eos_a):
        tok = eng.generate_greedy(emb, mask, MAXLEN, use_graph=True, **({} if e is None else {"stop_on_eos": e}))[0]
        assert torch.equal(tok, tok0 if e is None else want[e]), e


# ------------------------------------------------------------------------------------------------ model level
INSTR = ["w1 <|protein|> is w2 ? [ANSWER]", "describe w8 <|protein|> and <|protein|> now please [ANSWER]"]
SLOTS = [[0], [0, 1]]


def _inputs(prot, instr=INSTR, slots=SLOTS):
    return {"data": {"seq": prot, "seq_idx": torch.arange(prot.shape[0]), "text": [], "drug": None},
            "input": {"seq": [list(s) for s in slots], "text": [[] for _ in instr], "drug": None},
            "target": {"seq": None, "text": None, "drug": None}, "instructions": list(instr),
            "reference_indices": {"input": {"seq": [list(s) for s in slots]}, "target": {"text": None}}}


@functools.lru_cache(maxsize=None)
def _model(f32):
    from procyon_amd import synth
    from procyon_amd import synthetic_model as SM
    kw = dict(dtype=F32, as_loaded=True) if f32 else {}
    m = SM.build("small", device="cuda", max_new_tokens=32, **kw)
    m.eval()
    return m, synth.protein_tokens([90, 41], seed=3)


def _ulps(x, n):
    return n * float(torch.tensor(abs(float(x)), dtype=F32).clamp_min(2.0 ** -126).log2().floor().sub(23).exp2())


MODEL_PATHS = [("bf16", {}), ("bf16", {"decode_gemm": True}), ("bf16", {"decode_w8": True}), ("bf16", {"lookahead": 4}),
               ("bf16", {"lookahead": 4, "lookahead_step": "window"}), ("f32", {}), ("f32", {"decode_f32": "stream"}), ("f32", {"decode_f32": "device"})]


@pytest.mark.parametrize("family,kw", MODEL_PATHS, ids=[f + "-" + ("-".join(f"{k}={v}" for k, v in kw.items()) or "default") for f, kw in MODEL_PATHS])
def test_generate_stops(family, kw, monkeypatch):
    """generate(stop_on_eos=True): the text of stop_on_eos=False under truncate_on_eos, tokens up to every row's EOS and the record up to
    steps_run bit-equal, the EOS behind, "steps_run" in the internals; the EOS is a token row 0 emits at a step >= 1"""
    m, prot = _model(family == "f32")
    one = "lookahead" in kw
    mk = (lambda: _inputs(prot, INSTR[:1], SLOTS[:1])) if one else (lambda: _inputs(prot))
    N = 24
    base = m.generate(mk(), max_len=N, method="greedy", return_all_internals=True, **kw)
    eos = _pick_eos(base["out_tokens"][0, 0])
    monkeypatch.setattr(m.tokenizer, "eos_token_id", eos)
    off = m.generate(mk(), max_len=N, method="greedy", return_all_internals=True, **kw)
    assert torch.equal(off["out_tokens"], base["out_tokens"]) and "steps_run" not in off
    on = m.generate(mk(), max_len=N, method="greedy", return_all_internals=True, stop_on_eos=True, **kw)
    B = off["out_tokens"].shape[0]
    ref = R.stop_eos(off["out_tokens"][:, 0].T.tolist(), eos)
    n = ref["steps_run"]
    assert on["steps_run"] == [n] and ref["finished"][0]
    assert on["out_tokens"][:, 0].tolist() == [row[:N] for row in R.padded_tokens(ref, eos, N)]
    assert on["out_logits"].dim() == 4 and _record_same(on["out_logits"][:, 0], off["out_logits"][:, 0], off["out_tokens"][:, 0], eos, n)
    assert on["text"] == off["text"]
    assert m.tokenizer.eos_token not in on["text"][0][0]
    # log-probabilities: the partial sum up to the row's EOS.  The device paths: the pick without a stop replayed over the record, bit for
    # bit.  The host-driven fp32 loop ("ops") adds torch's log-softmax terms on the host side: the same torch operators on the record, within
    # one fp32 ulp of the sum per step.
    lg, tok = off["out_logits"][:, 0], off["out_tokens"][:, 0]
    if family == "f32" and not kw:
        gains = lg.cuda().log_softmax(-1).gather(2, tok.cuda()[:, :, None])[:, :, 0]
        lps = list(gains.cumsum(1).T)
    else:
        lps = _partial_sums("f32_greedy" if family == "f32" else "bf16_greedy", lg.cuda(), None, B)
    for b in range(B):
        e = R.first_eos(tok[b].tolist(), eos)
        e = e if e is not None and e < n else n - 1
        got, want = on["out_log_probs"][b, 0], lps[e][b].cpu()
        if family == "f32" and not kw:
            assert abs(float(got) - float(want)) <= _ulps(want, e + 1), (b, e, float(got), float(want))
        else:
            assert _same(got, want), (b, e, float(got), float(want))
    # without the option nothing is added; a tuple call returns the cut record too
    tup = m.generate(mk(), max_len=N, method="greedy", stop_on_eos=True, **kw)
    assert torch.equal(tup[0], on["out_tokens"]) and tup[3] == on["text"] and tup[2].shape == on["out_logits"].shape


@pytest.mark.parametrize("family,kw", [("bf16", {}), ("f32", {"decode_f32": "device"})], ids=["bf16", "f32-device"])
def test_generate_sampling_stops(family, kw, monkeypatch):
    """sampling with the generator seeded alike: the draws of stop_on_eos=False up to every row's EOS, the same text"""
    m, prot = _model(family == "f32")
    N = 16
    call = lambda **x: (torch.manual_seed(5), m.generate(_inputs(prot), max_len=N, method="temperature", temperature=0.8, nucleus_prob=None,
                                                          return_all_internals=True, **kw, **x))[1]
    base = call()
    eos = _pick_eos(base["out_tokens"][0, 0])
    monkeypatch.setattr(m.tokenizer, "eos_token_id", eos)
    off, on = call(), call(stop_on_eos=True)
    assert torch.equal(off["out_tokens"], base["out_tokens"])
    ref = R.stop_eos(off["out_tokens"][:, 0].T.tolist(), eos)
    n = ref["steps_run"]
    assert on["steps_run"] == [n] and on["out_tokens"][:, 0].tolist() == R.padded_tokens(ref, eos, N)
    assert on["text"] == off["text"] and _record_same(on["out_logits"][:, 0], off["out_logits"][:, 0], off["out_tokens"][:, 0], eos, n)
    # one prompt, 40 tokens: done is certain, and the decode steps that were enqueued stay inside the bound and below max_len - 1; with an
    # EOS the run never draws, the option changes nothing
    from procyon_amd.engine import STOP_CHUNK
    N = MAXLEN
    one = lambda **x: (torch.manual_seed(6), m.generate(_inputs(prot, INSTR[:1], SLOTS[:1]), max_len=N, method="temperature", temperature=0.8,
                                                         nucleus_prob=None, return_all_internals=True, **kw, **x))[1]
    if family == "f32":
        eng = m.text_encoder.engine_f32
        count = lambda: eng.select_count(1)                    # steps the fp32 sampling entries enqueued, replayed or not
    else:
        eng = m.text_encoder.engine
        count = lambda: _decode_steps(eng, "default")
    base = one()
    row = base["out_tokens"][0, 0]
    eos = _pick_eos(row)
    monkeypatch.setattr(m.tokenizer, "eos_token_id", eos)
    n0 = count()
    on = one(stop_on_eos=True)
    steps = count() - n0 - (1 if family == "f32" else 0)       # (fp32: one count is the pick on the prefill's logits)
    k = R.first_eos(row.tolist(), eos)
    assert on["steps_run"] == [k + 1] and on["out_tokens"][0, 0].tolist() == row.tolist()[:k + 1] + [eos] * (N - k - 1)
    assert steps <= R.enqueued_bound(k, STOP_CHUNK) and steps < N - 1, (steps, k)
    never = next(t for t in range(2000) if not bool((row == t).any()))
    monkeypatch.setattr(m.tokenizer, "eos_token_id", never)
    n0 = count()
    on = one(stop_on_eos=True)
    assert count() - n0 - (1 if family == "f32" else 0) == N - 1 and on["steps_run"] == [N]
    for key in ("out_tokens", "out_logits", "out_log_probs"):
        assert _same(on[key], base[key]), key


def test_generate_refuses_beam_and_other_values():
    m, prot = _model(False)
    with pytest.raises(ValueError, match="stop_on_eos"):
        m.generate(_inputs(prot), max_len=4, method="beam", beam_size=2, beam_group_size=1, stop_on_eos=True)
    with pytest.raises(ValueError, match="stop_on_eos"):
        m.generate(_inputs(prot), max_len=4, method="greedy", stop_on_eos=1)


from test_gpu_round3 import _service_checkpoint, instruct_env  # noqa: E402,F401  (the fixture that builds the instruction-tuning data tree)


def test_caption_bulk_with_the_option_gives_the_same_table(instruct_env):
    """pipelines.caption_bulk(stop_on_eos=True) on three proteins of a synthetic embedding-table checkpoint, the real generate() behind it:
    the table of the call without the option (its beam search ends on the device by itself; nothing is handed to generate, which refuses
    the option together with beam search); any value but False / True is refused before anything runs"""
    from procyon.training.training_args_IT import DataArgs
    from procyon_amd.checkpoint import from_pretrained
    from procyon_amd.pipelines import caption_bulk
    from procyon_amd.tokenizer import SyntheticTokenizer
    tok = SyntheticTokenizer(n_text=2000, base_vocab=2048, bos_token_id=2040, eos_token_id=2041)
    ckpt = str(instruct_env / "ckpt")
    _service_checkpoint(ckpt, vocab=len(tok) - 1)
    model, margs = from_pretrained(checkpoint_dir=ckpt, tokenizer=tok, max_new_tokens=16, max_pos=512)
    ids = [f"P{i:05d}" for i in (530, 7, 11)]
    kw = dict(max_len=6, beam_size=4, diversity_penalty=0.8, batch_size=2)
    off = caption_bulk(model, margs, DataArgs(), ids, "uniprot", "all", **kw)
    on = caption_bulk(model, margs, DataArgs(), ids, "uniprot", "all", stop_on_eos=True, **kw)
    assert list(on.columns) == ["uniprot_id", "response0", "response1"] and on.equals(off)
    with pytest.raises(ValueError, match="stop_on_eos"):
        caption_bulk(model, margs, DataArgs(), ids, "uniprot", "all", stop_on_eos=1, **kw)
