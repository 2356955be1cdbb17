"""GPU: fp32 generation on the streaming fp32 GEMV and the device-resident decode step (procyon_amd/csrc/pcy_f32_gemv.hip, include/pcy.h,
DESIGN.md 4.10).  Bars are the project's own: single operators R.OP_BAR = 2e-5 norm-wise and R.OP_MAXABS = 2e-4 against float64
(tests/f32_stream_ref.py), stacks < 1e-4 against the fp32 oracle, beam scores atol 1e-3.  tests/test_f32_stream_cpu.py shows on the CPU that
plain torch fp32 meets the operator bars on the same cases and that the fixtures' margins make token equality a fair demand."""
import ctypes as C

import pytest
import torch

import f32_ref as R
import f32_stream_ref as S
from conftest import record_parity, rel_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
SENT = -7.0


@pytest.fixture(scope="module")
def ops():
    from procyon_amd.engine_f32 import F32Ops
    return F32Ops()


def _window(t, left, right, above=1):
    """t [r, c] on the device as a column window of a wider sentinel-filled buffer -> (buffer, view)"""
    buf = torch.full((t.shape[0] + above, left + t.shape[1] + right), SENT, dtype=F32, device="cuda")
    view = buf[:t.shape[0], left:left + t.shape[1]]
    view.copy_(t)
    return buf, view


def _outside_intact(buf, rows, left, cols):
    m = torch.ones_like(buf, dtype=torch.bool)
    m[:rows, left:left + cols] = False
    return bool((buf[m] == SENT).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ 1. the GEMV against float64
@pytest.mark.parametrize("name", list(S.gemv_cases("store")))
@pytest.mark.parametrize("epi", list(S.EPIS))
def test_gemv_vs_float64(ops, epi, name):
    B, N, K = S.gemv_cases(epi)[name]
    c = S.gemv_case(epi, name)
    e = S.EPIS[epi]
    ref = S.gemv(c["x"], c["W"], c["W2"], c["resid"], e)
    W, W2 = c["W"].cuda(), (c["W2"].cuda() if e == S.EPI_SWIGLU else None)
    if name.startswith("window"):
        xb, x = _window(c["x"], 4, 4)
        yb, y = _window(torch.zeros(B, N), 2, 3)
        rb, r = _window(c["resid"], 1, 2)
        got = ops.gemv(x, W, W2, r if e == S.EPI_RESID else None, e, out=y)
        assert got.data_ptr() == y.data_ptr()
        assert _outside_intact(yb, B, 2, N) and _outside_intact(xb, B, 4, K) and _outside_intact(rb, B, 1, N)
        assert torch.equal(x.cpu(), c["x"]) and torch.equal(r.cpu(), c["resid"])
    elif name.startswith("alias") and e == S.EPI_RESID:
        y = c["resid"].cuda().clone()
        got = ops.gemv(c["x"].cuda(), W, W2, y, e, out=y)
    else:
        got = ops.gemv(c["x"].cuda(), W, W2, c["resid"].cuda() if e == S.EPI_RESID else None, e)
    got = got.cpu()
    er, em = R.rel64(got, ref), R.maxabs64(got, ref)
    print(f"gemv {epi} {name} B={B} N={N} K={K}: rel {er:.3e} maxabs {em:.3e}")
    assert er < R.OP_BAR and em < R.OP_MAXABS, (er, em)


# ------------------------------------------------------------------------------------------------ 2. row independence
@pytest.mark.parametrize("epi", list(S.EPIS))
def test_gemv_rows_do_not_depend_on_the_call(ops, epi):
    """row b of a 33-row call (two x tiles in the first pass, a second pass for row 32) has the bits of the one-row call on that row; NaN
    in every other row does not reach it; equal calls give equal bits"""
    B, N, K = S.gemv_cases(epi)["pass1_b33"]
    c = S.gemv_case(epi, "pass1_b33")
    e = S.EPIS[epi]
    x, W, W2, r = c["x"].cuda(), c["W"].cuda(), (c["W2"].cuda() if e == S.EPI_SWIGLU else None), (c["resid"].cuda() if e == S.EPI_RESID else None)
    full = ops.gemv(x, W, W2, r, e)
    assert torch.equal(_bits(full), _bits(ops.gemv(x, W, W2, r, e)))
    for b in (0, 15, 16, 31, 32):
        one = ops.gemv(x[b:b + 1], W, W2, None if r is None else r[b:b + 1], e)
        assert torch.equal(_bits(one[0]), _bits(full[b])), (epi, b)
        xn = torch.full_like(x, float("nan"))
        xn[b] = x[b]
        assert torch.equal(_bits(ops.gemv(xn, W, W2, r, e)[b]), _bits(full[b])), (epi, b, "NaN leaked")
    for nb in (16, 17):           # the tile count of the pass does not change a row either
        part = ops.gemv(x[:nb], W, W2, None if r is None else r[:nb], e)
        assert torch.equal(_bits(part), _bits(full[:nb])), (epi, nb)


def test_gemv_argument_errors_launch_nothing(ops):
    x, W, y = torch.zeros(2, 32, device="cuda"), torch.zeros(5, 32, device="cuda"), torch.full((2, 5), SENT, device="cuda")
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())
    call = lambda W_, W2_, x_, ldx, r_, ldr, y_, ldy, N, K, B, epi: ops.lib.pcy_f32_gemv(ops.h, p(W_), p(W2_), p(x_), ldx, p(r_), ldr, p(y_), ldy, N, K, B, epi)
    assert call(W, None, x, 32, None, 0, y, 5, 5, 32, 2, S.EPI_STORE) == 0
    torch.cuda.synchronize()
    y.fill_(SENT)
    bad = [(None, None, x, 32, None, 0, y, 5, 5, 32, 2, 0), (W, None, None, 32, None, 0, y, 5, 5, 32, 2, 0), (W, None, x, 32, None, 0, None, 5, 5, 32, 2, 0),
           (W, None, x, 32, None, 0, y, 5, 5, 30, 2, 0),        # K % 4
           (W, None, x, 34, None, 0, y, 5, 5, 32, 2, 0),        # unaligned rows of x
           (W, None, x, 16, None, 0, y, 5, 5, 32, 2, 0),        # rows shorter than K
           (W, None, x, 32, None, 0, y, 4, 5, 32, 2, 0),        # rows of y shorter than N
           (W, None, x, 32, None, 0, y, 5, 5, 32, 2, 1),        # RESID without resid
           (W, None, x, 32, None, 0, y, 5, 5, 32, 2, 4),        # SWIGLU without the up matrix
           (W, None, x, 32, None, 0, y, 5, 5, 32, 2, 2),        # not an epilogue of this operator
           (W, None, x, 32, None, 0, y, 5, 5, 32, 0, 0), (W, None, x, 32, None, 0, y, 5, 0, 32, 2, 0), (W, None, x[:, 1:], 32, None, 0, y, 5, 5, 28, 2, 0)]
    for a in bad:
        assert call(*a) == 1, a
    torch.cuda.synchronize()
    assert bool((y == SENT).all())


# ------------------------------------------------------------------------------------------------ 3. the attention at a device position
def _attn_run(ops, c, t, H, Hkv, dh, rows=slice(None)):
    qkv, kc, vc = c["qkv"][rows].cuda(), c["kc"][rows].cuda().contiguous(), c["vc"][rows].cuda().contiguous()
    o = torch.full((qkv.shape[0], H * dh), SENT, dtype=F32, device="cuda")
    pos = torch.tensor([t], dtype=torch.int32, device="cuda")
    ops.attn_decode_pos(qkv, kc, vc, pos, c["cos"].cuda(), c["sin"].cuda(), H, Hkv, dh, dh ** -0.5, out=o)
    return o.cpu(), kc.cpu(), vc.cpu()


def _attn_check(ops, H, Hkv, dh, t):
    c = S.attn_pos_case(t, H, Hkv, dh)
    o64, k64, v64 = S.attn_decode_pos(c["qkv"], c["kc"], c["vc"], t, c["cos"], c["sin"], H, Hkv, dh, dh ** -0.5)
    o, kc, vc = _attn_run(ops, c, t, H, Hkv, dh)
    er, em = R.rel64(o, o64), R.maxabs64(o, o64)
    ek = R.rel64(kc[:, t], k64[:, t])
    print(f"attn_decode_pos H={H} Hkv={Hkv} dh={dh} pos={t}: o rel {er:.3e} maxabs {em:.3e}, appended k rel {ek:.3e}")
    assert not torch.isnan(o).any(), "a slot above *pos reached the output"
    assert er < R.OP_BAR and em < R.OP_MAXABS, (er, em)
    assert ek < R.OP_BAR and torch.equal(vc[:, t], v64[:, t].float())
    other = torch.ones(kc.shape[1], dtype=torch.bool)
    other[t] = False
    assert torch.equal(_bits(kc[:, other]), _bits(c["kc"][:, other])) and torch.equal(_bits(vc[:, other]), _bits(c["vc"][:, other]))
    # a row's bits are the row's own: row 1 alone
    o1, k1, _ = _attn_run(ops, c, t, H, Hkv, dh, rows=slice(1, 2))
    assert torch.equal(_bits(o1[0]), _bits(o[1])) and torch.equal(_bits(k1[0, t]), _bits(kc[1, t]))


@pytest.mark.parametrize("t", S.ATTN_POS)
@pytest.mark.parametrize("H,Hkv,dh", R.DECODE_GEOMS)
def test_attn_decode_pos_vs_float64(ops, H, Hkv, dh, t):
    _attn_check(ops, H, Hkv, dh, t)


def test_attn_decode_pos_beyond_one_round_of_keys(ops):
    """600 slots: the 512 threads of a workgroup take a second round of keys"""
    _attn_check(ops, *R.DECODE_GEOMS[1], S.ATTN_POS_LONG)


def test_attn_decode_pos_outside_the_cache_writes_nothing(ops):
    H, Hkv, dh = R.DECODE_GEOMS[1]
    c = S.attn_pos_case(5, H, Hkv, dh)
    for t in (c["kc"].shape[1], -1):
        o, kc, vc = _attn_run(ops, c, t, H, Hkv, dh)
        assert bool((o == SENT).all()) and torch.equal(_bits(kc), _bits(c["kc"])) and torch.equal(_bits(vc), _bits(c["vc"]))
    # the size limit: score rows for the capacity must fit the LDS of a CU -> code 1, nothing launched
    kc = torch.zeros(1, 50000, Hkv * dh, device="cuda")
    with pytest.raises(Exception, match="LDS"):
        ops.attn_decode_pos(c["qkv"][:1].cuda(), kc, kc.clone(), torch.zeros(1, dtype=torch.int32, device="cuda"), c["cos"].cuda(), c["sin"].cuda(),
                            H, Hkv, dh, 1.0)


# ------------------------------------------------------------------------------------------------ 4. / 5. the step and the device loop
@pytest.fixture(scope="module")
def gen():
    from procyon_amd.engine import LlamaConfig
    from procyon_amd.engine_f32 import LlamaEngineF32
    g = S.gen_fixture()
    g["eng"] = LlamaEngineF32(g["sd"], LlamaConfig(**R.GEN_GEOM, max_pos=256))
    return g


def _prefilled(g):
    eng = g["eng"]
    B, T = g["ids"].shape
    cache = eng.new_cache(B, T + g["steps"])
    logits, _ = eng.prefill(eng.embed_tokens(g["ids"]), g["mask"], "last", cache=cache)
    return cache, logits


def _host_loop(g, graph):
    """prefill, then 5 steps of decode_stream with the argmax fed back through device memory -> (logits per step [6][B, V], tokens [B, 6], cache)"""
    eng = g["eng"]
    B, T = g["ids"].shape
    cache, logits = _prefilled(g)
    st = eng.new_gen_state(B, g["steps"])
    lgs, toks = [logits.clone()], [logits.argmax(-1)]
    for i in range(1, g["steps"]):
        st.set(pos=T + i - 1, next_tok=toks[-1])
        lgs.append(eng.decode_stream(cache, st, B, graph=graph).clone())
        toks.append(lgs[-1].argmax(-1))
    return lgs, torch.stack(toks, 1).cpu(), cache


def test_stream_step_on_the_padded_greedy_fixture(gen):
    """logits of every row (the left-padded ones included) and step < 1e-4 against the oracle's greedy loop, tokens equal (the fixture's
    smallest top-2 margin is 1.8e-3 of the row norm: tests/test_f32_stream_cpu.py); eager launches and the replayed graph bit-equal, in
    the logits and in the K / V they append; the step counter moves"""
    lib = gen["eng"].ops.lib
    n0 = lib.pcy_debug_f32_stream_count()
    lg_e, tok_e, cache_e = _host_loop(gen, graph=False)
    n1 = lib.pcy_debug_f32_stream_count()
    lg_g, tok_g, cache_g = _host_loop(gen, graph=True)
    n2 = lib.pcy_debug_f32_stream_count()
    assert n1 - n0 == gen["steps"] - 1 and 0 <= n2 - n1 <= 1, (n0, n1, n2)      # (a replay enqueues nothing: a capture counts once)
    errs = [[rel_err(lg_e[i][b].cpu(), gen["logits"][b, i]) for b in range(R.GEN_B)] for i in range(gen["steps"])]
    for i, e in enumerate(errs):
        print(f"step {i}: per-row logits error {['%.3e' % v for v in e]}")
    worst = max(max(e) for e in errs)
    record_parity("fp32/stream_padded_greedy", err_logits_worst_row_step=worst, tokens_equal=bool(torch.equal(tok_e, gen["toks"])))
    assert worst < 1e-4, errs
    assert torch.equal(tok_e, gen["toks"]), (tok_e, gen["toks"])
    for i in range(gen["steps"]):
        assert torch.equal(_bits(lg_e[i]), _bits(lg_g[i])), f"eager and graph differ at step {i}"
    assert torch.equal(tok_e, tok_g) and torch.equal(_bits(cache_e.k), _bits(cache_g.k)) and torch.equal(_bits(cache_e.v), _bits(cache_g.v))


def test_stream_step_rows_do_not_depend_on_the_batch(gen):
    """row 1 (the left-padded one) alone on a one-row cache: the bits of its logits in the 3-row step"""
    eng = gen["eng"]
    B, T = gen["ids"].shape
    cache, logits = _prefilled(gen)
    st = eng.new_gen_state(B, 2)
    st.set(pos=T, next_tok=logits.argmax(-1))
    full = eng.decode_stream(cache, st, B, graph=False).clone()
    cache1 = eng.new_cache(1, T + gen["steps"])
    cache2, _ = _prefilled(gen)
    cache1.k.copy_(cache2.k[:, 1:2]); cache1.v.copy_(cache2.v[:, 1:2])
    st1 = eng.new_gen_state(1, 2)
    st1.set(pos=T, next_tok=logits.argmax(-1)[1:2])
    one = eng.decode_stream(cache1, st1, 1, graph=False)
    assert torch.equal(_bits(one[0]), _bits(full[1]))
    assert torch.equal(_bits(cache1.k[:, 0, T]), _bits(cache.k[:, 1, T]))


def test_stream_step_refusals(gen):
    from procyon_amd import _lib as L
    eng = gen["eng"]
    cache, _ = _prefilled(gen)
    st = eng.new_gen_state(R.GEN_B, 2)
    with pytest.raises(L.PcyError, match="B=4"):
        eng.decode_stream(cache, st, 4, graph=False)
    keep = torch.ones(R.GEN_B, cache.Tmax, dtype=torch.uint8, device="cuda")
    st.c.keep = keep.data_ptr()
    with pytest.raises(L.PcyError, match="keep must be NULL"):
        eng.decode_stream(cache, st, R.GEN_B, graph=True)


def test_device_greedy_loop(gen):
    """pcy_f32_llama_greedy: pick on the prefill's logits, then 5 x (step + pick + advance) on the device -- tokens, the summed fp32
    log-softmax (atol 1e-3 against the oracle's) and the record rows; eager and replayed runs bit-equal; step by step, every record row is
    the step's logits"""
    eng = gen["eng"]
    B, T = gen["ids"].shape
    runs = {}
    for graph in (False, True):
        cache, logits = _prefilled(gen)
        st = eng.new_gen_state(B, gen["steps"], keep_logits=True)
        st.logits.copy_(logits)
        st.set(pos=T, step=0)
        eng.greedy_pick(cache, st, B, advance_pos=False)
        eng.greedy_steps(cache, st, B, gen["steps"] - 1, graph=graph)
        torch.cuda.synchronize()
        assert int(st.pos) == T + gen["steps"] - 1 and int(st.step) == gen["steps"]
        runs[graph] = (st.tokens_out.cpu().long(), st.logprob.cpu(), st.logits_all.clone(), st.logits.clone())
    tok, lp, rec, last = runs[True]
    assert torch.equal(tok, gen["toks"]), (tok, gen["toks"])
    print("logprob", lp, "oracle", gen["logprob"])
    assert torch.allclose(lp, gen["logprob"], atol=1e-3), (lp, gen["logprob"])
    e = max(rel_err(rec[i, b].cpu(), gen["logits"][b, i]) for i in range(gen["steps"]) for b in range(B))
    assert e < 1e-4, e
    assert torch.equal(_bits(rec[-1]), _bits(last))
    for a, b in zip(runs[False], runs[True]):
        assert torch.equal(_bits(a.float()), _bits(b.float()))
    # one step at a time: record row i is the logits of step i
    cache, logits = _prefilled(gen)
    st = eng.new_gen_state(B, gen["steps"], keep_logits=True)
    st.logits.copy_(logits)
    st.set(pos=T, step=0)
    eng.greedy_pick(cache, st, B, advance_pos=False)
    assert torch.equal(_bits(st.logits_all[0]), _bits(logits))
    for i in range(1, gen["steps"]):
        eng.greedy_steps(cache, st, B, 1, graph=True)
        assert torch.equal(_bits(st.logits_all[i]), _bits(st.logits)) and torch.equal(_bits(st.logits_all[i]), _bits(rec[i]))
        assert torch.equal(st.next_tok.cpu().long(), gen["toks"][:, i])


def test_greedy_pick_ties_take_the_lowest_index(gen):
    eng = gen["eng"]
    B, V = 2, R.GEN_GEOM["vocab"]
    cache = eng.new_cache(B, 4)
    st = eng.new_gen_state(B, 2)
    lg = torch.zeros(B, V)
    lg[0, [7, 300]] = 3.0
    lg[1, :] = float("-inf")
    lg[1, [V - 1, 100]] = -1.0
    st.logits.copy_(lg)
    st.set(pos=1, step=0)
    eng.greedy_pick(cache, st, B, advance_pos=True)
    torch.cuda.synchronize()
    assert st.next_tok.tolist() == [7, 100] and st.tokens_out[:, 0].tolist() == [7, 100] and int(st.pos) == 2 and int(st.step) == 1
    ref = lg.double().log_softmax(-1)[[0, 1], [7, 100]]
    assert torch.allclose(st.logprob.cpu().double(), ref, atol=1e-5)


def test_engine_beam_search_on_the_replayed_step(gen):
    """the oracle's own diverse beam search loop over an adapter that runs LlamaEngineF32.prefill and, for every cached step, the replayed
    graph with next_tok / *pos written on the device; the loop re-indexes the engine's K / V rows in place.  Tokens equal (the smallest
    selection gap is 4.9e-4 of the row norm, asserted > 2e-4 on the CPU), scores atol 1e-3, logits < 1e-4"""
    from oracle import llama_ref as LR
    eng = gen["eng"]
    emb, mask = S.beam_fixture(gen)
    t_ref, s_ref, l_ref, rel = S.beam_oracle(gen["sd"], gen["geom"], emb, mask, eos_id=2, **S.BEAM_KW)
    assert rel > S.BEAM_GAP
    state = {}

    def enc(input_embeds=None, input_ids=None, attn_masks=None, past_key_values=None):
        if past_key_values is None:
            BB, T, _ = input_embeds.shape
            state["cache"], state["t"] = eng.new_cache(BB, T + S.BEAM_KW["max_len"]), T
            state["st"] = eng.new_gen_state(BB, S.BEAM_KW["max_len"])
            logits, _ = eng.prefill(input_embeds, attn_masks, "last", cache=state["cache"])
        else:
            state["st"].set(pos=state["t"], next_tok=input_ids.view(-1).cuda())
            logits = eng.decode_stream(state["cache"], state["st"], input_ids.shape[0], graph=True)
            state["t"] += 1
        c = state["cache"]
        return logits.cpu()[:, None, :], [[c.k[l], c.v[l]] for l in range(c.k.shape[0])]

    t, s, lg = LR.beam_search(enc, emb, mask, vocab_size=gen["geom"].vocab, eos_id=2, **S.BEAM_KW)
    e_rows = [rel_err(lg[b], l_ref[b]) for b in range(2)]
    print(f"beam logits error per prompt {e_rows}")
    record_parity("fp32/stream_padded_beam", err_logits=max(e_rows), tokens_equal=bool(torch.equal(t, t_ref)))
    assert torch.equal(t, t_ref), (t, t_ref)
    assert torch.allclose(s, s_ref, atol=1e-3), (s, s_ref)
    assert max(e_rows) < 1e-4, e_rows


# ------------------------------------------------------------------------------------------------ 6. model level
def test_model_generates_on_the_stream_step():
    """UnifiedProCyon.generate(decode_f32="stream") on the tiny fp32 model of tests/test_gpu_fp32.py (never cast): greedy runs on the device
    loop, beam through the replayed graph with host-side selection -- the oracle's tokens, scores (atol 1e-3) and logits < 1e-4; sampling
    runs and returns the shapes of decode_f32="ops"; a bf16 model and any other value are ValueErrors"""
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
    # greedy
    t_ref, lg_ref, lp_ref = LR.greedy_generate(w["llama"], lgeom, gemb, gmask, 6)
    margin = float(S.top2_margins(lg_ref).min())
    print("greedy top-2 margin / norm:", margin)
    assert margin >= S.TOKEN_MARGIN, margin
    n0 = m.text_encoder.engine_f32.ops.lib.pcy_debug_f32_stream_count()
    toks, lp, lg, _ = m.generate(mk(ginstr, prot, gslots), max_len=6, method="greedy", decode_f32="stream")
    assert m.text_encoder.engine_f32.ops.lib.pcy_debug_f32_stream_count() > n0
    e_rows = [rel_err(lg[b, 0].float(), lg_ref[b]) for b in range(2)]
    print(f"greedy logits error per row {e_rows}")
    assert lg.dtype == F32 and tuple(toks.shape) == (2, 1, 6) and torch.equal(toks[:, 0], t_ref), (toks, t_ref)
    assert max(e_rows) < 1e-4, e_rows
    assert torch.allclose(lp[:, 0], lp_ref, atol=1e-3), (lp, lp_ref)
    # beam: the oracle's smallest selection gap first (on the CPU, from the oracle alone)
    kw = dict(max_len=5, beam_size=4, beam_group_size=2, diversity_penalty=0.8)
    tb_ref, sb_ref, lb_ref, rel = S.beam_oracle(w["llama"], lgeom, gemb, gmask, eos_id=m.tokenizer.eos_token_id, **kw)
    print("beam selection gap / row norm:", rel)
    assert rel > S.BEAM_GAP, rel
    tb, sb, lb, _ = m.generate(mk(ginstr, prot, gslots), method="beam", decode_f32="stream", **kw)
    eb_rows = [rel_err(lb[b].float(), lb_ref[b]) for b in range(2)]
    print(f"beam logits error per prompt {eb_rows}")
    record_parity("fp32/stream_model_small_generate", err_greedy_logits=max(e_rows), err_beam_logits=max(eb_rows),
                  greedy_tokens_equal=bool(torch.equal(toks[:, 0], t_ref)), beam_tokens_equal=bool(torch.equal(tb, tb_ref)))
    assert torch.equal(tb, tb_ref) and torch.allclose(sb, sb_ref, atol=1e-3), (tb, tb_ref, sb, sb_ref)
    assert max(eb_rows) < 1e-4, eb_rows
    # sampling keeps its host-side selection: shapes and dtypes of the default path
    ts, ls, gs, _ = m.generate(mk(ginstr, prot, gslots), max_len=4, method="nucleus", decode_f32="stream")
    to, lo, go, _ = m.generate(mk(ginstr, prot, gslots), max_len=4, method="nucleus")
    assert ts.shape == to.shape and ls.shape == lo.shape and gs.shape == go.shape and gs.dtype == go.dtype
    assert rel_err(gs[:, 0, 0].float(), go[:, 0, 0].float()) == 0.0          # step 0 is the prefill's logits on both paths
    # refusals
    with pytest.raises(ValueError, match="decode_f32"):
        m.generate(mk(ginstr, prot, gslots), max_len=3, method="greedy", decode_f32="fast")
    with pytest.raises(ValueError, match="decode_f32"):
        m.generate(mk(ginstr, prot, gslots), max_len=3, method="greedy", decode_f32=True)
    m.bfloat16()
    with pytest.raises(ValueError, match="bf16"):
        m.generate(mk(ginstr, prot, gslots), max_len=3, method="greedy", decode_f32="stream")
