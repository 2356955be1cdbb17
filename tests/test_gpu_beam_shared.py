"""Beam search on a shared-prefix cache (include/pcy.h pcy_kv_cache.prefix_k): the beams of a prompt read ONE copy of its
K / V and own only their suffix slots.  Nothing about the arithmetic changes -- the decode attention takes the address of a cached row from
the prefix panel of the row's prompt or from the row's suffix panel, and then runs the same loads, MFMAs and sums -- so every check here is a
BIT-identity against the plain cache that holds the same rows (prefill B prompts into a B x beam-row cache, replicate with pcy_kv_reorder):
the path `PCY_DISABLE=beam_kv_shared` still takes.  All through the C ABI, on the 2-layer full-width geometries of test_gpu_decode_wide.py."""
import pytest
import torch

from conftest import pcy_disable
from test_gpu_decode_wide import GEOMS, _gen_inputs, _oracle_embeds, _prompts

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N = 8                      # decode steps per case
KIND_SHARED = 16           # pcy_debug_dispatch_count: decode steps served from a shared-prefix cache
# (B, beam, T): 10, 10, 40 and 160 rows.  T = 21: the prefix boundary falls inside a 16-key tile; T = 250 + 8 steps: the suffix crosses the
# 256-key pass boundary; the first step of every case has an empty suffix (t == prefix_T)
CASES = [(1, 10, 21), (2, 5, 250), (4, 10, 21), (16, 10, 12)]


@pytest.fixture(scope="module", params=list(GEOMS))
def geo(request):
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    kw = GEOMS[request.param]
    return request.param, kw, LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, max_pos=512))


@pytest.fixture(autouse=True)
def _default_env(monkeypatch):
    for var in ("PCY_DISABLE", "PCY_NB_MAX", "PCY_MB_MAX", "PCY_AO_XMIN"):
        monkeypatch.delenv(var, raising=False)


def _count():
    from procyon_amd import _lib
    return int(_lib.load().pcy_debug_dispatch_count(KIND_SHARED))


def _prompt_batch(B, T, d, seed, ragged):
    g = torch.Generator().manual_seed(seed)
    emb = (torch.randn(B, T, d, generator=g) * 0.02).to(BF)
    mask = torch.ones(B, T)
    if ragged:
        for b in range(B):
            mask[b, :(b * 3 + 2) % 7] = 0           # left pads (row 0 has two): masked in the prefill AND in the decode steps
    return emb, mask


def _caches(eng, emb, mask, beam, max_new):
    """the same prefill twice: (plain) into rows 0..B-1 of a B*beam-row cache, then replicated -- today's layout; (shared) into a B-row cache of
    exactly T slots that the B*beam rows of a suffix-only cache share.  -> plain, shared, prefix, prefill logits repeated per beam"""
    B, T, _ = emb.shape
    BB = B * beam
    plain = eng.new_cache(BB, T + max_new)
    lg, _ = eng.prefill(emb.cuda(), mask, plain, "last")
    eng.kv_reorder(plain, torch.arange(BB, dtype=torch.int32) // beam, T)
    prefix = eng.new_cache(B, T)
    lg2, _ = eng.prefill(emb.cuda(), mask, prefix, "last")
    shared = eng.new_beam_cache(prefix, beam, max_new)
    assert torch.equal(lg, lg2)
    assert shared.k.shape == (eng.cfg.n_layers, BB, eng.cfg.n_kv_heads, max_new, eng.cfg.head_dim) and shared.capacity == T + max_new
    rows = torch.arange(BB, device="cuda") // beam
    assert torch.equal(prefix.k[:, rows], plain.k[:, :, :, :T]) and torch.equal(prefix.v[:, rows], plain.v[:, :, :, :T])
    return plain, shared, prefix, lg.repeat_interleave(beam, dim=0).contiguous()


def _parents(B, beam, step):
    """parent map of a step: parents stay inside their prompt, some rows keep their place, some parents are taken twice; varies with the step"""
    local = list(range(beam))
    local[1], local[3] = 0, 1
    if beam > 5:
        local[5], local[7] = 4, 3
    if step % 2:
        local[beam - 1], local[2] = beam - 2, 0
    return torch.tensor([b * beam + p for b in range(B) for p in local], dtype=torch.int32)


def _run_steps(eng, cache, V, BB, B, beam, T, keep, graph):
    """N decode steps with per-row distinct tokens, a K / V reorder over the generated slots after each -> logits of every step, and the
    generated K / V slots [T, T + i] as the cache sees them after every reorder"""
    from procyon_amd.engine import Context, GenState
    st = GenState(BB, V, 1, "cuda", keep=keep)
    lgs, ks, vs = [], [], []
    for i in range(N):
        st.pos.fill_(T + i)
        st.next_tok.copy_(((torch.arange(BB) * 37 + i * 101 + 5) % V).to(torch.int32))
        (eng.decode_graph if graph else eng.decode)(cache, st, BB)
        lgs.append(st.logits.clone())
        eng.kv_reorder(cache, _parents(B, beam, i), T + i + 1, t0=T)
        lo = 0 if cache.prefix is not None else T
        ks.append(cache.k[:, :, :, lo:lo + i + 1].clone())
        vs.append(cache.v[:, :, :, lo:lo + i + 1].clone())
    Context.get().sync()
    return lgs, ks, vs


def _check_steps(geo, monkeypatch, B, beam, T, graph=False, ragged=False, off=()):
    name, kw, eng = geo
    pcy_disable(monkeypatch, *off)
    BB, V = B * beam, kw["vocab"]
    emb, mask = _prompt_batch(B, T, kw["d"], seed=B * 1000 + T, ragged=ragged)
    plain, shared, prefix, _ = _caches(eng, emb, mask, beam, N)
    pk, pv = prefix.k.clone(), prefix.v.clone()
    keep = None
    if ragged:
        keep = torch.ones(BB, T + N, dtype=torch.uint8, device="cuda")
        keep[:, :T] = mask.repeat_interleave(beam, dim=0).to("cuda", torch.uint8)
    ref = _run_steps(eng, plain, V, BB, B, beam, T, keep, graph)
    n0 = _count()
    got = _run_steps(eng, shared, V, BB, B, beam, T, keep, graph)
    served = _count() - n0
    assert torch.isfinite(ref[0][-1].float()).all()
    for i in range(N):
        assert torch.equal(got[0][i], ref[0][i]), (name, B, beam, T, "logits of step", i)
        # suffix[:, b, :, j] == plain[:, b, :, T + j] for every generated slot so far, after the step's reorder
        assert torch.equal(got[1][i], ref[1][i]), (name, B, beam, T, "K after step", i)
        assert torch.equal(got[2][i], ref[2][i]), (name, B, beam, T, "V after step", i)
    assert torch.equal(prefix.k, pk) and torch.equal(prefix.v, pv), "a decode step or a reorder wrote into the shared prefix"
    if graph:
        assert served >= 1      # (a replayed step does not pass through the enqueue: the capture counts)
    else:
        assert served == N, f"{served} of {N} steps were counted as served from the shared-prefix cache"
    # the logical rows the cache reports: prefix rows repeated + suffix
    k_l, v_l = shared.layer(1, T + N)
    assert torch.equal(k_l, plain.k[1, :, :, :T + N]) and torch.equal(v_l, plain.v[1, :, :, :T + N])


@pytest.mark.parametrize("B,beam,T", CASES)
def test_shared_prefix_steps_bit_identical(geo, monkeypatch, B, beam, T):
    """8 eager decode steps + reorders on the shared cache against the plain cache: logits, generated K / V slots, untouched prefix, and
    dispatch kind 16 advanced once per step."""
    _check_steps(geo, monkeypatch, B, beam, T)


@pytest.mark.parametrize("B,beam,T", [(2, 5, 250), (4, 10, 21)])
def test_shared_prefix_steps_replayed(geo, monkeypatch, B, beam, T):
    """the same through pcy_llama_decode_graph (one capture, seven replays per cache)"""
    _check_steps(geo, monkeypatch, B, beam, T, graph=True)


@pytest.mark.parametrize("B,beam,T", [(4, 10, 21), (16, 10, 12)])
def test_shared_prefix_steps_with_a_ragged_keep_mask(geo, monkeypatch, B, beam, T):
    """left-padded prompts: the pads are masked inside the PREFIX; the mask rows are laid out in logical slots (row stride T + max_new)"""
    _check_steps(geo, monkeypatch, B, beam, T, ragged=True)


@pytest.mark.parametrize("B,beam,T", [(1, 10, 21), (2, 5, 250)])
def test_shared_prefix_steps_without_the_fused_qkv_finish(geo, monkeypatch, B, beam, T):
    """PCY_DISABLE=attn_qkv_finish: up to 32 rows the attention otherwise adds up the qkv projection's K-split partial sums itself
    (attn_dec_splitk_kernel); with the finish as its own launch the step takes attn_dec_kernel -- the other shared-prefix instantiation"""
    _check_steps(geo, monkeypatch, B, beam, T, off=("attn_qkv_finish",))


@pytest.mark.parametrize("B,beam", [(1, 10), (4, 10)])
def test_shared_prefix_replayed_beam_chain(geo, monkeypatch, B, beam):
    """pcy_llama_beam_steps (decode -> logits record -> beam step -> K / V reorder, one replayed chain per step), n = 8: 10 rows take the
    one-pass permute, 40 rows the two-launch gather; both read the slot count from the device and must count it from the prefix length on."""
    from procyon_amd.engine import BeamState, Context
    name, kw, eng = geo
    T, group, V, BB = 21, 5, kw["vocab"], B * beam
    emb, mask = _prompt_batch(B, T, kw["d"], seed=77 + B, ragged=False)
    plain, shared, prefix, logits = _caches(eng, emb, mask, beam, N + 1)
    pk, pv = prefix.k.clone(), prefix.v.clone()

    def run(cache):
        bs = BeamState(B, beam, N + 1, V - 1, prompt_len=T, device="cuda")
        st = bs.gen_state(V)
        rec = torch.zeros(N + 1, BB, V, dtype=BF, device="cuda")
        rec[0].copy_(logits)
        eng.beam_step(logits, bs, group, 0.8)
        eng.kv_reorder(cache, bs.src, T, t0=T)
        eng.beam_steps(cache, st, bs, group, 0.8, rec, N, kv_t0=T)
        out, n = bs.tokens()
        Context.get().sync()
        lo = 0 if cache.prefix is not None else T
        return dict(tokens=out.clone(), scores=bs.cur.clone(), src=bs.src.clone(), anc=bs.anc[:n].clone(), rec=rec[:n].clone(),
                    k=cache.k[:, :, :, lo:lo + N].clone(), v=cache.v[:, :, :, lo:lo + N].clone())

    ref = run(plain)
    n0 = _count()
    got = run(shared)
    assert _count() > n0
    assert ref["tokens"].shape[1] == N + 1 and torch.isfinite(ref["rec"].float()).all()
    for key in ref:
        assert torch.equal(got[key], ref[key]), (name, B, beam, key)
    assert torch.equal(prefix.k, pk) and torch.equal(prefix.v, pv)


# ---------------------------------------------------------------------------------------------- generate(method="beam") end to end (small model)
@pytest.fixture(scope="module")
def small():
    from oracle import esm_ref as ER
    from oracle import llama_ref as LR
    from procyon_amd import synth
    from procyon_amd import synthetic_model as SM
    model, w = SM.build("small", device="cuda", return_weights=True, max_new_tokens=32)
    g = w["geom"]
    prot = synth.protein_tokens([90, 41, 66, 23, 57], seed=3)
    return dict(model=model, w=w, lgeom=LR.LlamaGeom(**g["llama"]), egeom=ER.EsmGeom(**g["esm"]), prot=prot)


@pytest.fixture
def beam_caches(monkeypatch):
    """observes LlamaEngine.new_beam_cache: the caches every call built"""
    from procyon_amd.engine import LlamaEngine
    seen, orig = [], LlamaEngine.new_beam_cache

    def wrapped(self, prefix_cache, beam, max_new):
        c = orig(self, prefix_cache, beam, max_new)
        seen.append(c)
        return c
    monkeypatch.setattr(LlamaEngine, "new_beam_cache", wrapped)
    return seen


@pytest.mark.parametrize("group", [2, 5])
def test_generate_beam_runs_on_the_shared_cache(small, monkeypatch, beam_caches, group):
    """4 prompts x beam 10 at the default switches: the oracle's diverse beam search (tie-aware rule of tests/beam_oracle.py); the twin on the
    plain cache (PCY_DISABLE=beam_kv_shared) and the four-calls-per-step form (beam_graph) EQUAL in tokens, scores and logits; the cache the
    call allocated is B x T prefix slots + B*beam x max_new suffix slots."""
    from beam_oracle import assert_beam_matches_oracle
    from oracle import llama_ref as LR
    from procyon_amd.engine import Context
    m, w = small["model"], small["w"]
    n, beam = 4, 10
    instr, slots = _prompts(n, seed=40 + group)
    emb, mask = _oracle_embeds(small, _gen_inputs(small, instr, slots))
    enc = LR.make_text_encoder(w["llama"], small["lgeom"])
    trace = []
    kw = dict(max_len=6, beam_size=beam, beam_group_size=group, diversity_penalty=0.8)
    t_ref, s_ref, lg_ref = LR.beam_search(enc, emb, mask, vocab_size=small["lgeom"].vocab, eos_id=m.tokenizer.eos_token_id, trace=trace, **kw)

    def run(*off):
        pcy_disable(monkeypatch, *off)
        n0, c0 = _count(), len(beam_caches)
        res = m.generate(_gen_inputs(small, instr, slots), method="beam", **kw)[:3]
        Context.get().sync()
        return res, _count() - n0, beam_caches[c0:]

    res, served, caches = run()
    assert_beam_matches_oracle(*res, t_ref, s_ref, lg_ref, trace)
    assert served > 0 and len(caches) == 1
    g, T = w["geom"]["llama"], emb.shape[1]
    dh = g["d"] // g["n_heads"]
    assert caches[0].prefix.k.shape == caches[0].prefix.v.shape == (g["n_layers"], n, g["n_kv_heads"], T, dh)
    assert caches[0].k.shape == caches[0].v.shape == (g["n_layers"], n * beam, g["n_kv_heads"], 32, dh)       # max_new_tokens of the model
    twin, served_twin, caches_twin = run("beam_kv_shared")
    assert served_twin == 0 and not caches_twin
    eager, served_eager, caches_eager = run("beam_graph")
    assert served_eager > 0 and len(caches_eager) == 1
    for other in (twin, eager):
        for x, y in zip(other, res):
            assert torch.equal(x, y)


def test_generate_beam_5_rows_stay_on_the_plain_cache(small, monkeypatch, beam_caches):
    """1 prompt x beam 5 = 5 rows: inside the small-batch step's range, the plan keeps the plain cache whatever the switches say"""
    from procyon_amd.engine import Context
    m = small["model"]
    instr, slots = _prompts(1, seed=9)
    n0 = _count()
    tokens, _, logits, _ = m.generate(_gen_inputs(small, instr, slots), method="beam", max_len=6, beam_size=5, beam_group_size=5, diversity_penalty=0.8)
    Context.get().sync()
    assert tokens.shape[:2] == (1, 5) and torch.isfinite(logits.float()).all()
    assert _count() == n0 and not beam_caches


@pytest.mark.parametrize("n,beam,off,layout", [(2, 6, (), "shared"), (1, 4, (), "prefill_once"), (1, 4, ("beam_prefill_once",), "replicated")])
def test_generate_adds_nothing_to_generate_beam(small, monkeypatch, beam_caches, n, beam, off, layout):
    """`generate(method="beam")` is LlamaEngine.generate_beam + an unflatten: the driver called directly on the model's own prompt embeddings (the
    oracle's differ by the encoder's bf16 noise; bit-equality needs the same bits going in) gives the same tokens, scores and logits record on each
    cache layout: 12 rows (shared prefix), 4 rows (prefill once + replicate), 4 rows under PCY_DISABLE=beam_prefill_once (replicated prefill)."""
    from procyon_amd.engine import LlamaEngine
    m = small["model"]
    pcy_disable(monkeypatch, *off)
    replicated, orig = [], LlamaEngine.prefill_all
    monkeypatch.setattr(LlamaEngine, "prefill_all", lambda self, emb, *a, **k: replicated.append(emb.shape[0]) or orig(self, emb, *a, **k))
    instr, slots = _prompts(n, seed=70 + n)
    emb, _, mask, *_ = m._preprocessing(_gen_inputs(small, instr, slots), crop_off=True, no_pad=True, left_pad=True)
    direct = m.text_encoder.engine.generate_beam(emb, mask, 10, beam, 2, 0.8, m.tokenizer.eos_token_id, 32)
    assert direct[0].shape == (n * beam, 10) and direct[0].dtype == torch.int64 and not direct[0].is_cuda and direct[2].is_pinned()
    res = m.generate(dict(_gen_inputs(small, instr, slots), reference_indices={"target": {"text": None}, "input": {"seq": slots}}), method="beam",
                     max_len=10, beam_size=beam, beam_group_size=2, diversity_penalty=0.8, return_all_internals=True)
    assert len(beam_caches) == (2 if layout == "shared" else 0) and replicated == ([n * beam] * 2 if layout == "replicated" else [])
    for got, flat in zip((res["out_tokens"], res["out_log_probs"], res["out_logits"]), direct):
        assert torch.equal(got, flat.unflatten(0, (n, beam)))


# ---------------------------------------------------------------------------------------------- what a shared cache is refused for
def test_shared_cache_rejections(geo):
    """one row (the one-launch steps and the streaming loop read plain caches only: an argument error, not a fallback); the prefill"""
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import Context, GenState
    name, kw, eng = geo
    T = 16
    emb, mask = _prompt_batch(1, T, kw["d"], seed=3, ragged=False)
    prefix = eng.new_cache(1, T)
    eng.prefill(emb.cuda(), mask, prefix, "last")
    for rows in (1, 2):                                   # 2 rows: the streaming loop
        cache = eng.new_beam_cache(prefix, rows, 4)
        st = GenState(rows, kw["vocab"], 1, "cuda")
        st.pos.fill_(T)
        n0 = _count()
        for call in (eng.decode, eng.decode_graph):
            with pytest.raises(PcyError, match="shared-prefix"):
                call(cache, st, rows)
        assert _count() == n0
    with pytest.raises(PcyError, match="shared prefix"):
        eng.prefill(emb.cuda(), mask, eng.new_beam_cache(prefix, 10, 4), "last")
    Context.get().sync()


def test_a_capture_is_not_replayed_on_another_prefix(geo):
    """Two shared caches with the SAME suffix arrays and state but different prefixes: the second pcy_llama_decode_graph call must capture
    anew (the prefix pointers are part of the graph key) -- its logits are those of an eager step on that prefix."""
    from procyon_amd._lib import KvCache
    from procyon_amd.engine import Context, GenState
    name, kw, eng = geo
    B, beam, T = 1, 10, 21
    V = kw["vocab"]
    prefixes = []
    for seed in (1, 2):
        emb, mask = _prompt_batch(B, T, kw["d"], seed=seed, ragged=False)
        p = eng.new_cache(B, T)
        eng.prefill(emb.cuda(), mask, p, "last")
        prefixes.append(p)
    assert prefixes[0].k.data_ptr() != prefixes[1].k.data_ptr() and not torch.equal(prefixes[0].k, prefixes[1].k)
    st = GenState(beam, V, 1, "cuda")
    st.next_tok.copy_((torch.arange(beam) * 11 + 3).to(torch.int32))

    def step(call, cache):
        st.pos.fill_(T)
        call(cache, st, beam)
        Context.get().sync()
        return st.logits.clone()

    first = eng.new_beam_cache(prefixes[0], beam, 4)
    lg_a = step(eng.decode_graph, first)
    second = eng.new_beam_cache(prefixes[1], beam, 4)
    second.k, second.v = first.k, first.v               # the same suffix arrays: only the prefix fields of the descriptor differ
    second.c = KvCache(first.k.data_ptr(), first.v.data_ptr(), beam, 4, prefixes[1].k.data_ptr(), prefixes[1].v.data_ptr(), B, T, beam)
    lg_b = step(eng.decode_graph, second)
    lg_b_eager = step(eng.decode, eng.new_beam_cache(prefixes[1], beam, 4))
    assert not torch.equal(lg_a, lg_b_eager)
    assert torch.equal(lg_b, lg_b_eager)
