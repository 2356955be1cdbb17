"""The opt-in cached decode that streams e4m3 weights (pcy_gemv_w8, pcy_llama_decode_w8, pcy_llama_greedy_w8): weight-only
fp8 -- the activations stay bf16, the codes become fp32 in the kernel, the power-of-two row scale meets the finished sum once.

The test design rests on two facts held on the CPU by tests/test_decode_w8_cpu.py: dequant(quant_rows(w)) is a bf16 matrix, and quantising it
again gives the same values.  So the reference of the operator is plain bf16 `F.linear(x, W_deq)`, and an engine built from a state dict
whose projection weights were first put on the e4m3 grid (`sd_deq`) is a bf16 model whose weights EQUAL its e4m3 copies: the existing bf16
oracle on `sd_deq` is the oracle of the new step and the default bf16 step of the same engine is its twin up to the order of the sums.  No
new tolerance: `assert_bf16_close` with the arguments of tests/test_gpu_kernels.py at operator level, `check_oracle` (2e-2 and the near-tie
rule) at step level."""
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_bf16_close, pcy_disable, rel_err
from fulldepth_common import check_oracle, decode_counts
from test_gpu_decode_gemm import GEOMS, _gen_inputs, _prompts, small  # noqa: F401  (small: the module's fixture)
from test_gpu_kernels import rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
STORE, RESID, SWIGLU = 0, 1, 4
N_STEPS = 3    # cached decode steps per case


@pytest.fixture(scope="module")
def ctx():
    from procyon_amd.engine import Context
    return Context.get()


def _count():
    from procyon_amd import _lib
    return int(_lib.load().pcy_debug_decode_w8_count())


def _quant(ctx, w):
    """bf16 [N, K] (CPU) -> (codes uint8 [N, K] and scales fp32 [N] on the device, the dequantised matrix as bf16 on the CPU: exact)"""
    q, s = ctx.quant_rows_fp8(w.cuda())
    deq = q.cpu().view(torch.float8_e4m3fn).float() * s.cpu()[:, None]
    assert torch.equal(deq.to(BF).float(), deq)
    return q, s, deq.to(BF)


# ---------------------------------------------------------------------------------------------------------------- the operator
_ops = {}


def _op_case(ctx, N, K):
    """W [N, K] quantised, 8 rows of x, a residual, and the bf16 reference of all 8 rows: built once per shape"""
    if (N, K) not in _ops:
        x, W, r = rnd(8, K, seed=1), rnd(N, K, seed=2, std=0.05), rnd(8, N, seed=4)
        q, s, deq = _quant(ctx, W)
        _ops[(N, K)] = dict(x=x, r=r, q=q, s=s, deq=deq, lin=F.linear(x, deq))
    return _ops[(N, K)]


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("N,K", [(64, 4096), (70, 256), (130, 11008), (64, 14336), (1001, 1024)])
def test_gemv_w8_store_and_resid(ctx, N, K, B):
    """against F.linear(x, W_deq) with pcy_gemv's rounding points; the residual aliases y.  K = 256 and 11008 end inside a 1024-element
    k-iteration; B = 5 and 8 take two passes over the matrix."""
    c = _op_case(ctx, N, K)
    x, lin = c["x"][:B], c["lin"][:B]
    out = ctx.gemv_w8(c["q"], c["s"], x.cuda()).cpu()
    assert_bf16_close(out, lin, f"gemv_w8 B{B} {N}x{K} store", inter=None, max_frac=0.02)
    y = c["r"][:B].cuda()
    out = ctx.gemv_w8(c["q"], c["s"], x.cuda(), resid=y, epi=RESID, out=y).cpu()
    assert_bf16_close(out, lin + c["r"][:B], f"gemv_w8 B{B} {N}x{K} resid", inter=lin, max_frac=0.02)


@pytest.mark.parametrize("B", [1, 4, 5])
@pytest.mark.parametrize("cast", [0, 1])
def test_gemv_w8_fused_rms_and_swiglu(ctx, B, cast):
    """48 features at K = 4096 with the fused RMSNorm, both rounding orders of the norm; and the norm in front of a plain projection
    (the arguments of tests/test_gpu_kernels.py::test_gemv_fused_rms_and_swiglu)"""
    from oracle.llama_ref import rms_norm
    from procyon_amd.engine import interleave_gate_up
    K, Fh = 4096, 48
    x, w = rnd(B, K, seed=1), (1 + 0.02 * rnd(K, seed=6).float()).to(BF)
    q, s, deq = _quant(ctx, interleave_gate_up(rnd(Fh, K, seed=2, std=0.03), rnd(Fh, K, seed=3, std=0.03)))
    blocks = deq.view(Fh // 16, 2, 16, K)                                        # undo the 16-row gate/up interleave
    g, u = blocks[:, 0].reshape(Fh, K), blocks[:, 1].reshape(Fh, K)
    xn = rms_norm(x, w, 1e-5, "hf5" if cast == 0 else "hf431")
    out = ctx.gemv_w8(q, s, x.cuda(), epi=SWIGLU, rms_w=w.cuda(), rms_eps=1e-5, rms_cast=cast).cpu()
    assert out.shape == (B, Fh)
    assert_bf16_close(out, F.silu(F.linear(xn, g)) * F.linear(xn, u), "gemv_w8 rms+swiglu", ulps=2)
    out = ctx.gemv_w8(q, s, x.cuda(), epi=SWIGLU).cpu()                          # ... and without the norm
    assert_bf16_close(out, F.silu(F.linear(x, g)) * F.linear(x, u), "gemv_w8 swiglu", ulps=2)
    q, s, deq = _quant(ctx, rnd(72, K, seed=5, std=0.03))
    out = ctx.gemv_w8(q, s, x.cuda(), rms_w=w.cuda(), rms_eps=1e-5, rms_cast=cast).cpu()
    assert_bf16_close(out, F.linear(xn, deq), "gemv_w8 rms+store")


@pytest.mark.parametrize("K", [4096, 11008])
def test_gemv_w8_one_hot_picks_the_column(ctx, K):
    """x = one-hot at k: a single product is exact, so the result IS column k of W_deq -- a byte order, a lane-to-element map or a rotated
    k-iteration that is off by anything shows.  8 positions = one call of 4 + 4 rows; the weights differ in every element's code."""
    N = 130
    W = (((torch.arange(N * K).view(N, K) * 7) % 97 - 48).float() * 2.0 ** -4).to(BF)
    q, s, deq = _quant(ctx, W)
    ks = [0, 1, 3, 15, 16, 1023, 1024, K - 1]
    x = torch.zeros(len(ks), K, dtype=BF)
    for b, k in enumerate(ks):
        x[b, k] = 1.0
    out = ctx.gemv_w8(q, s, x.cuda()).cpu()
    for b, k in enumerate(ks):
        assert torch.equal(out[b], deq[:, k]), (K, k)
        one = ctx.gemv_w8(q, s, x[b:b + 1].cuda()).cpu()
        assert torch.equal(one[0], deq[:, k]), (K, k, "one row")


@pytest.mark.parametrize("B", [3, 4, 5, 8])
def test_gemv_w8_rows_do_not_depend_on_the_batch(ctx, B):
    """row r of a B-row call is bit-equal to the one-row call on that row: every epilogue, with and without the fused norm"""
    from procyon_amd.engine import interleave_gate_up
    c = _op_case(ctx, 130, 11008)
    w = (1 + 0.02 * rnd(4096, seed=6).float()).to(BF).cuda()
    gq, gs, _ = _quant(ctx, interleave_gate_up(rnd(48, 4096, seed=2, std=0.03), rnd(48, 4096, seed=3, std=0.03)))
    x2 = rnd(8, 4096, seed=7).cuda()
    x, r = c["x"][:B].cuda(), c["r"][:B].cuda()
    runs = [lambda x_, r_: ctx.gemv_w8(c["q"], c["s"], x_),
            lambda x_, r_: ctx.gemv_w8(c["q"], c["s"], x_, resid=r_, epi=RESID),
            lambda x_, r_: ctx.gemv_w8(gq, gs, x_, epi=SWIGLU, rms_w=w)]
    for i, run in enumerate(runs):
        xs = x2[:B] if i == 2 else x
        full = run(xs, r)
        for b in range(B):
            assert torch.equal(run(xs[b:b + 1], r[b:b + 1])[0], full[b]), (B, b, i)


def test_gemv_w8_row_scales_and_zero_rows(ctx):
    """rows scaled over 2^-20 .. 2^6: the scale meets the sum once, in fp32.  An all-zero row gives exact zeros, and zeros + the residual."""
    N, K, B = 54, 1024, 3
    W = rnd(N, K, seed=2).float() * (2.0 ** (torch.arange(N) % 27 - 20).float())[:, None]
    W[7] = 0
    W[53] = 0
    q, s, deq = _quant(ctx, W.to(BF))
    assert float(s.max() / s[s > 0].min()) >= 2.0 ** 24 and float(s[7]) == 1.0
    x, r = rnd(B, K, seed=1), rnd(B, N, seed=4)
    lin = F.linear(x.float(), deq.float()).to(BF)                  # (fp32 reference rounded once: rows 2^-20 small must not lose bits)
    out = ctx.gemv_w8(q, s, x.cuda()).cpu()
    assert_bf16_close(out / s.cpu()[None, :].to(BF), lin / s.cpu()[None, :].to(BF), "gemv_w8 scaled rows")   # per-column scale: exact powers of two
    assert not bool(out[:, 7].any()) and not bool(out[:, 53].any())
    out = ctx.gemv_w8(q, s, x.cuda(), resid=r.cuda(), epi=RESID).cpu()
    assert torch.equal(out[:, 7], r[:, 7]) and torch.equal(out[:, 53], r[:, 53])


# ---------------------------------------------------------------------------------------------------------------- the step
PROJ = ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj")
_engines = {}


def _geo(ctx, name):
    """(kw, sd_deq, engine built from sd_deq) of a geometry, once per session: every projection matrix of the state dict is put on the e4m3
    grid first, so the engine's bf16 weights equal its e4m3 copies"""
    if name not in _engines:
        from procyon_amd import synth
        from procyon_amd.engine import LlamaConfig, LlamaEngine
        kw = GEOMS[name]
        sd = dict(synth.llama_state_dict(**kw))
        for k in list(sd):
            if k.endswith(".weight") and k.split(".")[-2] in PROJ:
                sd[k] = _quant(ctx, sd[k].to(BF))[2]
        eng = LlamaEngine(sd, LlamaConfig(**kw, max_pos=512))
        eng._ensure_fp8_copies()
        for (q, s), w in zip(eng._keep8[0], eng._keep[0][:4]):         # value-idempotent: the copies dequantise to the bf16 weights
            assert torch.equal((q.view(torch.float8_e4m3fn).float() * s[:, None]).to(BF), w), name
        assert not bool(eng.desc.layers_fp8)                            # the prefill stays bf16
        _engines[name] = (kw, sd, eng)
    return _engines[name]


def _batch(B, T, d, seed):
    """embeddings [B, T, d] + a ragged mask [B, T]; from 3 rows on the last row is a copy of row 1"""
    g = torch.Generator().manual_seed(seed)
    emb = (torch.randn(B, T, d, generator=g) * 0.02).to(BF)
    mask = torch.ones(B, T)
    for b in range(B):
        mask[b, :(b * 7 + 3) % 11 if b % 3 != 2 else 0] = 0
    if B >= 3:
        emb[B - 1], mask[B - 1] = emb[1], mask[1]
    return emb, mask


def _open(eng, V, emb, mask, keep_logits=False):
    """prefill with the clean decode mask and the first pick -> cache, state"""
    from procyon_amd.engine import GenState
    n, T = mask.shape
    Tmax = T + N_STEPS + 2
    cache = eng.new_cache(n, Tmax)
    keep = torch.ones(n, Tmax, dtype=torch.uint8, device="cuda")
    keep[:, :T] = mask.to("cuda", torch.uint8)
    st = GenState(n, V, N_STEPS + 2, "cuda", keep_logits, keep)
    logits, _ = eng.prefill(emb.cuda(), mask, cache, "last")
    st.logits.copy_(logits); st.pos.fill_(T)
    eng.pick(cache, st, n, advance_pos=False)
    return cache, st, logits


def _result(cache, st, lg, T):
    return dict(logits=torch.stack(lg), tokens=st.tokens_out[:, :N_STEPS + 1].clone(), logprob=st.logprob.clone(),
                k=cache.k[:, :, :, T:T + N_STEPS].clone(), v=cache.v[:, :, :, T:T + N_STEPS].clone())


def _decode(eng, V, emb, mask, step, forced=None, alone=None):
    """prefill + N_STEPS greedy cached steps, one `step` + pick each -> dict of device tensors: logits [N_STEPS + 1, n, V], tokens
    [n, N_STEPS + 1], logprob [n], the appended K / V slots.  forced [n, N_STEPS + 1]: cached step s (from 0) is fed forced[:, s].
    alone = r: the batch is prefilled as a whole (the prefill's tiles depend on the row count), then row r's cache, mask and state move to a
    one-row cache and the cached steps run on that row alone (n = 1 in the result)."""
    from procyon_amd.engine import GenState
    n, T = mask.shape
    cache, st, logits = _open(eng, V, emb, mask)
    if alone is not None:
        r = alone
        one = eng.new_cache(1, cache.k.shape[3])
        one.k.copy_(cache.k[:, r:r + 1]); one.v.copy_(cache.v[:, r:r + 1])
        st1 = GenState(1, V, N_STEPS + 2, "cuda", False, st.keep[r:r + 1].clone())
        for name in ("pos", "step"):
            getattr(st1, name).copy_(getattr(st, name))
        for name in ("next_tok", "tokens_out", "logprob", "logits"):
            getattr(st1, name).copy_(getattr(st, name)[r:r + 1])
        eng.ctx.sync()
        cache, st, logits, n = one, st1, logits[r:r + 1], 1
    lg = [logits]
    for s_ in range(N_STEPS):
        if forced is not None:
            st.next_tok.copy_(forced[:, s_].to(torch.int32))
        step(cache, st, n)
        eng.pick(cache, st, n, advance_pos=True)
        lg.append(st.logits.clone())
    eng.ctx.sync()
    return _result(cache, st, lg, T)


def _greedy_w8(eng, V, emb, mask, use_graph):
    """the same steps through greedy_steps_w8, with the logits record"""
    n, T = mask.shape
    cache, st, logits = _open(eng, V, emb, mask, keep_logits=True)
    eng.greedy_steps_w8(cache, st, n, N_STEPS, use_graph)
    eng.ctx.sync()
    out = _result(cache, st, [logits] + [st.logits_all[s_].cuda() for s_ in range(1, N_STEPS + 1)], T)
    out["record"] = st.logits_all[:N_STEPS + 1].clone()
    return out


def _cpu(out, rows=None):
    sel = (lambda t, dim: t.cpu()) if rows is None else (lambda t, dim: t.index_select(dim, torch.tensor(rows, device=t.device)).cpu())
    return dict(logits=sel(out["logits"], 1), tokens=sel(out["tokens"], 0), logprob=sel(out["logprob"], 0), k=sel(out["k"], 1), v=sel(out["v"], 1))


@pytest.mark.parametrize("T", [21, 30])
@pytest.mark.parametrize("B", [1, 3, 4, 5, 8])
@pytest.mark.parametrize("name", list(GEOMS))
def test_decode_w8_step_vs_oracle_and_identities(ctx, monkeypatch, name, B, T):
    """B ragged rows, N_STEPS greedy steps on the new entry (T = 30: the appended slots 30..32 cross a 32-key block): (a) it ran -- its counter
    rises by the number of steps while the default step's dispatch counters stand still; (b) every row against the bf16 oracle on sd_deq;
    (c) the copy of row 1 bit-equal to its original, and row 1 run ALONE bit-equal to row 1 of the batch; (d) the call repeated gives the same
    bits; (e) the default bf16 step of the same engine, fed the same tokens, within check_oracle's 2e-2; (f) greedy_steps_w8 as a replayed
    graph and as an eager loop give the bits of (a) in tokens, log-probs, logits record and appended K / V."""
    kw, sd, eng = _geo(ctx, name)
    V = kw["vocab"]
    pcy_disable(monkeypatch)
    emb, mask = _batch(B, T, kw["d"], seed=B * 100 + T)
    n0, d0 = _count(), decode_counts()
    out = _decode(eng, V, emb, mask, eng.decode_w8)
    assert _count() - n0 == N_STEPS and decode_counts() == d0
    assert torch.isfinite(out["logits"].float()).all()
    rows = list(range(B))
    worst = check_oracle(sd, kw, emb, mask, _cpu(out), rows, ("decode_w8", name, B, T), N_STEPS)
    got = _cpu(out)
    if B >= 3:
        for key in got:
            dim = 1 if key in ("logits", "k", "v") else 0
            assert torch.equal(got[key].select(dim, B - 1), got[key].select(dim, 1)), (name, B, "copy", key)
    if B >= 2:
        alone = _cpu(_decode(eng, V, emb, mask, eng.decode_w8, alone=1))
        for key in got:
            dim = 1 if key in ("logits", "k", "v") else 0
            assert torch.equal(alone[key].select(dim, 0), got[key].select(dim, 1)), (name, B, "row 1 alone", key)
    again = _decode(eng, V, emb, mask, eng.decode_w8)
    for key in out:
        assert torch.equal(out[key], again[key]), (name, B, "repeat", key)
    twin = _decode(eng, V, emb, mask, eng.decode, forced=out["tokens"])
    err = max(rel_err(out["logits"][s_, b], twin["logits"][s_, b]) for s_ in range(N_STEPS + 1) for b in range(B))
    print(f"decode_w8 {name} B={B} T={T}: worst rel. err vs the oracle {worst:.3e}, vs the default bf16 step of the same engine {err:.3e}")
    assert err < 2e-2, (name, B, T, err)
    n1, d1 = _count(), decode_counts()
    eager, graph = _greedy_w8(eng, V, emb, mask, False), _greedy_w8(eng, V, emb, mask, True)
    assert N_STEPS <= _count() - n1 <= N_STEPS + 1 and decode_counts() == d1      # (eager: one count per step; graph: the capture alone)
    for key in eager:
        assert torch.equal(eager[key], graph[key]), (name, B, "graph vs eager", key)
    for key in out:
        assert torch.equal(out[key], eager[key]), (name, B, "greedy_steps_w8 vs decode_w8 + pick", key)


def test_generate_sampling_decode_w8_is_decode_w8_plus_sample_pick(ctx, monkeypatch):
    """generate_sampling(decode_w8=True) with injected uniform variates == a manual loop of decode_w8 + sample_pick"""
    kw, sd, eng = _geo(ctx, "small")
    pcy_disable(monkeypatch)
    B, T, L_, temp = 3, 13, 5, 0.7
    emb, mask = _batch(B, T, kw["d"], seed=77)
    u = torch.rand(L_ * B, generator=torch.Generator().manual_seed(5))
    n0, d0 = _count(), decode_counts()
    tok, lp, lg, _ = eng.generate_sampling(emb.cuda(), mask, L_, temperature=temp, nucleus_prob=None, keep_logits=True, uniforms=u, decode_w8=True)
    assert _count() - n0 == L_ - 1 and decode_counts() == d0
    tok, lp, lg = tok.clone(), lp.clone(), lg.clone()
    ud = u.cuda()
    cache, st = eng._prefill_for_generation(emb.cuda(), mask, L_, True)
    eng.sample_pick(cache, st, B, False, ud, temp, None)
    for _ in range(L_ - 1):
        eng.decode_w8(cache, st, B)
        eng.sample_pick(cache, st, B, True, ud, temp, None)
    eng.ctx.sync()
    assert torch.equal(tok, st.tokens_out.long()) and torch.equal(lp, st.logprob) and torch.equal(lg, st.logits_all.transpose(0, 1))
    assert torch.isfinite(lg.float()).all()


def test_generate_greedy_decode_w8_small_model(small):
    """`generate(method="greedy", decode_w8=True)` on the small synthetic model: the new step ran, and tokens, log-probs, logits and texts
    have the shapes of the default call (the tokens are those of the e4m3-rounded model: not compared)."""
    m = small["model"]
    instr, slots = _prompts(5, seed=23)
    L_ = 6
    ref = m.generate(_gen_inputs(small, instr, slots), max_len=L_, method="greedy")
    n0, d0 = _count(), decode_counts()
    got = m.generate(_gen_inputs(small, instr, slots), max_len=L_, method="greedy", decode_w8=True)
    assert _count() - n0 >= 1 and decode_counts() == d0              # (a replayed graph: only its capture counts)
    for a, b in zip(got[:3], ref[:3]):
        assert a.shape == b.shape and a.dtype == b.dtype
    assert got[0].shape == (5, 1, L_) and torch.isfinite(got[2].float()).all()
    assert len(got[3]) == len(ref[3]) == 5
    assert not bool(m.text_encoder.engine.desc.layers_fp8)           # the prefill is still what set_fp8 says


def test_decode_w8_argument_errors_launch_nothing(ctx, monkeypatch):
    """B = 9, a shared-prefix cache, w8 NULL, and K = 24 on the operator: each returns non-zero, leaves the counter where it was and a poisoned
    output buffer untouched."""
    import ctypes as C
    from procyon_amd import _lib as L
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import GenState
    kw, sd, eng = _geo(ctx, "small")
    pcy_disable(monkeypatch)
    T, V = 10, kw["vocab"]
    emb, mask = _batch(12, T, kw["d"], seed=9)
    cache = eng.new_cache(12, T + 4)
    eng.prefill(emb.cuda(), None, cache, "last")
    st = GenState(12, V, 4, "cuda")
    st.pos.fill_(T)
    st.logits.fill_(1.0)
    prefix = eng.new_cache(3, T)
    eng.prefill(emb[:3].cuda(), None, prefix, "last")
    shared = eng.new_shared_cache(prefix, 2, 4)
    eng.ctx.sync()

    def refused(call, c, match):
        k0, v0, n0, d0 = c.k.clone(), c.v.clone(), _count(), decode_counts()
        with pytest.raises(PcyError, match=match):
            call()
        eng.ctx.sync()
        assert _count() == n0 and decode_counts() == d0
        assert torch.equal(c.k, k0) and torch.equal(c.v, v0) and bool((st.logits == 1.0).all())

    refused(lambda: eng.decode_w8(cache, st, 9), cache, "outside")
    refused(lambda: eng.greedy_steps_w8(cache, st, 9, 2), cache, "outside")
    refused(lambda: eng.decode_w8(shared, st, 6), shared, "shared-prefix")
    null = C.POINTER(L.LlamaLayerFp8)()
    refused(lambda: L.check(ctx.lib.pcy_llama_decode_w8(ctx.h, C.byref(eng.desc), null, C.byref(cache.c), C.byref(st.c), 4), "pcy_llama_decode_w8"),
            cache, "w8 is NULL")
    refused(lambda: L.check(ctx.lib.pcy_llama_greedy_w8(ctx.h, C.byref(eng.desc), null, C.byref(cache.c), C.byref(st.c), 4, 2, 1), "pcy_llama_greedy_w8"),
            cache, "w8 is NULL")
    # the operator: K = 24 is no multiple of 16; 9 rows; an epilogue it does not have
    q, s = torch.zeros(32, 48, dtype=torch.uint8, device="cuda"), torch.ones(32, device="cuda")
    y = torch.full((9, 32), 3.0, dtype=BF, device="cuda")
    for K_, B_, epi, match in ((24, 2, STORE, "multiple of 16"), (48, 9, STORE, "outside"), (48, 2, 2, "epi")):
        n0 = _count()
        with pytest.raises(PcyError, match=match):
            ctx.gemv_w8(q[:, :K_].contiguous(), s, torch.ones(B_, K_, dtype=BF, device="cuda"), epi=epi, out=y)
        eng.ctx.sync()
        assert _count() == n0 and bool((y == 3.0).all())
    n0 = _count()
    eng.decode_w8(cache, st, 8)            # ... and a call inside the contract is served
    eng.ctx.sync()
    assert _count() == n0 + 1 and torch.isfinite(st.logits[:8].float()).all()
