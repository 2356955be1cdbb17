"""GPU: the lookahead pass on the decode loop -- the window attention (pcy_attn_window), the step (pcy_llama_decode_window /
LlamaEngine.decode_window), `generate_lookahead(step="window")` and `generate(lookahead_step="window")`.

Operator: against the oracle's eager formulas (LR.apply_rope, softmax(dtype=float32).to(bf16), the causal mask over the window: the reference
tests/test_gpu_extend.py builds for pcy_attn_extend) with the bars of tests/test_gpu_kernels.py::test_attn_decode unchanged (rel_err < 1e-3,
assert_bf16_close(max_frac=0.03, inter=0.05)); the appended K / V, the untouched slots, row independence, capacity independence and the
out-of-range positions bit for bit.
Engine: tests/test_gpu_lookahead.py with step="window" -- draft independence bit for bit at windows 4, 2 (streaming projections) and 5, at the
Llama-3-8B and Llama-2-7B widths; the record against the teacher-forced oracle under the bar that file computes; against plain greedy and
against step="extend" under its margin rule."""
import math

import pytest
import torch
import torch.nn.functional as F

from conftest import assert_bf16_close, record_parity, rel_err
from select_oracle import first_argmax
from test_gpu_lookahead import INSTR, MAXLEN, SEED, SLOTS, T_, W_, _forced, _gen_inputs, _prompt_ids, env  # noqa: F401  (env: the module fixture)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
N_LAYERS, LAYER = 2, 1      # the cache has two layers and the call names the second: the layer stride is part of the address


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF)


def bits(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def ctx():
    from procyon_amd.engine import Context
    return Context.get()


# ---------------------------------------------------------------------------------------------------------------- the operator
#          H  Hkv  dh   pos   W        ("C": the library's chunk length)
SHAPES = [(32, 8, 128, 37, 4),         # one query tile; a past that is no multiple of 32
          (32, 8, 128, 30, 5),         # the window crosses a 32-key block inside the first chunk
          (32, 8, 128, 636, 8),        # several chunks; the window crosses a block; two query tiles
          (32, 32, 128, 45, 4),        # G = 1
          (4, 2, 64, 5, 2),            # dh 64, W = 2
          (8, 1, 128, 0, 3),           # empty past, G = 8
          (32, 8, 128, 1030, 32),      # a long past, 128 queries
          (8, 2, 64, "C-1", 4),        # a past that ends one key short of a chunk boundary
          (8, 2, 64, "C", 4)]          # a past that ends exactly on a chunk boundary


def _pos(ctx, pos):
    c = ctx.attn_window_chunk()
    return {"C-1": c - 1, "C": c}.get(pos, pos)


def _cfg(H, Hkv, dh):
    from procyon_amd.engine import LlamaConfig
    return LlamaConfig(vocab=16, d=H * dh, n_layers=N_LAYERS, n_heads=H, n_kv_heads=Hkv, ffn=64)


def _cache(H, Hkv, dh, Tmax, k_past, v_past):
    """a one-row plain cache, NaN everywhere (both layers), then k_past / v_past [Hkv, pos, dh] in slots [0, pos) of LAYER"""
    from procyon_amd.engine import KVCache
    cache = KVCache(_cfg(H, Hkv, dh), 1, Tmax, "cuda")
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    t = k_past.shape[1]
    if t:
        cache.k[LAYER, 0, :, :t] = k_past.cuda()
        cache.v[LAYER, 0, :, :t] = v_past.cuda()
    return cache


_REF = {}


def _case(H, Hkv, dh, pos, W):
    """inputs and the oracle's result of a shape, computed once and shared: qkv [W, .], the past, o_ref [W, H*dh], the roped k and v [Hkv, W, dh]"""
    key = (H, Hkv, dh, pos, W)
    if key in _REF:
        return _REF[key]
    from oracle import llama_ref as LR
    from procyon_amd.engine import rope_tables
    qkv = rnd(W, (H + 2 * Hkv) * dh, seed=1)
    k_past, v_past = rnd(Hkv, pos, dh, seed=11), rnd(Hkv, pos, dh, seed=12)
    cos, sin = rope_tables(dh, 10000.0, pos + W, "cpu")
    q = qkv[:, :H * dh].view(1, W, H, dh).transpose(1, 2)
    k = qkv[:, H * dh:(H + Hkv) * dh].view(1, W, Hkv, dh).transpose(1, 2)
    v = qkv[:, (H + Hkv) * dh:].view(1, W, Hkv, dh).transpose(1, 2)
    q, k = LR.apply_rope(q, k, cos[pos:pos + W][None], sin[pos:pos + W][None])
    kk, vv = torch.cat([k_past[None], k], 2), torch.cat([v_past[None], v], 2)
    g = H // Hkv
    ke = kk[:, :, None].expand(1, Hkv, g, pos + W, dh).reshape(1, H, pos + W, dh)
    ve = vv[:, :, None].expand(1, Hkv, g, pos + W, dh).reshape(1, H, pos + W, dh)
    sc = torch.matmul(q, ke.transpose(2, 3)) * (dh ** -0.5)
    sc = sc + LR.build_additive_mask(None, 1, W, pos, BF)
    p = F.softmax(sc, dim=-1, dtype=torch.float32).to(BF)
    o = torch.matmul(p, ve).transpose(1, 2).contiguous().reshape(W, H * dh)
    _REF[key] = dict(qkv=qkv, k_past=k_past, v_past=v_past, o=o, k_new=k[0].contiguous(), v_new=v[0].contiguous())
    return _REF[key]


def _call(ctx, cache, qkv, pos, H, Hkv, dh, out=None):
    from procyon_amd.engine import rope_tables
    cos, sin = rope_tables(dh, 10000.0, max(cache.Tmax, 1) + 8, "cuda")
    pos_d = torch.tensor([pos], dtype=torch.int32, device="cuda")
    return ctx.attn_window(qkv.cuda(), cache, LAYER, pos_d, cos, sin, H, Hkv, dh, out=out).cpu()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"H{s[0]}kv{s[1]}dh{s[2]}-pos{s[3]}-W{s[4]}")
def test_operator_against_the_oracle(ctx, shape):
    H, Hkv, dh, pos, W = shape
    pos = _pos(ctx, pos)
    c = _case(H, Hkv, dh, pos, W)
    cache = _cache(H, Hkv, dh, pos + W + 3, c["k_past"], c["v_past"])          # (slots >= pos + W hold NaN)
    k0, v0 = bits(cache.k).clone(), bits(cache.v).clone()
    qkv_d = c["qkv"].cuda()
    out = _call(ctx, cache, qkv_d, pos, H, Hkv, dh)
    assert torch.equal(qkv_d.cpu(), c["qkv"]), "qkv is read only"
    assert not bool(torch.isnan(out.float()).any()), "NaN of the slots from pos + W on reached o"
    err = rel_err(out, c["o"])
    frac = (out != c["o"]).float().mean().item()
    print(f"attn_window {shape} pos {pos}: rel_err {err:.3e}, {frac:.4f} of elements differ")
    record_parity(f"look_window/op_H{H}kv{Hkv}dh{dh}_pos{shape[3]}_W{W}", rel_err=err, frac_differ=frac)
    assert err < 1e-3
    assert_bf16_close(out, c["o"], "attn_window", max_frac=0.03, inter=torch.full_like(c["o"], 0.05))
    # the appended K / V: the oracle's roped key and the V, bit for bit; every other slot of both layers untouched
    assert torch.equal(cache.k[LAYER, 0, :, pos:pos + W].cpu(), c["k_new"]) and torch.equal(cache.v[LAYER, 0, :, pos:pos + W].cpu(), c["v_new"])
    k1, v1 = bits(cache.k).clone(), bits(cache.v).clone()
    for a, b in ((k0, k1), (v0, v1)):
        same = a == b
        same[LAYER, 0, :, pos:pos + W] = True
        assert bool(same.all()), "a slot outside [pos, pos + W) of the named layer was written"
    # a repeated call: equal bits, in o and in the cache
    assert torch.equal(_call(ctx, cache, qkv_d, pos, H, Hkv, dh), out)
    assert torch.equal(bits(cache.k), k1) and torch.equal(bits(cache.v), v1)


@pytest.mark.parametrize("shape", [(32, 8, 128, 37, 4), (32, 8, 128, 636, 8), (4, 2, 64, 5, 2), (32, 32, 128, 45, 4)],
                         ids=lambda s: f"H{s[0]}kv{s[1]}dh{s[2]}-pos{s[3]}-W{s[4]}")
def test_operator_row_independence(ctx, shape):
    """rows > i of qkv replaced by other values and by NaN: rows <= i of o and their appended slots keep their bits (i = 0 and W - 2)"""
    H, Hkv, dh, pos, W = shape
    c = _case(H, Hkv, dh, pos, W)
    cache = _cache(H, Hkv, dh, pos + W + 3, c["k_past"], c["v_past"])
    out = _call(ctx, cache, c["qkv"], pos, H, Hkv, dh)
    k1, v1 = cache.k[LAYER, 0].cpu(), cache.v[LAYER, 0].cpu()
    other = rnd(*c["qkv"].shape, seed=99)
    for i in sorted({0, W - 2}):
        for fill in ("other", "nan"):
            q2 = c["qkv"].clone()
            q2[i + 1:] = other[i + 1:] if fill == "other" else float("nan")
            cache2 = _cache(H, Hkv, dh, pos + W + 3, c["k_past"], c["v_past"])
            out2 = _call(ctx, cache2, q2, pos, H, Hkv, dh)
            assert torch.equal(out2[:i + 1], out[:i + 1]), (shape, i, fill)
            assert torch.equal(cache2.k[LAYER, 0, :, :pos + i + 1].cpu(), k1[:, :pos + i + 1]), (shape, i, fill)
            assert torch.equal(cache2.v[LAYER, 0, :, :pos + i + 1].cpu(), v1[:, :pos + i + 1]), (shape, i, fill)


def test_operator_capacity_independence(ctx):
    """the same contents in caches of Tmax = pos + W and pos + W + 517: equal bits (the grid grows with the capacity, the live chunks do not)"""
    H, Hkv, dh, pos, W = 32, 8, 128, 636, 8
    c = _case(H, Hkv, dh, pos, W)
    outs = []
    for extra in (0, 517):
        cache = _cache(H, Hkv, dh, pos + W + extra, c["k_past"], c["v_past"])
        outs.append(_call(ctx, cache, c["qkv"], pos, H, Hkv, dh))
        assert torch.equal(cache.k[LAYER, 0, :, pos:pos + W].cpu(), c["k_new"])
    assert torch.equal(outs[0], outs[1])


def test_operator_position_outside_the_cache_writes_nothing(ctx):
    H, Hkv, dh, pos, W = 8, 2, 64, 37, 4
    c = _case(H, Hkv, dh, pos, W)
    Tmax = pos + W + 3
    for bad in (Tmax - W + 1, Tmax, -1, -W):
        cache = _cache(H, Hkv, dh, Tmax, c["k_past"], c["v_past"])
        k0, v0 = bits(cache.k).clone(), bits(cache.v).clone()
        o = torch.full((W, H * dh), 7.0, dtype=BF, device="cuda")
        _call(ctx, cache, c["qkv"], bad, H, Hkv, dh, out=o)
        assert torch.equal(bits(cache.k), k0) and torch.equal(bits(cache.v), v0), bad
        assert bool((o == 7.0).all()), bad
    cache = _cache(H, Hkv, dh, Tmax, c["k_past"], c["v_past"])                 # the last position that fits does write
    _call(ctx, cache, c["qkv"], Tmax - W, H, Hkv, dh)
    assert not bool(torch.isnan(cache.k[LAYER, 0, :, Tmax - W:].float()).any())


def test_operator_argument_errors_launch_nothing(ctx):
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import KVCache, rope_tables
    H, Hkv, dh, pos, W = 8, 2, 64, 5, 4
    cos, sin = rope_tables(dh, 10000.0, 128, "cuda")
    pos_d = torch.tensor([pos], dtype=torch.int32, device="cuda")
    qkv = rnd(W, (H + 2 * Hkv) * dh, seed=1).cuda()
    cfg = _cfg(H, Hkv, dh)
    prefix = KVCache(cfg, 1, 8, "cuda")
    two = KVCache(cfg, 2, 64, "cuda")
    one = KVCache(cfg, 1, 64, "cuda")
    shared = KVCache(cfg, 1, 64, "cuda", prefix=prefix, rows_per_prefix=1)
    grouped = KVCache.grouped(cfg, "cuda", prefix, [1], [8], 64)
    o = torch.full((W, H * dh), 7.0, dtype=BF, device="cuda")

    def refused(match, cache, q=qkv, h=H, hkv=Hkv, d=dh, out=None):
        out = o if out is None else out
        with pytest.raises(PcyError, match=match):
            ctx.attn_window(q, cache, LAYER, pos_d, cos, sin, h, hkv, d, out=out)
        for c_ in (one, two, shared, prefix):
            assert not bool(c_.k.any()) and not bool(c_.v.any())
        assert bool((o == 7.0).all())

    refused("shared-prefix or grouped", shared)
    refused("shared-prefix or grouped", grouped)
    refused("kv->B == 1", two)
    refused("outside \\[2, 32\\]", one, q=qkv[:1], out=o[:1])
    refused("outside \\[2, 32\\]", one, q=rnd(33, qkv.shape[1], seed=2).cuda(), out=torch.full((33, H * dh), 7.0, dtype=BF, device="cuda"))
    refused("head_dim", one, q=rnd(W, 12 * 32, seed=3).cuda(), h=8, hkv=2, d=32)
    refused("H/Hkv", one, q=rnd(W, 18 * 64, seed=4).cuda(), h=16, hkv=1, d=64, out=torch.full((W, 16 * 64), 7.0, dtype=BF, device="cuda"))
    refused("H/Hkv", one, q=rnd(W, 10 * 64, seed=4).cuda(), h=6, hkv=2, d=64, out=torch.full((W, 6 * 64), 7.0, dtype=BF, device="cuda"))
    refused("fewer than", KVCache(cfg, 1, 3, "cuda"))


# ---------------------------------------------------------------------------------------------------------------- the engine
def _run(eng, emb, ids, W, forced, max_len=MAXLEN, step="window"):
    """tests/test_gpu_lookahead.py::_run with `step`, and the window-step counter beside the lookahead ones"""
    lib = eng.ctx.lib
    n0 = [lib.pcy_debug_look_count(0), lib.pcy_debug_look_count(1), lib.pcy_debug_decode_window_count()]
    tok, lp, lg, (st, cache, look) = eng.generate_lookahead(emb.cuda(), ids, max_len, W, forced=forced, keep_logits=True, step=step)
    T = ids.numel()
    n1 = [lib.pcy_debug_look_count(0), lib.pcy_debug_look_count(1), lib.pcy_debug_decode_window_count()]
    return dict(tokens=tok.cpu()[0], logprob=lp.cpu().clone(), logits=lg[0].clone(), pos=int(st.pos), step=int(st.step),
                k=cache.k[:, :, :, :T + max_len - 1].cpu(), v=cache.v[:, :, :, :T + max_len - 1].cpu(), stats=look.stats(),
                hist=look.hist.cpu(), n_hist=int(look.n_hist), calls=[b - a for a, b in zip(n0, n1)])


def _abcd(eng, emb, ids, W, vocab, with_cd=True, max_len=MAXLEN):
    """D: prompt lookup; A: every draft wrong; B: every draft right; C: A's tokens with every third one wrong"""
    runs = {"D": _run(eng, emb, ids, W, None, max_len)}
    t = runs["D"]["tokens"]
    runs["A"] = _run(eng, emb, ids, W, _forced(t, vocab, 1), max_len)
    runs["B"] = _run(eng, emb, ids, W, _forced(runs["A"]["tokens"], vocab), max_len)
    if with_cd:
        runs["C"] = _run(eng, emb, ids, W, _forced(runs["A"]["tokens"], vocab, 3), max_len)
    return runs


def _assert_same_bits(runs, what):
    a = runs["A"]
    for name, r in runs.items():
        for key in ("tokens", "logprob", "logits", "k", "v", "hist"):
            assert torch.equal(a[key], r[key]), (what, name, key)
        assert (r["pos"], r["step"], r["n_hist"]) == (a["pos"], a["step"], a["n_hist"]), (what, name)
        p = r["stats"]["passes"]
        assert r["calls"] == [p, p, p], (what, name, r["calls"])       # draft, verify and the window step: once per pass each


@pytest.fixture(scope="module")
def runs(env):
    return _abcd(env["eng"], env["emb"], env["ids"], W_, env["lgeom"].vocab)


def test_draft_independence_window_4(env, runs):
    """A (every draft wrong), B (every draft right), C (every third wrong), D (prompt lookup) on step="window": tokens, log-prob, logits record,
    history and the cache slots [0, T + max_len - 1) bit-equal; the pass counts of tests/test_gpu_lookahead.py; one pcy_llama_decode_window
    call per pass.  Run A is also the test of the rejected rows: every pass leaves three slots of rejected K / V behind the new *pos, and
    its cache equals run B's, where no draft was ever rejected."""
    from procyon_amd.engine import lookahead_passes
    _assert_same_bits(runs, "window 4")
    a, ids, V = runs["A"], env["ids"].tolist(), env["lgeom"].vocab
    assert (a["pos"], a["step"], a["n_hist"]) == (T_ + MAXLEN - 1, MAXLEN, T_ + MAXLEN)
    assert a["hist"][:T_ + MAXLEN].tolist() == ids + a["tokens"].tolist()
    toks = a["tokens"]
    want = {"A": MAXLEN - 1, "B": math.ceil((MAXLEN - 1) / W_),
            "C": lookahead_passes(toks, ids, W_, (3, 1), _forced(toks, V, 3))[0], "D": lookahead_passes(toks, ids, W_, (3, 1))[0]}
    for name, r in runs.items():
        s = r["stats"]
        assert s["passes"] == want[name], (name, s)
        assert s["tokens"] == MAXLEN - 1 == sum((k + 1) * n for k, n in enumerate(s["accepted"])) and sum(s["accepted"]) == s["passes"]
    assert runs["A"]["stats"]["accepted"] == [MAXLEN - 1, 0, 0, 0]
    assert want["B"] < want["C"] < want["A"]


@pytest.mark.parametrize("W", [2, 5])
def test_draft_independence_other_windows(env, W):
    """A against B at window 2 (below the MFMA GEMVs' smallest batch: the streaming projections) and 5"""
    r = _abcd(env["eng"], env["emb"], env["ids"], W, env["lgeom"].vocab, with_cd=False)
    del r["D"]
    _assert_same_bits(r, f"window {W}")
    assert r["A"]["stats"]["passes"] == MAXLEN - 1 and r["B"]["stats"]["passes"] == math.ceil((MAXLEN - 1) / W)


@pytest.mark.parametrize("name,kw", [("llama3_8b", dict(vocab=4096, d=4096, n_layers=2, n_heads=32, n_kv_heads=8, ffn=14336)),
                                     ("llama2_7b", dict(vocab=4096, d=4096, n_layers=2, n_heads=32, n_kv_heads=32, ffn=11008))])
def test_wide_cases(name, kw):
    """the Llama-3-8B widths and the Llama-2-7B widths (another K split of the GEMVs, G = 1) with 2 layers, window 4, 12 tokens: A against B"""
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    sd = synth.llama_state_dict(**kw, device="cuda")
    eng = LlamaEngine(sd, LlamaConfig(**kw, max_pos=512))
    ids = _prompt_ids(5, 4096)
    emb = eng.embed_tokens(ids[None])
    t = _run(eng, emb, ids, 4, None, max_len=12)["tokens"]
    a = _run(eng, emb, ids, 4, _forced(t, 4096, 1), max_len=12)
    b = _run(eng, emb, ids, 4, _forced(a["tokens"], 4096), max_len=12)
    _assert_same_bits({"A": a, "B": b}, name)
    assert torch.equal(a["tokens"], t)
    assert a["stats"]["passes"] == 11 and b["stats"]["passes"] == 3


@pytest.fixture(scope="module")
def oracle(env, runs):
    """tests/test_gpu_lookahead.py's fixture on THIS file's run A: its tokens teacher-forced through the oracle, the EXISTING prefill on the same
    rows, D and the bar; the oracle's own greedy run for the margin rule"""
    from oracle import llama_ref as LR
    sd, geom, eng = env["w"]["llama"], env["lgeom"], env["eng"]
    toks = runs["A"]["tokens"]
    cat = torch.cat([env["emb"], F.embedding(toks[None, :-1], sd["model.embed_tokens.weight"])], 1)        # [1, T + max_len - 1, d]
    lg_ref = LR.llama_forward(sd, geom, inputs_embeds=cat, attn_mask=torch.ones(1, cat.shape[1]))["logits"][0, T_ - 1:]     # [max_len, V]
    n = cat.shape[1]
    own, _ = eng.prefill(cat.cuda(), None, eng.new_cache(1, n), torch.arange(T_ - 1, n, dtype=torch.int32))
    delta = float((own.cpu().float() - lg_ref.float()).abs().max())
    rows_ref = lg_ref.float()
    ce = F.cross_entropy(rows_ref, toks, reduction="none")
    l64 = torch.logsumexp(rows_ref.double(), -1)
    nll64 = l64 - rows_ref.double().gather(1, toks[:, None])[:, 0]
    err_a = float((ce.double() - nll64).abs().max())
    big = torch.maximum(l64.abs(), rows_ref.max(-1).values.double().abs()).max()
    op_bar = 8 * max(err_a, 2.0 ** (math.floor(math.log2(float(big))) - 23))
    bar = 2 * delta + 2 * 2.0 ** -7 * float(lg_ref.float().abs().max()) + op_bar
    g_tok, g_lg, _ = LR.greedy_generate(sd, geom, env["emb"], torch.ones(1, T_), MAXLEN)
    top = g_lg[0].float().topk(2, -1).values
    return dict(lg_ref=lg_ref, delta=delta, bar=bar, greedy_tokens=g_tok[0], greedy_margin=(top[:, 0] - top[:, 1]))


def test_against_the_oracle(runs, oracle):
    a = runs["A"]
    err = float((a["logits"].float() - oracle["lg_ref"].float()).abs().max())
    print(f"window-step record vs teacher-forced oracle: err {err:.3e} D {oracle['delta']:.3e} bar {oracle['bar']:.3e}")
    record_parity("look_window/vs_oracle", logits_err=err, delta=oracle["delta"], bar=oracle["bar"])
    assert err <= oracle["bar"] and oracle["bar"] < 0.5
    assert torch.equal(first_argmax(a["logits"].float()), a["tokens"])           # every committed token is the argmax of its own recorded row


def _margin_rule(tok, lg, a, what):
    """tests/test_gpu_lookahead.py::test_against_plain_greedy's rule between the run (tok, lg) and run `a`: the first differing index k is
    >= 16 (or there is none), and at k the first run's top-2 margin is below twice the largest logit difference between the two records"""
    diff = (tok != a["tokens"]).nonzero()
    k = int(diff[0]) if diff.numel() else None
    n = min(16, tok.numel()) if k is None else k + 1
    noise_all = float((lg[:n].float() - a["logits"][:n].float()).abs().max())
    print(f"{what}: first differing token {k}; largest logit difference over the rows before it {noise_all:.3e}")
    record_parity(f"look_window/{what}", first_diff=-1 if k is None else k, logits_diff=noise_all)
    if k is not None:
        assert k >= 16, k
        top = lg[k].float().topk(2).values
        noise = float((lg[k].float() - a["logits"][k].float()).abs().max())
        assert float(top[0] - top[1]) < 2 * noise, (k, float(top[0] - top[1]), noise)


def test_against_plain_greedy(env, runs, oracle):
    eng = env["eng"]
    m16 = float(oracle["greedy_margin"][:16].min())
    assert m16 >= 4 * oracle["delta"], (m16, oracle["delta"])
    tok, _, lg, _ = eng.generate_greedy(env["emb"].cuda(), torch.ones(1, T_), MAXLEN, keep_logits=True)
    _margin_rule(tok.cpu()[0], lg[0].clone(), runs["A"], "vs_plain_greedy")


def test_window_against_extend(env, runs, oracle):
    """the two passes are different arithmetic: the same margin rule between their records, no equal bits asserted"""
    assert float(oracle["greedy_margin"][:16].min()) >= 4 * oracle["delta"]
    e = _run(env["eng"], env["emb"], env["ids"], W_, _forced(runs["A"]["tokens"], env["lgeom"].vocab, 1), step="extend")
    assert e["calls"][2] == 0 and e["stats"]["passes"] >= 1                      # step="extend" never enters the window step
    _margin_rule(e["tokens"], e["logits"], runs["A"], "vs_extend")


def test_step_argument_errors(env):
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import GenState
    eng, emb, ids = env["eng"], env["emb"].cuda(), env["ids"]
    lib = eng.ctx.lib
    n0 = lib.pcy_debug_decode_window_count()
    with pytest.raises(ValueError, match="step="):
        eng.generate_lookahead(emb, ids, MAXLEN, W_, step="decode")
    V, d = eng.cfg.vocab, eng.cfg.d
    logits = torch.empty(W_, V, dtype=BF, device="cuda")
    x = emb[0, :W_].contiguous()
    cache = eng.new_cache(1, 64)
    st = GenState(1, V, 8, "cuda")
    st.pos.fill_(5)
    keep = torch.ones(1, 64, dtype=torch.uint8, device="cuda")
    with pytest.raises(PcyError, match="keep mask"):
        eng.decode_window(cache, GenState(1, V, 8, "cuda", False, keep), x, logits)
    with pytest.raises(PcyError, match="kv->B == 1"):
        eng.decode_window(eng.new_cache(2, 64), st, x, logits)
    with pytest.raises(PcyError, match="outside \\[2, 32\\]"):
        eng.decode_window(cache, st, x[:1], logits[:1])
    with pytest.raises(PcyError, match="fewer than"):
        eng.decode_window(eng.new_cache(1, 3), st, x, logits)
    assert not bool(cache.k.any()) and lib.pcy_debug_decode_window_count() == n0


def test_step_refuses_fp8_layers():
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    kw = dict(vocab=320, d=256, n_layers=1, n_heads=4, n_kv_heads=2, ffn=512)
    eng = LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, max_pos=128), fp8_prefill=True)
    ids = torch.arange(5)
    with pytest.raises(ValueError, match="fp8"):
        eng.generate_lookahead(eng.embed_tokens(ids[None]), ids, 4, 2, step="window")
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import GenState
    with pytest.raises(PcyError, match="fp8"):
        eng.decode_window(eng.new_cache(1, 32), GenState(1, 320, 4, "cuda"), eng.embed_tokens(ids[None])[0, :2].contiguous(),
                          torch.empty(2, 320, dtype=BF, device="cuda"))
    eng.set_fp8(False)
    assert eng.generate_lookahead(eng.embed_tokens(ids[None]), ids, 4, 2, step="window")[0].shape == (1, 4)


def test_generate_with_lookahead_step_window(env):
    """generate(lookahead=4, lookahead_step="window"): the tokens of `generate_lookahead(step="window")` called directly on the same prompt, the
    return shapes of the default step, "step": "window" in the internals; without lookahead_step the call is the parent's, bit for bit"""
    m, eng = env["model"], env["eng"]
    lib = eng.ctx.lib
    n0, w0 = lib.pcy_debug_look_count(1), lib.pcy_debug_decode_window_count()
    out = m.generate(_gen_inputs(env, INSTR, SLOTS), max_len=MAXLEN, method="greedy", lookahead=4, lookahead_step="window", return_all_internals=True)
    passes = lib.pcy_debug_look_count(1) - n0
    s = out["lookahead"]
    assert s["step"] == "window" and s["passes"] == passes == lib.pcy_debug_decode_window_count() - w0
    assert s["tokens"] == MAXLEN - 1 == sum((k + 1) * n for k, n in enumerate(s["accepted"])) and len(s["accepted"]) == 4
    assert out["out_tokens"].shape == (1, 1, MAXLEN) and out["out_logits"].shape == (1, 1, MAXLEN, eng.cfg.vocab) and out["out_log_probs"].shape == (1, 1)
    emb, ids, _, _, _, _ = m._preprocessing(_gen_inputs(env, INSTR, SLOTS), aaseq_type="protein", crop_off=True, no_pad=True, left_pad=True)
    hist = ids[0].clone()
    hist[hist == m.prot_replacement_idx] = -1
    tok, lp, lg, _ = eng.generate_lookahead(emb, hist, MAXLEN, 4, keep_logits=True, step="window")
    assert torch.equal(out["out_tokens"][0, 0], tok.cpu()[0]) and torch.equal(out["out_log_probs"][0], lp.cpu()) and torch.equal(out["out_logits"][0, 0], lg[0])
    tup = m.generate(_gen_inputs(env, INSTR, SLOTS), max_len=MAXLEN, method="greedy", lookahead=4, lookahead_step="window")
    assert torch.equal(tup[0], out["out_tokens"]) and torch.equal(tup[2], out["out_logits"]) and tup[3] == out["text"]
    # the default is the extension, and naming it changes nothing
    w1 = lib.pcy_debug_decode_window_count()
    p0 = m.generate(_gen_inputs(env, INSTR, SLOTS), max_len=MAXLEN, method="greedy", lookahead=4, return_all_internals=True)
    p1 = m.generate(_gen_inputs(env, INSTR, SLOTS), max_len=MAXLEN, method="greedy", lookahead=4, lookahead_step="extend", return_all_internals=True)
    assert lib.pcy_debug_decode_window_count() == w1
    for key in ("out_tokens", "out_logits", "out_log_probs"):
        assert torch.equal(p0[key], p1[key]), key
    assert p0["text"] == p1["text"] and p0["lookahead"] == p1["lookahead"]


def test_generate_lookahead_step_refusals(env):
    m = env["model"]
    with pytest.raises(ValueError, match="lookahead_step"):
        m.generate(_gen_inputs(env, INSTR, SLOTS), max_len=4, method="greedy", lookahead=4, lookahead_step="decode")
    with pytest.raises(ValueError, match="lookahead_step"):
        m.generate(_gen_inputs(env, INSTR, SLOTS), max_len=4, method="greedy", lookahead_step="window")
    for kw in (dict(method="sampling"), dict(method="beam")):
        with pytest.raises(ValueError):
            m.generate(_gen_inputs(env, INSTR, SLOTS), max_len=4, lookahead=4, lookahead_step="window", **kw)
    with pytest.raises(ValueError):
        m.generate(_gen_inputs(env, INSTR * 2, SLOTS * 2), max_len=4, method="greedy", lookahead=4, lookahead_step="window")
