"""GPU: extending a filled KV cache by S tokens per row -- the attention operator (pcy_attn_extend), the engine entry (pcy_llama_extend /
LlamaEngine.extend), the cached multi-token `LlamaPostTokenization.forward` and `UnifiedProCyon.score_candidates` -- against the oracle
(oracle.llama_ref: apply_rope, build_additive_mask, the eager attention of layer_forward, the two-phase llama_forward(past_kv=...)).

Operator bars: those of tests/test_gpu_kernels.py::test_attention_exact_rounding for the same arithmetic (rel_err < 1e-3, assert_bf16_close with
max_frac 0.03 and inter 0.5, the masked case with that file's masked inter 0.03); cache contents and the stated identities bit for bit.
Engine bar, as tests/test_gpu_score.py::test_against_oracle builds its own: 2 D + 2 * 2^-7 * max|logit| + the xent operator's bar, with D the
distance of the EXISTING `eng.prefill` of the concatenated rows to the oracle on the same rows (code the extension does not touch).
The layer-reduced full geometry (SM.build("full", llama_layers=2)) is not built here: synthesising its 128k-row embedding and lm_head and
running the oracle over them takes far longer than a few seconds; head_dim 128 and grouped heads are covered by the operator cases."""
import math

import pytest
import torch
import torch.nn.functional as F

import score_common as SC
from conftest import assert_bf16_close, record_parity, rel_err

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
POISON = 768.0      # (exact in bf16)


def rnd(*shape, seed=0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(BF)


@pytest.fixture(scope="module")
def ctx():
    from procyon_amd.engine import Context
    return Context.get()


# ---------------------------------------------------------------------------------------------------------------- the operator
#        H  Hkv  dh  prefix_T filled  S   B  rows_per_prefix  keep
CASES = [(8, 2, 128, 45, 0, 19, 4, 2, "none"),
         (4, 2, 64, 64, 0, 33, 3, 3, "none"),
         (4, 4, 128, 1, 0, 1, 2, 1, "none"),
         (8, 2, 128, 40, 10, 20, 4, 2, "none"),
         (32, 8, 128, 0, 300, 70, 2, 0, "none"),        # plain cache: t_past 300 of Tmax 400
         (4, 2, 64, 45, 0, 19, 4, 2, "pads")]
N_LAYERS, LAYER = 2, 1      # the cache has two layers and the call names the second: the layer stride is part of the address


def _cfg(H, Hkv, dh):
    from procyon_amd.engine import LlamaConfig
    return LlamaConfig(vocab=16, d=H * dh, n_layers=N_LAYERS, n_heads=H, n_kv_heads=Hkv, ffn=64)


def _fill(cache, layer, k_rows, v_rows):
    """poison everything, then put k_rows / v_rows [rows, Hkv, t, dh] into slots [0, t) of `layer`"""
    cache.k.fill_(POISON)
    cache.v.fill_(POISON)
    t = k_rows.shape[2]
    if t:
        cache.k[layer, :, :, :t] = k_rows.cuda()
        cache.v[layer, :, :, :t] = v_rows.cuda()


def _make_caches(case):
    """-> (the cache of the case, a plain cache with the same logical contents, K / V logical rows [B, Hkv, t_past, dh] on the CPU)"""
    from procyon_amd.engine import KVCache
    H, Hkv, dh, Tp, filled, S, B, rpp, _ = case
    cfg = _cfg(H, Hkv, dh)
    t_past = Tp + filled
    own_k, own_v = rnd(B, Hkv, filled, dh, seed=11), rnd(B, Hkv, filled, dh, seed=12)
    if Tp:
        Bp = (B + rpp - 1) // rpp
        pre_k, pre_v = rnd(Bp, Hkv, Tp, dh, seed=13), rnd(Bp, Hkv, Tp, dh, seed=14)
        prefix = KVCache(cfg, Bp, Tp, "cuda")
        _fill(prefix, LAYER, pre_k, pre_v)
        cache = KVCache(cfg, B, filled + S + 3, "cuda", prefix=prefix, rows_per_prefix=rpp)
        rows = torch.arange(B) // rpp
        k_log, v_log = torch.cat([pre_k[rows], own_k], 2), torch.cat([pre_v[rows], own_v], 2)
    else:
        cache = KVCache(cfg, B, 400, "cuda")
        k_log, v_log = own_k, own_v
    _fill(cache, LAYER, own_k, own_v)
    plain = KVCache(cfg, B, t_past + S + 3, "cuda")
    _fill(plain, LAYER, k_log, v_log)
    return cache, plain, k_log, v_log


def _keep_for(case):
    H, Hkv, dh, Tp, filled, S, B, rpp, mode = case
    if mode == "none":
        return None
    cap = Tp + filled + S + 3
    keep = torch.ones(B, cap, dtype=torch.uint8)
    keep[0:2, :5] = 0                 # left pads of the two prompts
    keep[2:4, :33] = 0
    keep[1, Tp + 15:] = 0             # right pads in two suffixes
    keep[2, Tp + 10:] = 0
    keep[3, :] = 0                    # one row with every byte 0: every query of it has no allowed key
    return keep


def _reference(case, qkv, k_log, v_log, keep):
    """oracle formulas: apply_rope at t_past + s, then layer_forward's eager attention under build_additive_mask"""
    from oracle import llama_ref as LR
    from procyon_amd.engine import rope_tables
    H, Hkv, dh, Tp, filled, S, B, rpp, _ = case
    t_past = Tp + filled
    cos, sin = rope_tables(dh, 10000.0, t_past + S, "cpu")
    q = qkv[:, :H * dh].view(B, S, H, dh).transpose(1, 2)
    k = qkv[:, H * dh:(H + Hkv) * dh].view(B, S, Hkv, dh).transpose(1, 2)
    v = qkv[:, (H + Hkv) * dh:].view(B, S, Hkv, dh).transpose(1, 2)
    c, s_ = cos[t_past:t_past + S][None].expand(B, S, -1), sin[t_past:t_past + S][None].expand(B, S, -1)
    q, k = LR.apply_rope(q, k, c, s_)
    kk, vv = torch.cat([k_log, k], 2), torch.cat([v_log, v], 2)
    g = H // Hkv
    ke = kk[:, :, None].expand(B, Hkv, g, t_past + S, dh).reshape(B, H, t_past + S, dh)
    ve = vv[:, :, None].expand(B, Hkv, g, t_past + S, dh).reshape(B, H, t_past + S, dh)
    sc = torch.matmul(q, ke.transpose(2, 3)) * (dh ** -0.5)
    sc = sc + LR.build_additive_mask(None if keep is None else keep[:, :t_past + S], B, S, t_past, BF)
    p = F.softmax(sc, dim=-1, dtype=torch.float32).to(BF)
    o = torch.matmul(p, ve).transpose(1, 2).contiguous().reshape(B * S, H * dh)
    return o, k, v


def _run(ctx, case, cache, qkv, keep, rows=None):
    from procyon_amd.engine import rope_tables
    H, Hkv, dh, Tp, filled, S, B, rpp, _ = case
    cos, sin = rope_tables(dh, 10000.0, Tp + filled + S + 8, "cuda")
    kd = None
    if keep is not None:
        kd = torch.zeros(cache.B, cache.capacity, dtype=torch.uint8)
        n = min(cache.capacity, keep.shape[1])
        kd[:, :n] = keep[:, :n]
        kd = kd.cuda()
    return ctx.attn_extend(qkv.cuda().clone(), cache, LAYER, Tp + filled, cos, sin, H, Hkv, dh, keep=kd, B=rows).cpu()


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"H{c[0]}kv{c[1]}dh{c[2]}-pre{c[3]}+{c[4]}-S{c[5]}-B{c[6]}x{c[7]}-{c[8]}")
def test_operator_against_the_oracle(ctx, case):
    H, Hkv, dh, Tp, filled, S, B, rpp, mode = case
    t_past = Tp + filled
    cache, plain, k_log, v_log = _make_caches(case)
    qkv = rnd(B * S, (H + 2 * Hkv) * dh, seed=1)
    keep = _keep_for(case)
    ref, k_new, v_new = _reference(case, qkv, k_log, v_log, keep)
    pre_before = None if cache.prefix is None else (cache.prefix.k.clone(), cache.prefix.v.clone())
    out = _run(ctx, case, cache, qkv, keep)
    err = rel_err(out, ref)
    print(f"attn_extend {case}: rel_err {err:.3e}, {(out != ref).float().mean().item():.4f} of elements differ")
    assert err < 1e-3
    assert_bf16_close(out, ref, "attn_extend", max_frac=0.03, inter=torch.full_like(ref, 0.03 if mode == "pads" else 0.5))
    # the cache after the call: new slots = roped k / projected v bit for bit, every other suffix slot still poison, the prefix untouched
    s0 = filled
    assert torch.equal(cache.k[LAYER, :, :, s0:s0 + S].cpu(), k_new) and torch.equal(cache.v[LAYER, :, :, s0:s0 + S].cpu(), v_new)
    assert bool((cache.k[LAYER, :, :, s0 + S:] == POISON).all()) and bool((cache.v[LAYER, :, :, s0 + S:] == POISON).all())
    assert bool((cache.k[1 - LAYER] == POISON).all()) and bool((cache.v[1 - LAYER] == POISON).all())
    if filled:
        assert torch.equal(cache.k[LAYER, :, :, :filled].cpu(), k_log[:, :, Tp:]) and torch.equal(cache.v[LAYER, :, :, :filled].cpu(), v_log[:, :, Tp:])
    if pre_before is not None:
        assert torch.equal(cache.prefix.k, pre_before[0]) and torch.equal(cache.prefix.v, pre_before[1])
    # exact identities
    assert torch.equal(_run(ctx, case, plain, qkv, keep), out), "shared-prefix cache vs plain cache with the same logical contents"
    assert torch.equal(plain.k[LAYER, :, :, t_past:t_past + S].cpu(), k_new)
    from procyon_amd.engine import KVCache
    for b in range(B):                                           # all rows at once vs each row alone
        one = KVCache(_cfg(H, Hkv, dh), 1, t_past + S + 3, "cuda")
        _fill(one, LAYER, k_log[b:b + 1], v_log[b:b + 1])
        kb = None if keep is None else keep[b:b + 1]
        assert torch.equal(_run(ctx, case, one, qkv[b * S:(b + 1) * S], kb), out[b * S:(b + 1) * S]), f"row {b} alone"
    _fill(plain, LAYER, k_log, v_log)
    cap = plain.capacity
    if keep is None:
        assert torch.equal(_run(ctx, case, plain, qkv, torch.ones(B, cap, dtype=torch.uint8)), out), "keep all ones vs keep = None"
        flip = torch.ones(B, cap, dtype=torch.uint8)
    else:
        k7 = keep[:, :cap].clone()
        k7[k7 != 0] = torch.tensor([7, 255, 2, 128], dtype=torch.uint8).repeat(int((k7 != 0).sum()) // 4 + 1)[:int((k7 != 0).sum())]
        assert torch.equal(_run(ctx, case, plain, qkv, k7), out), "non-zero bytes other than 1 count as kept"
        flip = keep[:, :cap].clone()
    flip[:, t_past + S:] = 1 - flip[:, t_past + S:].clamp(max=1)
    assert torch.equal(_run(ctx, case, plain, qkv, flip), out), "bytes at and above t_past + S are not read"


def test_operator_fully_masked_row_is_uniform_over_all_keys(ctx):
    """the all-zero row of the masked case, stated directly: every query's output is the mean of ALL t_past + S value rows, future ones included"""
    case = CASES[-1]
    H, Hkv, dh, Tp, filled, S, B, rpp, _ = case
    cache, _, k_log, v_log = _make_caches(case)
    qkv = rnd(B * S, (H + 2 * Hkv) * dh, seed=1)
    out = _run(ctx, case, cache, qkv, _keep_for(case))
    v_all = torch.cat([v_log[3], qkv[3 * S:4 * S, (H + Hkv) * dh:].view(S, Hkv, dh).transpose(0, 1)], 1)      # [Hkv, 64, dh]
    p = torch.full((Tp + S,), 1.0 / (Tp + S)).to(BF)
    mean = torch.matmul(p[None, None].float(), v_all.float())[:, 0].to(BF)                                    # [Hkv, dh]
    want = mean.repeat_interleave(H // Hkv, 0).reshape(1, H * dh).expand(S, -1)
    assert_bf16_close(out[3 * S:], want, "uniform row", max_frac=1.0)


def test_operator_argument_errors(ctx):
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import rope_tables
    case = CASES[0]
    H, Hkv, dh, Tp, filled, S, B, rpp, _ = case
    cache, plain, _, _ = _make_caches(case)
    before = cache.k.clone()
    cos, sin = rope_tables(dh, 10000.0, 128, "cuda")
    qkv = rnd(B * S, (H + 2 * Hkv) * dh, seed=1).cuda()
    with pytest.raises(PcyError, match="inside the shared prefix"):
        ctx.attn_extend(qkv, cache, LAYER, Tp - 1, cos, sin, H, Hkv, dh)
    with pytest.raises(PcyError, match="capacity"):
        ctx.attn_extend(qkv, cache, LAYER, Tp + 4, cos, sin, H, Hkv, dh)
    with pytest.raises(PcyError, match="head_dim"):
        ctx.attn_extend(rnd(B * S, 12 * 32, seed=1).cuda(), cache, LAYER, Tp, cos, sin, 8, 2, 32)
    assert torch.equal(cache.k, before)


# ---------------------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def env():
    from oracle import esm_ref as ER
    from oracle import llama_ref as LR
    e = SC.build_env()
    g = e["w"]["geom"]
    e["lgeom"], e["egeom"] = LR.LlamaGeom(**g["llama"]), ER.EsmGeom(**g["esm"])
    return e


P_, N_, TP_, S_ = 2, 3, 13, 9


@pytest.fixture(scope="module")
def work(env):
    """P = 2 prompts of 13 tokens (5 left pads in the second), N = 3 candidates of S = 9 tokens (right pads in two rows): the oracle's two-phase
    result, the existing prefill / score of the concatenated rows, D and the bar -- computed once"""
    from oracle import llama_ref as LR
    m = env["model"]
    eng = m.text_encoder.engine
    sd, geom = env["w"]["llama"], env["lgeom"]
    g = torch.Generator().manual_seed(21)
    B = P_ * N_
    pre_ids = torch.randint(0, 2000, (P_, TP_), generator=g)
    pmask = torch.ones(P_, TP_, dtype=torch.long)
    pmask[1, :5] = 0
    suf_ids = torch.randint(0, 2000, (B, S_), generator=g)
    smask = torch.ones(B, S_, dtype=torch.long)
    smask[1, 6:] = 0
    smask[5, 4:] = 0
    labels = torch.where(smask.bool(), suf_ids, torch.full_like(suf_ids, -100))
    labels[:, 0] = -100
    emb_w = sd["model.embed_tokens.weight"]
    pre_emb, suf_emb = F.embedding(pre_ids, emb_w), F.embedding(suf_ids, emb_w)
    r1 = LR.llama_forward(sd, geom, inputs_embeds=pre_emb, attn_mask=pmask)
    past = [(k.repeat_interleave(N_, 0), v.repeat_interleave(N_, 0)) for k, v in r1["past_kv"]]
    mask_all = torch.cat([pmask.repeat_interleave(N_, 0), smask], 1)
    r2 = LR.llama_forward(sd, geom, inputs_embeds=suf_emb, attn_mask=mask_all, past_kv=past)
    lg_ref = r2["logits"]                                                   # [B, S, V]
    V = lg_ref.shape[-1]
    ce = F.cross_entropy(lg_ref.float()[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100, reduction="none").view(B, S_ - 1)
    # the existing entry points on the concatenated rows
    cat_emb = torch.cat([pre_emb.repeat_interleave(N_, 0), suf_emb], 1).cuda()
    T = TP_ + S_
    own, _ = eng.prefill(cat_emb, mask_all, eng.new_cache(B, T), torch.arange(B * T, dtype=torch.int32))
    own = own.view(B, T, V)[:, TP_:].cpu()
    cat_labels = torch.cat([torch.full((B, TP_), -100), labels], 1)
    score_nll, score_n, _ = eng.score(cat_emb, mask_all, cat_labels)
    delta = float((own.float() - lg_ref.float()).abs().max())
    labelled = labels[:, 1:] != -100
    rows_ref = lg_ref[:, :-1][labelled].float()
    l64 = torch.logsumexp(rows_ref.double(), -1)
    nll64 = l64 - rows_ref.double().gather(1, labels[:, 1:][labelled][:, None])[:, 0]
    err_a = float((ce[labelled].double() - nll64).abs().max())
    big = torch.maximum(l64.abs(), rows_ref.max(-1).values.double().abs()).max()
    op_bar = 8 * max(err_a, 2.0 ** (math.floor(math.log2(float(big))) - 23))
    bar = 2 * delta + 2 * 2.0 ** -7 * float(lg_ref.float().abs().max()) + op_bar
    return dict(pre_ids=pre_ids, pmask=pmask, suf_ids=suf_ids, smask=smask, labels=labels, mask_all=mask_all, pre_emb=pre_emb, suf_emb=suf_emb,
                lg_ref=lg_ref, ce=ce, labelled=labelled, own=own, score_nll=score_nll.cpu()[:, TP_:], score_n=score_n, delta=delta, op_bar=op_bar,
                bar=bar, past2=r2["past_kv"], B=B, V=V)


def _extend_shared(env, work, **kw):
    eng = env["model"].text_encoder.engine
    prefix = eng.new_cache(P_, TP_)
    eng.prefill(work["pre_emb"].cuda(), work["pmask"], prefix, logit_rows=None)
    cache = eng.new_shared_cache(prefix, N_, S_)
    return eng.extend(cache, work["suf_emb"].cuda(), TP_, keep=work["mask_all"], **kw), cache


def test_engine_against_oracle_and_existing_entries(env, work):
    from procyon_amd import _lib
    lib = env["model"].text_encoder.engine.ctx.lib
    n0, x0 = lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND), lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT)
    (logits, hidden, token_nll, n_tok), cache = _extend_shared(env, work, logit_rows="all", labels=work["labels"], want_hidden=True)
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND) == n0 + 1 and lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT) == x0 + 1
    B, V, bar, labelled = work["B"], work["V"], work["bar"], work["labelled"]
    assert logits.shape == (B * S_, V) and hidden.shape == (B, S_, env["model"].text_encoder.cfg.d) and token_nll.shape == (B, S_)
    assert n_tok == int(labelled.sum()) == work["score_n"]
    lg = logits.view(B, S_, V).cpu().float()
    tn = token_nll.cpu()
    err_lg = float((lg - work["lg_ref"].float()).abs().max())
    err_tok = float((tn[:, 1:][labelled] - work["ce"][labelled]).abs().max())
    print(f"extend vs oracle: logits err {err_lg:.3e} token_nll err {err_tok:.3e} D {work['delta']:.3e} op_bar {work['op_bar']:.3e} bar {bar:.3e}")
    record_parity("extend/vs_oracle", logits_err=err_lg, token_nll_err=err_tok, delta=work["delta"], bar=bar)
    assert bool((tn[:, 0] == 0).all()) and bool((tn[:, 1:][~labelled] == 0).all())
    assert err_lg <= bar and err_tok <= bar
    assert bar < 0.5
    # ... and against what the parent offers for the same rows: prefill / score of the concatenated rows
    bar2 = 2 * work["delta"] + work["op_bar"]
    err_own = float((lg - work["own"].float()).abs().max())
    err_score = float((tn - work["score_nll"]).abs().max())
    print(f"extend vs prefill / score of the concatenated rows: logits {err_own:.3e} token_nll {err_score:.3e} bar {bar2:.3e}")
    record_parity("extend/vs_concatenated", logits_err=err_own, token_nll_err=err_score, bar=bar2)
    assert err_own <= bar2 and err_score <= bar2
    # the suffix K / V the call wrote: the oracle's rows [TP_, TP_ + S_) (a loose check of the append; the operator test holds the bits)
    for l in range(2):
        assert rel_err(cache.k[l].cpu(), work["past2"][l][0][:, :, TP_:]) < 2e-2


def test_engine_plain_cache_equals_shared_cache(env, work):
    """the same logical contents in a plain 6-row cache: same bits end to end"""
    eng = env["model"].text_encoder.engine
    (lg_s, _, nll_s, _), shared = _extend_shared(env, work, logit_rows="all", labels=work["labels"])
    plain = eng.new_cache(work["B"], TP_ + S_)
    for l in range(2):
        plain.k[l, :, :, :TP_] = shared.prefix.k[l].repeat_interleave(N_, 0)
        plain.v[l, :, :, :TP_] = shared.prefix.v[l].repeat_interleave(N_, 0)
    lg_p, _, nll_p, _ = eng.extend(plain, work["suf_emb"].cuda(), TP_, keep=work["mask_all"], logit_rows="all", labels=work["labels"])
    assert torch.equal(lg_p, lg_s) and torch.equal(nll_p, nll_s)
    assert torch.equal(plain.k[:, :, :, TP_:], shared.k) and torch.equal(plain.v[:, :, :, TP_:], shared.v)


def test_forward_with_cache_and_many_tokens(env, work):
    from oracle import llama_ref as LR
    from procyon_amd import _lib
    enc = env["model"].text_encoder
    lib = enc.engine.ctx.lib
    sd, geom = env["w"]["llama"], env["lgeom"]
    B = P_
    suf_ids, smask = work["suf_ids"][[0, 5]], work["smask"][[0, 5]]
    labels = work["labels"][[0, 5]]
    mask_all = torch.cat([work["pmask"], smask], 1)
    o1 = enc(input_ids=work["pre_ids"], attn_masks=work["pmask"], use_cache=True, lazy_hidden=True, want_hidden=False,
             logit_positions=torch.full((B,), TP_ - 1))
    n0 = lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND)
    o2 = enc(input_ids=suf_ids, past_key_values=o1.past_key_values, attn_masks=mask_all, full_labels=labels, compute_loss=True)
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND) == n0 + 1
    assert o2.logits.shape == (B, S_, work["V"]) and o2.past_key_values.t == TP_ + S_ and o2.past_key_values.cache is o1.past_key_values.cache
    assert o2.hidden_states[-1].shape == (B, S_, enc.cfg.d) and o2.token_nll.shape == (B, S_)
    assert o2.n_tokens == int((labels[:, 1:] != -100).sum())
    assert torch.equal(o2.loss, o2.token_nll.sum(1).sum() / o2.n_tokens)
    # lazy loss (compute_loss=False) = the same bits from a second pass; logit_positions pick rows of the same bits
    o2b = enc(input_ids=suf_ids, past_key_values=o1.past_key_values, attn_masks=mask_all, full_labels=labels, logit_positions=torch.tensor([8, 3]),
              want_hidden=False)
    assert o2b.hidden_states is None and o2b.logits.shape == (B, 1, work["V"])
    assert torch.equal(o2b.logits[:, 0], o2.logits[torch.arange(B), torch.tensor([8, 3])])
    assert torch.equal(o2b.loss, o2.loss) and torch.equal(o2b.token_nll, o2.token_nll)
    assert enc(input_embeds=enc.engine.embed_tokens(suf_ids), past_key_values=o1.past_key_values, attn_masks=mask_all).loss is None
    # oracle: the same two phases, then one more token without a mask (the decode quirk Q1)
    r1 = LR.llama_forward(sd, geom, input_ids=work["pre_ids"], attn_mask=work["pmask"])
    r2 = LR.llama_forward(sd, geom, input_ids=suf_ids, attn_mask=mask_all, past_kv=r1["past_kv"])
    bar = work["bar"]
    assert float((o2.logits.cpu().float() - r2["logits"].float()).abs().max()) <= bar
    nxt = torch.tensor([[17], [1234]])
    d0 = sum(lib.pcy_debug_dispatch_count(k) for k in _lib.DISPATCH_DECODE.values())
    n1 = lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND)
    o3 = enc(input_ids=nxt, past_key_values=o2.past_key_values)
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND) == n1                         # the [B,1] call is the decode step, not an extension
    assert sum(lib.pcy_debug_dispatch_count(k) for k in _lib.DISPATCH_DECODE.values()) >= d0   # (a replayed graph counts at capture only)
    assert o3.logits.shape == (B, 1, work["V"]) and o3.past_key_values.t == TP_ + S_ + 1 and o3.loss is None
    r3 = LR.llama_forward(sd, geom, input_ids=nxt, attn_mask=None, past_kv=r2["past_kv"])
    err = float((o3.logits.cpu().float() - r3["logits"].float()).abs().max())
    print(f"decode step behind the extension vs oracle: {err:.3e} (bar {bar:.3e})")
    record_parity("extend/then_decode_vs_oracle", logits_err=err, bar=bar)
    assert err <= bar
    # capacity: the message of the decode path
    with pytest.raises(ValueError, match="exhausted; raise max_new_tokens"):
        enc(input_ids=torch.zeros(B, 40, dtype=torch.long), past_key_values=o1.past_key_values)


def test_one_token_call_is_the_unchanged_decode_step(env, work):
    """[B,1] with a cache: the decode graph as before -- same bits as the engine's own decode on a twin cache, DISPATCH_EXTEND does not move"""
    from procyon_amd import _lib
    from procyon_amd.engine import GenState
    enc = env["model"].text_encoder
    eng, lib = enc.engine, enc.engine.ctx.lib
    o1 = enc(input_ids=work["pre_ids"], attn_masks=work["pmask"], use_cache=True, lazy_hidden=True, want_hidden=False)
    twin = eng.new_cache(P_, o1.past_key_values.cache.Tmax)
    twin.k.copy_(o1.past_key_values.cache.k)
    twin.v.copy_(o1.past_key_values.cache.v)
    nxt = torch.tensor([[5], [77]])
    n0 = lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND)
    o = enc(input_ids=nxt, past_key_values=o1.past_key_values)
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND) == n0
    st = GenState(P_, enc.cfg.vocab, 1, eng.device)
    st.pos.fill_(TP_)
    st.next_tok.copy_(nxt.view(-1).to(torch.int32))
    eng.decode_graph(twin, st, P_)
    assert torch.equal(o.logits.view(P_, -1), st.logits)


def test_engine_argument_errors_leave_the_cache_alone(env, work):
    from procyon_amd._lib import PcyError
    eng = env["model"].text_encoder.engine
    prefix = eng.new_cache(P_, TP_)
    eng.prefill(work["pre_emb"].cuda(), work["pmask"], prefix, logit_rows=None)
    cache = eng.new_shared_cache(prefix, N_, S_)
    cache.k.fill_(POISON)
    cache.v.fill_(POISON)
    snap = (cache.k.clone(), cache.v.clone(), prefix.k.clone(), prefix.v.clone())
    emb = work["suf_emb"].cuda()
    d = emb.shape[2]
    with pytest.raises(PcyError, match="capacity"):
        eng.extend(cache, emb, TP_ + 1)                                           # t_past + S beyond the logical capacity
    with pytest.raises(PcyError, match="inside the shared prefix"):
        eng.extend(cache, emb[:, :2], TP_ - 1)                                    # a shared cache with t_past < prefix_T
    with pytest.raises(PcyError, match="exceeds cache rows"):
        eng.extend(cache, torch.cat([emb, emb[:1]], 0), TP_)                      # B beyond the cache's rows
    cache.c.rows_per_prefix = 2
    try:
        with pytest.raises(PcyError, match="prefix rows"):
            eng.extend(cache, emb, TP_)                                           # B beyond prefix_B * rows_per_prefix
    finally:
        cache.c.rows_per_prefix = N_
    with pytest.raises(PcyError, match="S=0"):
        eng.extend(cache, torch.zeros(6, 0, d, dtype=BF, device="cuda"), TP_)     # S < 1
    big = eng.new_cache(1, 4200)
    with pytest.raises(PcyError, match="rope table"):
        eng.extend(big, emb[:1], 4090)                                            # t_past + S > max_pos
    assert bool((big.k == 0).all())
    eng.quantize_fp8()
    try:
        with pytest.raises(PcyError, match="fp8"):
            eng.extend(cache, emb, TP_)                                           # fp8 layers
    finally:
        eng.set_fp8(False)
    for a, b in zip(snap, (cache.k, cache.v, prefix.k, prefix.v)):
        assert torch.equal(a, b)
    # after all the refusals the same call still works
    lg, _, _, _ = eng.extend(cache, emb, TP_, keep=work["mask_all"], logit_rows="last")
    assert lg.shape == (6, work["V"]) and bool(torch.isfinite(lg.float()).all())


# ---------------------------------------------------------------------------------------------------------------- the model
def _split(instr):
    head, tail = instr.split("[ANSWER]")
    return head + "[ANSWER]", tail.strip()


def test_score_candidates_against_score_text(env, work):
    from procyon_amd import _lib
    m = env["model"]
    lib = m.text_encoder.engine.ctx.lib
    prompts, tails = zip(*[_split(i) for i in SC.INSTR])
    cands = [[t, "w7 w8", "alpha beta gamma delta epsilon zeta eta theta iota"] for t in tails]
    n0, x0 = lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND), lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT)
    res = m.score_candidates(SC.make_inputs(env, instr=list(prompts)), cands)
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND) == n0 + 1 and lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT) == x0 + 1
    assert res["cache"].prefix.B == 3 and res["cache"].B == 9 and res["cache"].rows_per_prefix == 3      # the prompts were prefilled ONCE each
    S = res["plan"]["S"]
    assert res["token_nll"].shape == (3, 3, S) and res["seq_nll"].shape == res["n_tokens"].shape == res["mean_nll"].shape == res["order"].shape == (3, 3)
    # score_text of the 9 concatenated rows
    rows = [p + " " + c for p, cs in zip(prompts, cands) for c in cs]
    slots = [s for s in SC.SLOTS for _ in range(3)]
    st = m.score_text(SC.make_inputs(env, instr=rows, slots=slots))
    n_ref = st["n_tokens"].view(3, 3)
    assert torch.equal(res["n_tokens"].cpu(), n_ref.cpu())
    diff = (res["seq_nll"].cpu() - st["seq_nll"].view(3, 3).cpu()).abs()
    print(f"score_candidates vs score_text: seq_nll diff {diff.max().item():.3e}, per token {(diff / n_ref.cpu()).max().item():.3e} (bar {work['bar']:.3e})")
    record_parity("extend/score_candidates_vs_score_text", seq_nll_diff=float(diff.max()), per_token=float((diff / n_ref.cpu()).max()), bar=work["bar"])
    assert bool((diff <= work["bar"] * n_ref.cpu()).all())
    assert torch.equal(res["mean_nll"], res["seq_nll"] / res["n_tokens"])
    assert torch.equal(res["order"], torch.argsort(res["mean_nll"], dim=1, stable=True))
    with pytest.raises(ValueError, match="same number of candidates"):
        m.score_candidates(SC.make_inputs(env, instr=list(prompts)), [["a"], ["b", "c"], ["d"]])


def test_score_candidates_ranks_the_greedy_continuation_first(env, work):
    """the construction of tests/test_gpu_score.py::test_ranking_greedy_continuation_beats_random_tokens through the public call: the model's
    own greedy continuation of a prompt against random words in its place.  Words hash to ids, so the ids are turned back into words through
    a table of the words " w0", " w1", ... (a continuation that leaves the table -- a special token -- takes the next prompt)."""
    m = env["model"]
    tok = m.tokenizer
    back = {}
    for i in range(60000):
        back.setdefault(tok._word_id(f" w{i}"), f"w{i}")
    n_new = 8
    g = torch.Generator().manual_seed(11)
    chosen = None
    for k in range(12):
        instr = [f"w{k} <|protein|> is w2 ? [ANSWER]"]
        tokens, _, _, _ = m.generate(SC.make_inputs(env, instr=instr, slots=[[0]]), max_len=n_new, method="greedy", truncate_on_eos=False)
        ids = tokens.reshape(-1)[:n_new].tolist()
        if all(i in back for i in ids):
            chosen = (instr, ids)
            break
    assert chosen is not None, "no prompt whose greedy continuation stays inside the word table"
    instr, ids = chosen
    rand = [int(i) for i in torch.randint(0, 2000, (n_new,), generator=g) if int(i) in back][:n_new]
    words = lambda xs: " ".join(back[i] for i in xs)
    res = m.score_candidates(SC.make_inputs(env, instr=instr, slots=[[0]]), [[words(rand), words(ids)]])
    # the candidate really is the continuation: its suffix tokens are [ANSWER] + the greedy ids + eos
    assert res["plan"]["suffix_ids"][1, 1:1 + n_new].tolist() == ids
    print(f"greedy vs random candidates: mean_nll {res['mean_nll'].tolist()}")
    assert res["order"].tolist() == [[1, 0]]
    # the ranking means something only if the gap exceeds what the arithmetic can move a per-token mean by: the engine bar, once per side
    # (measured on an MI355X: 7.549 against 6.609 with a bar of 3.7e-2; the means include the closing eos, which costs both sides alike)
    assert float(res["mean_nll"][0, 0]) - float(res["mean_nll"][0, 1]) > 2 * work["bar"]
