"""GPU: the packed extension attention (pcy_attn_extend_packed / attn_ext_packed_kernel), the engine entry that uses it
(pcy_llama_extend_packed / LlamaEngine.extend(packed=True), score_candidates(packed=True)) and `UnifiedProCyon.forward(share_prefix=True)`.

The packed operator must give the bits of the unpacked one (pcy_attn_extend): `o`, the K / V slots written, everything else untouched -- on
twin caches, for shapes where a 64-slot tile spans several rows, is cut inside a row, ends with a prompt that is short of rows, has
t_past > Tp, Tp < 32 with masks that differ inside a prompt, and a plain cache.  It is also held to the oracle formulas with the bars of
tests/test_gpu_extend.py::test_operator_against_the_oracle (that file's `_reference`, restated here).
Model bar: 2 D + 2 * 2^-7 * max|logit| with D the distance of the EXISTING `forward`'s answer logits to the oracle on the same embeddings."""
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
CASES = [(8, 2, 128, 45, 0, 5, 6, 3, "none"),          # G*S = 20: a tile spans four rows; 60 packed queries per prompt, tiles do not cross it
         (4, 2, 64, 64, 0, 33, 3, 3, "none"),          # G*S = 66 > 64: a row's queries are cut by a tile edge; Tp % 32 == 0: no straddling block
         (4, 4, 128, 1, 0, 1, 2, 1, "none"),           # the smallest shape
         (8, 2, 128, 40, 10, 20, 4, 2, "none"),        # t_past > Tp
         (8, 2, 128, 45, 0, 5, 5, 3, "none"),          # the last prompt is short of rows
         (32, 8, 128, 0, 300, 70, 2, 0, "none"),       # plain cache: t_past 300 of Tmax 400
         (4, 2, 64, 7, 0, 19, 4, 2, "pads"),           # Tp < 32; masks that differ inside a prompt, one row without any kept key
         (8, 2, 128, 70, 0, 5, 4, 2, "prefix_pads")]   # two shared-phase blocks scored under PREFIX masks that differ between the rows of a prompt
N_LAYERS, LAYER = 2, 1
IDS = lambda c: f"H{c[0]}kv{c[1]}dh{c[2]}-pre{c[3]}+{c[4]}-S{c[5]}-B{c[6]}x{c[7]}-{c[8]}"


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


def _make_cache(case):
    """-> (the cache of the case, K / V logical rows [B, Hkv, t_past, dh] on the CPU); deterministic: two calls give twins"""
    from procyon_amd.engine import KVCache
    H, Hkv, dh, Tp, filled, S, B, rpp, _ = case
    cfg = _cfg(H, Hkv, dh)
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
    return cache, k_log, v_log


def _keep_for(case):
    H, Hkv, dh, Tp, filled, S, B, rpp, mode = case
    if mode == "none":
        return None
    cap = Tp + filled + S + 3
    keep = torch.ones(B, cap, dtype=torch.uint8)
    if mode == "prefix_pads":         # rows 0 / 1 share a prefix panel, rows 2 / 3 the other: every row masks other prefix keys
        keep[0, :5] = 0
        keep[1, :37] = 0              # (beyond the first 32-key block)
        keep[1, 50] = 0
        keep[2, 10:20] = 0
        keep[2, 40:64:3] = 0
        keep[3, Tp + 3:] = 0          # an untouched prefix beside it, right pads in the suffix
        return keep
    keep[0:2, :5] = 0                 # left pads of the two prompts: rows 0 / 1 share a prefix panel and so do rows 2 / 3 ...
    keep[2:4, :33] = 0
    keep[1, Tp + 15:] = 0             # ... but their masks differ (right pads in two suffixes)
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


def _run(ctx, case, cache, qkv, keep, packed, rows=None):
    from procyon_amd.engine import rope_tables
    H, Hkv, dh, Tp, filled, S, B, rpp, _ = case
    cos, sin = rope_tables(dh, 10000.0, Tp + filled + S + 8, "cuda")
    kd = None
    if keep is not None:
        kd = torch.zeros(cache.B, cache.capacity, dtype=torch.uint8)
        n = min(cache.capacity, keep.shape[1])
        kd[:, :n] = keep[:, :n]
        kd = kd.cuda()
    return ctx.attn_extend(qkv.cuda().clone(), cache, LAYER, Tp + filled, cos, sin, H, Hkv, dh, keep=kd, B=rows, packed=packed).cpu()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_packed_operator_equals_the_unpacked_one_and_the_oracle(ctx, case):
    from procyon_amd.engine import KVCache
    H, Hkv, dh, Tp, filled, S, B, rpp, mode = case
    t_past = Tp + filled
    cache_u, k_log, v_log = _make_cache(case)
    cache_p, _, _ = _make_cache(case)
    assert torch.equal(cache_u.k, cache_p.k) and torch.equal(cache_u.v, cache_p.v)          # twins
    qkv = rnd(B * S, (H + 2 * Hkv) * dh, seed=1)
    keep = _keep_for(case)
    pre_before = None if cache_p.prefix is None else (cache_p.prefix.k.clone(), cache_p.prefix.v.clone())
    out_u = _run(ctx, case, cache_u, qkv, keep, False)
    out_p = _run(ctx, case, cache_p, qkv, keep, True)
    print(f"attn_extend packed vs unpacked {case}: {(out_p != out_u).float().mean().item():.4f} of elements differ")
    assert torch.equal(out_p, out_u)
    # the cache: the twins stay twins (the slots written AND the poison), stated once more slot by slot for the packed one
    assert torch.equal(cache_p.k, cache_u.k) and torch.equal(cache_p.v, cache_u.v)
    ref, k_new, v_new = _reference(case, qkv, k_log, v_log, keep)
    s0 = filled
    assert torch.equal(cache_p.k[LAYER, :, :, s0:s0 + S].cpu(), k_new) and torch.equal(cache_p.v[LAYER, :, :, s0:s0 + S].cpu(), v_new)
    assert bool((cache_p.k[LAYER, :, :, s0 + S:] == POISON).all()) and bool((cache_p.v[LAYER, :, :, s0 + S:] == POISON).all())
    assert bool((cache_p.k[1 - LAYER] == POISON).all()) and bool((cache_p.v[1 - LAYER] == POISON).all())
    if filled:
        assert torch.equal(cache_p.k[LAYER, :, :, :filled].cpu(), k_log[:, :, Tp:]) and torch.equal(cache_p.v[LAYER, :, :, :filled].cpu(), v_log[:, :, Tp:])
    if pre_before is not None:
        assert torch.equal(cache_p.prefix.k, pre_before[0]) and torch.equal(cache_p.prefix.v, pre_before[1])
    # the oracle formulas, with the bars of the unpacked operator's test
    err = rel_err(out_p, ref)
    print(f"attn_extend packed {case}: rel_err {err:.3e}, {(out_p != ref).float().mean().item():.4f} of elements differ")
    assert err < 1e-3
    assert_bf16_close(out_p, ref, "attn_extend packed", max_frac=0.03, inter=torch.full_like(ref, 0.5 if mode == "none" else 0.03))
    # all rows at once = each row alone (a one-row plain cache with the row's logical contents)
    for b in range(B):
        one = KVCache(_cfg(H, Hkv, dh), 1, t_past + S + 3, "cuda")
        _fill(one, LAYER, k_log[b:b + 1], v_log[b:b + 1])
        kb = None if keep is None else keep[b:b + 1]
        assert torch.equal(_run(ctx, case, one, qkv[b * S:(b + 1) * S], kb, True), out_p[b * S:(b + 1) * S]), f"row {b} alone"
    if keep is None:
        _fill(cache_p, LAYER, k_log[:, :, Tp:], v_log[:, :, Tp:])
        ones = torch.ones(B, cache_p.capacity, dtype=torch.uint8)
        assert torch.equal(_run(ctx, case, cache_p, qkv, ones, True), out_p), "keep all ones vs keep = None"


def test_packed_operator_fewer_rows_than_the_cache_holds(ctx):
    """B below the cache's rows, and not a multiple of rows_per_prefix: rows 0..3 of a 6-row cache with 3 rows per prefix"""
    case = CASES[0]
    H, Hkv, dh, Tp, filled, S, B, rpp, _ = case
    cache_u, _, _ = _make_cache(case)
    cache_p, _, _ = _make_cache(case)
    qkv = rnd(B * S, (H + 2 * Hkv) * dh, seed=1)[:4 * S]
    out_u = _run(ctx, case, cache_u, qkv, None, False, rows=4)
    out_p = _run(ctx, case, cache_p, qkv, None, True, rows=4)
    assert torch.equal(out_p, out_u)
    assert torch.equal(cache_p.k, cache_u.k) and torch.equal(cache_p.v, cache_u.v)
    assert bool((cache_p.k[:, 4:] == POISON).all()) and bool((cache_p.v[:, 4:] == POISON).all())


def test_packed_operator_argument_errors(ctx):
    """the refusals of pcy_attn_extend, with its messages; nothing is written"""
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import rope_tables
    case = (8, 2, 128, 45, 0, 19, 4, 2, "none")
    H, Hkv, dh, Tp, filled, S, B, rpp, _ = case
    cache, _, _ = _make_cache(case)
    before = cache.k.clone()
    cos, sin = rope_tables(dh, 10000.0, 128, "cuda")
    qkv = rnd(B * S, (H + 2 * Hkv) * dh, seed=1).cuda()
    calls = [("inside the shared prefix", lambda p: ctx.attn_extend(qkv, cache, LAYER, Tp - 1, cos, sin, H, Hkv, dh, packed=p)),
             ("capacity", lambda p: ctx.attn_extend(qkv, cache, LAYER, Tp + 4, cos, sin, H, Hkv, dh, packed=p)),
             ("head_dim", lambda p: ctx.attn_extend(rnd(B * S, 12 * 32, seed=1).cuda(), cache, LAYER, Tp, cos, sin, 8, 2, 32, packed=p))]
    for match, call in calls:
        msgs = []
        for packed in (False, True):
            with pytest.raises(PcyError, match=match) as ei:
                call(packed)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1]
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


P_, N_, TP_, S_ = 2, 3, 13, 9      # the shapes of tests/test_gpu_extend.py's `work`


@pytest.fixture(scope="module")
def work(env):
    sd = env["w"]["llama"]
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
    return dict(pmask=pmask, labels=labels, mask_all=torch.cat([pmask.repeat_interleave(N_, 0), smask], 1),
                pre_emb=F.embedding(pre_ids, emb_w), suf_emb=F.embedding(suf_ids, emb_w))


def _extend_shared(env, work, **kw):
    eng = env["model"].text_encoder.engine
    prefix = eng.new_cache(P_, TP_)
    eng.prefill(work["pre_emb"].cuda(), work["pmask"], prefix, logit_rows=None)
    cache = eng.new_shared_cache(prefix, N_, S_)
    return eng.extend(cache, work["suf_emb"].cuda(), TP_, keep=work["mask_all"], **kw), cache


def test_engine_packed_equals_unpacked(env, work):
    from procyon_amd import _lib
    lib = env["model"].text_encoder.engine.ctx.lib
    count = lambda: (lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND), lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND_PACKED))
    kw = dict(logit_rows="all", labels=work["labels"], want_hidden=True)
    e0, p0 = count()
    (lg_u, hid_u, nll_u, n_u), cache_u = _extend_shared(env, work, **kw)
    assert count() == (e0 + 1, p0)                                       # the default path does not touch counter 19
    (lg_p, hid_p, nll_p, n_p), cache_p = _extend_shared(env, work, packed=True, **kw)
    assert count() == (e0 + 2, p0 + 1)                                   # one packed call: kind 18 and kind 19 move by one each
    assert n_u == n_p and n_p == int((work["labels"][:, 1:] != -100).sum())
    assert torch.equal(lg_p, lg_u) and torch.equal(nll_p, nll_u) and torch.equal(hid_p, hid_u)
    assert torch.equal(cache_p.k, cache_u.k) and torch.equal(cache_p.v, cache_u.v)
    assert bool(torch.isfinite(lg_p.float()).all())
    # a plain cache with the same logical contents, packed: the same bits again
    eng = env["model"].text_encoder.engine
    plain = eng.new_cache(P_ * N_, TP_ + S_)
    for l in range(2):
        plain.k[l, :, :, :TP_] = cache_p.prefix.k[l].repeat_interleave(N_, 0)
        plain.v[l, :, :, :TP_] = cache_p.prefix.v[l].repeat_interleave(N_, 0)
    lg_q, _, nll_q, _ = eng.extend(plain, work["suf_emb"].cuda(), TP_, keep=work["mask_all"], logit_rows="all", labels=work["labels"], packed=True)
    assert torch.equal(lg_q, lg_p) and torch.equal(nll_q, nll_p)


def _split(instr):
    head, tail = instr.split("[ANSWER]")
    return head + "[ANSWER]", tail.strip()


def test_score_candidates_packed_equals_unpacked(env):
    from procyon_amd import _lib
    m = env["model"]
    lib = m.text_encoder.engine.ctx.lib
    prompts, tails = zip(*[_split(i) for i in SC.INSTR])
    cands = [[t, "w7 w8", "alpha beta gamma delta epsilon zeta eta theta iota"] for t in tails]
    res_u = m.score_candidates(SC.make_inputs(env, instr=list(prompts)), cands)
    p0 = lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND_PACKED)
    res_p = m.score_candidates(SC.make_inputs(env, instr=list(prompts)), cands, packed=True)
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND_PACKED) == p0 + 1
    for k in ("token_nll", "seq_nll", "mean_nll", "order", "n_tokens"):
        assert torch.equal(res_p[k], res_u[k]), k
    assert torch.equal(res_p["cache"].k, res_u["cache"].k) and torch.equal(res_p["cache"].v, res_u["cache"].v)


# ---------------------------------------------------------------------------------------------------------------- the model
QA_HEAD = ("w11 w12 w13 <|protein|> binds <|protein|> ? [ANSWER] yes w14 w15 w16 w17 w18 w19 w20 w21 <|protein|> binds")      # two shared slots + the
QA_TAILS = ["", "w5", "w5 w6", "", "w7", "w8 w6"]                                                                      # receptor of the question
QA_SLOTS = [[0, 1, 0, 2 + i] for i in range(6)]


@pytest.fixture(scope="module")
def qa(env):
    """six QA rows: ~20 shared tokens with two shared slots and the receptor, then the row's own peptide and none / one / two trailing words
    (ragged: the suffixes carry right pads).  The oracle on the full rows' embeddings and the EXISTING forward, computed once."""
    from oracle import llama_ref as LR
    from procyon_amd import synth
    m = env["model"]
    prot = synth.protein_tokens([90, 41, 30, 35, 52, 47, 33, 61], seed=3)
    instr = [QA_HEAD + " <|protein|> " + (t + " " if t else "") + "? [ANSWER]" for t in QA_TAILS]

    def inputs():
        return {"data": {"seq": prot, "seq_idx": torch.arange(prot.shape[0]), "text": [], "drug": None},
                "input": {"seq": [list(s) for s in QA_SLOTS], "text": [[] for _ in instr], "drug": None},
                "target": {"seq": None, "text": None, "drug": None}, "instructions": list(instr)}

    emb, ids, am, *_ = m._preprocessing(inputs(), crop_off=False)
    real = int(am.sum(1).max())
    B = len(instr)
    pos = torch.tensor([int((ids[i] == m.answer_idx).nonzero()[:, 0].max()) for i in range(B)])
    ref = LR.llama_forward(env["w"]["llama"], env["lgeom"], inputs_embeds=emb[:, :real].cpu(), attn_mask=am[:, :real])["logits"]
    ref = ref[torch.arange(B), pos].float()                                                 # [B, V]
    own = m.forward(inputs())
    assert torch.equal(own["answer_positions"], pos)
    D = float((own["outputs"].answer_logits[:, 0].cpu().float() - ref).abs().max())
    bar = 2 * D + 2 * 2.0 ** -7 * float(ref.abs().max())
    slot3 = int((ids[0] == m.prot_replacement_idx).nonzero()[3, 0])
    return dict(inputs=inputs, ids=ids, pos=pos, ref=ref, own=own["outputs"].answer_logits[:, 0].cpu(), D=D, bar=bar, Tp=slot3, B=B, real=real)


def test_forward_share_prefix_against_the_oracle(env, qa):
    from procyon_amd import _lib
    m = env["model"]
    lib = m.text_encoder.engine.ctx.lib
    count = lambda: (lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND), lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND_PACKED))
    B, pos = qa["B"], qa["pos"]
    e0, p0 = count()
    out_p = m.forward(qa["inputs"](), share_prefix=True)                                    # packed=True is the default of this path
    assert count() == (e0 + 1, p0 + 1)
    out_u = m.forward(qa["inputs"](), share_prefix=True, packed=False)
    assert count() == (e0 + 2, p0 + 1)
    plan = out_p["prefix_plan"]
    # the cut: in front of the last slot (the ids agree beyond it in rows 0 and 3; the peptides differ); ragged suffixes
    assert plan["Tp"] == qa["Tp"] and plan["Tp"] >= 16 and plan["S"] == int(pos.max()) - qa["Tp"] + 1
    assert plan["suffix_mask"].sum(1).tolist() == [3, 4, 5, 3, 4, 5] and torch.equal(plan["answer_pos"], pos)
    assert torch.equal(out_p["answer_positions"], pos) and torch.equal(out_p["text_toks"], qa["ids"])
    assert set(out_p) == set(m.forward(qa["inputs"]())) | {"prefix_plan"}
    lg_p, lg_u = out_p["outputs"].answer_logits, out_u["outputs"].answer_logits
    assert lg_p.shape == (B, 1, qa["ref"].shape[-1]) and lg_p.dtype == BF
    assert torch.equal(lg_p, lg_u), "packed and unpacked extension attention"
    err = float((lg_p[:, 0].cpu().float() - qa["ref"]).abs().max())
    err_own = float((lg_p[:, 0].cpu().float() - qa["own"].float()).abs().max())
    print(f"forward(share_prefix) vs oracle: {err:.3e}; vs the ordinary forward: {err_own:.3e}; D {qa['D']:.3e} bar {qa['bar']:.3e}")
    record_parity("qa_prefix/vs_oracle", logits_err=err, delta=qa["D"], bar=qa["bar"])
    record_parity("qa_prefix/vs_forward", logits_err=err_own, bar=qa["bar"])
    assert err <= qa["bar"]
    assert qa["bar"] < 0.5
    # outputs.logits: the answer rows come back as they are; anything else is the ordinary full pass
    lz = out_p["outputs"].logits
    assert lz.shape == (B, qa["real"], qa["ref"].shape[-1])
    assert torch.equal(lz[torch.arange(B), pos], lg_p[:, 0]) and lz._full_t is None          # the answer rows, nothing materialised
    full = lz[:, 0]                                                                          # materialises [B, T, V] (the existing fallback)
    assert full.shape == (B, qa["ref"].shape[-1]) and bool(torch.isfinite(full.float()).all())


def test_forward_share_prefix_suffixes_of_one_length_run_without_a_mask(env, qa):
    """rows 0 and 3 alone: both suffixes are `<|protein|> ? [ANSWER]`, the plan's suffix mask is all ones and `forward` hands the extension no
    mask at all (the kernel's unmasked block path).  A row's bits depend on its own row only, and keep = ones is keep = None: the bits of
    the six-row call, whose ragged suffixes needed a mask."""
    m = env["model"]
    six = m.forward(qa["inputs"](), share_prefix=True)["outputs"].answer_logits
    inp = qa["inputs"]()
    inp["instructions"] = [inp["instructions"][i] for i in (0, 3)]
    inp["input"]["seq"] = [inp["input"]["seq"][i] for i in (0, 3)]
    inp["input"]["text"] = [[], []]
    seen = {}
    eng = m.text_encoder.engine
    real_extend = eng.extend
    eng.extend = lambda *a, **k: (seen.update(keep=k.get("keep")), real_extend(*a, **k))[1]
    try:
        two = m.forward(inp, share_prefix=True)
    finally:
        del eng.extend
    assert "keep" in seen and seen["keep"] is None and bool(two["prefix_plan"]["suffix_mask"].all())
    assert two["prefix_plan"]["Tp"] == qa["Tp"] and two["prefix_plan"]["S"] == 3
    assert torch.equal(two["outputs"].answer_logits, six[[0, 3]])


def test_forward_share_prefix_without_a_common_prefix_takes_the_ordinary_path(env, qa):
    from procyon_amd import _lib
    m = env["model"]
    lib = m.text_encoder.engine.ctx.lib
    inp = qa["inputs"]()
    inp["instructions"] = [f"w{40 + i} " + s for i, s in enumerate(inp["instructions"])]
    ids, _ = m._prepare_text_inputs_and_tokenize(list(inp["instructions"]), [[] for _ in range(6)])
    shared = next(t for t in range(ids.shape[1]) if not bool((ids[:, t] == ids[0, t]).all()))
    e0 = lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND)
    out = m.forward(inp, share_prefix=True)
    if shared == 0:                                                                          # (no bos column: nothing shared at all)
        assert "prefix_plan" not in out and lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND) == e0
    else:                                                                                    # the bos column alone is shared
        assert out["prefix_plan"]["Tp"] == shared and lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND) == e0 + 1
    lg = out["outputs"].answer_logits
    assert bool(torch.isfinite(lg.float()).all())
    assert torch.equal(m.forward(inp, share_prefix=True, packed=False)["outputs"].answer_logits, lg)


def test_forward_share_prefix_rejects(env, qa):
    m = env["model"]
    eng = m.text_encoder.engine
    with pytest.raises(ValueError, match="retrieval"):
        m.forward(qa["inputs"](), share_prefix=True, retrieval=True)
    with pytest.raises(ValueError, match="compute_loss"):
        m.forward(qa["inputs"](), share_prefix=True, compute_loss=True)
    with pytest.raises(ValueError, match="full_logits"):
        m.forward(qa["inputs"](), share_prefix=True, full_logits=True)
    m.dtype = torch.float32                                                                  # the fp32 family
    try:
        with pytest.raises(NotImplementedError, match="bf16 engine"):
            m.forward(qa["inputs"](), share_prefix=True)
    finally:
        m.dtype = BF
    m.config.use_protein_struct = True                                                       # structure tokens: dropped at random per call
    try:
        with pytest.raises(NotImplementedError, match="structure tokens"):
            m.forward(qa["inputs"](), share_prefix=True)
    finally:
        m.config.use_protein_struct = False
    eng.quantize_fp8()
    try:
        with pytest.raises(NotImplementedError, match="fp8"):
            m.forward(qa["inputs"](), share_prefix=True)
    finally:
        eng.set_fp8(False)
    out = m.forward(qa["inputs"](), share_prefix=True)                                       # after the refusals the call still works
    assert float((out["outputs"].answer_logits[:, 0].cpu().float() - qa["ref"]).abs().max()) <= qa["bar"]
