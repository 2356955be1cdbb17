"""GPU: the fp32 family's loss and many-token cache extension -- the operators `pcy_f32_lm_head_xent` and `pcy_f32_attn_extend`
(procyon_amd/csrc/pcy_f32.hip), `LlamaEngineF32.score / extend / extend_behind`, the fp32 paths of `LlamaPostTokenization.forward` and
`UnifiedProCyon.score_text / score_candidates` -- against the float64 references of tests/f32_score_ref.py and the oracle.

lm_head_xent: `label_logit` and `row_max` are free of any summation order and must be the bits `F32Ops.linear(x, W)` stores; `lse` / `nll`
are compared with float64 on those same fp32 logits (pulled to the host) under the project's bar of DESIGN.md 4.5,
    8 x max(torch's own fp32 cross_entropy / logsumexp error against float64 on the same logits, one fp32 ulp at max(|lse|, |row max|)).
The vocabularies 2311, 8327, 65543 and 65671 are 7 modulo 128 (331, the vocabulary of the engine tests, leaves 75 columns in its last
tile): the last tile is always ragged.  8327 = 66 column blocks (the finish merge takes a second pass per lane), 65671 = 257 blocks of two
tiles, 65543 = 256 blocks of two tiles and a last one of one (tests/test_f32_score_ref_cpu.py pins these partitions).
attn_extend: the single-operator bars of tests/f32_ref.py, per row and head.
Engine / model against the oracle: |token_nll - oracle| <= 2 D + the operator's bar, D = the sup-norm distance of the engine's OWN prefill
logits at the scored rows to the oracle's (LSE and the label logit are each 1-Lipschitz in the sup norm; the prefill is code this feature
does not change), D capped at OP_MAXABS x max|oracle logit|."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import f32_ref as R
import f32_score_ref as S
from conftest import record_parity

pytestmark = pytest.mark.gpu
F32 = torch.float32
_CACHE = {}


@pytest.fixture(scope="module")
def ops():
    from procyon_amd.engine_f32 import F32Ops
    return F32Ops()


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


# ------------------------------------------------------------------------------------------------ lm_head_xent
XENT_SHAPES = [(331, 64), (331, 256), (2311, 64), (2311, 256)]
XENT_PARTITION = [(8327, 64), (65671, 64), (65543, 64)]      # second finish pass; two tiles per block; a shorter last block


def _case(ops, V, d, kind):
    """per (V, d, set), once: inputs on the device, the M = 257 `F32Ops.linear` logits on the host, their float64 reference and bar"""
    key = (V, d, kind)
    if key not in _CACHE:
        x, W, tg = S.xent_case(V, d, kind)
        xd, Wd, tgd = x.cuda(), W.cuda(), tg.to(torch.int32).cuda()
        G = ops.linear(xd, Wd)
        bar, err_a, ref = S.xent_bar(G.cpu(), tg)
        _CACHE[key] = dict(x=xd, W=Wd, tg=tgd, tg_host=tg, G=G, bar=bar, err_a=err_a, ref=ref)
    return _CACHE[key]


def _check_rows(ops, c, r0, r1, key):
    """score rows [r0, r1) of case c: exact label / max, lse / nll under the bar; -> the four outputs"""
    x, tg = c["x"][r0:r1].contiguous(), c["tg"][r0:r1].contiguous()
    nll, lse, row_max, label = ops.lm_head_xent(x, c["W"], tg, want_parts=True)
    G = c["G"][r0:r1]
    assert nll.dtype == F32 and nll.shape == (r1 - r0,)
    assert torch.equal(label, G.gather(1, tg[:, None].long())[:, 0]), "label_logit is not the bits F32Ops.linear stores"
    assert torch.equal(row_max, G.max(-1).values), "row_max is not the max of the F32Ops.linear row"
    nll64, lse64 = c["ref"][0][r0:r1], c["ref"][1][r0:r1]
    bar = c["bar"][r0:r1]
    e_lse, e_nll = (lse.cpu().double() - lse64).abs(), (nll.cpu().double() - nll64).abs()
    print(f"{key}: lse err {float(e_lse.max()):.3e} nll err {float(e_nll.max()):.3e} torch-fp32 err {c['err_a']:.3e} bar {float(bar.min()):.3e}")
    record_parity(key, lse_err=f"{float(e_lse.max()):.3e}", nll_err=f"{float(e_nll.max()):.3e}", torch_fp32_err=f"{c['err_a']:.3e}",
                  bar=f"{float(bar.min()):.3e}")
    assert bool((e_lse <= bar).all()) and bool((e_nll <= bar).all()), (key, float(e_lse.max()), float(e_nll.max()), float(bar.min()))
    return nll, lse, row_max, label


@pytest.mark.parametrize("kind", S.XENT_SETS)
@pytest.mark.parametrize("V,d", XENT_SHAPES + XENT_PARTITION)
@pytest.mark.parametrize("M", [1, 130, 257])
def test_xent_matches_linear_logits(ops, M, V, d, kind):
    if (V, d) in XENT_PARTITION and M == 257:
        M = 129                                       # (the partition cases: two row tiles are enough)
    c = _case(ops, V, d, kind)
    assert c["tg_host"][:9].tolist() == S.planted_targets(V)
    if M > 1:       # the planted faults would cost more than the bar on these rows (arithmetic on the reference logits, nothing planted in the kernel)
        dropped, padded = S.fault_costs(c["G"][:M].cpu())
        if kind == "negative":
            assert bool((padded > 100 * c["bar"][:M]).all())
        if kind == "peaked":
            assert bool((dropped > 100 * c["bar"][:M]).all())
    out = _check_rows(ops, c, 0, M, f"fp32_score/xent_{kind}_V{V}_d{d}_M{M}")
    # nll alone (NULL optional outputs) and a second run: the same bits
    assert torch.equal(ops.lm_head_xent(c["x"][:M].contiguous(), c["W"], c["tg"][:M].contiguous()), out[0])
    again = ops.lm_head_xent(c["x"][:M].contiguous(), c["W"], c["tg"][:M].contiguous(), want_parts=True)
    assert all(torch.equal(a, b) for a, b in zip(again, out))


@pytest.mark.parametrize("kind", S.XENT_SETS)
@pytest.mark.parametrize("V,d", [(331, 64), (2311, 256), (8327, 64)])
def test_xent_row_invariance(ops, V, d, kind):
    """a row's bits depend neither on M nor on which other rows are scored: 257 rows at once = 65 + 192 = row by row"""
    c = _case(ops, V, d, kind)
    x, W, tg = c["x"], c["W"], c["tg"]
    whole = ops.lm_head_xent(x, W, tg, want_parts=True)
    a = ops.lm_head_xent(x[:65].contiguous(), W, tg[:65].contiguous(), want_parts=True)
    b = ops.lm_head_xent(x[65:].contiguous(), W, tg[65:].contiguous(), want_parts=True)
    for i in range(4):
        assert torch.equal(torch.cat([a[i], b[i]]), whole[i]), i
    for r in (0, 5, 8, 64, 65, 127, 128, 200, 256):
        one = ops.lm_head_xent(x[r:r + 1].contiguous(), W, tg[r:r + 1].contiguous(), want_parts=True)
        for i in range(4):
            assert torch.equal(one[i], whole[i][r:r + 1]), (r, i)


def test_xent_row_chunks(ops):
    """more than 1024 rows: the second chunk reuses the workspace; same bits as the rows scored alone"""
    c = _case(ops, 331, 64, "random")
    x = c["x"].repeat(5, 1)[:1100].contiguous()
    tg = c["tg"].repeat(5)[:1100].contiguous()
    whole = ops.lm_head_xent(x, c["W"], tg, want_parts=True)
    ref = ops.lm_head_xent(c["x"], c["W"], c["tg"], want_parts=True)
    for i in range(4):
        assert torch.equal(whole[i], ref[i].repeat(5)[:1100]), i


def test_xent_edge_arguments(ops):
    from procyon_amd._lib import PcyError
    c = _case(ops, 2311, 256, "random")
    x, W, tg = c["x"], c["W"], c["tg"]
    assert ops.lm_head_xent(x[:0].contiguous(), W, tg[:0].contiguous()).shape == (0,)            # M == 0: nothing to do
    bad = tg[:4].clone()
    bad[1], bad[2] = 2311, -1                                                                     # no such column: NaN in that row only
    nll = ops.lm_head_xent(x[:4].contiguous(), W, bad)
    good = ops.lm_head_xent(x[:4].contiguous(), W, tg[:4].contiguous())
    assert math.isnan(float(nll[1])) and math.isnan(float(nll[2])) and torch.equal(nll[[0, 3]], good[[0, 3]])
    # a strided x (ldx > d): a column window of a wider buffer
    wide = torch.full((130, 256 + 64), float("nan"), device="cuda")
    wide[:, :256] = x[:130]
    view = wide[:, :256]
    assert view.stride(0) == 320 and not view.is_contiguous()
    got = ops.lm_head_xent(view, W, tg[:130].contiguous(), want_parts=True)
    ref = ops.lm_head_xent(x[:130].contiguous(), W, tg[:130].contiguous(), want_parts=True)
    assert all(torch.equal(a, b) for a, b in zip(got, ref))
    # refused: d % 16 != 0 (the library), rows the 16-byte loads cannot read, wrong dtypes (the wrapper)
    with pytest.raises(PcyError):
        ops.lm_head_xent(x[:4, :248].contiguous(), W[:, :248].contiguous(), tg[:4].contiguous())
    for bad_x in (torch.zeros(4, 257, device="cuda")[:, 1:], torch.zeros(4, 258, device="cuda")[:, :256], x[:4].double(), x[:4].cpu(),
                  torch.zeros(4, 512, device="cuda")[:, ::2]):
        with pytest.raises(TypeError):
            ops.lm_head_xent(bad_x, W, tg[:4].contiguous())
    with pytest.raises(TypeError):
        ops.lm_head_xent(x[:4].contiguous(), W, tg[:4].long())
    assert torch.equal(ops.lm_head_xent(x[:4].contiguous(), W, tg[:4].contiguous()), good)      # after the refusals the call still works


# ------------------------------------------------------------------------------------------------ attn_extend
def _per_head(out, ref, B, Sn, H, dh, key):
    e, m = R.rel64(out.cpu(), ref), R.maxabs64(out.cpu(), ref)
    record_parity(f"fp32_score/{key}", rel_err=f"{e:.3e}", max_abs_over_max=f"{m:.3e}")
    assert bool(out.isfinite().all()), key
    assert e <= R.OP_BAR and m < R.OP_MAXABS, (key, e, m)
    o, r = out.cpu().view(B, Sn, H, dh), ref.view(B, Sn, H, dh)
    for b in range(B):                                # per row and head: a swapped row, cache row or KV head is a large error on that slice
        for h in range(H):
            assert R.rel64(o[b, :, h], r[b, :, h]) <= R.OP_BAR, (key, b, h)


@pytest.mark.parametrize("H,Hkv,dh", S.EXT_GEOMS)
@pytest.mark.parametrize("Sn", S.EXT_S)
@pytest.mark.parametrize("t_past", S.EXT_TPAST)
def test_attn_extend(ops, t_past, Sn, H, Hkv, dh):
    """S new queries per row against t_past cached slots + the new keys: the 64-lane key stride below, at and above one pass; grouped heads;
    NaN in every cache slot >= t_past must not reach the output.  Plain, then with a key mask (one old and one new slot per row, and every key
    of one query: the keyless rule) and 4 rows mapped onto 2 cache rows."""
    c = S.extend_case(t_past, Sn, H, Hkv, dh)
    qkv, kc, vc = c["qkv"].cuda(), c["kc"].cuda(), c["vc"].cuda()
    scale = dh ** -0.5
    out = ops.attn_extend(qkv, Sn, kc, vc, t_past, H, Hkv, dh, scale)
    ref = S.attn_extend(c["qkv"], c["kc"], c["vc"], t_past, Sn, H, Hkv, dh, scale)
    _per_head(out, ref, S.EXT_B, Sn, H, dh, f"attn_extend[{t_past}+{Sn}-{H}x{Hkv}x{dh}]")
    out = ops.attn_extend(qkv, Sn, kc[:S.EXT_P].contiguous(), vc[:S.EXT_P].contiguous(), t_past, H, Hkv, dh, scale, keep=c["keep"].cuda(),
                          cache_rows=c["cache_row"].cuda())
    ref = S.attn_extend(c["qkv"], c["kc"], c["vc"], t_past, Sn, H, Hkv, dh, scale, keep=c["keep"], cache_row=c["cache_row"])
    _per_head(out, ref, S.EXT_B, Sn, H, dh, f"attn_extend_masked[{t_past}+{Sn}-{H}x{Hkv}x{dh}]")
    dead = S.keyless_queries(c["keep"], S.EXT_B, Sn, t_past)
    assert bool(dead[Sn]), "query 0 of row 1 has no kept key"
    assert R.rel64(out.cpu()[dead], ref[dead]) <= R.OP_BAR and R.rel64(out.cpu()[~dead], ref[~dead]) <= R.OP_BAR
    assert torch.equal(ops.attn_extend(qkv, Sn, kc[:S.EXT_P].contiguous(), vc[:S.EXT_P].contiguous(), t_past, H, Hkv, dh, scale, keep=c["keep"].cuda(),
                                       cache_rows=c["cache_row"].cuda()), out)


@pytest.mark.parametrize("H,Hkv,dh", S.EXT_GEOMS)
@pytest.mark.parametrize("t_past", S.EXT_TPAST)
def test_attn_extend_one_token_is_attn_decode(ops, t_past, H, Hkv, dh):
    """S == 1 without keep / cache_row: bit-equal to pcy_f32_attn_decode on the same cache with the new K / V written at slot t_past"""
    c = S.extend_case(t_past, 1, H, Hkv, dh)
    qkv, kc, vc = c["qkv"].cuda(), c["kc"].cuda(), c["vc"].cuda()
    out = ops.attn_extend(qkv, 1, kc, vc, t_past, H, Hkv, dh, dh ** -0.5)
    kc[:, t_past] = qkv[:, H * dh:(H + Hkv) * dh]
    vc[:, t_past] = qkv[:, (H + Hkv) * dh:]
    dec = ops.attn_decode(qkv[:, :H * dh], kc, vc, t_past + 1, H, Hkv, dh, dh ** -0.5)
    assert torch.equal(out, dec)


def test_attn_extend_refusals(ops):
    from procyon_amd import _lib
    from procyon_amd._lib import PcyError
    H, Hkv, dh = 1, 1, 16
    Tmax = 40960                                      # (16 + 40960 + 1) floats > 160 KB - 1 KB of LDS
    kc = torch.zeros(1, Tmax, dh, device="cuda")
    qkv = torch.zeros(1, 3 * dh, device="cuda")
    o = torch.full((1, dh), float("nan"), device="cuda")
    rc = ops.lib.pcy_f32_attn_extend(ops.h, _p(qkv), 3 * dh, _p(kc), _p(kc), dh, Tmax, None, None, 0, _p(o), dh, 1, 1, Tmax, H, Hkv, dh, 0.25)
    torch.cuda.synchronize()
    assert rc == 1 and b"LDS" in ops.lib.pcy_last_error() and bool(o.isnan().all())            # refused, nothing launched
    with pytest.raises(PcyError):
        ops.attn_extend(qkv, 1, kc, kc, Tmax, H, Hkv, dh, 0.25)
    with pytest.raises(PcyError):                                                               # more past than the cache holds
        ops.attn_extend(qkv, 1, kc[:, :8].contiguous(), kc[:, :8].contiguous(), 9, H, Hkv, dh, 0.25)
    small = kc[:, :8].contiguous()
    good = ops.attn_extend(qkv, 1, small, small, 4, H, Hkv, dh, 0.25)
    for bad in (qkv.double(), qkv.cpu(), torch.zeros(1, 6 * dh, device="cuda")[:, ::2], torch.zeros(2, 3 * dh + 1, device="cuda")[:, :3 * dh],
                torch.zeros(1, 2 * dh, device="cuda")):
        with pytest.raises(TypeError):
            ops.attn_extend(bad, 1, small, small, 4, H, Hkv, dh, 0.25)
    with pytest.raises(TypeError):
        ops.attn_extend(qkv, 1, small, small, 4, H, Hkv, dh, 0.25, keep=torch.ones(1, 5, device="cuda"))           # not uint8
    with pytest.raises(TypeError):
        ops.attn_extend(qkv, 1, small, small, 4, H, Hkv, dh, 0.25, keep=torch.ones(1, 4, dtype=torch.uint8, device="cuda"))   # too short
    with pytest.raises(ValueError):
        ops.attn_extend(qkv, 1, small, small, 4, H, Hkv, dh, 0.25, cache_rows=torch.tensor([1], dtype=torch.int32, device="cuda"))
    assert torch.equal(ops.attn_extend(qkv, 1, small, small, 4, H, Hkv, dh, 0.25), good)


# ------------------------------------------------------------------------------------------------ engine
@pytest.fixture(scope="module")
def eng_env():
    """the fp32 Llama of the engine tests (V 331, d 256, 3 layers, GQA 4/2) and one batch: B = 3, T = 41, row 1 left-padded by 7"""
    from oracle import llama_ref as LR
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig
    from procyon_amd.engine_f32 import LlamaEngineF32
    sd = synth.llama_state_dict(**R.GEN_GEOM, dtype=F32)
    geom = LR.LlamaGeom(**R.GEN_GEOM)
    eng = LlamaEngineF32(sd, LlamaConfig(**R.GEN_GEOM, max_pos=256))
    g = torch.Generator().manual_seed(3)
    B, T = 3, 41
    ids = torch.randint(0, R.GEN_GEOM["vocab"], (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, :7] = 0
    emb = F.embedding(ids, sd["model.embed_tokens.weight"])
    labels = ids.clone()
    labels[0, :20], labels[1, :30], labels[2, :9] = -100, -100, -100            # labels behind a chosen column
    labels[2, 35:] = -100
    ref = LR.llama_forward(sd, geom, inputs_embeds=emb, attn_mask=mask)["logits"]
    return dict(sd=sd, geom=geom, eng=eng, ids=ids, mask=mask, emb=emb, labels=labels, ref=ref, B=B, T=T, V=R.GEN_GEOM["vocab"])


def _oracle_bar(ref_rows, own_rows, targets):
    """(bar, D, oracle nll [n] float64-accurate fp32 cross entropy) for scored rows: 2 D + the operator's bar, D capped"""
    delta = float((ref_rows - own_rows).abs().max())
    assert delta <= R.OP_MAXABS * float(ref_rows.abs().max()), delta
    op_bar, _, _ = S.xent_bar(ref_rows, targets)
    return 2 * delta + float(op_bar.max()), delta


def test_engine_score_vs_oracle(eng_env):
    e = eng_env
    eng, B, T, V = e["eng"], e["B"], e["T"], e["V"]
    lab = e["labels"]
    labelled = lab[:, 1:] != -100
    token_nll, n, logits = eng.score(e["emb"].cuda(), e["mask"], lab, logit_rows="last")
    assert token_nll.dtype == F32 and token_nll.shape == (B, T) and n == int(labelled.sum()) and n > 30
    tn = token_nll.cpu()
    assert bool((tn[:, 0] == 0).all()) and bool((tn[:, 1:][~labelled] == 0).all()) and bool((tn[:, 1:][labelled] > 0).all())
    own_all, _ = eng.prefill(e["emb"].cuda(), e["mask"], "all")
    own = own_all.view(B, T, V).cpu()
    assert torch.equal(logits.cpu(), own[:, -1])                                                # the logit rows carry the bits of `prefill`
    ce = F.cross_entropy(e["ref"][:, :-1].reshape(-1, V), lab[:, 1:].reshape(-1), ignore_index=-100, reduction="none").view(B, T - 1)
    bar, delta = _oracle_bar(e["ref"][:, :-1][labelled], own[:, :-1][labelled], lab[:, 1:][labelled])
    err = float((tn[:, 1:][labelled] - ce[labelled]).abs().max())
    print(f"fp32 engine score vs oracle: err {err:.3e} D {delta:.3e} bar {bar:.3e}")
    record_parity("fp32_score/engine_score_vs_oracle", token_nll_err=f"{err:.3e}", delta=f"{delta:.3e}", bar=f"{bar:.3e}")
    assert err <= bar and bar < 0.05              # far below the ~ log V a shifted / mis-mapped row costs
    # the one-pass values again without logit rows; nothing to score: nothing runs
    t2, n2, lg2 = eng.score(e["emb"].cuda(), e["mask"], lab)
    assert torch.equal(t2, token_nll) and n2 == n and lg2 is None
    t0, n0, lg0 = eng.score(e["emb"].cuda(), e["mask"], torch.full_like(lab, -100))
    assert n0 == 0 and lg0 is None and not bool(t0.any())
    bad = lab.clone()
    bad[0, 30] = V
    with pytest.raises(ValueError):
        eng.score(e["emb"].cuda(), e["mask"], bad)


def test_engine_extend_vs_oracle_and_prefill(eng_env):
    """prefill 12 tokens (left pads {0, 5, 1}), then S = 5 more"""
    from oracle import llama_ref as LR
    e = eng_env
    eng, sd, geom, V = e["eng"], e["sd"], e["geom"], e["V"]
    TP, Sn = R.GEN_T, 5
    ids0, mask0 = R.gen_case()
    g = torch.Generator().manual_seed(5)
    ids = torch.cat([ids0, torch.randint(0, V, (R.GEN_B, Sn + 1), generator=g)], 1)
    mask = torch.cat([mask0, torch.ones(R.GEN_B, Sn, dtype=torch.long)], 1)
    emb = F.embedding(ids, sd["model.embed_tokens.weight"])
    B = R.GEN_B
    past = LR.llama_forward(sd, geom, inputs_embeds=emb[:, :TP], attn_mask=mask0)["past_kv"]
    ref = LR.llama_forward(sd, geom, inputs_embeds=emb[:, TP:TP + Sn], attn_mask=mask, past_kv=past)["logits"]
    cache = eng.new_cache(B, TP + Sn + 2)
    eng.prefill(emb[:, :TP].cuda(), mask0, None, cache=cache)
    labels = ids[:, TP:TP + Sn].clone()
    labels[1, :2] = -100
    snap = cache.k[:, :, :TP].clone(), cache.v[:, :, :TP].clone()
    logits, hidden, token_nll, n = eng.extend(cache, emb[:, TP:TP + Sn].cuda(), TP, keep=mask, logit_rows="all", labels=labels, want_hidden=True)
    lg = logits.view(B, Sn, V).cpu()
    whole = eng.new_cache(B, TP + Sn)
    full_lg, full_h = eng.prefill(emb[:, :TP + Sn].cuda(), mask, "all", want_hidden=True, cache=whole)
    full = full_lg.view(B, TP + Sn, V).cpu()[:, TP:]
    e_or, e_pf = R.rel64(lg, ref), R.rel64(lg, full)
    e_h = R.rel64(hidden.cpu(), full_h.cpu()[:, TP:])
    e_k = max(R.rel64(cache.k[:, :, TP:TP + Sn].cpu(), whole.k[:, :, TP:].cpu()), R.rel64(cache.v[:, :, TP:TP + Sn].cpu(), whole.v[:, :, TP:].cpu()))
    record_parity("fp32_score/engine_extend", err_oracle=f"{e_or:.3e}", err_prefill=f"{e_pf:.3e}", err_hidden=f"{e_h:.3e}", err_kv=f"{e_k:.3e}")
    assert e_or < 1e-4 and e_pf < 1e-4 and e_h < 1e-4 and e_k < 1e-4, (e_or, e_pf, e_h, e_k)
    assert torch.equal(cache.k[:, :, :TP], snap[0]) and torch.equal(cache.v[:, :, :TP], snap[1])   # the past is left alone
    # labels on the extension against `score` of the concatenation
    cat_labels = torch.cat([torch.full((B, TP), -100), labels], 1)
    cat_labels[:, TP] = -100                     # (the extension cannot score its first token: its predecessor's row is in the cache)
    t_cat, n_cat, _ = eng.score(emb[:, :TP + Sn].cuda(), mask, cat_labels)
    labelled = labels[:, 1:] != -100
    assert n == n_cat == int(labelled.sum()) and token_nll.shape == (B, Sn)
    bar, _ = _oracle_bar(ref[:, :-1][labelled], lg[:, :-1][labelled], labels[:, 1:][labelled])
    diff = float((token_nll.cpu() - t_cat.cpu()[:, TP:]).abs().max())
    ce = F.cross_entropy(ref[:, :-1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100, reduction="none").view(B, Sn - 1)
    err = float((token_nll.cpu()[:, 1:][labelled] - ce[labelled]).abs().max())
    record_parity("fp32_score/engine_extend_labels", vs_score=f"{diff:.3e}", vs_oracle=f"{err:.3e}", bar=f"{bar:.3e}")
    assert diff <= bar and err <= bar and bar < 0.05
    assert bool((token_nll.cpu()[:, 0] == 0).all()) and bool((token_nll.cpu()[:, 1:][~labelled] == 0).all())
    # a decode step on the extended cache: no mask after the prefill, as the reference decodes (it reads the pad slots of the 12-token prefill)
    nxt = ids[:, TP + Sn]
    r2 = LR.llama_forward(sd, geom, inputs_embeds=emb[:, TP:TP + Sn], attn_mask=mask, past_kv=past)["past_kv"]
    step_ref = LR.llama_forward(sd, geom, input_ids=nxt[:, None], attn_mask=None, past_kv=r2)["logits"][:, 0]
    step = eng.decode(cache, nxt, TP + Sn)
    e_step = R.rel64(step.cpu(), step_ref)
    assert e_step < 1e-4, e_step
    # capacity
    with pytest.raises(ValueError):
        eng.extend(cache, emb[:, :4].cuda(), TP + Sn)
    with pytest.raises(ValueError):
        eng.extend(cache, emb[:, :Sn].cuda(), TP, keep=mask[:, :TP])


def test_engine_extend_behind_vs_rows_one_by_one(eng_env):
    """2 left-padded prompts x 3 suffixes (right-padded) against the same rows run one by one: prefill of prompt + suffix under the joint mask"""
    e = eng_env
    eng, sd, V = e["eng"], e["sd"], e["V"]
    P, N, TP, Sn = 2, 3, 10, 6
    g = torch.Generator().manual_seed(9)
    pids = torch.randint(0, V, (P, TP), generator=g)
    pmask = torch.ones(P, TP, dtype=torch.long)
    pmask[1, :4] = 0
    sids = torch.randint(0, V, (P * N, Sn), generator=g)
    smask = torch.ones(P * N, Sn, dtype=torch.long)
    for r, ln in enumerate((6, 3, 5, 2, 6, 4)):
        smask[r, ln:] = 0
    labels = torch.where(smask.bool(), sids, torch.full_like(sids, -100))
    tab = sd["model.embed_tokens.weight"]
    logits, _, token_nll, n, cache = eng.extend_behind(F.embedding(pids, tab).cuda(), pmask, F.embedding(sids, tab).cuda(), smask,
                                                       rows_per_prefix=N, logit_rows="all", labels=labels)
    assert cache.B == P and cache.Tmax == TP and n == int((labels[:, 1:] != -100).sum())           # the prompts were prefilled ONCE each
    lg = logits.view(P * N, Sn, V).cpu()
    worst = worst_nll = 0.0
    for r in range(P * N):
        p, ln = r // N, int(smask[r].sum())
        ids = torch.cat([pids[p], sids[r, :ln]])[None]
        m = torch.cat([pmask[p], torch.ones(ln, dtype=torch.long)])[None]
        lab = torch.cat([torch.full((TP + 1,), -100), sids[r, 1:ln]])[None]      # (the extension does not score its first token)
        one, _ = eng.prefill(F.embedding(ids, tab).cuda(), m, "all")
        one = one.cpu()[TP:]
        worst = max(worst, R.rel64(lg[r, :ln], one))
        t1, _, _ = eng.score(F.embedding(ids, tab).cuda(), m, lab)
        diff = float((token_nll[r, :ln].cpu() - t1.cpu()[0, TP:]).abs().max())
        assert not bool(token_nll[r, ln:].any()) and not bool(token_nll[r, 0])
        if ln > 1:      # the same 1-Lipschitz bound between the two engine paths: 2 x their logit distance + the operator's bar on these logits
            bar = 2 * float((lg[r, :ln] - one).abs().max()) + float(S.xent_bar(one[:ln - 1], sids[r, 1:ln])[0].max())
            assert diff <= bar and bar < 0.05, (r, diff, bar)
        worst_nll = max(worst_nll, diff)
    record_parity("fp32_score/engine_extend_behind", err_logits=f"{worst:.3e}", nll_diff=f"{worst_nll:.3e}")
    assert worst < 1e-4
    with pytest.raises(TypeError):
        eng.extend_behind(F.embedding(pids, tab).cuda(), pmask, F.embedding(sids, tab).cuda(), smask, rows_per_prefix=N, groups=([3, 3], [TP, TP]))


# ------------------------------------------------------------------------------------------------ model
INSTR = ["w1 <|protein|> is w2 ? [ANSWER] yes w3 w4 w5",
         "w4 <|protein|> ? [ANSWER] alpha beta gamma delta epsilon zeta eta",
         "describe w8 <|protein|> and <|protein|> now please [ANSWER] q r"]
SLOTS = [[0], [1], [0, 1]]


@pytest.fixture(scope="module")
def menv():
    from oracle import esm_ref as ER
    from oracle import llama_ref as LR
    from procyon_amd import synth
    from procyon_amd import synthetic_model as SM
    m, w = SM.build("small", device="cuda", return_weights=True, max_new_tokens=8, dtype=F32, as_loaded=True)
    m.eval()
    assert m.dtype == F32
    return dict(model=m, w=w, prot=synth.protein_tokens([90, 41], seed=3), lgeom=LR.LlamaGeom(**w["geom"]["llama"]),
                egeom=ER.EsmGeom(**w["geom"]["esm"]))


def _inputs(env, instr=INSTR, slots=SLOTS):
    prot = env["prot"]
    return {"data": {"seq": prot, "seq_idx": torch.arange(prot.shape[0]), "text": [], "drug": None},
            "input": {"seq": [list(s) for s in slots], "text": [[] for _ in instr], "drug": None},
            "target": {"seq": None, "text": None, "drug": None}, "instructions": list(instr)}


def _oracle_logits(env, inputs):
    from oracle import llama_ref as LR
    from oracle import procyon_ref as PR
    m, w = env["model"], env["w"]
    z = PR.esm_plm_forward(w["esm"], env["egeom"], inputs["data"]["seq"], pooling="mean")
    idx = [i for row in inputs["input"]["seq"] for i in row]
    soft = PR.mlp_forward(z[idx], w["projs"]["aaseq"])
    ids, mask = m._prepare_text_inputs_and_tokenize(list(inputs["instructions"]), [[] for _ in inputs["instructions"]], crop_off=True,
                                                    no_pad=False, left_pad=False)
    emb, _ = PR.prepare_input_embeddings(w["llama"]["model.embed_tokens.weight"], ids.long(), m.prot_replacement_idx, soft,
                                         ret_idx=m.prot_retrieval_idx)
    real = int(mask.sum(1).max())
    return LR.llama_forward(w["llama"], env["lgeom"], inputs_embeds=emb[:, :real], attn_mask=mask[:, :real])["logits"], real


@pytest.fixture(scope="module")
def mscored(menv):
    """the one-pass scoring forward of the three prompts, the oracle's logits and the bar against them, once"""
    m = menv["model"]
    out = m.forward(_inputs(menv), compute_loss=True, get_full_labels=True)
    o = out["outputs"]
    real = o.token_nll.shape[1]
    lab = out["full_labels"][:, :real]
    labelled = lab[:, 1:] != -100
    lg_ref, real_ref = _oracle_logits(menv, _inputs(menv))
    assert real_ref == real
    own = m.forward(_inputs(menv), full_logits=True)["outputs"].logits.cpu()
    bar, delta = _oracle_bar(lg_ref[:, :-1][labelled], own[:, :-1][labelled], lab[:, 1:][labelled])
    return dict(out=out, o=o, real=real, lab=lab, labelled=labelled, lg_ref=lg_ref, bar=bar, delta=delta)


def test_model_loss_vs_oracle(menv, mscored):
    m = menv["model"]
    o, real, lab, labelled, lg_ref, bar, delta = (mscored[k] for k in ("o", "real", "lab", "labelled", "lg_ref", "bar", "delta"))
    assert o.token_nll.dtype == F32 and o.token_nll.shape == (3, real) and o.n_tokens == int(labelled.sum()) >= 4 + 7 + 2
    assert o.loss.dim() == 0 and torch.equal(o.loss, o.token_nll.sum(1).sum() / o.n_tokens)
    lazy = m.forward(_inputs(menv), get_full_labels=True)["outputs"]            # the lazy `.loss`: a second, deterministic pass
    assert torch.equal(lazy.answer_logits, o.answer_logits)
    assert torch.equal(lazy.loss, o.loss) and torch.equal(lazy.token_nll, o.token_nll) and lazy.n_tokens == o.n_tokens
    V = lg_ref.shape[-1]
    ce = F.cross_entropy(lg_ref[:, :-1].reshape(-1, V), lab[:, 1:].reshape(-1), ignore_index=-100, reduction="none").view(3, real - 1)
    loss_ref = F.cross_entropy(lg_ref[:, :-1].reshape(-1, V), lab[:, 1:].reshape(-1), ignore_index=-100)
    err_tok = float((o.token_nll.cpu()[:, 1:][labelled] - ce[labelled]).abs().max())
    err_loss = abs(float(o.loss) - float(loss_ref))
    record_parity("fp32_score/model_loss_vs_oracle", token_nll_err=f"{err_tok:.3e}", loss_err=f"{err_loss:.3e}", delta=f"{delta:.3e}", bar=f"{bar:.3e}")
    assert err_tok <= bar and err_loss <= bar and bar < 0.05
    # without labels `.loss` stays None; nothing labelled: NaN loss, n_tokens == 0
    enc = m.text_encoder
    emb = torch.randn(1, 5, enc.cfg.d, device="cuda")
    assert enc(input_embeds=emb, lazy_hidden=True).loss is None
    none = enc(input_embeds=emb, full_labels=torch.full((1, 5), -100), compute_loss=True, lazy_hidden=True)
    assert math.isnan(float(none.loss)) and none.n_tokens == 0 and not bool(none.token_nll.any())
    # score_text: the dictionary of tests/test_gpu_score.py::test_score_text
    s = m.score_text(_inputs(menv))
    assert torch.equal(s["token_nll"], o.token_nll) and torch.equal(s["loss"], o.loss)
    assert s["seq_nll"].shape == (3,) and s["n_tokens"].tolist() == labelled.sum(1).tolist()
    assert torch.equal(s["seq_nll"].sum() / int(s["n_tokens"].sum()), s["loss"]) and torch.equal(s["perplexity"], torch.exp(s["loss"]))


def test_model_score_candidates_vs_score_text(menv, mscored):
    m = menv["model"]
    bar = mscored["bar"]
    prompts = [i.split("[ANSWER]")[0] + "[ANSWER]" for i in INSTR[:2]]
    cands = [["yes w3 w4 w5", "w7 w8", "alpha beta gamma delta epsilon zeta eta theta iota"] for _ in prompts]
    res = m.score_candidates(_inputs(menv, instr=prompts, slots=SLOTS[:2]), cands, packed=True)       # packed: accepted and ignored
    Sn = res["plan"]["S"]
    assert res["token_nll"].shape == (2, 3, Sn) and res["token_nll"].dtype == F32 and res["cache"].B == 2      # the prompts were prefilled ONCE each
    rows = [p + " " + c for p, cs in zip(prompts, cands) for c in cs]
    st = m.score_text(_inputs(menv, instr=rows, slots=[s for s in SLOTS[:2] for _ in range(3)]))
    n_ref = st["n_tokens"].view(2, 3).cpu()
    assert torch.equal(res["n_tokens"].cpu(), n_ref)
    # every row's token_nll: the labelled tokens in order (the two layouts pad differently)
    worst = 0.0
    for r in range(6):
        a = res["token_nll"].view(6, Sn)[r].cpu()
        b = st["token_nll"][r].cpu()
        a, b = a[a != 0], b[b != 0]
        assert a.numel() == b.numel() == int(n_ref.view(-1)[r])
        worst = max(worst, float((a - b).abs().max()))
    record_parity("fp32_score/score_candidates_vs_score_text", token_nll_diff=f"{worst:.3e}", bar=f"{bar:.3e}")
    assert worst <= bar
    assert torch.equal(res["mean_nll"], res["seq_nll"] / res["n_tokens"])
    mean_ref = (st["seq_nll"].view(2, 3).cpu() / n_ref)
    gaps = mean_ref.sort(1).values.diff(dim=1)
    assert float(gaps.min()) > 2 * bar, "the candidates do not differ by a clear margin"
    assert torch.equal(res["order"].cpu(), torch.argsort(mean_ref, dim=1, stable=True))


def test_text_encoder_hf_contract_on_an_fp32_past(menv):
    from procyon_amd.model.pmc_llama import _PastF32
    m = menv["model"]
    enc = m.text_encoder
    eng = enc.engine_f32
    g = torch.Generator().manual_seed(21)
    B, T = 2, 9
    ids = torch.randint(0, 2000, (B, T + 4), generator=g)
    mask = torch.ones(B, T, dtype=torch.long)
    mask[1, :3] = 0
    emb = eng.embed_tokens(ids)
    out = enc(input_embeds=emb[:, :T], attn_masks=mask, use_cache=True, logit_positions=torch.tensor([T - 1, T - 1]))
    past = out.past_key_values
    assert isinstance(past, _PastF32) and past.t == T
    # [B,1]: still the decode step, bit for bit
    snap = past.cache.k.clone(), past.cache.v.clone()
    step = enc(input_ids=ids[:, T:T + 1], past_key_values=past)
    ref_cache = eng.new_cache(B, past.cache.Tmax)
    ref_cache.k.copy_(snap[0]); ref_cache.v.copy_(snap[1])
    assert torch.equal(step.logits[:, 0], eng.decode(ref_cache, ids[:, T], T)) and step.past_key_values.t == T + 1 and step.loss is None
    # [B,3] with the fp32 past: the extension, against one prefill over everything
    full_mask = torch.cat([mask, torch.ones(B, 4, dtype=torch.long)], 1)
    labels = ids[:, T + 1:T + 4]
    ext = enc(input_ids=ids[:, T + 1:T + 4], past_key_values=step.past_key_values, attn_masks=full_mask, full_labels=labels, compute_loss=True)
    assert ext.logits.shape == (B, 3, enc.cfg.vocab) and ext.logits.dtype == F32 and ext.past_key_values.t == T + 4
    whole = enc(input_embeds=emb, attn_masks=full_mask)      # (row 1 is left-padded: its unmasked decode step read the pad slots, the prefill does not)
    assert R.rel64(ext.logits.cpu()[0], whole.logits.cpu()[0, T + 1:]) < 1e-4 and bool(ext.logits.isfinite().all())
    assert ext.n_tokens == 2 * B and ext.token_nll.shape == (B, 3) and float(ext.loss) > 0
    lazy = enc(input_embeds=emb[:, T + 1:T + 4], past_key_values=step.past_key_values, attn_masks=full_mask, full_labels=labels,
               logit_positions=torch.tensor([2, 2]))
    assert torch.equal(lazy.logits[:, 0], ext.logits[:, 2]) and torch.equal(lazy.loss, ext.loss) and torch.equal(lazy.token_nll, ext.token_nll)
    with pytest.raises(ValueError):                                                              # capacity
        enc(input_ids=ids[:, :9], past_key_values=ext.past_key_values)
    # fp32 embeds with a bf16 past remain an error
    bf_past = enc(input_ids=ids[:, :T], use_cache=True).past_key_values
    assert not isinstance(bf_past, _PastF32)
    with pytest.raises(RuntimeError):
        enc(input_embeds=emb[:, T:T + 2], past_key_values=bf_past)


def test_fp32_model_keeps_its_refusals(menv):
    m = menv["model"]
    prompts = [i.split("[ANSWER]")[0] + "[ANSWER]" for i in INSTR[:2]]
    with pytest.raises(NotImplementedError):
        m.score_candidates(_inputs(menv, instr=prompts, slots=SLOTS[:2]), [["a"], ["b", "c"]], ragged=True)
    with pytest.raises(NotImplementedError, match="bf16 engine"):
        m.forward(_inputs(menv), share_prefix=True)
    with pytest.raises(NotImplementedError, match="bf16 engine"):
        m.generate(_inputs(menv, instr=prompts[:1], slots=SLOTS[:1]), max_len=4, method="greedy", lookahead=4)
