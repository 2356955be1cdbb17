"""CPU: the float64 references of tests/f32_score_ref.py against the oracle (`oracle.llama_ref.llama_forward(..., past_kv=...)`,
`F.cross_entropy`), plain torch fp32 on the same inputs under the same bars, the workspace arithmetic of `pcy_f32_lm_head_xent`, and
the declarations / ctypes signatures of the two new entry points."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import f32_ref as R
import f32_score_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64


@pytest.mark.parametrize("kind", S.XENT_SETS)
@pytest.mark.parametrize("V,d", [(331, 64), (2311, 256)])
def test_xent_reference_is_cross_entropy(V, d, kind):
    x, W, tg = S.xent_case(V, d, kind)
    L = (x @ W.T).float()
    nll, lse, mx, lab = S.lm_head_xent(L, tg)
    assert torch.allclose(nll, F.cross_entropy(L.double(), tg, reduction="none"), rtol=0, atol=1e-12)
    assert torch.allclose(lse, torch.logsumexp(L.double(), -1), rtol=0, atol=1e-12)
    assert torch.equal(mx, L.double().max(-1).values) and torch.equal(lab, L.double().gather(1, tg[:, None])[:, 0])
    # plain torch fp32 (and the restatement evaluated in fp32) meet the bar the GPU operator is held to
    bar, err_a, _ = S.xent_bar(L, tg)
    nll32, lse32, _, _ = S.lm_head_xent(L, tg, dt=F32)
    assert bool(((nll32.double() - nll).abs() <= bar).all()) and bool(((lse32.double() - lse).abs() <= bar).all())
    assert err_a <= float(bar.min())
    # the planted sets make the faults of a ragged row reduction cost more than the bar
    dropped, padded = S.fault_costs(L)
    if kind == "negative":
        assert bool((L <= -18).all()) and bool((L >= -22).all())
        assert bool((padded > 100 * bar).all()) and float(padded.min()) > 1.0
    if kind == "peaked":
        assert 85 <= float(L.max()) <= 92 + 3
        assert bool((dropped > 100 * bar).all()) and float(dropped.min()) > 1.0


def test_xent_reference_bad_targets():
    L = R.rnd(4, 9, seed=5)
    tg = torch.tensor([0, 9, -1, 8])
    nll, _, _, lab = S.lm_head_xent(L, tg)
    assert nll.isnan().tolist() == [False, True, True, False] and lab.isnan().tolist() == [False, True, True, False]


def test_ws_bytes_arithmetic():
    """host arithmetic only: callable without a device"""
    import __graft_entry__ as g
    g.build()
    from procyon_amd import _lib
    lib = _lib.load()
    for V in (331, 2311, 8327, 65543, 65671, 65799, 128263):
        cb, ncb = S.col_blocks(V)
        assert ncb <= S.MAX_BLOCKS and cb * ncb * S.TILE >= V > cb * (ncb - 1) * S.TILE
        for M in (1, 130, 1024, 1025, 32768):
            got = lib.pcy_f32_lm_head_xent_ws_bytes(M, V)
            assert got == S.ws_bytes(M, V) and got <= min(M, 1024) * (ncb * 8 + 4), (M, V, got)
    assert lib.pcy_f32_lm_head_xent_ws_bytes(0, 331) == 0
    # the saving against [M, V] fp32 logits
    assert lib.pcy_f32_lm_head_xent_ws_bytes(32768, 128263) * 1000 <= 32768 * 128263 * 4
    # the partitions the GPU test relies on
    assert S.col_blocks(2311) == (1, 19) and S.col_blocks(8327) == (1, 66) and S.col_blocks(65543) == (2, 257) and S.col_blocks(65671) == (2, 257)


def test_new_symbols_declared_and_bound():
    from procyon_amd import _lib
    src = open(os.path.join(ROOT, "include", "pcy.h")).read()
    for name, nargs in (("pcy_f32_lm_head_xent", 12), ("pcy_f32_lm_head_xent_ws_bytes", 2), ("pcy_f32_attn_extend", 19)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", src)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, (name, m.group(1))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
    assert _lib.ABI_VERSION == 13 and "#define PCY_ABI_VERSION 13" in src.replace("  ", " ")


# ------------------------------------------------------------------------------------------------ cache extension against the oracle
def _oracle_layer_with(attn, sd, geom, emb_new, past, t_past, keep):
    """one decoder layer + final norm + lm_head over the new tokens, restated from the oracle's primitives with `attn` in the place of its
    attention: the logits llama_forward(..., past_kv=...) must give"""
    from oracle import llama_ref as LR
    B, S_, _ = emb_new.shape
    H, Hkv, dh = geom.n_heads, geom.n_kv_heads, geom.dh
    lw = LR._layer_weights(sd, 0)
    cos_t, sin_t = LR.rope_tables(geom, emb_new.dtype, t_past + S_)
    cos, sin = cos_t[t_past:][None].expand(B, S_, -1), sin_t[t_past:][None].expand(B, S_, -1)
    x = LR.rms_norm(emb_new, lw["input_layernorm.weight"], geom.rms_eps, geom.rms_cast)
    q = F.linear(x, lw["self_attn.q_proj.weight"]).view(B, S_, H, dh).transpose(1, 2)
    k = F.linear(x, lw["self_attn.k_proj.weight"]).view(B, S_, Hkv, dh).transpose(1, 2)
    v = F.linear(x, lw["self_attn.v_proj.weight"]).view(B, S_, Hkv, dh)
    q, k = LR.apply_rope(q, k, cos, sin)
    qkv = torch.cat([q.transpose(1, 2).reshape(B * S_, H * dh), k.transpose(1, 2).reshape(B * S_, Hkv * dh), v.reshape(B * S_, Hkv * dh)], 1)
    kc = past[0][0].transpose(1, 2).reshape(B, t_past, Hkv * dh)            # token-major, as the fp32 cache holds them
    vc = past[0][1].transpose(1, 2).reshape(B, t_past, Hkv * dh)
    o = attn(qkv, kc, vc, t_past, S_, H, Hkv, dh, dh ** -0.5, keep=keep).to(emb_new.dtype).view(B, S_, H * dh)
    h = emb_new + F.linear(o, lw["self_attn.o_proj.weight"])
    x = LR.rms_norm(h, lw["post_attention_layernorm.weight"], geom.rms_eps, geom.rms_cast)
    h = h + F.linear(F.silu(F.linear(x, lw["mlp.gate_proj.weight"])) * F.linear(x, lw["mlp.up_proj.weight"]), lw["mlp.down_proj.weight"])
    return F.linear(LR.rms_norm(h, sd["model.norm.weight"], geom.rms_eps, geom.rms_cast), sd["lm_head.weight"])


@pytest.mark.parametrize("t_past,S_", [(0, 5), (7, 1), (7, 5)])
def test_attn_extend_reference_is_the_oracles_cached_forward(t_past, S_):
    """one fp32 layer, GQA 4/2: a left-padded row, a masked new key, and a row whose first new query has no kept key at all"""
    from oracle import llama_ref as LR
    from procyon_amd import synth
    kw = dict(vocab=97, d=128, n_layers=1, n_heads=4, n_kv_heads=2, ffn=256)
    sd, geom = synth.llama_state_dict(**kw, dtype=F32), LR.LlamaGeom(**kw)
    B = 3
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(0, 97, (B, t_past + S_), generator=g)
    emb = F.embedding(ids, sd["model.embed_tokens.weight"])
    mask = torch.ones(B, t_past + S_, dtype=torch.long)
    mask[1, :t_past + 1] = 0                                      # row 1: every key up to its first new one is masked
    if t_past > 2:
        mask[2, :2] = 0                                           # row 2: left pads
    if S_ > 2:
        mask[0, t_past + 2] = 0                                   # row 0: a masked new key
    past = None
    if t_past:
        past = LR.llama_forward(sd, geom, inputs_embeds=emb[:, :t_past], attn_mask=mask[:, :t_past])["past_kv"]
        ref = LR.llama_forward(sd, geom, inputs_embeds=emb[:, t_past:], attn_mask=mask, past_kv=past)["logits"]
    else:
        ref = LR.llama_forward(sd, geom, inputs_embeds=emb, attn_mask=mask)["logits"]
        past = [(torch.zeros(B, 2, 0, geom.dh), torch.zeros(B, 2, 0, geom.dh))]
    assert bool(S.keyless_queries(mask, B, S_, t_past).view(B, S_)[1, 0])
    for dt in (F64, F32):
        got = _oracle_layer_with(lambda *a, **k: S.attn_extend(*a, **k, dt=dt), sd, geom, emb[:, t_past:], past, t_past, mask)
        e = R.rel64(got, ref)
        assert e <= R.OP_BAR and R.maxabs64(got, ref) < R.OP_MAXABS, (dt, e)


@pytest.mark.parametrize("t_past,S_", [(0, 1), (1, 5), (64, 66)])
def test_attn_extend_plain_fp32_meets_the_bars(t_past, S_):
    """the input set of the GPU test, evaluated in fp32 by plain torch: the bars are reachable; S == 1 without mask is the decode reference"""
    H, Hkv, dh = 8, 2, 64
    c = S.extend_case(t_past, S_, H, Hkv, dh)
    for keep, cr in ((None, None), (c["keep"], c["cache_row"])):
        a = (c["qkv"], c["kc"], c["vc"], t_past, S_, H, Hkv, dh, dh ** -0.5)
        ref = S.attn_extend(*a, keep=keep, cache_row=cr)
        got = S.attn_extend(*a, keep=keep, cache_row=cr, dt=F32)
        assert bool(ref.isfinite().all())
        assert R.rel64(got, ref) <= R.OP_BAR and R.maxabs64(got, ref) < R.OP_MAXABS
    if S_ == 1:
        kc, vc = c["kc"].clone(), c["vc"].clone()
        kc[:, t_past] = c["qkv"][:, H * dh:(H + Hkv) * dh]
        vc[:, t_past] = c["qkv"][:, (H + Hkv) * dh:]
        dec = R.attn_decode(c["qkv"][:, :H * dh], kc, vc, t_past + 1, H, Hkv, dh, dh ** -0.5)
        assert R.rel64(S.attn_extend(c["qkv"], c["kc"], c["vc"], t_past, 1, H, Hkv, dh, dh ** -0.5), dec) < 1e-14
