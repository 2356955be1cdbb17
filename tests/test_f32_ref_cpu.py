"""CPU: the float64 references of tests/f32_ref.py, which the GPU operator tests (tests/test_gpu_fp32_ops.py) compare against.
(a) each agrees with the oracle's fp32 function it restates to <= 1e-6 (norm-wise relative) on the test inputs;
(b) on every input set the GPU tests use, the same operator evaluated in plain torch fp32 stays within the GPU bar of the float64
    reference -- the bar is reachable by an fp32 implementation at these inputs;
(c) the padded-generation inputs can see a prefill attention that zeroes key-less query rows: the oracle with that defect moves more
    than 100 x the 1e-4 stack bar from the oracle proper on a padded row at decode step 1."""
import pytest
import torch
import torch.nn.functional as F

import f32_ref as R
from oracle import esm_ref as ER
from oracle import llama_ref as LR
from oracle import procyon_ref as PR

F32 = torch.float32
AGREE = 1e-6


def _oracle_attention(q, k, v, cu, keep, H, Hkv, dh, causal, scale):
    """the attention inside llama_ref.layer_forward (scores, additive finfo.min mask, fp32 softmax, P . V) in fp32, one sequence at a
    time; the mask is build_additive_mask (causal) or the key-padding mask of esm_ref.esm_forward (bidirectional)"""
    out = torch.zeros(q.shape[0], H * dh)
    g = H // Hkv
    for s_ in range(cu.numel() - 1):
        t0, t1 = int(cu[s_]), int(cu[s_ + 1])
        n = t1 - t0
        qq = q[t0:t1].view(1, n, H, dh).transpose(1, 2)
        kk = k[t0:t1].view(1, n, Hkv, dh).transpose(1, 2)
        vv = v[t0:t1].view(1, n, Hkv, dh).transpose(1, 2)
        kk = kk[:, :, None].expand(1, Hkv, g, n, dh).reshape(1, H, n, dh)
        vv = vv[:, :, None].expand(1, Hkv, g, n, dh).reshape(1, H, n, dh)
        if causal:
            add = LR.build_additive_mask(None if keep is None else keep[None, t0:t1], 1, n, 0, F32)
        else:
            add = torch.where(keep[t0:t1].bool()[None, None, None, :], torch.zeros((), dtype=F32), torch.full((), torch.finfo(F32).min, dtype=F32))
        s = torch.matmul(qq, kk.transpose(2, 3)) * scale + add
        p = F.softmax(s, dim=-1, dtype=torch.float32)
        out[t0:t1] = torch.matmul(p, vv).transpose(1, 2).reshape(n, H * dh)
    return out


def _within_bar(lo, ref, what, maxabs=True):
    e = R.rel64(lo, ref)
    assert e <= R.OP_BAR, (what, e)
    if maxabs:
        assert R.maxabs64(lo, ref) <= R.OP_MAXABS, (what, R.maxabs64(lo, ref))


# ------------------------------------------------------------------------------------------------ linear
@pytest.mark.parametrize("name", list(R.LINEAR_CASES))
@pytest.mark.parametrize("mode", R.LINEAR_MODES)
def test_linear_ref(name, mode):
    c = R.linear_case(name)
    bias, resid, act = R.linear_args(c, mode)
    ref = R.linear(c["A"], c["W"], bias, resid, act)
    orc = F.linear(c["A"], c["W"], bias)
    orc = F.gelu(orc) if act else orc
    orc = orc + resid if resid is not None else orc
    assert R.rel64(orc, ref) <= AGREE
    _within_bar(R.linear(c["A"], c["W"], bias, resid, act, dt=F32), ref, (name, mode))


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("d", R.NORM_DIMS)
def test_norm_refs(d):
    c = R.norm_case(d)
    ln, rms = R.layernorm(c["x"], c["w"], c["b"], c["eps"]), R.rmsnorm(c["x"], c["w"], c["eps"])
    assert R.rel64(F.layer_norm(c["x"], (d,), c["w"], c["b"], c["eps"]), ln) <= AGREE
    assert R.rel64(LR.rms_norm(c["x"], c["w"], c["eps"]), rms) <= AGREE
    _within_bar(R.layernorm(c["x"], c["w"], c["b"], c["eps"], dt=F32), ln, ("layernorm", d))
    _within_bar(R.rmsnorm(c["x"], c["w"], c["eps"], dt=F32), rms, ("rmsnorm", d))


# ------------------------------------------------------------------------------------------------ rope
@pytest.mark.parametrize("nh,dh", R.ROPE_GEOMS)
@pytest.mark.parametrize("prescale", [0.0, 0.125])
def test_rope_ref(nh, dh, prescale):
    c = R.rope_case(nh, dh)
    T, c0 = c["buf"].shape[0], R.ROPE_COL0
    ref = R.rope(c["buf"], c0, nh, dh, c["pos"], c["cos"], c["sin"], prescale)
    assert torch.equal(ref[:, :c0], c["buf"][:, :c0].double()) and torch.equal(ref[:, c0 + nh * dh:], c["buf"][:, c0 + nh * dh:].double())
    cos_o, sin_o = LR.rope_tables(LR.LlamaGeom(vocab=1, d=nh * dh, n_layers=1, n_heads=nh, n_kv_heads=nh, ffn=1), F32, R.ROPE_NPOS)
    assert torch.equal(cos_o, c["cos"]) and torch.equal(sin_o, c["sin"])
    x = c["buf"][:, c0:c0 + nh * dh].view(1, T, nh, dh).transpose(1, 2)
    x = x * prescale if prescale else x
    qo, _ = LR.apply_rope(x, x, cos_o[c["pos"].long()][None], sin_o[c["pos"].long()][None])
    assert R.rel64(qo.transpose(1, 2).reshape(T, nh * dh), ref[:, c0:c0 + nh * dh]) <= AGREE
    _within_bar(R.rope(c["buf"], c0, nh, dh, c["pos"], c["cos"], c["sin"], prescale, dt=F32), ref, ("rope", nh, dh, prescale))


# ------------------------------------------------------------------------------------------------ attention
@pytest.mark.parametrize("causal", [True, False])
def test_attention_ref(causal):
    c = R.attn_case()
    H, Hkv, dh = R.ATTN_GEOM
    q, k, v = R.attn_windows(c["qkv"])
    if not causal:                        # bidirectional: every sequence keeps a key (a sequence of pads only has no reference value)
        assert all(int(c["keep"][int(a):int(b)].sum()) > 0 for a, b in zip(c["cu"][:-1], c["cu"][1:]))
    ref = R.attention(q, k, v, c["cu"], c["keep"], H, Hkv, dh, causal, dh ** -0.5)
    orc = _oracle_attention(q, k, v, c["cu"], c["keep"], H, Hkv, dh, causal, dh ** -0.5)
    dead = R.keyless_rows(c["cu"], c["keep"], causal)
    assert int(dead.sum()) == (sum(R.ATTN_PADS) if causal else 0)
    assert R.rel64(orc, ref) <= AGREE
    if causal:                            # the uniform rule, on its rows alone
        assert R.rel64(orc[dead], ref[dead]) <= AGREE
        t0 = int(c["cu"][3])
        assert R.rel64(ref[t0, :dh], v[t0:t0 + 65, :dh].double().mean(0)) <= 1e-12
    _within_bar(R.attention(q, k, v, c["cu"], c["keep"], H, Hkv, dh, causal, dh ** -0.5, dt=F32), ref, ("attention", causal))


@pytest.mark.parametrize("H,Hkv,dh", R.DECODE_GEOMS)
@pytest.mark.parametrize("nkeys", R.DECODE_NKEYS)
def test_attn_decode_ref(nkeys, H, Hkv, dh):
    c = R.decode_case(nkeys, H, Hkv, dh)
    q = c["qkv"][:, :H * dh]
    ref = R.attn_decode(q, c["kc"], c["vc"], nkeys, H, Hkv, dh, dh ** -0.5)
    assert bool(ref.isfinite().all())
    # the oracle's attention with a one-token query: per row, the query as the last of nkeys tokens of a causal sequence
    B = q.shape[0]
    for b in range(B):
        qq = torch.zeros(nkeys, H * dh)
        qq[-1] = q[b]
        cu = torch.tensor([0, nkeys], dtype=torch.int32)
        orc = _oracle_attention(qq, c["kc"][b, :nkeys], c["vc"][b, :nkeys], cu, None, H, Hkv, dh, True, dh ** -0.5)[-1]
        assert R.rel64(orc, ref[b]) <= AGREE
    _within_bar(R.attn_decode(q, c["kc"], c["vc"], nkeys, H, Hkv, dh, dh ** -0.5, dt=F32), ref, ("attn_decode", nkeys, H, Hkv, dh))


# ------------------------------------------------------------------------------------------------ ESM embedding, pooling
@pytest.mark.parametrize("d", [320, 100])
@pytest.mark.parametrize("mask_pads,pads", R.ESM_VARIANTS)
def test_esm_embed_ref(d, mask_pads, pads):
    c = R.esm_case(d, pads)
    ref = R.esm_embed(c["table"], c["tokens"], c["cu"], mask_pads)
    sd = {"esm.embeddings.word_embeddings.weight": c["table"]}
    orc = torch.cat([ER.embed(sd, c["tokens"][int(a):int(b)][None].long(), F32, mask_pads=bool(mask_pads))[0]
                     for a, b in zip(c["cu"][:-1], c["cu"][1:])])
    assert R.rel64(orc, ref) <= AGREE
    zero = (c["tokens"] == R.MASK_ID) | ((c["tokens"] == R.PAD_ID) if mask_pads else torch.zeros_like(c["tokens"], dtype=torch.bool))
    assert bool((ref[zero] == 0).all()) and bool((ref[~zero].abs().sum(-1) > 0).all())
    assert int((c["tokens"] == R.PAD_ID).sum()) > 0 if pads else int((c["tokens"] == R.PAD_ID).sum()) == 0
    _within_bar(R.esm_embed(c["table"], c["tokens"], c["cu"], mask_pads, dt=F32), ref, ("esm_embed", d, mask_pads, pads))


@pytest.mark.parametrize("d", R.POOL_DIMS)
@pytest.mark.parametrize("mode,nan", [(0, False), (0, True), (1, False), (1, True), (2, False)])
def test_pool_ref(d, mode, nan):
    c = R.pool_case(d, nan)
    ref = R.pool(c["h"], R.POOL_SEG, R.POOL_RNG, mode)
    assert bool(ref.isfinite().all())
    # ProteinPooler's own input: one padded row per range, the protein of each row, the pad mask
    S = max(ln for _, ln in R.POOL_RNG)
    z = torch.zeros(len(R.POOL_RNG), S, d)
    padmask = torch.ones(len(R.POOL_RNG), S, dtype=torch.bool)
    keys = torch.zeros(len(R.POOL_RNG), dtype=torch.long)
    for p in range(len(R.POOL_SEG) - 1):
        keys[R.POOL_SEG[p]:R.POOL_SEG[p + 1]] = p
    for r, (st, ln) in enumerate(R.POOL_RNG):
        z[r, :ln] = c["h"][st:st + ln]
        padmask[r, :ln] = False
    orc = PR.protein_pooler(z, keys, padmask, method="max" if mode == 2 else "mean", correction=mode == 1)
    assert R.rel64(orc, ref) <= AGREE
    _within_bar(R.pool(c["h"], R.POOL_SEG, R.POOL_RNG, mode, dt=F32), ref, ("pool", d, mode, nan))


# ------------------------------------------------------------------------------------------------ gathers, SiLU-mul
def test_gather_and_silu_refs():
    for d in R.EMBED_DIMS:
        c = R.embed_case(d)
        out = R.embed(c["table"], c["ids"], c["soft"], c["soft_map"])
        assert torch.equal(out[0], c["table"][0]) and torch.equal(out[1], c["table"][-1]) and torch.equal(out[2], c["soft"][2])
        assert torch.equal(R.embed(c["table"], c["ids"]), F.embedding(c["ids"].long(), c["table"]))
    c = R.acc_case()
    once = R.acc_rows(c["dst"], c["src"], c["rows"], c["d"])
    twice = R.acc_rows(once, c["src2"], c["rows"], c["d"])
    lo = R.acc_rows(R.acc_rows(c["dst"], c["src"], c["rows"], c["d"], dt=F32), c["src2"], c["rows"], c["d"], dt=F32)
    _within_bar(lo, twice, "acc_rows")
    for n in (1, R.SILU_BIG):
        c = R.silu_case(n)
        ref = R.silu_mul(c["g"], c["u"])
        assert bool(ref.isfinite().all())
        assert R.rel64(F.silu(c["g"]) * c["u"], ref) <= AGREE
        lo = R.silu_mul(c["g"], c["u"], dt=F32)
        _within_bar(lo, ref, ("silu_mul", n))
        assert bool(((lo.double() - ref).abs() <= R.OP_BAR * ref.abs() + 1e-30).all())


# ------------------------------------------------------------------------------------------------ padded generation can see the defect
def test_padded_generation_inputs_see_zeroed_keyless_rows(monkeypatch):
    from procyon_amd import synth
    sd = synth.llama_state_dict(**R.GEN_GEOM, dtype=F32)
    geom = LR.LlamaGeom(**R.GEN_GEOM)
    ids, mask = R.gen_case()
    emb = F.embedding(ids, sd["model.embed_tokens.weight"])
    toks, logits, _ = LR.greedy_generate(sd, geom, emb, mask, R.GEN_STEPS, clean_decode_mask=False)
    orig = F.softmax
    minv = torch.finfo(F32).min

    def zeroing_softmax(s, dim=-1, dtype=None):
        p = orig(s, dim=dim, dtype=dtype)
        return p * (~(s == minv).all(dim, keepdim=True)).to(p.dtype)       # a row of finfo.min throughout has no kept key

    monkeypatch.setattr(LR.F, "softmax", zeroing_softmax)
    toks_z, logits_z, _ = LR.greedy_generate(sd, geom, emb, mask, R.GEN_STEPS, clean_decode_mask=False)
    monkeypatch.undo()
    assert torch.equal(toks[:, 0], toks_z[:, 0])                # step 0 reads real rows only: same first token, comparable step 1
    err = [R.rel64(logits_z[b, 1], logits[b, 1]) for b in range(R.GEN_B)]
    padded = [b for b, p in enumerate(R.GEN_PADS) if p]
    assert max(err[b] for b in padded) > 100 * 1e-4, err
    assert err[0] <= 1e-4, err                                  # the un-padded row cannot see it
