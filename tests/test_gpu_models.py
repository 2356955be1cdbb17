"""GPU parity of the model-level C-ABI entry points (ESM encode+pool, Llama prefill/decode/greedy)
against the oracle on the same seeded synthetic weights, and against the committed golden vectors
(full-width Llama-3-8B / ESM2-650M single layers produced by HF 5.15 in the build container).

Tolerances.  north_star asks for 1e-3 relative on bf16 logits/embeddings.  A bf16 pipeline that
materialises every intermediate in bf16 is not reproducible to that level even between two exact-class
CPU implementations (conftest.alt_accumulation: ~1.7e-3 after ONE ESM2-650M layer, ~3e-3 on one
Llama-3-8B layer's logits), so multi-layer bars are `parity_bar(floor)` = max(1e-3, 2 x the measured
CPU-vs-CPU floor on the same inputs); single ops are held to the strict elementwise bar in
test_gpu_kernels.py.  Argmax ids are compared under teacher forcing; a mismatch is accepted only where the
oracle's own top-2 margin lies inside the measured logits error (reported as `near_ties`)."""
import pytest
import torch

from conftest import alt_accumulation, assert_no_further_from_truth, assert_bf16_close, parity_bar, pcy_disable, rel_err
from fulldepth_common import served_by

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

SM_LLAMA = dict(vocab=320, d=256, n_layers=2, n_heads=4, n_kv_heads=2, ffn=512)
SM_ESM = dict(d=128, n_layers=2, n_heads=2, ffn=256)


def llama_pair(geom_kw, theta=1e4, rms_cast="hf5"):
    from oracle import llama_ref as LR
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    kw = dict(geom_kw)
    sd = synth.llama_state_dict(**kw)
    geom = LR.LlamaGeom(**kw, rope_theta=theta, rms_cast=rms_cast)
    eng = LlamaEngine(sd, LlamaConfig(**kw, rope_theta=theta, rms_cast=rms_cast, max_pos=2048))
    return sd, geom, eng


def esm_pair(kw, rope_math="fp32_once"):
    from oracle import esm_ref as ER
    from procyon_amd import synth
    from procyon_amd.engine import EsmConfig, EsmEngine
    sd = synth.esm_state_dict(**kw)
    return sd, ER.EsmGeom(**kw, rope_math=rope_math), EsmEngine(sd, EsmConfig(**kw, rope_math=rope_math))


@pytest.mark.parametrize("attn", ["exact", "fast"])
@pytest.mark.parametrize("mask_pads", [True, False])
@pytest.mark.parametrize("rope_math", ["fp32_once", "model_dtype"])
def test_esm_small(mask_pads, rope_math, attn, monkeypatch):
    """attn = "exact": the two-pass kernel with the reference's rounding points, held to the bf16 oracle at the reproducibility
    bar; "fast" (the default): the single-pass kernel, held to an fp32 evaluation of the same weights -- no further from it than
    the reference's own bf16 arithmetic (conftest.assert_no_further_from_truth)."""
    from oracle import esm_ref as ER
    from procyon_amd import synth
    monkeypatch.setenv("PCY_ESM_ATTN", attn)
    sd, geom, eng = esm_pair(SM_ESM, rope_math)
    toks = synth.protein_tokens([70, 33, 1, 129, 64], seed=3)
    toks[0, 5] = 32
    ref = ER.esm_forward(sd, geom, toks, mask_pads=mask_pads)
    out = eng.hidden_states(toks, mask_pads=mask_pads).cpu()
    keep = (toks != 1) if mask_pads else torch.ones_like(toks, dtype=torch.bool)
    if attn == "fast":
        truth = ER.esm_forward({k: v.float() for k, v in sd.items()}, geom, toks, mask_pads=mask_pads)
        assert_no_further_from_truth(out[keep], ref[keep], truth[keep], "esm small, single-pass attention")
        return
    with alt_accumulation():
        twin = ER.esm_forward(sd, geom, toks, mask_pads=mask_pads)
    floor = rel_err(twin[keep], ref[keep])
    err = rel_err(out[keep], ref[keep])
    print(f"esm small: gpu-vs-oracle {err:.2e}, cpu-vs-cpu floor {floor:.2e}")
    assert err < parity_bar(floor)


@pytest.mark.parametrize("attn", ["exact", "fast"])
def test_esm_650m_layer_golden(golden, attn, monkeypatch):
    """one full-width ESM2-650M layer (d1280 H20 F5120) vs the HF-5.15 golden vector (exact-rounding attention), and vs an fp32
    evaluation of the same layer by the oracle (single-pass attention)."""
    from oracle import esm_ref as ER
    from procyon_amd import synth
    from procyon_amd.engine import EsmConfig, EsmEngine
    monkeypatch.setenv("PCY_ESM_ATTN", attn)
    g = golden("g5_esm")
    kw = dict(d=1280, n_layers=1, n_heads=20, ffn=5120)
    sd = synth.esm_state_dict(**kw)
    eng = EsmEngine(sd, EsmConfig(**kw, rope_inv_freq_bf16=True))
    toks = g["tokens_650m"]
    out = eng.hidden_states(toks).cpu()
    keep = toks != 1
    if attn == "fast":
        truth = ER.esm_forward({k: v.float() for k, v in sd.items()}, ER.EsmGeom(**kw), toks)
        assert_no_further_from_truth(out[keep], g["h_650m_1layer_bf16"][keep], truth[keep], "esm650 layer, single-pass attention")
        return
    err = rel_err(out[keep], g["h_650m_1layer_bf16"][keep])
    print(f"esm650 layer vs HF golden: {err:.2e} (CPU-vs-CPU floor on this fixture: 1.7e-3)")
    assert err < 2.5e-3


@pytest.mark.parametrize("pooling,corr", [("mean", False), ("mean", True), ("max", False)])
def test_esm_plm_forward_split_pool(pooling, corr):
    """A1+A2+A3 with long proteins: chunk splitting (small max_protein_len), pooling over chunks."""
    from oracle import procyon_ref as PR
    from procyon_amd import synth
    sd, geom, eng = esm_pair(SM_ESM)
    toks = synth.protein_tokens([150, 20, 64, 65, 129], seed=4)
    ref = PR.esm_plm_forward(sd, geom, toks, pooling=pooling, correction=corr, max_protein_len=64)
    with alt_accumulation():
        twin = PR.esm_plm_forward(sd, geom, toks, pooling=pooling, correction=corr, max_protein_len=64)
    out = eng.forward(toks, pooling=pooling, correction=corr, max_protein_len=64).cpu()
    assert out.shape == ref.shape
    assert rel_err(out, ref) < parity_bar(rel_err(twin, ref))


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("theta,cast", [(1e4, "hf5"), (5e5, "hf431")])
def test_llama_small_prefill_decode(ragged, theta, cast):
    from oracle import llama_ref as LR
    from procyon_amd.engine import GenState
    sd, geom, eng = llama_pair(SM_LLAMA, theta, cast)
    g = torch.Generator().manual_seed(5)
    B, T, NDEC = 3, 45, 6
    emb = (torch.randn(B, T, SM_LLAMA["d"], generator=g) * 0.05).to(BF)
    mask = torch.ones(B, T)
    if ragged:
        mask[1, :7] = 0
        mask[2, :33] = 0
    r = LR.llama_forward(sd, geom, inputs_embeds=emb, attn_mask=mask, want_hidden=True)
    with alt_accumulation():
        tw = LR.llama_forward(sd, geom, inputs_embeds=emb, attn_mask=mask, want_hidden=True)
    cache = eng.new_cache(B, T + NDEC + 1)
    logits, hidden = eng.prefill(emb.cuda(), mask, cache, "last", want_hidden=True)
    valid = mask.bool()
    floor = rel_err(tw["logits"][:, -1], r["logits"][:, -1])
    bar = parity_bar(floor)
    print(f"llama small prefill: logits err {rel_err(logits.cpu(), r['logits'][:, -1]):.2e}, floor {floor:.2e}")
    assert rel_err(hidden.cpu()[valid], r["hidden_states"][-1][valid]) < bar
    assert rel_err(logits.cpu(), r["logits"][:, -1]) < bar
    k0, v0 = cache.layer(0, T)
    assert rel_err(k0.cpu(), r["past_kv"][0][0]) < 1e-3   # first layer: single ops only -> strict bar
    assert rel_err(v0.cpu(), r["past_kv"][0][1]) < 1e-3
    # pad query rows: the reference softmax is uniform over all keys (finfo.min mask) -> K/V at pad slots match too
    k1, _ = cache.layer(1, T)
    assert rel_err(k1.cpu(), r["past_kv"][1][0]) < bar
    # teacher-forced decode (no mask, position = cache length; Q1/Q2)
    st = GenState(B, SM_LLAMA["vocab"], NDEC + 1, "cuda")
    st.pos.fill_(T)
    past = r["past_kv"]
    tok = r["logits"][:, -1].argmax(-1)
    near_ties = 0
    for s in range(NDEC):
        st.next_tok.copy_(tok.to(torch.int32))
        eng.decode(cache, st, B)
        st.pos += 1
        ro = LR.llama_forward(sd, geom, input_ids=tok[:, None], attn_mask=None, past_kv=past)
        past = ro["past_kv"]
        lo, lg = ro["logits"][:, -1], st.logits.cpu()
        assert rel_err(lg, lo) < 2 * bar, s
        top2 = lo.float().topk(2, -1).values
        for b in range(B):
            if int(lg[b].float().argmax()) != int(lo[b].float().argmax()):
                noise = float((lg[b].float() - lo[b].float()).abs().max())
                assert float(top2[b, 0] - top2[b, 1]) <= 4 * noise, f"argmax mismatch outside the noise at step {s}"
                near_ties += 1
        tok = lo.argmax(-1)
    print("near_ties", near_ties)


def test_llama_greedy_matches_oracle():
    """`_generate_sampling(greedy=True)`: tokens vs the oracle on a small model (free running);
    hipGraph replay == eager launches."""
    from oracle import llama_ref as LR
    sd, geom, eng = llama_pair(SM_LLAMA)
    g = torch.Generator().manual_seed(11)
    B, T, N = 2, 20, 24
    emb = (torch.randn(B, T, SM_LLAMA["d"], generator=g) * 0.05).to(BF)
    mask = torch.ones(B, T)
    tok_ref, lg_ref, lp_ref = LR.greedy_generate(sd, geom, emb, mask, N)
    tok, lp, lg, _ = eng.generate_greedy(emb.cuda(), mask, N, keep_logits=True, use_graph=False)
    tok2, lp2, _, _ = eng.generate_greedy(emb.cuda(), mask, N, keep_logits=False, use_graph=True)
    assert torch.equal(tok.cpu(), tok2.cpu()), "graph replay differs from eager launches"
    tok = tok.cpu()
    # free-running comparison up to the first divergence; a divergence must be a bf16 near-tie in the oracle
    for b in range(B):
        for s in range(N):
            if tok[b, s] != tok_ref[b, s]:
                top2 = lg_ref[b, s].float().topk(2).values
                noise = float((lg[b, s].cpu().float() - lg_ref[b, s].float()).abs().max())
                assert float(top2[0] - top2[1]) <= 4 * noise, (b, s)
                break
            assert rel_err(lg[b, s].cpu(), lg_ref[b, s]) < 1e-2
    same = (tok == tok_ref).all(1)
    assert torch.allclose(lp.cpu()[same], lp_ref[same], atol=0.25)


def test_llama3_8b_layer_golden(golden):
    """one full-width Llama-3-8B layer (d4096 H32 Hkv8 F14336) vs the HF-5.15 golden: prefill + 1 decode step."""
    from procyon_amd import synth
    from procyon_amd.engine import GenState, LlamaConfig, LlamaEngine
    g = golden("g6_llama")
    kw = dict(vocab=512, d=4096, n_layers=1, n_heads=32, n_kv_heads=8, ffn=14336)
    eng = LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, rope_inv_freq_bf16=True, max_pos=256))
    cache = eng.new_cache(1, 32)
    logits, hidden = eng.prefill(g["fw_embeds"].cuda(), None, cache, "last", want_hidden=True)
    eh, el = rel_err(hidden.cpu(), g["fw_prefill_hidden"]), rel_err(logits.cpu(), g["fw_prefill_logits_last"])
    print(f"llama3-8b layer vs HF golden: hidden {eh:.2e} logits {el:.2e} (CPU-vs-CPU floors 2.5e-3 / 3.0e-3)")
    assert eh < 4e-3 and el < 5e-3
    assert int(logits.float().argmax()) == int(g["fw_dec_token"])
    st = GenState(1, 512, 2, "cuda")
    st.pos.fill_(24)
    st.next_tok.copy_(g["fw_dec_token"].view(-1).to(torch.int32))
    eng.decode(cache, st, 1)
    assert rel_err(st.logits.cpu(), g["fw_dec_logits"]) < 5e-3
    assert int(st.logits.float().argmax()) == int(g["fw_dec_logits"].float().argmax())


@pytest.mark.parametrize("rows,src,t,disable", [(4, [2, 2, 0, 1], 9, ""), (4, [2, 2, 0, 1], 9, "kv_permute"), (4, [0, 1, 2, 3], 16, ""),
                                               (8, [7, 0, 0, 3, 3, 5, 1, 2], 13, ""), (12, [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10], 16, ""),
                                               (33, list(range(1, 33)) + [0], 5, "")])
def test_kv_reorder(monkeypatch, rows, src, t, disable):
    """cache[:, b, :, :t] = cache[:, src[b], :, :t] for every layer, K and V (model_unified.py:830-832): the one-pass in-place permutation
    (kv_permute_kernel: <= 8 and <= 32 rows), the identity (nothing touched), the two-launch form through the scratch copy
    (PCY_DISABLE=kv_permute, and > 32 rows); slots from t on keep their contents."""
    if disable:
        monkeypatch.setenv("PCY_DISABLE", disable)
    sd, geom, eng = llama_pair(SM_LLAMA)
    cache = eng.new_cache(rows, 16)
    cache.k.copy_(torch.randn(cache.k.shape).to(BF))
    cache.v.copy_(torch.randn(cache.v.shape).to(BF))
    k0, v0 = cache.k.clone(), cache.v.clone()
    src = torch.tensor(src)
    eng.kv_reorder(cache, src, t)
    assert torch.equal(cache.k[:, :, :, :t], k0[:, src.cuda()][:, :, :, :t])
    assert torch.equal(cache.v[:, :, :, :t], v0[:, src.cuda()][:, :, :, :t])
    assert torch.equal(cache.k[:, :, :, t:], k0[:, :, :, t:]) and torch.equal(cache.v[:, :, :, t:], v0[:, :, :, t:])


@pytest.mark.parametrize("T,N,n_layers", [(300, 24, 3), (600, 10, 2), (1100, 6, 2)])   # 600 / 1100: key split + score exchange on
def test_decode_attn_o_fused_launch_bit_identical(monkeypatch, T, N, n_layers):
    """attn_o_kernel (the step below the per-layer launch): decode attention and o projection in one launch -- Wo rows wait in registers while the
    attention workgroups run, hand-over by per-workgroup flags.  Same per-lane accumulation order, reduction tree and
    rounding points as the two-launch path, so logits, tokens and the appended K/V must be BIT-identical to PCY_DISABLE=attn_o,
    eager and under hipGraph replay, over enough steps that a stale flag or a missed hand-over would show; no watchdog."""
    from procyon_amd import synth
    from procyon_amd.engine import Context, GenState, LlamaConfig, LlamaEngine
    kw = dict(vocab=4096, d=4096, n_layers=n_layers, n_heads=32, n_kv_heads=8, ffn=14336)
    eng = LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, max_pos=2048))   # T = 1100: more than one 1024-key group
    torch.manual_seed(4)
    emb = (torch.randn(1, T, 4096) * 0.02).to(BF).cuda()

    monkeypatch.setenv("PCY_AO_XMIN", "384")   # key split + score exchange between the slice workgroups from 384 keys on (default 768)

    def run(ao, use_graph):
        pcy_disable(monkeypatch, "decode_layer", "" if ao else "attn_o")     # (the per-layer / all-layer launches have their own test below)
        cache = eng.new_cache(1, T + N + 2)
        st = GenState(1, kw["vocab"], N + 2, "cuda")
        logits, _ = eng.prefill(emb, None, cache, "last")
        st.logits.copy_(logits); st.pos.fill_(T)
        eng.pick(cache, st, 1, advance_pos=False)
        out = []
        for _ in range(N):
            eng.greedy_steps(cache, st, 1, 1, use_graph=use_graph)
            out.append(st.logits[0].clone())
        Context.get().sync()
        return torch.stack(out).cpu(), st.tokens_out[0, :N + 1].cpu(), cache.k[:, 0, :, T:T + N].cpu(), cache.v[:, 0, :, T:T + N].cpu()

    ref = run(False, False)
    for use_graph in (False, True, True):    # the second graph run starts at the epoch / flag state the first one left
        got = run(True, use_graph)
        for x, y in zip(got, ref):
            assert torch.equal(x, y), use_graph


@pytest.mark.parametrize("T,N,n_layers,cap", [(300, 24, 3, 0), (40, 12, 2, 0), (1100, 6, 2, 0), (765, 8, 2, 4096)])
def test_decode_layer_launch_bit_identical(monkeypatch, T, N, n_layers, cap):
    """The batch-1 decode step runs ALL decoder layers in one launch (decode_step_kernel; PCY_DISABLE=decode_step: one launch per layer,
    decode_layer_kernel; PCY_DISABLE=decode_layer: launch by launch), the residual stream crossing the layer boundaries as tagged words: qkv
    projection, attention (cache rows requested before the new token's q / k / v arrive), o projection, gate/up + SwiGLU and down,
    the vectors between the stages as {tag : bf16} words inside the launch.  Same per-row arithmetic and the same order of the
    RMSNorm statistics as the stand-alone launches: logits, tokens, log-probabilities and the appended K/V must be BIT-identical
    to the launch-per-stage step (with and without the fused attention + o launch), eager and under hipGraph replay, over enough
    steps that a stale tag or a vector read too early would show -- T = 1100 also crosses into the key-split exchange of the
    attention workgroups, T = 765..773 walks over its threshold (768 keys) inside one run with a 4096-slot cache (the attention's
    LDS image then exceeds 64 KB); the watchdog word must stay clear (Context.sync raises on it).  With and without the gate/up batch
    that the projection workgroups park in LDS during the attention (PCY_DISABLE=lds_prefetch)."""
    from procyon_amd import synth
    from procyon_amd.engine import Context, GenState, LlamaConfig, LlamaEngine
    kw = dict(vocab=4096, d=4096, n_layers=n_layers, n_heads=32, n_kv_heads=8, ffn=14336)
    eng = LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, max_pos=max(2048, cap)))
    torch.manual_seed(4)
    emb = (torch.randn(1, T, 4096) * 0.02).to(BF).cuda()

    def run(layer, attn_o, use_graph, step=False, lds=True):
        pcy_disable(monkeypatch, "" if layer else "decode_layer", "" if step else "decode_step", "" if attn_o else "attn_o",
                    "" if lds else "lds_prefetch")
        cache = eng.new_cache(1, cap or T + N + 2)
        st = GenState(1, kw["vocab"], N + 2, "cuda")
        logits, _ = eng.prefill(emb, None, cache, "last")
        st.logits.copy_(logits); st.pos.fill_(T)
        eng.pick(cache, st, 1, advance_pos=False)
        out = []
        # each side must have run what it names (dispatch counters): a fused launch that declines -- its LDS image grows with the cache capacity,
        # 4096 slots in the last case -- falls back to the launches with the same bits; a replayed run counts its capture only
        kind = "loop_stream" if not (layer and attn_o) else "step_gqa" if step else "layer"
        n_eager = sum(2 if i % 3 == 1 else 1 for i in range(N) if i % 3 != 2)
        with served_by(kind, None if use_graph else n_eager):
            for i in range(N):
                if i % 3 == 2:
                    continue
                eng.greedy_steps(cache, st, 1, 2 if i % 3 == 1 else 1, use_graph=use_graph)
                out.append(st.logits[0].clone())
        Context.get().sync()
        return (torch.stack(out).cpu(), st.tokens_out[0, :N + 1].cpu(), st.logprob.cpu().clone(), cache.k[:, 0, :, T:T + N].cpu(),
                cache.v[:, 0, :, T:T + N].cpu())

    ref = run(False, False, False)
    # (lds: the projection workgroups keep a gate/up batch in LDS while the attention runs -- default; off = the round-3 form)
    for layer, attn_o, use_graph, step, lds in ((False, True, False, False, True), (True, True, False, False, True), (True, True, True, False, True),
                                                 (True, True, False, True, True), (True, True, True, True, True), (True, True, True, True, True),
                                                 (True, True, True, True, False), (True, True, False, False, False)):
        got = run(layer, attn_o, use_graph, step, lds)
        for x, y in zip(got, ref):
            assert torch.equal(x, y), (layer, attn_o, use_graph, step, lds)


def test_decode_layers_only_entry_runs_the_layer_launches():
    """pcy_llama_decode_layers (the bench's roofline leg): passes over the decoder layers of a step without embedding / lm_head /
    pick.  It must leave the step's outputs (logits, tokens, position) untouched and a following ordinary step must still match
    a run that never called it (the tag counters advance, the slots are rewritten)."""
    from procyon_amd import synth
    from procyon_amd.engine import Context, GenState, LlamaConfig, LlamaEngine
    kw = dict(vocab=4096, d=4096, n_layers=2, n_heads=32, n_kv_heads=8, ffn=14336)
    eng = LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, max_pos=512))
    torch.manual_seed(5)
    emb = (torch.randn(1, 70, 4096) * 0.02).to(BF).cuda()

    def run(with_layers_only):
        cache = eng.new_cache(1, 96)
        st = GenState(1, kw["vocab"], 16, "cuda")
        logits, _ = eng.prefill(emb, None, cache, "last")
        st.logits.copy_(logits); st.pos.fill_(70)
        eng.pick(cache, st, 1, advance_pos=False)
        eng.greedy_steps(cache, st, 1, 3, use_graph=False)
        before = (st.logits.clone(), st.tokens_out.clone(), int(st.pos.item()))
        if with_layers_only:
            eng.decode_layers(cache, st, 1, 3)
            Context.get().sync()
            assert torch.equal(st.logits, before[0]) and torch.equal(st.tokens_out, before[1]) and int(st.pos.item()) == before[2]
        eng.greedy_steps(cache, st, 1, 3, use_graph=False)
        Context.get().sync()
        return st.logits.cpu().clone(), st.tokens_out.cpu().clone()

    a, b = run(False), run(True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_prefill_splitk_finish_norm_fusion_bit_identical(monkeypatch):
    """Single-prompt prefill (M <= 1024: the o and down projections run K-split): the finish launch of the residual epilogue also
    writes the RMSNorm of its result (PCY_DISABLE=finish_norm: residual finish + rmsnorm as two launches), and rope, K/V cache scatter
    and V transpose run as one launch (PCY_DISABLE=prefill_post_qkv: three).  Same element assignment, accumulation order and block
    reduction: last-row logits, final hidden state and the K/V cache must be bit-identical."""
    from procyon_amd import synth
    from procyon_amd.engine import Context, LlamaConfig, LlamaEngine
    kw = dict(vocab=2048, d=4096, n_layers=3, n_heads=32, n_kv_heads=8, ffn=14336)
    eng = LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, max_pos=1024))
    torch.manual_seed(6)
    outs = []
    for T in (512, 200):
        emb = (torch.randn(1, T, 4096) * 0.02).to(BF).cuda()
        res = []
        for fused in ("1", "0"):
            pcy_disable(monkeypatch, *(() if fused == "1" else ("finish_norm", "prefill_post_qkv")))   # the latter: rope + K/V scatter + V transpose as one launch / three
            cache = eng.new_cache(1, T + 4)
            logits, hidden = eng.prefill(emb, None, cache, "last", want_hidden=True)
            Context.get().sync()
            res.append((logits.cpu().clone(), hidden.cpu().clone(), cache.k[:, 0, :, :T].cpu().clone(), cache.v[:, 0, :, :T].cpu().clone()))
        for a, b in zip(*res):
            assert torch.equal(a, b), T


def test_batched_decode_finish_norm_fusion_bit_identical(monkeypatch):
    """Batched decode (B > 4, skinny-MFMA GEMVs with K split): the finish kernel of the o / down projections also writes the
    RMSNorm that follows (default; PCY_DISABLE=finish_norm: two launches).  Same element assignment and reduction order as the two separate
    launches, so logits, tokens and K/V must be bit-identical to the two-launch form, eager and under graph replay."""
    from procyon_amd import synth
    from procyon_amd.engine import GenState, LlamaConfig, LlamaEngine
    kw = dict(vocab=4096, d=4096, n_layers=2, n_heads=32, n_kv_heads=8, ffn=14336)
    eng = LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, max_pos=256))
    T, N = 33, 5
    for B in (7, 20, 40, 64):     # (above 32 rows: 32-row GEMV passes, the finish not fused with the norm)
        torch.manual_seed(B)
        emb = (torch.randn(B, T, 4096) * 0.02).to(BF).cuda()

        def run(fused, use_graph):
            pcy_disable(monkeypatch, "" if fused else "finish_norm")
            cache = eng.new_cache(B, T + N + 2)
            st = GenState(B, kw["vocab"], N + 2, "cuda")
            logits, _ = eng.prefill(emb, None, cache, "last")
            st.logits.copy_(logits); st.pos.fill_(T)
            eng.pick(cache, st, B, advance_pos=False)
            out = []
            for _ in range(N):
                eng.greedy_steps(cache, st, B, 1, use_graph=use_graph)
                out.append(st.logits.clone())
            return torch.stack(out).cpu(), st.tokens_out[:, :N + 1].cpu(), cache.k[:, :B, :, T:T + N].cpu()

        ref = run(False, False)
        for use_graph in (False, True):
            got = run(True, use_graph)
            for x, y in zip(got, ref):
                assert torch.equal(x, y), (B, use_graph)


def test_batched_decode_qkv_finish_in_attention_bit_identical(monkeypatch):
    """Batched decode: the K-split partial sums of the qkv projection are added up by the attention workgroup that needs them
    (attn_dec_splitk_kernel, default) instead of by a finish launch (PCY_DISABLE=attn_qkv_finish).  Same split order, same rounding: logits,
    tokens and the appended K/V rows are bit-identical, eager and under graph replay; batches of 5..64 rows incl. a ragged keep mask."""
    from procyon_amd import synth
    from procyon_amd.engine import GenState, LlamaConfig, LlamaEngine
    kw = dict(vocab=4096, d=4096, n_layers=2, n_heads=32, n_kv_heads=8, ffn=14336)
    eng = LlamaEngine(synth.llama_state_dict(**kw), LlamaConfig(**kw, max_pos=256))
    T, N = 40, 4
    for B in (5, 20, 32, 40, 64):     # (above 32 rows: 32-row GEMV passes, the qkv finish as its own launch)
        torch.manual_seed(B)
        emb = (torch.randn(B, T, 4096) * 0.02).to(BF).cuda()

        def run(separate, use_graph):
            pcy_disable(monkeypatch, "attn_qkv_finish" if separate else "")
            cache = eng.new_cache(B, T + N + 2)
            st = GenState(B, kw["vocab"], N + 2, "cuda")
            logits, _ = eng.prefill(emb, None, cache, "last")
            st.logits.copy_(logits); st.pos.fill_(T)
            eng.pick(cache, st, B, advance_pos=False)
            out = []
            for _ in range(N):
                eng.greedy_steps(cache, st, B, 1, use_graph=use_graph)
                out.append(st.logits.clone())
            return (torch.stack(out).cpu(), st.tokens_out[:, :N + 1].cpu(), cache.k[:, :B, :, T:T + N].cpu(), cache.v[:, :B, :, T:T + N].cpu())

        ref = run(True, False)
        for use_graph in (False, True):
            got = run(False, use_graph)
            for x, y in zip(got, ref):
                assert torch.equal(x, y), (B, use_graph)


def test_llama2_7b_geometry_layer():
    """BASELINE configs[0] geometry (ProCyon-Split text side: Llama-2-7B, multi-head attention H = Hkv = 32, F = 11008, odd
    vocabulary 32007) at full width, one layer: prefill + 3 cached decode steps against the oracle.  Exercises G = 1 in both
    attention kernels, K = 11008 (not a multiple of 512) in the GEMV / split-K paths and an odd vocabulary in the picks."""
    from oracle import llama_ref as LR
    kw = dict(vocab=32007, d=4096, n_layers=1, n_heads=32, n_kv_heads=32, ffn=11008)
    sd, geom, eng = llama_pair(kw)
    T, N = 40, 4
    torch.manual_seed(5)
    emb = (torch.randn(2, T, 4096) * 0.02).to(BF)
    mask = torch.ones(2, T)
    mask[1, :7] = 0      # one left-padded row
    tok_ref, lg_ref, _ = LR.greedy_generate(sd, geom, emb, mask, N)
    tok, _, lg, _ = eng.generate_greedy(emb.cuda(), mask, N, keep_logits=True)
    for s_ in range(N):
        assert rel_err(lg[:, s_].cpu(), lg_ref[:, s_]) < 8e-3, s_
    for b in range(2):
        for s_ in range(N):
            if tok[b, s_] != tok_ref[b, s_]:
                top2 = lg_ref[b, s_].float().topk(2).values
                noise = float((lg[b, s_].cpu().float() - lg_ref[b, s_].float()).abs().max())
                assert float(top2[0] - top2[1]) <= 4 * noise, (b, s_)
                break


@pytest.mark.parametrize("name,kw", [("esm2-3b", dict(d=2560, n_layers=1, n_heads=40, ffn=10240)),
                                     ("esm2-150m", dict(d=640, n_layers=2, n_heads=20, ffn=2560))])
def test_esm_other_sizes_layer(name, kw):
    """The other encoder sizes the reference can be configured with (procyon/model/esm.py:378-421): ESM2-3B (d2560, head_dim 64:
    the fused-rotary 256x256 GEMM path, D = 2560 embeddings of ProCyon-Full's 3B variant) and ESM2-150M (head_dim 32: the
    separate rotary kernel and the dh = 32 attention instantiation) at full width against the oracle."""
    from oracle import esm_ref as ER
    from procyon_amd import synth
    sd, geom, eng = esm_pair(kw)
    toks = synth.protein_tokens([300, 45, 301], seed=8)
    ref = ER.esm_forward(sd, geom, toks, mask_pads=True)
    with alt_accumulation():
        twin = ER.esm_forward(sd, geom, toks, mask_pads=True)
    out = eng.hidden_states(toks).cpu()
    keep = toks != 1
    floor, err = rel_err(twin[keep], ref[keep]), rel_err(out[keep], ref[keep])
    print(f"{name}: gpu-vs-oracle {err:.2e}, cpu-vs-cpu floor {floor:.2e}")
    assert err < parity_bar(floor)
