"""GPU: the fp32 operator family and engines (procyon_amd/csrc/pcy_f32.hip, procyon_amd/engine_f32.py) -- the arithmetic of the
reference's callers that never call `.bfloat16()` (/root/reference/examples/paper_analyses/protpep_qa_scores.py:55-58,
/root/reference/scripts/qa_filter_captions.py:17-18, /root/reference/scripts/caption_bulk.py:72-73) -- against the oracle evaluated in
fp32 on the same fp32 weights.  Bar: <= 1e-4 relative on every stack (two fp32 evaluations differ by accumulation order only),
<= 2e-5 on single ops."""
import pytest
import torch
import torch.nn.functional as F

from conftest import record_parity, rel_err

pytestmark = pytest.mark.gpu
F32 = torch.float32


def rnd(*shape, seed=0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * std


@pytest.fixture(scope="module")
def ops():
    from procyon_amd.engine_f32 import F32Ops
    return F32Ops()


@pytest.mark.parametrize("M,N,K", [(200, 384, 256), (1026, 1280, 1280), (130, 1001, 128), (17, 256, 5120), (77, 333, 100)])
@pytest.mark.parametrize("mode", ["plain", "bias_gelu", "bias_resid"])
def test_f32_linear(ops, M, N, K, mode):
    """pcy_f32_linear: the MFMA path (K % 16 == 0) and the plain fallback (K = 100), ragged M / N, bias + gelu, bias + residual"""
    A, W, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, std=0.05), rnd(N, seed=3, std=0.1), rnd(M, N, seed=4)
    bias = None if mode == "plain" else b
    ref = F.linear(A, W, bias)
    if mode == "bias_gelu":
        ref = F.gelu(ref)
    if mode == "bias_resid":
        ref = ref + r
    out = ops.linear(A.cuda(), W.cuda(), None if bias is None else bias.cuda(), r.cuda() if mode == "bias_resid" else None,
                     act=1 if mode == "bias_gelu" else 0).cpu()
    e = rel_err(out, ref)
    assert e < 2e-5, e
    assert float((out - ref).abs().max()) < 2e-4 * float(ref.abs().max())


def test_f32_norms_rope_silu(ops):
    x, w, b = rnd(37, 1280, seed=1) * 3 + 0.5, rnd(1280, seed=2) * 0.1 + 1, rnd(1280, seed=3) * 0.1
    assert rel_err(ops.layernorm(x.cuda(), w.cuda(), b.cuda(), 1e-5).cpu(), F.layer_norm(x, (1280,), w, b, 1e-5)) < 2e-6
    from oracle import llama_ref as LR
    assert rel_err(ops.rmsnorm(x.cuda(), w.cuda(), 1e-5).cpu(), LR.rms_norm(x, w, 1e-5)) < 2e-6
    g, u = rnd(50, 300, seed=4) * 2, rnd(50, 300, seed=5)
    assert rel_err(ops.silu_mul(g.cuda(), u.cuda()).cpu(), F.silu(g) * u) < 2e-6
    # rotary on a [tokens, 3 heads x 64] window with prescale, vs the oracle's formula
    from procyon_amd.engine_f32 import _rope_tables_f32
    dh, nh, T = 64, 3, 29
    cos, sin = _rope_tables_f32(dh, 10000.0, 64, "cuda")
    buf = rnd(T, 8 + nh * dh + 5, seed=6)
    pos = torch.randint(0, 64, (T,), generator=torch.Generator().manual_seed(7)).to(torch.int32)
    q = buf[:, 8:8 + nh * dh].reshape(T, nh, dh) * 0.125
    c, s_ = cos.cpu()[pos.long()][:, None], sin.cpu()[pos.long()][:, None]
    ref = buf.clone()
    ref[:, 8:8 + nh * dh] = (q * c + LR.rotate_half(q) * s_).reshape(T, nh * dh)
    d = buf.cuda().contiguous()
    ops.rope(d, 8, nh, dh, pos.cuda(), cos, sin, prescale=0.125)
    assert rel_err(d.cpu(), ref) < 1e-6 and torch.equal(d.cpu()[:, :8], buf[:, :8])


@pytest.mark.parametrize("causal,H,Hkv,dh", [(True, 8, 2, 16), (False, 4, 4, 64), (True, 4, 4, 128)])
def test_f32_attention(ops, causal, H, Hkv, dh):
    """packed sequences of ragged length, grouped heads, causal / bidirectional, a key-keep mask (left pads); the causal pad query rows
    have no kept key and hold the reference's uniform average of V over every key of their sequence"""
    lens = [33, 1, 70, 128]
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32)
    ntok = int(cu[-1])
    qkv = rnd(ntok, (H + 2 * Hkv) * dh, seed=1)
    keep = torch.ones(ntok, dtype=torch.uint8)
    keep[int(cu[2]):int(cu[2]) + 9] = 0            # sequence 2 starts with 9 pads
    scale = dh ** -0.5
    out = ops.attention(qkv.cuda(), 0, qkv.cuda(), H * dh, qkv.cuda(), (H + Hkv) * dh, cu.cuda(), keep.cuda(), len(lens), max(lens), H, Hkv, dh, causal, scale).cpu()
    for s_, n in enumerate(lens):
        t0 = int(cu[s_])
        q = qkv[t0:t0 + n, :H * dh].view(n, H, dh).transpose(0, 1)
        k = qkv[t0:t0 + n, H * dh:(H + Hkv) * dh].view(n, Hkv, dh).transpose(0, 1).repeat_interleave(H // Hkv, 0)
        v = qkv[t0:t0 + n, (H + Hkv) * dh:].view(n, Hkv, dh).transpose(0, 1).repeat_interleave(H // Hkv, 0)
        sc = (q @ k.transpose(1, 2)) * scale
        allowed = keep[t0:t0 + n].bool()[None, None, :].expand(1, n, n).clone()
        if causal:
            allowed &= torch.tril(torch.ones(n, n, dtype=torch.bool))[None]
        sc = sc.masked_fill(~allowed, float("-inf"))
        live = allowed[0].any(-1)                   # rows with at least one kept key
        sc[:, ~live] = 0.0                          # a pad query row: the reference's softmax of a finfo.min row, uniform over ALL n keys
        ref = (sc.softmax(-1) @ v).transpose(0, 1).reshape(n, H * dh)
        assert rel_err(out[t0:t0 + n][live], ref[live]) < 2e-6, s_
        if bool((~live).any()):
            assert rel_err(out[t0:t0 + n][~live], ref[~live]) < 2e-6, s_


def test_f32_esm_engine_vs_oracle():
    """ESM2 (4 layers, d = 320, 5 heads of 64) on fp32 weights, ragged proteins incl. one that is split into chunks: hidden states and
    the mean / corrected-mean / max pooled embeddings vs the oracle in fp32"""
    from oracle import esm_ref as ER
    from oracle import procyon_ref as PR
    from procyon_amd import synth
    from procyon_amd.engine import EsmConfig
    from procyon_amd.engine_f32 import EsmEngineF32
    kw = dict(d=320, n_layers=4, n_heads=5, ffn=1280)
    sd = synth.esm_state_dict(**kw, dtype=F32)
    eng = EsmEngineF32(sd, EsmConfig(**kw))
    toks = synth.protein_tokens([100, 37, 260], seed=1)
    ref = ER.esm_forward(sd, ER.EsmGeom(**kw), toks)
    out = eng.hidden_states(toks).cpu()
    keep = toks != 1
    e = rel_err(out[keep], ref[keep])
    record_parity("fp32/esm_small_hidden", err_hip_oracle_fp32=e)
    assert e < 1e-4, e
    for pooling, corr in (("mean", False), ("mean", True), ("max", False)):
        z_ref = PR.esm_plm_forward(sd, ER.EsmGeom(**kw), toks, pooling=pooling, correction=corr, max_protein_len=128)
        z = eng.forward(toks, pooling=pooling, correction=corr, max_protein_len=128).cpu()
        assert z.shape == z_ref.shape and rel_err(z, z_ref) < 1e-4, (pooling, corr, rel_err(z, z_ref))


def test_f32_llama_engine_vs_oracle():
    """Llama prefill (3 layers, GQA 4/2, head_dim 64) on fp32 weights: logits at chosen rows, final hidden states, the L+1-state sum,
    with a left-padded row, vs the oracle in fp32"""
    from oracle import llama_ref as LR
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig
    from procyon_amd.engine_f32 import LlamaEngineF32
    kw = dict(vocab=331, d=256, n_layers=3, n_heads=4, n_kv_heads=2, ffn=512)
    sd = synth.llama_state_dict(**kw, dtype=F32)
    eng = LlamaEngineF32(sd, LlamaConfig(**kw, max_pos=256))
    g = torch.Generator().manual_seed(3)
    B, T = 3, 41
    ids = torch.randint(0, 331, (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.long); mask[1, :7] = 0
    emb = eng.embed_tokens(ids)
    assert torch.equal(emb.cpu(), F.embedding(ids, sd["model.embed_tokens.weight"]))
    r = LR.llama_forward(sd, LR.LlamaGeom(**kw), inputs_embeds=emb.cpu(), attn_mask=mask, want_hidden=True)
    rows = torch.tensor([40, 2 * T - 1, 2 * T + 5])
    logits, hidden, hsum = eng.prefill(emb, mask, rows, want_hidden=True, sum_rows=rows)
    valid = mask.bool()
    e_h = rel_err(hidden.cpu()[valid], r["hidden_states"][-1][valid])
    e_l = rel_err(logits.cpu(), r["logits"].reshape(B * T, -1)[rows])
    e_s = rel_err(hsum.cpu(), torch.stack(r["hidden_states"], -1).sum(-1).reshape(B * T, -1)[rows])
    record_parity("fp32/llama_small_prefill", err_hidden=e_h, err_logits=e_l, err_hidden_sum=e_s)
    assert e_h < 1e-4 and e_l < 1e-4 and e_s < 1e-4, (e_h, e_l, e_s)


def test_fp32_model_runs_as_the_unchanged_fp32_callers_drive_it():
    """The model exactly as protpep_qa_scores.py:55-58 / qa_filter_captions.py:17-18 use it -- built from an fp32 checkpoint, `.eval()`,
    NO `.bfloat16()` -- answers `forward` (QA yes/no at [ANSWER]; retrieval [PROT] embedding, ret_token_access last / all) and
    `forward_sequences` AND `generate` (greedy, diverse beam) in fp32 arithmetic, <= 1e-4 from the oracle pipeline in fp32; after
    `.bfloat16()` the same object runs the bf16 engine and its fp32 copies are gone."""
    from oracle import esm_ref as ER
    from oracle import llama_ref as LR
    from oracle import procyon_ref as PR
    from procyon_amd import synth
    from procyon_amd import synthetic_model as SM
    m, w = SM.build("small", device="cuda", return_weights=True, max_new_tokens=8, dtype=F32, as_loaded=True)
    m.eval()
    assert m.dtype == F32
    lgeom, egeom = LR.LlamaGeom(**w["geom"]["llama"]), ER.EsmGeom(**w["geom"]["esm"])
    prot = synth.protein_tokens([90, 41], seed=3)
    mk = lambda instr, seq, slots, texts=(), text_slots=(): {
        "data": {"seq": seq, "seq_idx": None if seq is None else torch.arange(seq.shape[0]), "text": list(texts), "drug": None},
        "input": {"seq": slots, "text": [list(t) for t in text_slots], "drug": None},
        "target": {"seq": None, "text": None, "drug": None}, "instructions": list(instr)}
    # forward_sequences
    out = m.forward_sequences(prot, get_soft_tokens=True)
    ref = PR.forward_sequences(w["esm"], egeom, prot, w["projs"]["shared"], w["projs"]["aaseq"], pooling="mean")
    for k in ("original", "shared", "token"):
        assert out[k].dtype == F32 and rel_err(out[k].cpu(), ref[k]) < 1e-4, k
    # QA
    instr = ["w1 <|protein|> is w2 ? [ANSWER] yes w3 <|protein|> ? [ANSWER]", "w4 <|protein|> ? [ANSWER]"]
    slots = [[0, 1], [1]]
    z = PR.esm_plm_forward(w["esm"], egeom, prot, pooling="mean")
    soft = PR.mlp_forward(z[[0, 1, 1]], w["projs"]["aaseq"])
    ids, mask = m._prepare_text_inputs_and_tokenize(list(instr), [[], []], crop_off=True, no_pad=False, left_pad=False)
    emb, _ = PR.prepare_input_embeddings(w["llama"]["model.embed_tokens.weight"], ids.long(), m.prot_replacement_idx, soft, ret_idx=m.prot_retrieval_idx)
    real = int(mask.sum(1).max())
    r = LR.llama_forward(w["llama"], lgeom, inputs_embeds=emb[:, :real], attn_mask=mask[:, :real])
    yes_ref, no_ref, _ = PR.qa_yes_no_probs(r["logits"], ids[:, :real], m.answer_idx, m.yes_token, m.no_token)
    o = m.forward(mk(instr, prot, slots, text_slots=[[], []]), retrieval=False)
    lg = o["outputs"].answer_logits[:, 0]
    assert lg.dtype == F32
    probs = lg.softmax(-1).cpu()
    pos = o["answer_positions"]
    e_qa = rel_err(lg.cpu(), torch.stack([r["logits"][i, pos[i]] for i in range(2)]))
    assert e_qa < 1e-4, e_qa
    assert torch.allclose(probs[:, m.yes_token], yes_ref, rtol=1e-3, atol=1e-9) and torch.allclose(probs[:, m.no_token], no_ref, rtol=1e-3, atol=1e-9)
    # retrieval, ret_token_access last and all
    instr = ["w1 w2 w3 describe [PROT]", "w9 [EXT] find [PROT]"]
    inp = mk(instr, None, None, texts=["alpha beta gamma"], text_slots=[[], [0]])
    ids, mask = m._prepare_text_inputs_and_tokenize(list(instr), [[], ["alpha beta gamma"]], no_pad=False)
    real = int(mask.sum(1).max())
    emb_ref, ret = PR.prepare_input_embeddings(w["llama"]["model.embed_tokens.weight"], ids.long(), m.prot_replacement_idx, None, ret_idx=m.prot_retrieval_idx)
    r = LR.llama_forward(w["llama"], lgeom, inputs_embeds=emb_ref[:, :real], attn_mask=mask[:, :real], want_hidden=True)
    errs = {}
    for access in ("last", "all"):
        m.config.ret_token_access = access
        got = m.forward(mk(instr, None, None, texts=["alpha beta gamma"], text_slots=[[], [0]]), retrieval=True)["contrastive_out"]["positive"]["text"]
        refv = PR.retrieval_text_embedding(r["hidden_states"], ret[:, :real], w["projs"]["lm"], access)
        errs[access] = rel_err(got.cpu(), refv)
        assert got.dtype == F32 and errs[access] < 1e-4, (access, errs[access])
    m.config.ret_token_access = "last"
    record_parity("fp32/model_small_as_loaded", err_qa_logits=e_qa, err_retrieval_last=errs["last"], err_retrieval_all=errs["all"])
    # generation in fp32 (/root/reference/scripts/caption_bulk.py:70-73 never casts the model and calls generate(method="beam")): greedy and
    # diverse beam search on the fp32 operator family against the oracle's loops in fp32 -- same tokens, logits <= 1e-4
    ginstr = ["w4 <|protein|> w5 [ANSWER]"]
    gslots = [[1]]
    gids, gmask = m._prepare_text_inputs_and_tokenize(list(ginstr), [[]], crop_off=True, no_pad=True, left_pad=True)
    gsoft = PR.mlp_forward(z[[1]], w["projs"]["aaseq"])
    gemb, _ = PR.prepare_input_embeddings(w["llama"]["model.embed_tokens.weight"], gids.long(), m.prot_replacement_idx, gsoft, ret_idx=m.prot_retrieval_idx)
    t_ref, lg_ref, _ = LR.greedy_generate(w["llama"], lgeom, gemb, gmask, 6)
    toks, lp, lg, _ = m.generate(mk(ginstr, prot, gslots, text_slots=[[]]), max_len=6, method="greedy")
    assert lg.dtype == F32 and torch.equal(toks[:, 0], t_ref), (toks, t_ref)
    e_gen = rel_err(lg[:, 0].float(), lg_ref)
    enc = LR.make_text_encoder(w["llama"], lgeom)
    tb_ref, sb_ref, lb_ref = LR.beam_search(enc, gemb, gmask, vocab_size=lgeom.vocab, eos_id=m.tokenizer.eos_token_id, max_len=5,
                                            beam_size=4, beam_group_size=2, diversity_penalty=0.8)
    tb, sb, lb, _ = m.generate(mk(ginstr, prot, gslots, text_slots=[[]]), max_len=5, method="beam", beam_size=4, beam_group_size=2, diversity_penalty=0.8)
    assert torch.equal(tb, tb_ref) and torch.allclose(sb, sb_ref, atol=1e-3), (tb, tb_ref, sb, sb_ref)
    e_beam = rel_err(lb.float(), lb_ref)
    record_parity("fp32/model_small_generate", err_greedy_logits=e_gen, err_beam_logits=e_beam, greedy_tokens_equal=True, beam_tokens_equal=True)
    assert e_gen < 1e-4 and e_beam < 1e-4, (e_gen, e_beam)
    # .bfloat16(): the bf16 engine takes over, the fp32 copies are dropped
    m.bfloat16()
    assert m.text_encoder._src_f32 is None and m.protein_seq_encoder._src_f32 is None and m.aaseq_shared_projector.src_f32 is None
    ob = m.forward_sequences(prot)
    assert ob["shared"].dtype == torch.bfloat16 and rel_err(ob["shared"].float().cpu(), ref["shared"]) < 2e-2
    with pytest.raises(RuntimeError, match="fp32"):      # the fp32 weights are gone: .float() says so at once
        m.float()


# ---- padded generation in fp32: the cached decode attends every slot without a mask (reference quirk Q1), so it reads the K / V that the
# prefill computed from LEFT-PAD rows; those rows have no kept key and take the reference's uniform average (include/pcy.h,
# pcy_f32_attention).  tests/test_f32_ref_cpu.py keeps it permanent that these inputs see a prefill that zeroes them instead.
@pytest.fixture(scope="module")
def padded_gen():
    """the fp32 Llama of the engine test (3 layers, GQA 4/2, head_dim 64), B = 3 prompts of T = 12 with left pads {0, 5, 1}; the oracle's
    prefill K / V and its 6 greedy steps, computed once"""
    import f32_ref as R
    from oracle import llama_ref as LR
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig
    from procyon_amd.engine_f32 import LlamaEngineF32
    sd = synth.llama_state_dict(**R.GEN_GEOM, dtype=F32)
    geom = LR.LlamaGeom(**R.GEN_GEOM)
    eng = LlamaEngineF32(sd, LlamaConfig(**R.GEN_GEOM, max_pos=256))
    ids, mask = R.gen_case()
    emb = F.embedding(ids, sd["model.embed_tokens.weight"])
    past = LR.llama_forward(sd, geom, inputs_embeds=emb, attn_mask=mask, logits_rows="last")["past_kv"]
    toks, logits, _ = LR.greedy_generate(sd, geom, emb, mask, R.GEN_STEPS, clean_decode_mask=False)
    return dict(sd=sd, geom=geom, eng=eng, ids=ids, mask=mask, emb=emb, past=past, toks=toks, logits=logits, pads=R.GEN_PADS, steps=R.GEN_STEPS)


def test_f32_padded_greedy_engine_vs_oracle(padded_gen):
    """LlamaEngineF32.prefill(cache=...) + decode, 6 greedy tokens: the K / V of the pad slots of every layer after the prefill, the
    tokens, and the logits of every step on EVERY row (the padded ones included) vs the oracle's loop, <= 1e-4"""
    g = padded_gen
    eng, ids, mask = g["eng"], g["ids"], g["mask"]
    B, T = ids.shape
    cache = eng.new_cache(B, T + g["steps"])
    emb = eng.embed_tokens(ids)
    assert torch.equal(emb.cpu(), g["emb"])
    logits, _ = eng.prefill(emb, mask, "last", cache=cache)
    e_pad = {"k": 0.0, "v": 0.0}
    for l, (k_ref, v_ref) in enumerate(g["past"]):                  # [B, Hkv, T, dh]
        for b, p in enumerate(g["pads"]):
            if p == 0:
                continue
            for name, got, ref in (("k", cache.k, k_ref), ("v", cache.v, v_ref)):
                e = rel_err(got[l, b, :p].cpu(), ref[b, :, :p].transpose(0, 1).reshape(p, -1))
                print(f"pad-slot {name} layer {l} row {b}: {e:.3e}")
                e_pad[name] = max(e_pad[name], e)
    toks, errs = [], []
    for i in range(g["steps"]):
        if i:
            logits = eng.decode(cache, toks[-1], T + i - 1)
        lg = logits.cpu()
        errs.append([rel_err(lg[b], g["logits"][b, i]) for b in range(B)])
        print(f"step {i}: per-row logits error {['%.3e' % e for e in errs[-1]]}")
        toks.append(lg.argmax(-1))
    toks = torch.stack(toks, 1)
    e_lg = max(max(r) for r in errs)
    record_parity("fp32/llama_padded_greedy", err_pad_slot_k=e_pad["k"], err_pad_slot_v=e_pad["v"], err_logits_worst_row_step=e_lg,
                  tokens_equal=bool(torch.equal(toks, g["toks"])))
    assert e_pad["k"] < 1e-4 and e_pad["v"] < 1e-4, e_pad
    assert torch.equal(toks, g["toks"]), (toks, g["toks"])
    assert e_lg < 1e-4, errs


def test_f32_padded_beam_engine_vs_oracle(padded_gen):
    """diverse beam search (beam 4 / group 2 / penalty 0.8, 5 steps) over B = 2 prompts, one left-padded: the oracle's own loop
    (llama_ref.beam_search, as the model test drives it) once over the oracle's text encoder and once over an adapter that runs
    LlamaEngineF32 prefill / decode and hands the loop the engine's K / V caches to re-index -- same tokens, scores, logits <= 1e-4"""
    from oracle import llama_ref as LR
    g = padded_gen
    eng = g["eng"]
    emb, mask = g["emb"][:2], g["mask"][:2]
    assert g["pads"][0] == 0 and g["pads"][1] > 0
    kw = dict(vocab_size=g["geom"].vocab, eos_id=2, max_len=5, beam_size=4, beam_group_size=2, diversity_penalty=0.8)
    t_ref, s_ref, l_ref = LR.beam_search(LR.make_text_encoder(g["sd"], g["geom"]), emb, mask, **kw)
    state = {}

    def enc(input_embeds=None, input_ids=None, attn_masks=None, past_key_values=None):
        if past_key_values is None:
            BB, T, _ = input_embeds.shape
            state["cache"], state["t"] = eng.new_cache(BB, T + kw["max_len"]), T
            logits, _ = eng.prefill(input_embeds, attn_masks, "last", cache=state["cache"])
        else:
            logits = eng.decode(state["cache"], input_ids.view(-1), state["t"])
            state["t"] += 1
        c = state["cache"]
        # (views of the engine's caches, batch first: the loop's in-place `layer[0][gs:ge] = layer[0][orig]` moves the engine's rows)
        return logits.cpu()[:, None, :], [[c.k[l], c.v[l]] for l in range(c.k.shape[0])]

    t, s, lg = LR.beam_search(enc, emb, mask, **kw)
    e = rel_err(lg, l_ref)
    e_rows = [rel_err(lg[b], l_ref[b]) for b in range(2)]
    print(f"beam logits error {e:.3e}, per prompt {e_rows}")
    record_parity("fp32/llama_padded_beam", err_logits=e, err_logits_padded_prompt=e_rows[1], tokens_equal=bool(torch.equal(t, t_ref)))
    assert torch.equal(t, t_ref), (t, t_ref)
    assert torch.allclose(s, s_ref, atol=1e-3), (s, s_ref)
    assert max(e_rows) < 1e-4, e_rows


def test_fp32_model_generates_from_left_padded_prompts():
    """`UnifiedProCyon.generate(method="greedy")` on the small synthetic fp32 model (never cast) with two instructions of different token
    length, so that one row is left-padded: tokens and logits of every row vs the oracle pipeline in fp32, as the single-prompt block of
    the test above compares them; the same batch through method="beam" (the engine's cache re-ordering under a padded row)"""
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
    ginstr = ["w4 <|protein|> w5 [ANSWER]", "w1 w2 w3 w6 <|protein|> is w7 w8 ? [ANSWER]"]
    gslots = [[1], [0]]
    gids, gmask = m._prepare_text_inputs_and_tokenize(list(ginstr), [[], []], crop_off=True, no_pad=True, left_pad=True)
    npad = (gmask == 0).sum(1)
    assert int(npad[0]) > 0 and int(npad[1]) == 0 and bool((gmask[0, :int(npad[0])] == 0).all())        # row 0 is left-padded
    z = PR.esm_plm_forward(w["esm"], egeom, prot, pooling="mean")
    gsoft = PR.mlp_forward(z[[1, 0]], w["projs"]["aaseq"])
    gemb, _ = PR.prepare_input_embeddings(w["llama"]["model.embed_tokens.weight"], gids.long(), m.prot_replacement_idx, gsoft, ret_idx=m.prot_retrieval_idx)
    t_ref, lg_ref, _ = LR.greedy_generate(w["llama"], lgeom, gemb, gmask, 6)
    toks, lp, lg, _ = m.generate(mk(ginstr, prot, gslots), max_len=6, method="greedy")
    e_rows = [rel_err(lg[b, 0].float(), lg_ref[b]) for b in range(2)]
    print(f"greedy logits error per row {e_rows}")
    enc = LR.make_text_encoder(w["llama"], lgeom)
    tb_ref, sb_ref, lb_ref = LR.beam_search(enc, gemb, gmask, vocab_size=lgeom.vocab, eos_id=m.tokenizer.eos_token_id, max_len=5,
                                            beam_size=4, beam_group_size=2, diversity_penalty=0.8)
    tb, sb, lb, _ = m.generate(mk(ginstr, prot, gslots), max_len=5, method="beam", beam_size=4, beam_group_size=2, diversity_penalty=0.8)
    eb_rows = [rel_err(lb[b].float(), lb_ref[b]) for b in range(2)]
    print(f"beam logits error per prompt {eb_rows}")
    record_parity("fp32/model_small_generate_padded", err_greedy_logits_padded_row=e_rows[0], err_greedy_logits_full_row=e_rows[1],
                  err_beam_logits_padded_row=eb_rows[0], err_beam_logits_full_row=eb_rows[1],
                  greedy_tokens_equal=bool(torch.equal(toks[:, 0], t_ref)), beam_tokens_equal=bool(torch.equal(tb, tb_ref)))
    assert lg.dtype == F32 and torch.equal(toks[:, 0], t_ref), (toks, t_ref)
    assert max(e_rows) < 1e-4, e_rows
    assert torch.equal(tb, tb_ref) and torch.allclose(sb, sb_ref, atol=1e-3), (tb, tb_ref, sb, sb_ref)
    assert max(eb_rows) < 1e-4, eb_rows
