"""CPU: the oracle (oracle/) against the golden fixtures produced from the reference's own
extracted functions and the container's HF Llama/ESM (tests/golden/make_golden.py)."""
import pytest
import torch

from conftest import assert_bf16_close, rel_err
from oracle import esm_ref as ER
from oracle import llama_ref as LR
from oracle import procyon_ref as PR
from procyon_amd import synth

TINY = dict(vocab=300, d=128, n_layers=2, n_heads=8, n_kv_heads=2, ffn=256)


@pytest.fixture(autouse=True)
def native_cpu_gemm(monkeypatch):
    """The oracle on torch's own CPU GEMM, as g5 / g6 were recorded (make_golden.native_cpu_gemm): oneDNN's bf16 kernels sum in an
    order that depends on the host's ISA and thread count, which moved the full-width layers past the 1-ulp bar on other hosts."""
    monkeypatch.setattr(torch.backends.mkldnn, "enabled", False)


def test_g1_split(golden):
    g = golden("g1_split")
    for n in range(6):
        rows, keys, eos = PR.batched_split_long_seq(g[f"in{n}"])
        assert torch.equal(rows, g[f"rows{n}"]), n
        assert torch.equal(keys, g[f"keys{n}"]), n
        assert eos == g[f"eos{n}"].tolist(), n


def test_g1_split_known_shapes():
    # 2049 residues -> rows of 1026/1026/3 tokens
    toks = synth.protein_tokens([2049], seed=1)
    rows, keys, _ = PR.batched_split_long_seq(toks)
    assert rows.shape == (3, 1026) and keys.tolist() == [0, 0, 0]
    assert [(r != 1).sum().item() for r in rows] == [1026, 1026, 3]


def test_g2_pool(golden):
    g = golden("g2_pool")
    for nm in ("f32", "bf16"):
        for method, corr in (("mean", 0), ("mean", 1), ("max", 0)):
            r = PR.protein_pooler(g[f"z_{nm}"], g["keys"], g["pad"], method, bool(corr))
            assert torch.equal(r, g[f"out_{nm}_{method}_{corr}"]), (nm, method, corr)


def test_g3_mlp(golden):
    g = golden("g3_mlp")
    for nl in (1, 3):
        for nm in ("f32", "bf16"):
            layers = [(g[f"w_{nl}_{nm}_{i}"], g.get(f"b_{nl}_{nm}_{i}")) for i in range(nl)]
            y = PR.mlp_forward(g[f"x_{nl}_{nm}"], layers)
            if nm == "f32":
                assert torch.allclose(y, g[f"y_{nl}_{nm}"], atol=1e-6)
            else:
                assert_bf16_close(y, g[f"y_{nl}_{nm}"], f"mlp{nl}")


def test_g4_pad_splice(golden):
    g = golden("g4_pad_splice")
    ts = [torch.arange(5), torch.arange(2) + 10, torch.arange(7) + 20]
    bt, am = PR.left_pad_tensors(ts, pad_value=99)
    assert torch.equal(bt, g["lp_tok"]) and torch.equal(am, g["lp_mask"])
    for roll in (0, 1):
        z, ret = PR.prepare_input_embeddings(
            g["emb_w"], g["ids"], 31, g["prot_soft"], 33, [g["struct_soft0"], g["struct_soft1"], []],
            34, g["drug_soft"], ret_idx=32, roll_num=roll)
        assert torch.equal(z, g[f"z_roll{roll}"])
        assert torch.equal(ret, g[f"ret_roll{roll}"])


def _esm_sd(d, L, H, F, dt):
    return {k: v.to(dt) for k, v in synth.esm_state_dict(d, L, H, F, dtype=torch.float32).items()}


def test_g5_esm(golden):
    g = golden("g5_esm")
    for nm, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        sd = _esm_sd(64, 2, 4, 128, dt)
        geom = ER.EsmGeom(64, 2, 4, 128, rope_table="bf16_inv_freq")
        for tag, mp in (("masked", True), ("nomask", False)):
            h = ER.esm_forward(sd, geom, g["tokens"], mask_pads=mp)
            if nm == "f32":
                assert torch.allclose(h, g[f"h_{tag}_{nm}"], atol=2e-5), tag
            else:
                assert_bf16_close(h, g[f"h_{tag}_{nm}"], f"esm {tag}")


def test_g5_esm_full_width_layer(golden):
    g = golden("g5_esm")
    sd = _esm_sd(1280, 1, 20, 5120, torch.bfloat16)
    geom = ER.EsmGeom(1280, 1, 20, 5120, rope_table="bf16_inv_freq")
    h = ER.esm_forward(sd, geom, g["tokens_650m"], mask_pads=True)
    assert_bf16_close(h, g["h_650m_1layer_bf16"], "esm650 layer")


def _llama_sd(dt, **kw):
    return {k: v.to(dt) for k, v in synth.llama_state_dict(dtype=torch.float32, **kw).items()}


def test_g6_llama_prefill_decode(golden):
    g = golden("g6_llama")
    for theta in (10000, 500000):
        for nm, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            sd = _llama_sd(dt, **TINY)
            geom = LR.LlamaGeom(**TINY, rope_theta=float(theta), rope_table="bf16_inv_freq")
            for mname in ("eq", "rag"):
                tag = f"{nm}_{theta}_{mname}"
                mask = torch.ones(2, 12) if mname == "eq" else g["mask_rag"]
                r = LR.llama_forward(sd, geom, inputs_embeds=g["embeds"].to(dt), attn_mask=mask, want_hidden=True)

                def chk(a, b, what):
                    if nm == "f32":
                        assert torch.allclose(a, b, atol=2e-5), what
                    else:
                        assert_bf16_close(a, b, what)
                chk(r["logits"], g[f"prefill_logits_{tag}"], "logits " + tag)
                chk(torch.stack(r["hidden_states"]), g[f"prefill_hidden_{tag}"], "hidden " + tag)
                chk(r["past_kv"][0][0], g[f"prefill_k0_{tag}"], "k0 " + tag)
                chk(r["past_kv"][1][1], g[f"prefill_v1_{tag}"], "v1 " + tag)
                past = r["past_kv"]
                toks = g[f"dec_in_tokens_{tag}"]
                for s in range(toks.shape[1]):  # teacher-forced on the golden tokens, no mask (Q1)
                    r = LR.llama_forward(sd, geom, input_ids=toks[:, s:s + 1], attn_mask=None, past_kv=past)
                    past = r["past_kv"]
                    chk(r["logits"][:, -1], g[f"dec_logits_{tag}"][:, s], f"dec{s} " + tag)
                    if s + 1 < toks.shape[1]:
                        assert torch.equal(r["logits"][:, -1].argmax(-1), toks[:, s + 1])


def test_g6_llama_full_width_layer(golden):
    g = golden("g6_llama")
    FW = dict(vocab=512, d=4096, n_layers=1, n_heads=32, n_kv_heads=8, ffn=14336)
    sd = _llama_sd(torch.bfloat16, **FW)
    geom = LR.LlamaGeom(**FW, rope_table="bf16_inv_freq")
    r = LR.llama_forward(sd, geom, inputs_embeds=g["fw_embeds"], attn_mask=torch.ones(1, 24), want_hidden=True)
    assert_bf16_close(r["hidden_states"][-1], g["fw_prefill_hidden"], "fw hidden")
    assert_bf16_close(r["logits"][:, -1], g["fw_prefill_logits_last"], "fw logits")
    r2 = LR.llama_forward(sd, geom, input_ids=g["fw_dec_token"], attn_mask=None, past_kv=r["past_kv"])
    assert_bf16_close(r2["logits"][:, -1], g["fw_dec_logits"], "fw dec logits")


def test_g7_greedy_beam_nucleus(golden):
    g = golden("g7_generate")
    for nm, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        sd = _llama_sd(dt, **TINY)
        geom = LR.LlamaGeom(**TINY, rope_table="bf16_inv_freq")
        emb = g["embeds"].to(dt)
        mask = torch.ones(2, 10)
        tok, lg, lp = LR.greedy_generate(sd, geom, emb, mask, 16)
        assert torch.equal(tok, g[f"greedy_tokens_{nm}"][:, 0]), nm
        assert torch.allclose(lp, g[f"greedy_logprob_{nm}"][:, 0], atol=1e-3 if nm == "f32" else 0.5)
        enc = LR.make_text_encoder(sd, geom)
        for bs, gs, pen in ((4, 2, 0.8), (4, 4, 0.0), (6, 1, 0.5)):
            t, s, _ = LR.beam_search(enc, emb, mask, vocab_size=300, eos_id=299, max_len=10, beam_size=bs,
                                     beam_group_size=gs, diversity_penalty=pen)
            assert torch.equal(t, g[f"beam_tokens_{nm}_{bs}_{gs}"]), (nm, bs, gs)
            assert torch.allclose(s, g[f"beam_scores_{nm}_{bs}_{gs}"], atol=1e-4 if nm == "f32" else 0.3)
    # EOS early stop
    sd = _llama_sd(torch.float32, **TINY)
    geom = LR.LlamaGeom(**TINY)
    enc = LR.make_text_encoder(sd, geom)
    t, s, lg = LR.beam_search(enc, g["embeds"][:1], torch.ones(1, 10), vocab_size=300, eos_id=int(g["beam_eos_id"]),
                              max_len=12, beam_size=2, beam_group_size=2, diversity_penalty=0.0)
    assert torch.equal(t, g["beam_eos_tokens"]) and lg.shape[2] == int(g["beam_eos_steps"])
    for p in (90, 50):
        assert torch.equal(LR.nucleus_mask(g["nucleus_probs"], p / 100), g[f"nucleus_mask_{p}"])


def test_g8_qa(golden):
    g = golden("g8_qa")
    assert torch.equal(PR.get_after_answer_tokens(g["toks"], 50), g["after_answer"])


def test_g9_e2e_tiny(golden):
    """Config-1 shaped plumbing run: protein -> ESM -> pool -> projector -> splice -> 64 greedy tokens."""
    g = golden("g9_e2e_tiny")
    dt = torch.float32
    esd = _esm_sd(64, 2, 4, 128, dt)
    pooled = PR.esm_plm_forward(esd, ER.EsmGeom(64, 2, 4, 128), g["protein_tokens"])
    assert torch.allclose(pooled, g["pooled"], atol=1e-5)
    soft = PR.mlp_forward(pooled, synth.mlp_layers(3, 64, 128, 96, seed_off=0, dtype=dt))
    assert torch.allclose(soft, g["soft_token"], atol=1e-5)
    sd = _llama_sd(dt, **TINY)
    z, _ = PR.prepare_input_embeddings(sd["model.embed_tokens.weight"], g["prompt_ids"], 290, soft)
    tok, lg, lp = LR.greedy_generate(sd, LR.LlamaGeom(**TINY), z, torch.ones(1, 32), 64)
    assert torch.equal(tok, g["tokens"][:, 0])
    assert torch.allclose(lg[:, -1], g["logits_last"][:, 0], atol=1e-4)
