"""Decode steps of MORE than 32 rows: what the reference's evaluation callers run by default (16 prompts x beam 10 = 160 rows per step), any
beam search over 4 or more prompts at beam 10, and a greedy batch of 33 or more prompts.  Above 32 rows the batched step cuts every GEMV into
32-row passes over the weights (pcy_launch_gemv), the qkv projection's K-split finish runs as its own launch instead of inside the attention,
the finish of the o / down projections is not fused with the next RMSNorm, and the beam search's K / V reorder takes the two-launch
kv_gather_kernel form (in the replayed chain: slot count read from the device).

Three geometries at full width, two layers: Llama-3-8B (ProCyon-Full's decoder), Llama-2-7B (ProCyon-Split's: H = Hkv = 32, ffn 11008) and
the small synthetic decoder.  Held to (a) the oracle on a few sampled rows -- rows do not interact, so the CPU only runs those -- (b) the same
rows decoded as 32-row batches of their own: BIT-identical, and (c) copies of one row placed in different 32-row passes: BIT-identical."""
import pytest
import torch

from beam_oracle import assert_beam_matches_oracle
from conftest import pcy_disable, rel_err
from fulldepth_common import check_oracle

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GEOMS = {
    "llama8b": dict(vocab=4096, d=4096, n_layers=2, n_heads=32, n_kv_heads=8, ffn=14336),
    "split": dict(vocab=2048, d=4096, n_layers=2, n_heads=32, n_kv_heads=32, ffn=11008),
    "small": dict(vocab=128263 - 128000 + 2048, d=256, n_layers=2, n_heads=4, n_kv_heads=2, ffn=512),   # synthetic_model "small"
}
N = 3          # cached decode steps per case
# (B, T): T varies; every batch is ragged (left-padded rows, the pads masked in the prefill AND in the decode steps)
CASES = [(33, 24), (40, 21), (64, 17), (160, 12)]


@pytest.fixture(scope="module", params=list(GEOMS))
def geo(request):
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    kw = GEOMS[request.param]
    sd = synth.llama_state_dict(**kw)
    return request.param, kw, sd, LlamaEngine(sd, LlamaConfig(**kw, max_pos=512))


def _batch(B, T, d, seed):
    """embeddings [B, T, d] + a ragged mask [B, T]; row 32 is a copy of row 1 and row B-1 a copy of row 2 (for B = 33 they coincide: row 32
    is then a copy of row 2) -- the copies sit in other 32-row passes than their originals."""
    g = torch.Generator().manual_seed(seed)
    emb = (torch.randn(B, T, d, generator=g) * 0.02).to(BF)
    mask = torch.ones(B, T)
    for b in range(B):
        mask[b, :(b * 7) % 11 if b % 3 else 0] = 0
    for dst, src in ((32, 1), (B - 1, 2)):
        emb[dst], mask[dst] = emb[src], mask[src]
    return emb, mask


def _decode(eng, V, emb, mask, use_graph, init=None):
    """prefill (or `init`: the post-prefill cache rows and logits of a wider batch) + N greedy cached steps with the clean decode mask.
    -> dict of device tensors: logits [N+1, n, V], tokens [n, N+1], logprob [n], the appended K / V slots; `snap`: the post-prefill state."""
    from procyon_amd.engine import Context, GenState
    n, T = mask.shape
    Tmax = T + N + 2
    cache = eng.new_cache(n, Tmax)
    keep = torch.ones(n, Tmax, dtype=torch.uint8, device="cuda")
    keep[:, :T] = mask.to("cuda", torch.uint8)
    st = GenState(n, V, N + 2, "cuda", keep=keep)
    if init is None:
        logits, _ = eng.prefill(emb.cuda(), mask, cache, "last")
    else:
        cache.k.copy_(init[0]); cache.v.copy_(init[1])
        logits = init[2]
    snap = (cache.k.clone(), cache.v.clone(), logits.clone())
    st.logits.copy_(logits); st.pos.fill_(T)
    eng.pick(cache, st, n, advance_pos=False)
    lg = [logits]
    for _ in range(N):
        eng.greedy_steps(cache, st, n, 1, use_graph=use_graph)
        lg.append(st.logits.clone())
    Context.get().sync()
    return dict(logits=torch.stack(lg), tokens=st.tokens_out[:, :N + 1].clone(), logprob=st.logprob.clone(),
                k=cache.k[:, :, :, T:T + N].clone(), v=cache.v[:, :, :, T:T + N].clone()), snap


def _rows(out, rows):
    """the sampled rows of every output, on the CPU"""
    r = torch.tensor(rows, device="cuda")
    return dict(logits=out["logits"][:, r].cpu(), tokens=out["tokens"][r].cpu(), logprob=out["logprob"][r].cpu(),
                k=out["k"][:, r].cpu(), v=out["v"][:, r].cpu())


def _sampled_rows(B):
    """0, 31, 32, B-1 and one row inside every other 32-row pass"""
    rows = {0, 31, 32, B - 1}
    for c0 in range(64, B - 1, 32):
        rows.add(c0 + (c0 // 32 * 5) % 32)
    return sorted(r for r in rows if r < B)


@pytest.mark.parametrize("B,T", CASES)
def test_wide_decode_step_vs_oracle_and_32_row_chunks(geo, monkeypatch, B, T):
    """A B-row greedy step (B > 32), eager and replayed: (a) the sampled rows against the oracle; (b) every full 32-row pass against the same
    rows decoded as a 32-row batch of their own from the same post-prefill cache -- logits of every step, tokens, log-probs and the appended
    K / V rows BIT-identical (a row's bits must not depend on its batch mates); (c) the copies of rows 1 and 2 in later passes (incl. the
    remainder pass: 1 row at B = 33, 8 rows at B = 40) bit-identical to their originals; (d) replay bit-identical to the eager launches."""
    name, kw, sd, eng = geo
    pcy_disable(monkeypatch)
    monkeypatch.delenv("PCY_MB_MAX", raising=False)
    emb, mask = _batch(B, T, kw["d"], seed=B * 100 + T)
    out, snap = _decode(eng, kw["vocab"], emb, mask, use_graph=False)
    assert torch.isfinite(out["logits"].float()).all()
    rep, _ = _decode(eng, kw["vocab"], emb, mask, use_graph=True)
    for key in out:
        assert torch.equal(out[key], rep[key]), (name, B, "replay", key)
    # (a) the oracle on the sampled rows
    rows = _sampled_rows(B)
    check_oracle(sd, kw, emb, mask, _rows(out, rows), rows, (name, B), N)
    # (c) copies in other passes
    for dst, src in ((32, 1), (B - 1, 2)) if B > 33 else ((32, 2),):
        a, b_ = _rows(out, [dst]), _rows(out, [src])
        for key in a:
            assert torch.equal(a[key], b_[key]), (name, B, dst, src, key)
    # (b) full 32-row passes as batches of their own
    for c0 in range(0, B - 31, 32):
        sl = slice(c0, c0 + 32)
        sub, _ = _decode(eng, kw["vocab"], emb[sl], mask[sl], use_graph=False, init=(snap[0][:, sl], snap[1][:, sl], snap[2][sl]))
        full = dict(logits=out["logits"][:, sl], tokens=out["tokens"][sl], logprob=out["logprob"][sl], k=out["k"][:, sl], v=out["v"][:, sl])
        for key in sub:
            assert torch.equal(sub[key], full[key]), (name, B, c0, key)


@pytest.mark.parametrize("off", ["gemv_mfma4", "gemv_lds"])
def test_wide_decode_gemv_twins_bit_identical(geo, monkeypatch, off):
    """40 rows (a full pass + an 8-row remainder): the older GEMV schedules (PCY_DISABLE=gemv_mfma4: gemv_mfma3_kernel; gemv_lds: weights
    through registers) keep the bits of the default, eager and replayed."""
    name, kw, sd, eng = geo
    monkeypatch.delenv("PCY_MB_MAX", raising=False)
    B, T = 40, 21
    emb, mask = _batch(B, T, kw["d"], seed=7)
    pcy_disable(monkeypatch)
    ref, _ = _decode(eng, kw["vocab"], emb, mask, use_graph=False)
    pcy_disable(monkeypatch, off)
    for use_graph in (False, True):
        got, _ = _decode(eng, kw["vocab"], emb, mask, use_graph=use_graph)
        for key in got:
            assert torch.equal(got[key], ref[key]), (name, off, use_graph, key)


# ---------------------------------------------------------------------------------------------- generate() above 32 rows (small model)
@pytest.fixture(scope="module")
def small():
    from oracle import esm_ref as ER
    from oracle import llama_ref as LR
    from procyon_amd import synth
    from procyon_amd import synthetic_model as SM
    model, w = SM.build("small", device="cuda", return_weights=True, max_new_tokens=32)
    g = w["geom"]
    prot = synth.protein_tokens([90, 41, 66, 23, 57], seed=3)
    return dict(model=model, w=w, lgeom=LR.LlamaGeom(**g["llama"]), egeom=ER.EsmGeom(**g["esm"]), prot=prot)


def _prompts(n, seed):
    """n ragged prompts with one or two protein slots each -> (instructions, protein slots)"""
    g = torch.Generator().manual_seed(seed)
    instr, slots = [], []
    for i in range(n):
        words = lambda k: " ".join(f"w{int(x)}" for x in torch.randint(1, 10, (k,), generator=g))
        two = i % 3 == 1
        instr.append(f"{words(1 + i % 4)} <|protein|> " + (f"and {words(1 + i % 2)} <|protein|> " if two else "") + f"{words(1 + (i * 5) % 7)} [ANSWER]")
        slots.append([i % 5, (i + 2) % 5] if two else [i % 5])
    return instr, slots


def _gen_inputs(env, instr, slots):
    prot = env["prot"]
    return {"data": {"seq": prot, "seq_idx": torch.arange(prot.shape[0]), "text": [], "drug": None},
            "input": {"seq": [list(s) for s in slots], "text": [[] for _ in slots], "drug": None},
            "target": {"seq": None, "text": None, "drug": None}, "instructions": list(instr)}


def _oracle_embeds(env, inputs):
    """the oracle's `_preprocessing`: ESM -> pool -> token projector -> tokenise (left-padded) / splice"""
    from oracle import procyon_ref as PR
    m, w = env["model"], env["w"]
    z = PR.esm_plm_forward(w["esm"], env["egeom"], inputs["data"]["seq"], pooling="mean")
    idx = [i for row in inputs["input"]["seq"] for i in row]
    soft = PR.mlp_forward(z[idx], w["projs"]["aaseq"])
    ids, mask = m._prepare_text_inputs_and_tokenize(list(inputs["instructions"]), [[] for _ in inputs["input"]["seq"]],
                                                    crop_off=True, no_pad=True, left_pad=True)
    emb, _ = PR.prepare_input_embeddings(w["llama"]["model.embed_tokens.weight"], ids.long(), m.prot_replacement_idx, soft,
                                         ret_idx=m.prot_retrieval_idx)
    return emb, mask


@pytest.mark.parametrize("n,group", [(4, 2), (4, 5), (16, 2), (16, 5)])
def test_generate_beam_over_32_rows_matches_oracle(small, n, group):
    """`generate(method="beam")`, beam 10: 4 prompts (40 rows per step) and 16 prompts (160 rows: the evaluation plugin's default batch),
    group sizes 2 and 5, against the oracle's diverse beam search; per prompt, the tie-aware rule of tests/beam_oracle.py."""
    from oracle import llama_ref as LR
    m, w = small["model"], small["w"]
    instr, slots = _prompts(n, seed=n * 10 + group)
    emb, mask = _oracle_embeds(small, _gen_inputs(small, instr, slots))
    enc = LR.make_text_encoder(w["llama"], small["lgeom"])
    trace = []
    kw = dict(max_len=6, beam_size=10, beam_group_size=group, diversity_penalty=0.8)
    t_ref, s_ref, lg_ref = LR.beam_search(enc, emb, mask, vocab_size=small["lgeom"].vocab, eos_id=m.tokenizer.eos_token_id, trace=trace, **kw)
    tokens, scores, logits, _ = m.generate(_gen_inputs(small, instr, slots), method="beam", **kw)
    assert_beam_matches_oracle(tokens, scores, logits, t_ref, s_ref, lg_ref, trace)


def test_generate_beam_160_rows_variants_agree(small, monkeypatch):
    """16 prompts x beam 10: the replayed chain (two-launch K / V reorder with the slot count read from the device: the one-pass permute
    covers <= 32 rows only), the four calls per step (PCY_DISABLE=beam_graph) and the reorder over every slot (beam_kv_suffix) give EQUAL
    tokens, scores and logits records."""
    from procyon_amd.engine import Context
    m = small["model"]
    instr, slots = _prompts(16, seed=5)
    kw = dict(max_len=9, method="beam", beam_size=10, beam_group_size=5, diversity_penalty=0.8)
    res = []
    for off in ("", "beam_graph", "beam_kv_suffix", "beam_graph,beam_kv_suffix"):
        pcy_disable(monkeypatch, *off.split(","))
        res.append(m.generate(_gen_inputs(small, instr, slots), **kw)[:3])
        Context.get().sync()
    assert torch.isfinite(res[0][2].float()).all()
    for r in res[1:]:
        for x, y in zip(r, res[0]):
            assert torch.equal(x, y)


def test_generate_greedy_40_prompts_matches_oracle(small):
    """`generate(method="greedy")` over 40 prompts (a 40-row step) against the oracle's greedy loop: step-0 logits within the bf16 noise,
    and every row's tokens equal up to the first step whose oracle top-2 margin lies inside 4 x the logit noise."""
    from oracle import llama_ref as LR
    m, w = small["model"], small["w"]
    instr, slots = _prompts(40, seed=11)
    emb, mask = _oracle_embeds(small, _gen_inputs(small, instr, slots))
    L_ = 8
    tok_ref, lg_ref, _ = LR.greedy_generate(w["llama"], small["lgeom"], emb, mask, L_)
    tokens, _, logits, _ = m.generate(_gen_inputs(small, instr, slots), max_len=L_, method="greedy")
    assert tokens.shape == (40, 1, L_)
    assert rel_err(logits[:, 0, 0], lg_ref[:, 0]) < 1e-2
    for b in range(40):
        for s_ in range(L_):
            if tokens[b, 0, s_] != tok_ref[b, s_]:
                top2 = lg_ref[b, s_].float().topk(2).values
                noise = float((logits[b, 0, s_].float() - lg_ref[b, s_].float()).abs().max())
                assert float(top2[0] - top2[1]) <= 4 * noise, (b, s_)
                break
            assert rel_err(logits[b, 0, s_], lg_ref[b, s_]) < 2e-2, (b, s_)
