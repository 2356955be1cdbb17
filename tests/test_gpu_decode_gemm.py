"""The opt-in decode step for more than 32 rows that reads the weights once (pcy_llama_decode_gemm): every projection and lm_head
one MFMA GEMM over all B rows, the attention the default loop's launch.  Its bits are NOT the default step's; what is promised, and held here:
the oracle on sampled rows (the project's bar and near-tie rule, fulldepth_common.check_oracle), bit-identity of equal rows within a call
whatever M tile they sit in, bit-identity of a repeated call, equal results on the shared-prefix and the plain beam cache, the drivers
(`generate` beam / greedy / sampling with decode_gemm=True, "auto") against the oracle, a counter of its own that proves the step ran while
the default step's counters stand still, and argument errors that launch nothing.

The batches, the sampled rows and the generate() inputs restate those of tests/test_gpu_decode_wide.py (the default path above 32 rows)."""
import pytest
import torch

from beam_oracle import assert_beam_matches_oracle
from conftest import pcy_disable, rel_err
from fulldepth_common import check_oracle, decode_counts

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GEOMS = {
    "llama8b": dict(vocab=4096, d=4096, n_layers=2, n_heads=32, n_kv_heads=8, ffn=14336),
    "split": dict(vocab=2048, d=4096, n_layers=2, n_heads=32, n_kv_heads=32, ffn=11008),
    "small": dict(vocab=128263 - 128000 + 2048, d=256, n_layers=2, n_heads=4, n_kv_heads=2, ffn=512),   # synthetic_model "small"
}
N = 3          # cached decode steps per case
# (geometry, B, T): every batch is ragged.  33: one row past a 32-row tile; (40, 30): the appended slots 30..32 cross a 32-key block;
# 257 (small geometry only): one row past a 256-row tile
CASES = [(g, B, T) for g in GEOMS for B, T in ((33, 24), (40, 21), (160, 12), (40, 30))] + [("small", 257, 9)]

_engines = {}


def _geo(name):
    """(kw, state dict, engine) of a geometry, built once per session"""
    if name not in _engines:
        from procyon_amd import synth
        from procyon_amd.engine import LlamaConfig, LlamaEngine
        kw = GEOMS[name]
        sd = synth.llama_state_dict(**kw)
        _engines[name] = (kw, sd, LlamaEngine(sd, LlamaConfig(**kw, max_pos=512)))
    return _engines[name]


def _count():
    from procyon_amd import _lib
    return int(_lib.load().pcy_debug_decode_gemm_count())


def _batch(B, T, d, seed):
    """embeddings [B, T, d] + a ragged mask [B, T]; row 32 is a copy of row 1 and row B-1 a copy of row 2 (for B = 33 they coincide: row 32
    is then a copy of row 2) -- the copies sit in other rows of an M tile, or in another M tile, than their originals."""
    g = torch.Generator().manual_seed(seed)
    emb = (torch.randn(B, T, d, generator=g) * 0.02).to(BF)
    mask = torch.ones(B, T)
    for b in range(B):
        mask[b, :(b * 7) % 11 if b % 3 else 0] = 0
    for dst, src in ((32, 1), (B - 1, 2)):
        emb[dst], mask[dst] = emb[src], mask[src]
    return emb, mask


def _decode(eng, V, emb, mask):
    """prefill + N greedy cached steps on the new step with the clean decode mask.
    -> dict of device tensors: logits [N+1, n, V], tokens [n, N+1], logprob [n], the appended K / V slots."""
    from procyon_amd.engine import Context, GenState
    n, T = mask.shape
    Tmax = T + N + 2
    cache = eng.new_cache(n, Tmax)
    keep = torch.ones(n, Tmax, dtype=torch.uint8, device="cuda")
    keep[:, :T] = mask.to("cuda", torch.uint8)
    st = GenState(n, V, N + 2, "cuda", keep=keep)
    logits, _ = eng.prefill(emb.cuda(), mask, cache, "last")
    st.logits.copy_(logits); st.pos.fill_(T)
    eng.pick(cache, st, n, advance_pos=False)
    lg = [logits]
    for _ in range(N):
        eng.decode_gemm(cache, st, n)
        eng.pick(cache, st, n, advance_pos=True)
        lg.append(st.logits.clone())
    Context.get().sync()
    return dict(logits=torch.stack(lg), tokens=st.tokens_out[:, :N + 1].clone(), logprob=st.logprob.clone(),
                k=cache.k[:, :, :, T:T + N].clone(), v=cache.v[:, :, :, T:T + N].clone())


def _rows(out, rows):
    """the sampled rows of every output, on the CPU"""
    r = torch.tensor(rows, device="cuda")
    return dict(logits=out["logits"][:, r].cpu(), tokens=out["tokens"][r].cpu(), logprob=out["logprob"][r].cpu(),
                k=out["k"][:, r].cpu(), v=out["v"][:, r].cpu())


def _sampled_rows(B):
    """0, 31, 32, B-1 and one row inside every other 32-row span"""
    rows = {0, 31, 32, B - 1}
    for c0 in range(64, B - 1, 32):
        rows.add(c0 + (c0 // 32 * 5) % 32)
    return sorted(r for r in rows if r < B)


@pytest.mark.parametrize("name,B,T", CASES)
def test_decode_gemm_step_vs_oracle_and_identities(monkeypatch, name, B, T):
    """A B-row greedy step on the new entry: (a) it ran -- its counter rises by exactly the number of steps while the default step's
    dispatch counters stand still; (b) the sampled rows against the oracle; (c) the copies of rows 1 and 2 bit-identical to their originals
    in logits, tokens, log-probs and appended K / V; (d) the same call made twice gives the same bits."""
    kw, sd, eng = _geo(name)
    pcy_disable(monkeypatch)
    emb, mask = _batch(B, T, kw["d"], seed=B * 100 + T)
    n0, d0 = _count(), decode_counts()
    out = _decode(eng, kw["vocab"], emb, mask)
    assert _count() - n0 == N and decode_counts() == d0
    assert torch.isfinite(out["logits"].float()).all()
    rows = _sampled_rows(B)
    worst = check_oracle(sd, kw, emb, mask, _rows(out, rows), rows, (name, B), N)
    print(f"decode_gemm {name} B={B} T={T}: worst rel. err vs the oracle {worst:.3e} on rows {rows}")
    for dst, src in ((32, 1), (B - 1, 2)) if B > 33 else ((32, 2),):
        a, b_ = _rows(out, [dst]), _rows(out, [src])
        for key in a:
            assert torch.equal(a[key], b_[key]), (name, B, dst, src, key)
    again = _decode(eng, kw["vocab"], emb, mask)
    for key in out:
        assert torch.equal(out[key], again[key]), (name, B, "repeat", key)


@pytest.mark.parametrize("name", list(GEOMS))
def test_generate_beam_decode_gemm_shared_and_plain_cache_agree(monkeypatch, name):
    """4 prompts x beam 10 (40 rows): generate_beam(decode_gemm=True) on the shared-prefix cache and, with PCY_DISABLE=beam_kv_shared, on
    the plain cache give EQUAL tokens, scores and logits records -- from the first decode step on, where every row's own suffix is still
    empty (*pos == prefix_T)."""
    kw, sd, eng = _geo(name)
    B, T, beam, L_ = 4, 13, 10, 5
    g = torch.Generator().manual_seed(31)
    emb = (torch.randn(B, T, kw["d"], generator=g) * 0.02).to(BF).cuda()
    mask = torch.ones(B, T)
    mask[1, :3] = 0; mask[3, :5] = 0
    res = []
    for off in ((), ("beam_kv_shared",)):
        pcy_disable(monkeypatch, *off)
        n0, d0 = _count(), decode_counts()
        res.append(eng.generate_beam(emb, mask, L_, beam, 2, 0.8, -1, L_ + 3, decode_gemm=True))
        assert _count() - n0 == L_ - 1 and decode_counts() == d0, (name, off)
    assert torch.isfinite(res[0][2].float()).all() and res[0][2].shape[:2] == (B * beam, L_)
    for x, y in zip(res[0], res[1]):
        assert torch.equal(x, y), name


# ---------------------------------------------------------------------------------------------- generate() on the new step (small model)
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
def test_generate_beam_decode_gemm_matches_oracle(small, n, group):
    """`generate(method="beam", decode_gemm=True)`, beam 10: 4 prompts (40 rows per step) and 16 prompts (160 rows), group sizes 2 and 5,
    against the oracle's diverse beam search; per prompt, the tie-aware rule of tests/beam_oracle.py."""
    from oracle import llama_ref as LR
    m, w = small["model"], small["w"]
    instr, slots = _prompts(n, seed=n * 10 + group)
    emb, mask = _oracle_embeds(small, _gen_inputs(small, instr, slots))
    enc = LR.make_text_encoder(w["llama"], small["lgeom"])
    trace = []
    kw = dict(max_len=6, beam_size=10, beam_group_size=group, diversity_penalty=0.8)
    t_ref, s_ref, lg_ref = LR.beam_search(enc, emb, mask, vocab_size=small["lgeom"].vocab, eos_id=m.tokenizer.eos_token_id, trace=trace, **kw)
    n0, d0 = _count(), decode_counts()
    tokens, scores, logits, _ = m.generate(_gen_inputs(small, instr, slots), method="beam", decode_gemm=True, **kw)
    assert _count() - n0 == kw["max_len"] - 1 and decode_counts() == d0      # (the EOS flag is looked at every 8 steps: none inside 6)
    assert_beam_matches_oracle(tokens, scores, logits, t_ref, s_ref, lg_ref, trace)


def test_generate_greedy_decode_gemm_40_prompts_matches_oracle(small):
    """`generate(method="greedy", decode_gemm=True)` over 40 prompts against the oracle's greedy loop: step-0 logits within the bf16 noise,
    and every row's tokens equal up to the first step whose oracle top-2 margin lies inside 4 x the logit noise."""
    from oracle import llama_ref as LR
    m, w = small["model"], small["w"]
    instr, slots = _prompts(40, seed=11)
    emb, mask = _oracle_embeds(small, _gen_inputs(small, instr, slots))
    L_ = 8
    tok_ref, lg_ref, _ = LR.greedy_generate(w["llama"], small["lgeom"], emb, mask, L_)
    n0, d0 = _count(), decode_counts()
    tokens, _, logits, _ = m.generate(_gen_inputs(small, instr, slots), max_len=L_, method="greedy", decode_gemm=True)
    assert _count() - n0 == L_ - 1 and decode_counts() == d0
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


def test_generate_sampling_decode_gemm_40_rows(small):
    """Sampling over 40 rows with injected uniform variates on the new step: (a) two calls with the same variates draw the same tokens and
    keep the same logits record; (b) every step's logits, the oracle teacher-forced on the drawn tokens, within check_oracle's bar
    (rel. err < 2e-2 per row and step); (c) the kernel's pre-sampling probability vector of step 1 against `_sampling_probs` of that step's
    logits: both are an fp32 softmax rounded once to bf16 whose normalisers add up in different orders, so a probability may differ by one
    bf16 ulp (<= 2^-7 relative) and no more."""
    from oracle import llama_ref as LR
    m, w = small["model"], small["w"]
    eng = m.text_encoder.engine
    instr, slots = _prompts(40, seed=17)
    emb, mask = _oracle_embeds(small, _gen_inputs(small, instr, slots))
    B, L_, temp = 40, 4, 0.7
    V = small["lgeom"].vocab
    u = torch.rand(L_ * B, generator=torch.Generator().manual_seed(5))
    n0, d0 = _count(), decode_counts()
    tok, lp, lg, (st, cache, _) = eng.generate_sampling(emb.cuda(), mask, L_, temperature=temp, nucleus_prob=None, keep_logits=True, uniforms=u,
                                                        decode_gemm=True)
    assert _count() - n0 == L_ - 1 and decode_counts() == d0
    tok, lg = tok.cpu(), lg.clone()
    tok2, _, lg2, _ = eng.generate_sampling(emb.cuda(), mask, L_, temperature=temp, nucleus_prob=None, keep_logits=True, uniforms=u, decode_gemm=True)
    assert torch.equal(tok, tok2.cpu()) and torch.equal(lg, lg2)
    # (b) the oracle, teacher-forced on the drawn tokens
    r = LR.llama_forward(w["llama"], small["lgeom"], inputs_embeds=emb, attn_mask=mask, logits_rows="last")
    for s_ in range(L_):
        if s_:      # (no mask in the cached steps: quirk Q1, as oracle.llama_ref.greedy_generate)
            r = LR.llama_forward(w["llama"], small["lgeom"], input_ids=tok[:, s_ - 1:s_].long(), attn_mask=None, past_kv=r["past_kv"], logits_rows="last")
        ref = r["logits"][:, -1].float()
        for b in range(B):
            assert rel_err(lg[b, s_].float(), ref[b]) < 2e-2, (b, s_, rel_err(lg[b, s_].float(), ref[b]))
    # (c) the probability vector the kernel forms from step 1's logits
    st.logits.copy_(lg[:, 1]); st.step.zero_()
    probs = torch.empty(B, V, dtype=BF, device="cuda")
    eng.sample_pick(cache, st, B, False, u.cuda(), temp, None, probs)
    eng.ctx.sync()
    p, p_ref = probs.cpu().float(), m._sampling_probs(lg[:, 1], temp, None).float()
    assert bool((p_ref > 0).any()) and ((p - p_ref).abs() <= 2.0 ** -7 * p_ref).all()


def test_decode_gemm_auto_follows_the_plan(monkeypatch):
    """decode_gemm="auto": one row below DECODE_GEMM_MIN_ROWS the counter stays put and the outputs are bit-equal to decode_gemm=False; at 160
    rows the new step runs."""
    from procyon_amd.engine import DECODE_GEMM_MIN_ROWS, decode_gemm_plan
    kw, sd, eng = _geo("small")
    pcy_disable(monkeypatch)
    L_ = 4
    B = DECODE_GEMM_MIN_ROWS - 1
    assert B >= 32 and not decode_gemm_plan(B, False, False) and decode_gemm_plan(160, False, False)
    emb, mask = _batch(max(B, 34), 11, kw["d"], seed=3)
    emb, mask = emb[:B].cuda(), mask[:B]
    n0 = _count()
    ref = eng.generate_greedy(emb, mask, L_, keep_logits=True, decode_gemm=False)[:3]
    got = eng.generate_greedy(emb, mask, L_, keep_logits=True, decode_gemm="auto")[:3]
    assert _count() == n0
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    emb, mask = _batch(160, 11, kw["d"], seed=4)
    eng.generate_greedy(emb.cuda(), mask, L_, decode_gemm="auto")
    assert _count() - n0 == L_ - 1


def test_decode_gemm_argument_errors_launch_nothing(monkeypatch):
    """A grouped cache, an engine with fp8 layers switched on, B beyond the cache's rows: PcyError, the cache and the logits unchanged, the
    counter unchanged."""
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import Context, GenState
    kw, sd, eng = _geo("small")
    pcy_disable(monkeypatch)
    B, T, V = 40, 10, kw["vocab"]
    emb, mask = _batch(B, T, kw["d"], seed=9)
    cache = eng.new_cache(B, T + 4)
    logits, _ = eng.prefill(emb.cuda(), None, cache, "last")
    st = GenState(64, V, 4, "cuda")
    st.pos.fill_(T)
    st.logits.fill_(1.0)
    prefix = eng.new_cache(4, T)
    eng.prefill(emb[:4].cuda(), None, prefix, "last")
    grouped = eng.new_grouped_cache(prefix, [10, 10, 10, 10], [T, T - 1, T, T - 2], 4)
    Context.get().sync()

    def refused(c, rows, match):
        k0, v0, n0, d0 = c.k.clone(), c.v.clone(), _count(), decode_counts()
        with pytest.raises(PcyError, match=match):
            eng.decode_gemm(c, st, rows)
        Context.get().sync()
        assert _count() == n0 and decode_counts() == d0
        assert torch.equal(c.k, k0) and torch.equal(c.v, v0) and bool((st.logits == 1.0).all())

    refused(grouped, B, "grouped")
    refused(cache, B + 1, "cache rows")
    eng.quantize_fp8()
    try:
        refused(cache, B, "fp8")
    finally:
        eng.set_fp8(False)
    n0 = _count()
    eng.decode_gemm(cache, st, B)          # ... and the same call is served once the fp8 layers are off
    Context.get().sync()
    assert _count() == n0 + 1 and torch.isfinite(st.logits[:B].float()).all()
