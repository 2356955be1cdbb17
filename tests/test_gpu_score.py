"""GPU: teacher-forced text scoring end to end -- `forward(compute_loss=True)`, the lazy `.loss`, `score_text`, `LlamaEngine.score` -- on
the small synthetic model against the oracle pipeline (oracle.llama_ref logits + the pinned HF loss definition, tests/test_score_cpu.py).

Bound against the oracle, per scored token and for `.loss`: with D the sup-norm distance, over the scored rows, between the model's OWN
`forward(full_logits=True)` logits and the oracle's,
    |token_nll - oracle| <= 2 D + 2 * 2^-7 * max|logit| + the operator's bar (tests/test_gpu_xent.py)
(LSE and the label logit are each 1-Lipschitz in the sup norm; the second term covers the GEMV-vs-GEMM rounding of the two lm_head paths).
Errors of the plumbing -- shift, masks, cropping, row map -- are O(1) and cannot hide under it."""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import score_common as SC
from conftest import record_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


@pytest.fixture(scope="module")
def env():
    from oracle import esm_ref as ER
    from oracle import llama_ref as LR
    e = SC.build_env()
    g = e["w"]["geom"]
    e["lgeom"], e["egeom"] = LR.LlamaGeom(**g["llama"]), ER.EsmGeom(**g["esm"])
    return e


@pytest.fixture(scope="module")
def scored(env):
    """the one-pass scoring forward of the three prompts, once"""
    m = env["model"]
    out = m.forward(SC.make_inputs(env), compute_loss=True, get_full_labels=True)
    real = out["outputs"].token_nll.shape[1]
    return dict(out=out, o=out["outputs"], labels=out["full_labels"], real=real)


def _oracle_logits(env, inputs):
    """oracle restatement of `_preprocessing` (as tests/test_gpu_unified.py) + the oracle decoder -> logits [B, real, V], real"""
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
    r = LR.llama_forward(w["llama"], env["lgeom"], inputs_embeds=emb[:, :real], attn_mask=mask[:, :real])
    return r["logits"], real


def test_counts_and_zeros(scored):
    o, lab, real = scored["o"], scored["labels"], scored["real"]
    assert lab.shape[1] >= real and o.token_nll.dtype == torch.float32 and o.token_nll.shape == (3, real)
    labelled = lab[:, 1:real] != -100
    assert o.n_tokens == int(labelled.sum()) and o.n_tokens >= 4 + 7 + 2       # the words behind [ANSWER] (+ the closing eos tokens)
    tn = o.token_nll.cpu()
    assert bool((tn[:, 0] == 0).all()) and bool((tn[:, 1:][~labelled] == 0).all())
    assert bool((tn[:, 1:][labelled] > 0).all())
    assert o.loss.dim() == 0 and o.loss.dtype == torch.float32
    assert torch.equal(o.loss, o.token_nll.sum(1).sum() / o.n_tokens)


def test_against_oracle(env, scored):
    m = env["model"]
    o, lab, real = scored["o"], scored["labels"][:, :scored["real"]], scored["real"]
    lg_ref, real_ref = _oracle_logits(env, SC.make_inputs(env))
    assert real_ref == real
    V = lg_ref.shape[-1]
    labelled = lab[:, 1:] != -100
    # oracle loss by the pinned definition, per token and as HF's mean
    ce = F.cross_entropy(lg_ref.float()[:, :-1].reshape(-1, V), lab[:, 1:].reshape(-1), ignore_index=-100, reduction="none").view(3, real - 1)
    loss_ref = F.cross_entropy(lg_ref.float()[:, :-1].reshape(-1, V), lab[:, 1:].reshape(-1), ignore_index=-100)
    # D: the model's own full logits against the oracle's, on the scored rows
    own = m.forward(SC.make_inputs(env), full_logits=True)["outputs"].logits.cpu()
    rows_ref, rows_own = lg_ref[:, :-1][labelled].float(), own[:, :-1][labelled].float()
    delta = float((rows_ref - rows_own).abs().max())
    # the operator's bar on these logits: 8 x max(torch's own fp32 error, one fp32 ulp at max(|lse|, |row max|))
    l64 = torch.logsumexp(rows_ref.double(), -1)
    nll64 = l64 - rows_ref.double().gather(1, lab[:, 1:][labelled][:, None])[:, 0]
    err_a = float((ce[labelled].double() - nll64).abs().max())
    big = torch.maximum(l64.abs(), rows_ref.max(-1).values.double().abs()).max()
    op_bar = 8 * max(err_a, 2.0 ** (math.floor(math.log2(float(big))) - 23))
    bar = 2 * delta + 2 * 2.0 ** -7 * float(rows_ref.abs().max()) + op_bar
    err_tok = float((o.token_nll.cpu()[:, 1:][labelled] - ce[labelled]).abs().max())
    err_loss = abs(float(o.loss) - float(loss_ref))
    print(f"score vs oracle: token_nll err {err_tok:.3e} loss err {err_loss:.3e} (loss {float(loss_ref):.4f}) D {delta:.3e} bar {bar:.3e}")
    record_parity("score/forward_vs_oracle", token_nll_err=err_tok, loss_err=err_loss, delta=delta, bar=bar, loss=float(loss_ref))
    assert err_tok <= bar and err_loss <= bar
    assert bar < 0.5      # the bound is far below what a shifted / mis-mapped row would cost (the loss of a random model is ~log V)


def test_lazy_loss_and_answer_logits_equal_the_one_pass_values(env, scored):
    from procyon_amd import _lib
    m, o = env["model"], scored["o"]
    lib = m.text_encoder.engine.ctx.lib
    n0 = lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT)
    out = m.forward(SC.make_inputs(env), get_full_labels=True)          # today's call: nothing extra runs in it
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT) == n0
    lazy = out["outputs"]
    assert torch.equal(lazy.answer_logits, o.answer_logits)              # the scoring pass hands back the same answer-row bits
    assert torch.equal(lazy.loss, o.loss) and torch.equal(lazy.token_nll, o.token_nll) and lazy.n_tokens == o.n_tokens
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT) == n0 + 1   # ... from ONE second pass, cached
    # nothing to score with: no loss
    enc = m.text_encoder
    emb = torch.randn(1, 5, enc.cfg.d).to(BF).cuda()
    assert enc(input_embeds=emb, lazy_hidden=True).loss is None


def test_score_text(env, scored):
    m = env["model"]
    s = m.score_text(SC.make_inputs(env))
    assert torch.equal(s["token_nll"], scored["o"].token_nll) and torch.equal(s["loss"], scored["o"].loss)
    assert s["seq_nll"].shape == (3,) and s["n_tokens"].tolist() == (scored["labels"][:, 1:scored["real"]] != -100).sum(1).tolist()
    assert torch.equal(s["seq_nll"].sum() / int(s["n_tokens"].sum()), s["loss"])
    assert torch.equal(s["perplexity"], torch.exp(s["loss"]))


def test_ranking_greedy_continuation_beats_random_tokens(env):
    """caption ranking: the model's own greedy continuation of a prompt is more likely than random tokens in its place.  Token ids of
    the synthetic tokenizer cannot be turned back into words, so the candidates are built as ids on the text encoder's engine."""
    m = env["model"]
    eng = m.text_encoder.engine
    n_new, T0 = 8, 12
    g = torch.Generator().manual_seed(11)
    prompt = torch.randint(0, 2000, (1, T0), generator=g)
    prompt[0, -1] = m.answer_idx
    tok, _, _, _ = eng.generate_greedy(eng.embed_tokens(prompt), torch.ones(1, T0), n_new)
    greedy = tok.view(1, -1).cpu().long()[:, :n_new]
    rand = torch.randint(0, 2000, (1, n_new), generator=g)
    ids = torch.cat([torch.cat([prompt, greedy], 1), torch.cat([prompt, rand], 1)], 0)
    labels = ids.clone()
    labels[:, :T0] = -100
    token_nll, n, _ = eng.score(eng.embed_tokens(ids), torch.ones(2, T0 + n_new), labels)
    seq = token_nll.sum(1).cpu()
    assert n == 2 * n_new and float(seq[1]) > float(seq[0]), seq


def test_bad_labels_and_empty_batches(env):
    from procyon_amd import _lib
    m = env["model"]
    enc, eng = m.text_encoder, m.text_encoder.engine
    V = enc.cfg.vocab
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 2000, (2, 9), generator=g)
    emb = eng.embed_tokens(ids)
    bad = ids.clone()
    bad[1, 4] = V
    with pytest.raises(ValueError):
        eng.score(emb, None, bad)
    with pytest.raises(ValueError):
        enc(input_embeds=emb, full_labels=bad, compute_loss=True, lazy_hidden=True)
    none = torch.full_like(ids, -100)
    lib = eng.ctx.lib
    n0 = lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT)
    token_nll, n, logits = eng.score(emb, None, none)
    assert n == 0 and logits is None and not bool(token_nll.any())
    out = enc(input_embeds=emb, full_labels=none, compute_loss=True, lazy_hidden=True, logit_positions=torch.tensor([8, 8]))
    assert math.isnan(float(out.loss)) and out.n_tokens == 0 and not bool(out.token_nll.any())
    assert lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT) == n0          # no scoring launch for a batch without labels
    ref = enc(input_embeds=emb, lazy_hidden=True, logit_positions=torch.tensor([8, 8]))
    assert torch.equal(out.logits, ref.logits)


def test_workspace_poison_changes_nothing(env, tmp_path):
    """PCY_DEBUG_POISON_WS=1 (read once per process: a child) fills the workspace with NaN patterns before every use; a kernel that read a
    partial, a label logit or a gathered row it had not written would show"""
    here = SC.scoring_results(env)
    path = str(tmp_path / "poison.pt")
    envv = dict(os.environ, PCY_DEBUG_POISON_WS="1")
    subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "score_common.py"), path], check=True, env=envv,
                   timeout=300)
    there = torch.load(path)
    assert set(here) == set(there)
    for k in here:
        assert torch.equal(here[k], there[k]), k
