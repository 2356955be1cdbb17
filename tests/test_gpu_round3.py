"""GPU tests added in round 3 for kernels / paths that shipped without one (round-2 review items 1 and 7):
  * `pcy_retrieval_topk` (bf16 similarities + rank kernel) and `pcy_retrieval_topk_f32` / `pcy_retrieval_scores_f32` vs a
    stable descending argsort of the oracle's scores, incl. exact ties, and `get_proteins_from_embedding` through them;
  * the dlopen'ed RCCL leg: `pcy_comm_unique_id -> pcy_comm_init -> pcy_allgather` on a world-1 communicator, and
    `embed_sharded` under backend "nccl", world 1;
  * the fused batch-1 decode launch beside a competing kernel on a second stream: identical tokens or a clean error;
  * nucleus sampling ignores the temperature (model_unified.py:899-901)."""
import os
import socket

import pytest
import torch

from conftest import pcy_disable, rel_err

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def rnd(*shape, seed=0, std=1.0, dtype=BF):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(dtype)


@pytest.fixture(scope="module")
def ctx():
    from procyon_amd.engine import Context
    return Context.get()


def _stable_desc(scores):
    """indices of a stable descending sort of each row (ties: the lower index first)"""
    return torch.argsort(scores, dim=-1, descending=True, stable=True)


@pytest.mark.parametrize("Q,N,k", [(1, 513, 1), (1, 513, 10), (1, 513, 513), (40, 513, 10), (1, 18174, 20), (40, 18174, 10), (2, 18174, 18174)])
def test_retrieval_topk_bf16_vs_stable_argsort(ctx, Q, N, k):
    """`pcy_retrieval_topk`: the SAME bf16 similarities as `pcy_retrieval_scores` (checked against the oracle there), ranked;
    bf16 cosines tie by the hundred at N = 18174, so the order is checked against a stable argsort of the kernel's own scores
    and the scores against the oracle."""
    from oracle.procyon_ref import retrieval_scores
    D = 1280
    q, t = rnd(Q, D, seed=1), rnd(N, D, seed=2)
    sims = ctx.retrieval_scores(q.cuda(), t.cuda()).cpu()
    idx, sc = ctx.retrieval_topk(q.cuda(), t.cuda(), k)
    idx, sc = idx.cpu(), sc.cpu()
    assert idx.shape == (Q, k) and sc.shape == (Q, k) and sc.dtype == BF
    order = _stable_desc(sims.float())[:, :k]
    assert torch.equal(idx, order)
    assert torch.equal(sc, torch.gather(sims, 1, order))
    ref = retrieval_scores(q, t)
    assert rel_err(sc.double(), torch.gather(ref, 1, order)) < 1e-2


@pytest.mark.parametrize("tdtype", [torch.float32, BF])
@pytest.mark.parametrize("Q,N,k", [(1, 513, 10), (40, 513, None), (1, 18174, 20), (9, 18174, 10), (3, 100003, 50)])
def test_retrieval_topk_f32_vs_oracle(ctx, Q, N, k, tdtype):
    """fp32 scoring of the shim entry points: scores within fp32 rounding of the oracle's F.normalize + matmul, ranking equal to the
    stable argsort of the kernel's own scores, and equal to the oracle's ranking wherever neighbouring scores are further
    apart than the fp32 accumulation noise."""
    import torch.nn.functional as F
    D = 1280
    q = rnd(Q, D, seed=3, dtype=torch.float32)
    t = rnd(N, D, seed=4, dtype=tdtype)
    ref = F.normalize(q.double()) @ F.normalize(t.double()).T
    sims = ctx.retrieval_scores_f32(q, t).cpu()
    assert sims.dtype == torch.float32 and float((sims.double() - ref).abs().max()) < 2e-6
    idx, sc = ctx.retrieval_topk_f32(q, t, k)
    idx, sc = idx.cpu(), sc.cpu()
    kk = N if k is None else k
    order = _stable_desc(sims)[:, :kk]
    assert torch.equal(idx, order) and torch.equal(sc, torch.gather(sims, 1, order))
    ref_order = _stable_desc(ref)[:, :kk]
    ref_sorted = torch.gather(ref, 1, ref_order)
    clear = torch.ones_like(ref_order, dtype=torch.bool)          # positions whose neighbours in the reference ranking are > 1e-5 away
    gap = (ref_sorted[:, :-1] - ref_sorted[:, 1:]) > 1e-5
    clear[:, 1:] &= gap
    clear[:, :-1] &= gap
    assert torch.equal(idx[clear], ref_order[clear])
    assert clear.float().mean() > 0.5


def test_retrieval_rank_exact_ties_and_signed_zero(ctx):
    """duplicated target rows give bit-equal scores: the lower index must come first; -0.0 ties with +0.0 (torch semantics)"""
    D, N = 64, 700
    t = rnd(N, D, seed=5, dtype=torch.float32)
    t[100] = t[7]; t[650] = t[7]; t[300] = t[299]
    t[500] = 0.0                                                # zero row: cosine +0.0
    q = rnd(2, D, seed=6, dtype=torch.float32)
    idx, sc = ctx.retrieval_topk_f32(q, t, None)
    idx, sc = idx.cpu(), sc.cpu()
    for r in range(2):
        pos = {int(i): p for p, i in enumerate(idx[r].tolist())}
        assert pos[7] + 1 == pos[100] and pos[100] + 1 == pos[650] and pos[299] + 1 == pos[300]
        assert sorted(idx[r].tolist()) == list(range(N))
        assert bool((sc[r, :-1] >= sc[r, 1:]).all())
    # bf16 kernel: a row of +0.0 / -0.0 scores sorts purely by index
    tb = torch.zeros(300, 64, dtype=BF)
    tb[::2, 0] = 1.0
    tb[1::2, 0] = -1.0
    qb = torch.zeros(1, 64, dtype=BF); qb[0, 1] = 1.0          # orthogonal to every target: scores are +0.0 and -0.0
    idx_b, sc_b = ctx.retrieval_topk(qb.cuda(), tb.cuda(), None)
    assert float(sc_b.float().abs().max()) == 0.0 and idx_b.cpu()[0].tolist() == list(range(300))


def test_get_proteins_from_embedding_through_the_device_ranking(ctx):
    """`get_proteins_from_embedding` / `get_proteins_from_batched_embeddings` (data/inference_utils.py:921-999) over the fp32 kernels"""
    import pandas as pd
    import torch.nn.functional as F
    from procyon.data.inference_utils import get_proteins_from_batched_embeddings, get_proteins_from_embedding
    N, D = 2000, 1280
    emb = rnd(N, D, seed=7, dtype=torch.float32)
    query = rnd(1, D, seed=8)                                   # bf16, as the bf16 model produces it
    ids = pd.DataFrame({"protein_id": [f"P{i:05d}" for i in range(N)], "name": [f"n{i}" for i in range(N)]})
    df = get_proteins_from_embedding(emb, query_embeddings=query, protein_ids=ids, top_k=20)
    ref = (F.normalize(query.double()) @ F.normalize(emb.double()).T)[0]
    order = torch.argsort(ref, descending=True)[:20]
    assert list(df.columns) == ["uniprot_id", "name", "sim_score"] and len(df) == 20
    assert df["uniprot_id"].tolist() == [f"P{int(i):05d}" for i in order]
    assert max(abs(a - float(b)) for a, b in zip(df["sim_score"].tolist(), ref[order])) < 2e-6
    out = {"contrastive_out": {"positive": {"text": torch.cat([query, query * 0 + 1]).cuda()}}}
    df2 = get_proteins_from_embedding(emb, model_out=out, protein_ids=ids, top_k=None)
    assert len(df2) == N and df2["uniprot_id"].tolist()[:20] == df["uniprot_id"].tolist()
    sims = get_proteins_from_batched_embeddings(emb, query_embeddings=torch.cat([query, query]).float())
    assert sims.shape == (2, N) and sims.dtype == torch.float32 and sims.device.type == "cpu"
    assert float((sims[0].double() - ref).abs().max()) < 2e-6


# ---------------------------------------------------------------------------------------------- RCCL leg
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def test_world1_rccl_communicator_through_the_c_abi(ctx):
    """`pcy_comm_unique_id -> pcy_comm_init -> pcy_allgather -> pcy_comm_destroy` on a one-rank communicator: the dlopen'ed RCCL
    links, initialises and moves the bytes on the engine's stream (recv == send)."""
    import ctypes as C
    from procyon_amd import _lib as L
    lib = ctx.lib
    idbuf = C.create_string_buffer(128)
    L.check(lib.pcy_comm_unique_id(idbuf), "pcy_comm_unique_id")
    assert any(b != 0 for b in idbuf.raw)
    comm = C.c_void_p()
    L.check(lib.pcy_comm_init(ctx.h, 1, 0, idbuf, C.byref(comm)), "pcy_comm_init")
    assert comm.value
    send = rnd(125, 1280, seed=9).cuda()
    recv = torch.zeros_like(send)
    L.check(lib.pcy_allgather(ctx.h, comm, C.c_void_p(send.data_ptr()), C.c_void_p(recv.data_ptr()), send.numel() * 2), "pcy_allgather")
    ctx.sync()
    assert torch.equal(recv, send)
    lib.pcy_comm_destroy(comm)


def test_embed_sharded_under_nccl_world1():
    """the sharded retrieval path with backend "nccl" (= RCCL), world size 1: `embed_sharded` takes the C-ABI all-gather branch"""
    import torch.distributed as td
    from procyon_amd import distributed as D
    from procyon_amd import synth
    from procyon_amd.engine import EsmConfig, EsmEngine
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    td.init_process_group("nccl", rank=0, world_size=1)
    try:
        kw = dict(d=128, n_layers=2, n_heads=2, ffn=256)
        eng = EsmEngine(synth.esm_state_dict(**kw), EsmConfig(**kw))
        lens = [40, 25, 61, 18, 33, 47, 52]
        toks = synth.protein_tokens(lens, seed=3)
        calls = []
        orig = D.PcyComm.all_gather

        def spy(self, local):
            calls.append(tuple(local.shape))
            return orig(self, local)

        D.PcyComm.all_gather = spy
        try:
            out = D.embed_sharded(lambda t: eng.forward(t), lambda idx: toks[torch.tensor(idx)], len(lens), batch_size=3)
        finally:
            D.PcyComm.all_gather = orig
        torch.cuda.synchronize()
        assert calls == [(7, 128)]
        # row i == the protein encoded alone in its own batch of 3 (packing invariance makes the batch mates irrelevant)
        ref = torch.cat([eng.forward(toks[s:s + 3]) for s in range(0, 7, 3)])
        assert torch.equal(out, ref)
    finally:
        td.destroy_process_group()


# ---------------------------------------------------------------------------------------------- hardening of the fused decode launch
def test_fused_decode_beside_a_competing_kernel_is_identical_or_a_clean_error():
    """The batch-1 decode step runs all 32 layers as ONE launch whose 256 workgroups hand vectors to each other; they must all
    be resident.  A long-running kernel on a second stream takes CUs away: the step must then either still produce the tokens of
    the undisturbed run, or fail with a PcyError from an ABI call (watchdog -> host-visible sticky error) -- never return
    silently different tokens and never hang."""
    from procyon_amd import _lib as L
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    kw = dict(vocab=4096, d=4096, n_layers=4, n_heads=32, n_kv_heads=8, ffn=14336)     # the geometry the fused launch covers
    eng = LlamaEngine(synth.llama_state_dict(**kw, device="cuda"), LlamaConfig(**kw, max_pos=512))
    emb = eng.embed_tokens(torch.randint(0, 4096, (1, 48), generator=torch.Generator().manual_seed(1)))
    tok_ref, _, _, _ = eng.generate_greedy(emb, None, 65)
    eng.ctx.sync()
    tok_ref = tok_ref.cpu()
    side = torch.cuda.Stream()
    a = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
    outcome = None
    try:
        with torch.cuda.stream(side):
            for _ in range(40):                                  # ~10 ms of full-chip GEMM per iteration, queued ahead
                a @ a
        tok, _, _, _ = eng.generate_greedy(emb, None, 65)
        eng.ctx.sync()
        outcome = "identical" if torch.equal(tok.cpu(), tok_ref) else "different"
    except L.PcyError as e:
        assert "timed out" in str(e)
        outcome = "clean error"
    finally:
        torch.cuda.synchronize()
    print("fused decode beside a competing GEMM stream:", outcome)
    assert outcome in ("identical", "clean error")
    # the context recovers: the sticky word was consumed by the failing call
    tok2, _, _, _ = eng.generate_greedy(emb, None, 65)
    eng.ctx.sync()
    assert torch.equal(tok2.cpu(), tok_ref)


def test_nucleus_ignores_temperature():
    """model_unified.py:899-901: the nucleus branch is softmax(logits) * mask; `temperature` only enters the plain sampling branch"""
    from procyon_amd import synth
    from procyon_amd.engine import GenState, LlamaConfig, LlamaEngine
    kw = dict(vocab=2000, d=256, n_layers=2, n_heads=4, n_kv_heads=2, ffn=512)
    eng = LlamaEngine(synth.llama_state_dict(**kw, device="cuda"), LlamaConfig(**kw, max_pos=128))
    emb = eng.embed_tokens(torch.randint(0, 2000, (2, 9), generator=torch.Generator().manual_seed(2)))
    u = torch.rand(12 * 2, generator=torch.Generator().manual_seed(3))
    a = eng.generate_sampling(emb, None, 12, temperature=1.0, nucleus_prob=0.9, uniforms=u)[0].cpu()
    b = eng.generate_sampling(emb, None, 12, temperature=0.5, nucleus_prob=0.9, uniforms=u)[0].cpu()
    c = eng.generate_sampling(emb, None, 12, temperature=0.5, nucleus_prob=None, uniforms=u)[0].cpu()
    d = eng.generate_sampling(emb, None, 12, temperature=1.0, nucleus_prob=None, uniforms=u)[0].cpu()
    assert torch.equal(a, b)
    assert not torch.equal(c, d)          # ... while plain sampling does depend on it


# ---------------------------------------------------------------------------------------------- single-pass ESM attention
def _attn_fp64(q, k, v, lens, H, dh):
    outs, t0 = [], 0
    for n in lens:
        qs, ks, vs = (x[t0:t0 + n].double().view(n, H, dh).transpose(0, 1) for x in (q, k, v))
        p = torch.softmax(qs @ ks.transpose(1, 2), dim=-1)
        outs.append((p @ vs).transpose(0, 1).reshape(n, H * dh))
        t0 += n
    return torch.cat(outs)


def _dispatch(kind):
    from procyon_amd import _lib as L
    return L.load().pcy_debug_dispatch_count(kind)


@pytest.mark.parametrize("lens", [[1026], [64, 1, 33, 700, 257, 1026, 63, 65, 128]])
def test_attention_single_pass_vs_fp64(ctx, monkeypatch, lens):
    """`attn_fast64_kernel` (head_dim 64, bidirectional, varlen): against an fp64 evaluation of the same bf16 inputs it must be at
    least as close as the exact-rounding two-pass kernel (which reproduces the reference's bf16 rounding points), on ragged
    lengths incl. 1, 63/64/65 (tile edges) and 1026 (the ESM chunk size)."""
    from procyon_amd import _lib as L
    H, dh = 3, 64
    n = sum(lens)
    q, k, v = rnd(n, H * dh, seed=1, std=0.35), rnd(n, H * dh, seed=2), rnd(n, H * dh, seed=3)
    ref = _attn_fp64(q, k, v, lens, H, dh)
    monkeypatch.setenv("PCY_ESM_ATTN", "exact")
    n0 = _dispatch(L.DISPATCH_ATTN_FAST)
    exact = ctx.attention(q.cuda(), k.cuda(), v.cuda(), lens, H, H, dh, False, 1.0).cpu()
    assert _dispatch(L.DISPATCH_ATTN_FAST) == n0
    monkeypatch.setenv("PCY_ESM_ATTN", "fast")
    fast = ctx.attention(q.cuda(), k.cuda(), v.cuda(), lens, H, H, dh, False, 1.0).cpu()
    assert _dispatch(L.DISPATCH_ATTN_FAST) == n0 + 1
    e_exact, e_fast = rel_err(exact.double(), ref), rel_err(fast.double(), ref)
    worst = float((fast.double() - ref).abs().max())
    print(f"lens {lens[:3]}..: err(exact, fp64) {e_exact:.3e}  err(fast, fp64) {e_fast:.3e}  max|fast - fp64| {worst:.3e}  err(fast, exact) {rel_err(fast.double(), exact.double()):.3e}")
    assert e_fast <= 1.1 * e_exact and e_fast < 4e-3
    assert worst < 0.05


def test_attention_single_pass_forced_rescale_and_outliers(ctx, monkeypatch):
    """The deferred-maximum branch is data dependent and rare on random data (CDNA4 guide, rule 26): spike single keys against
    single queries so that a row's maximum jumps by far more than the 2^10 threshold in a chosen LATE tile (and in the first
    one, and twice in a row), and compare the full tensor with fp64."""
    H, dh, n = 2, 64, 1026
    g = torch.Generator().manual_seed(5)
    q = torch.randn(n, H * dh, generator=g) * 0.3
    k, v = torch.randn(n, H * dh, generator=g), torch.randn(n, H * dh, generator=g)
    for (qi, ki, gain) in [(5, 700, 40.0), (5, 900, 90.0), (37, 3, 60.0), (64, 64, 50.0), (1025, 1024, 45.0), (300, 1025, 70.0), (301, 31, 55.0)]:
        k[ki, :dh] = q[qi, :dh] * gain / float(q[qi, :dh].norm() ** 2) * 8.0       # q.k = 8 * gain / ... : a score far above the rest of the row
    q, k, v = q.to(BF), k.to(BF), v.to(BF)
    ref = _attn_fp64(q, k, v, [n], H, dh)
    monkeypatch.setenv("PCY_ESM_ATTN", "fast")
    out = ctx.attention(q.cuda(), k.cuda(), v.cuda(), [n], H, H, dh, False, 1.0).cpu()
    assert torch.isfinite(out.float()).all()
    err = rel_err(out.double(), ref)
    worst = float((out.double() - ref).abs().max())
    print(f"spiked keys: err(fast, fp64) {err:.3e}  max abs {worst:.3e}")
    assert err < 4e-3 and worst < 0.06
    # rows dominated by one key: the output is that key's V row
    assert rel_err(out[5, :dh].double(), ref[5, :dh]) < 4e-3


def test_esm_layer_stack_fast_vs_exact_attention(monkeypatch):
    """encoder level: the single-pass attention moves a 4-layer ESM2-650M-width stack by no more than the reference's own bf16
    reproducibility floor (two CPU evaluations with different accumulation orders differ by as much)"""
    from procyon_amd import synth
    from procyon_amd.engine import EsmConfig, EsmEngine
    kw = dict(d=1280, n_layers=4, n_heads=20, ffn=5120)
    eng = EsmEngine(synth.esm_state_dict(**kw, device="cuda"), EsmConfig(**kw))
    toks = synth.protein_tokens([1024, 300, 77], seed=4)
    monkeypatch.setenv("PCY_ESM_ATTN", "exact")
    a = eng.hidden_states(toks).float()
    monkeypatch.setenv("PCY_ESM_ATTN", "fast")
    b = eng.hidden_states(toks).float()
    e = rel_err(b, a)
    print(f"4-layer ESM2-650M-width stack: err(fast attention, exact attention) {e:.3e}")
    assert e < 8e-3


# ---------------------------------------------------------------------------------------------- full sub-module outputs (waist contract)
def test_llama_forward_full_logits_and_hidden_states_tuple():
    """`LlamaPostTokenization.forward` with the reference's arguments only returns the reference's object (pmc_llama.py:575-596):
    `.logits` [B,T,V] for every row and `.hidden_states` = the L+1 tuple (embeddings, layer outputs, final-normed last state),
    which route B of INTEGRATION.md (the reference's own UnifiedProCyon over these sub-modules) reads at model_unified.py:556-563."""
    from oracle import llama_ref as LR
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig
    from procyon_amd.model import LlamaPostTokenization
    kw = dict(vocab=331, d=256, n_layers=3, n_heads=4, n_kv_heads=2, ffn=512)
    sd = synth.llama_state_dict(**kw)
    enc = LlamaPostTokenization({k: v.clone() for k, v in sd.items()}, LlamaConfig(**kw, max_pos=256), torch.device("cuda"), 8)
    g = torch.Generator().manual_seed(3)
    B, T = 2, 70                                   # 140 rows > 64: the lm_head runs as a GEMM
    ids = torch.randint(0, 331, (B, T), generator=g)
    mask = torch.ones(B, T, dtype=torch.long); mask[1, -9:] = 0
    emb = torch.nn.functional.embedding(ids, sd["model.embed_tokens.weight"])
    out = enc(input_embeds=emb.cuda(), attn_masks=mask)
    ref = LR.llama_forward(sd, LR.LlamaGeom(**kw), inputs_embeds=emb, attn_mask=mask, want_hidden=True)
    assert out.logits.shape == (B, T, 331) and len(out.hidden_states) == kw["n_layers"] + 1
    assert isinstance(out.hidden_states, tuple)                # torch.stack takes tuples / lists of tensors only
    valid = mask.bool()
    assert rel_err(out.logits.cpu()[valid], ref["logits"][valid]) < 1e-2
    hs = [h.cpu() for h in out.hidden_states]
    assert torch.equal(hs[0], emb)
    for i, (a, b) in enumerate(zip(hs, ref["hidden_states"])):
        assert a.shape == (B, T, 256) and rel_err(a[valid], b[valid]) < 6e-3, i
    # the engine-backed model's fast path (lazy_hidden=True): the last state == the tuple's, other accesses materialise the rest
    lazy = enc(input_embeds=emb.cuda(), attn_masks=mask, lazy_hidden=True)
    assert not isinstance(lazy.hidden_states, tuple) and torch.equal(lazy.hidden_states[-1].cpu(), hs[-1])
    assert torch.equal(lazy.hidden_states[1].cpu(), hs[1]) and len(lazy.hidden_states) == len(hs)
    # what ret_token_access='all' does with it, EXACTLY as the reference writes it (model_unified.py:563)
    summed = torch.stack(out.hidden_states, dim=-1).sum(dim=-1).cpu()
    assert rel_err(summed[valid], torch.stack(ref["hidden_states"], dim=-1).sum(dim=-1)[valid]) < 6e-3
    # eager form + the engine's row-limited sum agree with the tuple
    out2 = enc(input_embeds=emb.cuda(), attn_masks=mask, output_hidden_states=True, hidden_sum_positions=torch.tensor([3, 80]))
    assert torch.equal(out2.hidden_states[2], out.hidden_states[2])
    assert rel_err(out2.hidden_state_sum_rows.cpu(), summed.view(B * T, -1)[[3, 80]]) < 4e-3


def test_esm_plm_forward_aggregate_false_states_and_mlm_logits():
    """`ESM_PLM.forward(tokens, aggregate=False)` (esm.py:547-558): per-position states of split proteins laid end to end
    (`reverse_batched_split`) and the masked-LM logits, against the oracle's encoder + an op-by-op restatement of the head"""
    import torch.nn.functional as F
    from oracle import esm_ref as ER
    from oracle import procyon_ref as PR
    from procyon_amd import synth
    from procyon_amd.engine import EsmConfig
    from procyon_amd.model import ESM_PLM
    from procyon_amd.sequences import reverse_batched_split
    kw = dict(d=128, n_layers=2, n_heads=2, ffn=256)
    sd = synth.esm_state_dict(**kw)
    g = torch.Generator().manual_seed(8)
    r = lambda *s, std=0.05: (torch.randn(*s, generator=g) * std).to(BF)
    head = {"lm_head.dense.weight": r(128, 128), "lm_head.dense.bias": r(128), "lm_head.layer_norm.weight": (1 + r(128)).to(BF),
            "lm_head.layer_norm.bias": r(128), "lm_head.bias": r(33)}
    plm = ESM_PLM({**sd, **head}, EsmConfig(**kw), pooling_method="mean", max_protein_len=64, device=torch.device("cuda"))
    toks = synth.protein_tokens([150, 30, 64, 65], seed=5)       # 150 -> 3 chunks, 65 -> 2 chunks at max_protein_len 64
    z, logits = plm(toks, aggregate=False)
    rows, keys, eos = PR.batched_split_long_seq(toks, max_protein_len=64)
    h = ER.esm_forward(sd, ER.EsmGeom(**kw), rows)
    h = h * (rows != 1)[..., None]                              # pad positions: zero here
    z_ref = reverse_batched_split(h, keys, eos)
    assert z.shape == z_ref.shape == (4, 152, 128)
    assert rel_err(z.cpu(), z_ref) < 8e-3
    y = F.linear(h, head["lm_head.dense.weight"], head["lm_head.dense.bias"])
    y = ((y * 0.5) * (1.0 + torch.erf(y / 2 ** 0.5)))           # fair-esm `gelu`, each op materialised in bf16
    y = F.layer_norm(y, (128,), head["lm_head.layer_norm.weight"], head["lm_head.layer_norm.bias"], 1e-5)
    lg_ref = reverse_batched_split(F.linear(y, sd["esm.embeddings.word_embeddings.weight"], head["lm_head.bias"]), keys, eos)
    assert logits.shape == lg_ref.shape == (4, 152, 33)
    real = torch.zeros(4, 152, dtype=torch.bool)
    for i, n in enumerate([150, 30, 64, 65]):
        real[i, :n + 2] = True
    assert rel_err(logits.cpu()[real], lg_ref[real]) < 1.5e-2
    # a checkpoint without the head: states only
    z2, lg2 = ESM_PLM(sd, EsmConfig(**kw), pooling_method="mean", max_protein_len=64, device=torch.device("cuda"))(toks, aggregate=False)
    assert lg2 is None and torch.equal(z2, z)


# ---------------------------------------------------------------------------------------------- bulk scripts + service (row f4)
def _service_checkpoint(root, vocab, n_prot=20000, D=128):
    """checkpoint directory of an embedding-table model (use_aaseq_embeddings=True, the shipped ProCyon-Full layout): Llama-geometry
    decoder with head_dim 128, projectors, protein_seq_embeddings [n_prot, D], and the cached target matrix of the service"""
    from procyon.training.training_args_IT import DataArgs, ModelArgs
    from procyon_amd import synth
    kw = dict(vocab=vocab, d=256, n_layers=2, n_heads=2, n_kv_heads=1, ffn=512)
    sd = {"text_encoder.model." + k: v for k, v in synth.llama_state_dict(**kw).items()}
    for name, (i, o), off in (("token_projectors.aaseq", (D, 256), 0), ("aaseq_shared_projector", (D, D), 20), ("aaseq_lm_projector", (256, D), 40)):
        for j, (w, b) in zip((0, 3, 6), synth.mlp_layers(3, i, o, 128, off)):
            sd[f"{name}.{j}.weight"], sd[f"{name}.{j}.bias"] = w, b
    g = torch.Generator().manual_seed(77)
    table = (torch.randn(n_prot, D, generator=g) * 0.5).to(BF)
    sd["protein_seq_embeddings.weight"] = table
    os.makedirs(root, exist_ok=True)
    torch.save(ModelArgs(use_aaseq_embeddings=True, ret_token_access="last", protein_pooling_opt="mean", max_text_len=160), os.path.join(root, "model_args.pt"))
    torch.save(DataArgs(data_dir="/x"), os.path.join(root, "data_args.pt"))
    torch.save(sd, os.path.join(root, "txllm_model_ckpt.pt"))
    return sd, table


@pytest.fixture()
def instruct_env(tmp_path, monkeypatch):
    import gzip
    import json
    import synth_instruct as SI
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with gzip.open(os.path.join(root, "tests", "golden", "g11_prompts.json.gz"), "rt") as f:
        tasks = json.load(f)["tasks"]
    with gzip.open(os.path.join(root, "tests", "golden", "g13_input_builders.json.gz"), "rt") as f:
        tables = json.load(f)["tables"]
    data, home = SI.build_tree(str(tmp_path), tasks, tables)
    monkeypatch.setenv("DATA_DIR", data)
    monkeypatch.setenv("HOME_DIR", home)
    import procyon.data.constants as C
    import procyon.data.inference_utils as IU
    C._cache = None
    IU._LAZY.clear()
    return tmp_path


def test_bulk_caption_then_qa_filter_pipeline_matches_the_one_by_one_loops(instruct_env):
    """scripts/caption_bulk.py:99-148 and scripts/qa_filter_captions.py:63-100 batched across proteins / pairs: the tables equal those
    of the scripts' own one-prompt-per-call loops (restated here), the running pickle appears when the loop would have written it."""
    import pandas as pd
    from procyon.data.inference_utils import ProCyonQAInference, create_caption_input_simple, create_qa_input_simple, uniprot_id_to_index
    from procyon_amd.checkpoint import from_pretrained
    from procyon_amd.pipelines import caption_bulk, chunk_rows, qa_filter_captions
    from procyon_amd.tokenizer import SyntheticTokenizer
    tok = SyntheticTokenizer(n_text=2000, base_vocab=2048, bos_token_id=2040, eos_token_id=2041)
    ckpt = str(instruct_env / "ckpt")
    _service_checkpoint(ckpt, vocab=len(tok) - 1)
    model, margs = from_pretrained(checkpoint_dir=ckpt, tokenizer=tok, max_new_tokens=16, max_pos=512)
    from procyon.training.training_args_IT import DataArgs
    dargs = DataArgs()
    ids = [f"P{i:05d}" for i in (530, 7, 11, 19999, 5, 4242, 77)]
    save = str(instruct_env / "captions.out")
    seen = []
    real_to_pickle = pd.DataFrame.to_pickle

    def spy(self, path, *a, **k):
        seen.append(len(self))
        return real_to_pickle(self, path, *a, **k)

    pd.DataFrame.to_pickle = spy
    try:
        df = caption_bulk(model, margs, dargs, ids, "uniprot", "all", max_len=6, beam_size=4, diversity_penalty=0.8, save_path=save, batch_size=3)
    finally:
        pd.DataFrame.to_pickle = real_to_pickle
    assert list(df.columns) == ["uniprot_id", "response0", "response1"] and df["uniprot_id"].tolist() == ids
    assert seen == [6]                                            # i = 5 is the only i % 5 == 0, i > 0 among 7 proteins: rows 0..5
    assert pd.read_csv(save, index_col=0).shape == (7, 3)
    # the script's loop: one protein per generate call
    for i, u in enumerate(ids):
        inp = create_caption_input_simple(input_aaseq_ids=[uniprot_id_to_index(u)], data_args=dargs, instruction_source_dataset="uniprot",
                                          instruction_source_relation="all", aaseq_type="protein", task_type="caption", icl_example_number=1)
        _, _, _, text = model.generate(inputs=inp, aaseq_type="protein", max_len=6, method="beam", beam_size=4, beam_group_size=2,
                                       diversity_penalty=0.8)
        want = [t.split("<|end_of_text|>")[0] for j, t in enumerate(text[0]) if j % 2 == 0]
        assert [df["response0"].iloc[i], df["response1"].iloc[i]] == want, u
    # QA filter over the captions (template: omim_all_qa)
    qa = qa_filter_captions(model, dargs, df, "omim", "all", batch_size=4)
    assert list(qa.columns) == ["uniprot_id", "response_num", "caption_output", "yes", "no"] and len(qa) == 14
    assert qa["response_num"].tolist() == ["response0", "response1"] * 7
    qam = ProCyonQAInference(model, device=model.device)
    for k in (0, 5, 13):
        u, cap = qa["uniprot_id"].iloc[k], qa["caption_output"].iloc[k]
        one = qam(create_qa_input_simple(input_aaseq_ids=[uniprot_id_to_index(u)], data_args=dargs, input_description=cap,
                                         instruction_source_dataset="omim", instruction_source_relation="all", aaseq_type="protein",
                                         icl_example_number=1))["pred"]
        assert abs(one[0, qam.yes_token].item() - qa["yes"].iloc[k]) < 2e-3 * max(1e-3, abs(qa["yes"].iloc[k])) + 1e-6
        assert abs(one[0, qam.no_token].item() - qa["no"].iloc[k]) < 2e-3 * max(1e-3, abs(qa["no"].iloc[k])) + 1e-6
    # chunking rules of the two scripts
    assert chunk_rows(10, None, None) == (0, 10) and chunk_rows(10, 3, 0, "qa_filter_captions") == (0, 4)
    assert chunk_rows(10, 3, 2, "qa_filter_captions") == (8, 10) and chunk_rows(10, 3, 1, "caption_bulk") == (4, 8)


def test_fastapi_service_round_trip_on_a_synthetic_checkpoint(instruct_env, monkeypatch):
    """procyon/app/main.py: start-up loads $CHECKPOINT_PATH through `startup_retrieval` (tokenizer files from $LLAMA3_PATH -- a real
    PreTrainedTokenizerFast built in the container), POST /retrieve ranks the cached target matrix on the device."""
    import pandas as pd
    import torch.nn.functional as F
    import synth_tokenizer as ST
    from fastapi.testclient import TestClient
    from procyon_amd.checkpoint import hf_tokenizer
    tokdir = ST.build(str(instruct_env / "llama3"))
    tk = hf_tokenizer(tokdir)
    ckpt = str(instruct_env / "ckpt")
    _, table = _service_checkpoint(ckpt, vocab=len(tk) - 1)
    g = torch.Generator().manual_seed(5)
    targets = torch.randn(20000, 128, generator=g)                           # fp32, as the reference's cached matrix
    torch.save((targets, list(range(20000))), os.path.join(ckpt, "protein_target_embeddings.pkl"))
    for k, v in (("CHECKPOINT_PATH", ckpt), ("LLAMA3_PATH", tokdir)):
        monkeypatch.setenv(k, v)
    import procyon.app.main as APP
    with TestClient(APP.app) as client:
        r = client.post("/retrieve", json={"task_desc": "Find proteins linked to the condition.", "disease_desc": "a disease description",
                                           "instruction_source_dataset": "disgenet", "k": 7})
        assert r.status_code == 200, r.text
        rows = r.json()["results"]
        assert len(rows) == 7 and set(rows[0]) == {"uniprot_id", "name", "sim_score"}
        sims = [x["sim_score"] for x in rows]
        assert sims == sorted(sims, reverse=True)
        # the same query straight through the model: identical ranking
        model = APP.state["model"]
        from procyon.data.inference_utils import create_input_retrieval
        inp = create_input_retrieval(input_description="a disease description", data_args=APP.state["data_args"],
                                     task_definition="Find proteins linked to the condition.", instruction_source_dataset="disgenet")
        q = model(inputs=inp, retrieval=True, aaseq_type="protein")["contrastive_out"]["positive"]["text"][0].float().cpu()
        ref = F.normalize(q[None].double()) @ F.normalize(targets.double()).T
        top = torch.argsort(ref[0], descending=True)[:7].tolist()
        assert [x["uniprot_id"] for x in rows] == [f"P{i:05d}" for i in top]
        bad = client.post("/retrieve", json={"task_desc": "t", "disease_desc": "d", "instruction_source_dataset": "uniprot"})
        assert bad.status_code == 422
        allr = client.post("/retrieve", json={"task_desc": "t", "disease_desc": "d", "instruction_source_dataset": "disgenet"})
        assert allr.status_code == 200 and len(allr.json()["results"]) == 20000


# ---------------------------------------------------------------------------------------------- round 3, later: row order of the 256 x 256 GEMM, V path of the attention
@pytest.mark.parametrize("epi", [0, 1, 3, 4])
@pytest.mark.parametrize("M,N,K", [(2048 + 300, 1280 + 256 + 8, 1280), (2304, 2560, 2560)])
def test_gemm_permuted_row_order_bit_identical(ctx, monkeypatch, M, N, K, epi):
    """PCY_GEMM_PERM (mask per epilogue): the 256 x 256 kernels read the W rows in an order that leaves a lane 8 consecutive features
    (16-byte epilogue pieces) -- a relabelling of MFMA rows, so every epilogue (plain, residual, ESM GELU, SwiGLU; ragged M and N
    edges) must give the bits of the natural order."""
    from procyon_amd import _lib as L
    from procyon_amd.engine import interleave_gate_up
    A, b = rnd(M, K, seed=1).cuda(), rnd(N, seed=3).cuda()
    if epi == 4:
        N = N // 32 * 32
        W = interleave_gate_up(rnd(N // 2, K, seed=2, std=0.05), rnd(N // 2, K, seed=4, std=0.05)).cuda()
        b = None
    else:
        W = rnd(N, K, seed=2, std=0.05).cuda()
    r = rnd(M, N, seed=5).cuda() if epi == 1 else None
    outs = []
    for mask in ("0", "31"):
        monkeypatch.setenv("PCY_GEMM_PERM", mask)
        n0 = _dispatch(L.DISPATCH_GEMM_BIG) + _dispatch(L.DISPATCH_GEMM_BIG_PERSIST)
        outs.append(ctx.gemm(A, W, b, r, epi).cpu())
        assert _dispatch(L.DISPATCH_GEMM_BIG) + _dispatch(L.DISPATCH_GEMM_BIG_PERSIST) == n0 + 1     # the 256 x 256 kernels
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


@pytest.mark.parametrize("epi", [0, 1, 4])
def test_gemm_fp8_permuted_row_order_bit_identical(ctx, monkeypatch, epi):
    """the same for the e4m3 kernels (dequantisation scales applied inside the permuted epilogue)"""
    from procyon_amd import _lib as L
    from procyon_amd.engine import interleave_gate_up
    M, N, K = 700, 1536 + 64, 1024
    a8, sa = ctx.quant_rows_fp8(rnd(M, K, seed=1).cuda())
    W = rnd(N, K, seed=2, std=0.05)
    if epi == 4:
        W = interleave_gate_up(W[: N // 2].contiguous(), rnd(N // 2, K, seed=4, std=0.05))
    q8, sw = ctx.quant_rows_fp8(W.cuda())
    r = rnd(M, N, seed=5).cuda() if epi == 1 else None
    outs = []
    for mask in ("0", "31"):
        monkeypatch.setenv("PCY_GEMM_PERM", mask)
        n0 = _dispatch(L.DISPATCH_GEMM_FP8)
        outs.append(ctx.gemm_fp8(a8, sa, q8, sw, resid=r, epi=epi).cpu())
        assert _dispatch(L.DISPATCH_GEMM_FP8) == n0 + 1
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


def test_esm_layer_row_order_and_v_path_bit_identical(monkeypatch):
    """encoder level, one full-width ESM2-650M layer over ragged packed proteins (the only way to the fused-rotary epilogue): natural vs
    permuted W row order, and the single-pass attention reading V token-major (ds_read_b64_tr_b16) vs from a transposed copy -- all
    four combinations the same bits."""
    from procyon_amd import synth
    from procyon_amd.engine import EsmConfig, EsmEngine
    kw = dict(d=1280, n_layers=2, n_heads=20, ffn=5120)
    eng = EsmEngine(synth.esm_state_dict(**kw, device="cuda"), EsmConfig(**kw))
    toks = synth.protein_tokens([1024, 300, 77, 65, 1, 640], seed=4)
    monkeypatch.setenv("PCY_ESM_ATTN", "fast")
    outs = {}
    for mask in ("0", "7", "31"):
        for vrow in ("0", "1"):
            monkeypatch.setenv("PCY_GEMM_PERM", mask)
            pcy_disable(monkeypatch, "" if vrow == "1" else "fa_vrow")
            outs[(mask, vrow)] = eng.hidden_states(toks).cpu()
    keep = toks != 1
    ref = outs[("0", "0")]
    assert torch.isfinite(ref[keep].float()).all()
    for key, o in outs.items():
        assert torch.equal(o[keep].view(torch.int16), ref[keep].view(torch.int16)), key


@pytest.mark.parametrize("lens", [[1026], [64, 1, 33, 700, 257, 1026, 63, 65, 128], [79], [67, 3, 642]])
def test_attention_single_pass_v_token_major_bit_identical(ctx, monkeypatch, lens):
    """op level: `attn_fast64_kernel<VROW>` (V tiles [keys][dh] in LDS, transposing reads) against the same kernel over a transposed
    copy of V -- the same MFMA operands, so the same bits; V columns at a head offset inside a wider row (as in qkv)."""
    H, dh = 3, 64
    n = sum(lens)
    q, k, v = rnd(n, H * dh, seed=1, std=0.35).cuda(), rnd(n, H * dh, seed=2).cuda(), rnd(n, H * dh, seed=3).cuda()
    monkeypatch.setenv("PCY_ESM_ATTN", "fast")
    outs = []
    for vrow in ("0", "1"):
        pcy_disable(monkeypatch, "" if vrow == "1" else "fa_vrow")
        outs.append(ctx.attention(q, k, v, lens, H, H, dh, False, 1.0).cpu())
    assert torch.isfinite(outs[0].float()).all()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    # run to run: a tile read before its LDS-DMA has landed shows up as bits that change between launches (an experiment on this
    # kernel -- the last wave of a sequence running its first query group alone -- did exactly that and was dropped for it)
    for _ in range(24):
        again = ctx.attention(q, k, v, lens, H, H, dh, False, 1.0).cpu()
        assert torch.equal(again.view(torch.int16), outs[1].view(torch.int16))


@pytest.mark.parametrize("select", ["0", "1"])
def test_gemm_esm_gelu_fast_table_epilogue_every_in_range_value(ctx, monkeypatch, select):
    """The persistent 256 x 256 ESM-GELU kernel looks a wave tile up WITHOUT per-element range tests when every value of the tile lies
    inside the table (2^-25 <= |x| < 2^7; pattern << 1 is the gather address of a sparse table image) and redoes the tile with the
    select form otherwise (test_gemm_esm_gelu_epilogue_every_bf16_value feeds every pattern: always the select form).  Here every one of
    the 2 x 4096 in-range patterns, only those, through the kernel -- all waves take the fast form (PCY_DISABLE=gelu_fast: none does) --
    against the reference's op-by-op bf16 chain, bit for bit; a second matrix with ONE out-of-range value per 64 x 128 wave tile."""
    import math
    from procyon_amd import _lib as L
    mag = torch.arange(102 << 7, (102 + 32) << 7, dtype=torch.int32)
    bits = torch.cat([mag, mag | 0x8000]).to(torch.int16)            # 8192 patterns
    vals = bits.view(BF).repeat(16)                                    # 131072 values
    W = vals.view(2048, 64).contiguous()                               # out[m][n] = W[n][m % 64]
    M = 2048
    A = torch.zeros(M, 64, dtype=BF)
    A[torch.arange(M), torch.arange(M) % 64] = 1.0
    pcy_disable(monkeypatch, "gelu_fast" if select == "1" else "")
    n0 = _dispatch(L.DISPATCH_GEMM_BIG_PERSIST)
    out = ctx.gemm(A.cuda(), W.cuda(), torch.zeros(2048, dtype=BF).cuda(), None, 3).cpu()
    assert _dispatch(L.DISPATCH_GEMM_BIG_PERSIST) == n0 + 1
    x = W.t().contiguous()[torch.arange(M) % 64]
    ref = x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    # one tiny / one huge value somewhere in every wave tile: those waves fall back, the result is the same function
    W2 = W.clone()
    W2[::128, 3] = 1e-9
    W2[64::128, 5] = -300.0
    out2 = ctx.gemm(A.cuda(), W2.cuda(), torch.zeros(2048, dtype=BF).cuda(), None, 3).cpu()
    x2 = W2.t().contiguous()[torch.arange(M) % 64]
    ref2 = x2 * 0.5 * (1.0 + torch.erf(x2 / math.sqrt(2.0)))
    assert torch.equal(out2.view(torch.int16), ref2.view(torch.int16))


def test_bench_line_contract_and_internal_consistency():
    """`bench.py` (the driver's contract): ONE JSON line with the contract's keys, and numbers that agree with each other -- value x
    ms_per_step = tokens per step (an edit of the retrieval leg once overwrote the headline's elapsed time), roofline.frac =
    achieved / peak < 1, achieved = bytes / launch time.  A reduced run: 25 retrieval proteins, no configs block, no CPU baseline."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--full", "--no-configs", "--no-cpu-baseline",
                          "--retrieval-proteins", "25"], capture_output=True, text=True, timeout=900, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "tokens/s" and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["dtype"] == "bf16" and "workload" in d["config"]
    tokens = 256
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - tokens) < 0.02 * tokens, (d["value"], d["ms_per_step"])
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and 0.3 < r["frac"] < 1.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert abs(r["achieved"] - r["bytes_per_launch"] / 1e9 / (r["avg_launch_us"] / 1e6)) < 0.01 * r["achieved"]
    assert d["retrieval"]["proteins_per_s"] > 0 and d["retrieval"]["n_proteins"] == 25


def test_bench_plain_run_is_the_headline_and_dumps_the_last_step(tmp_path):
    """`bench.py` without --full: the headline line alone (no phases / roofline / retrieval / configs / CPU baseline), and
    --dump-outputs writes what the last timed step's `generate` returned -- token ids, log-probabilities, a seeded sample of the
    logits record -- as float .npy files within 64 MB."""
    import json
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tokens = 64                                            # 64 x 128263 logits: above the dump's sample size, so the sample is taken
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "2", "--warmup", "1", "--tokens", str(tokens),
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert k in d, k
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "tokens/s" and d["dtype"] == "bf16" and d["higher_is_better"] is True
    assert abs(d["value"] * d["ms_per_step"] / 1e3 - tokens) < 0.02 * tokens, (d["value"], d["ms_per_step"])
    for k in ("phases", "roofline", "retrieval", "configs", "cpu_baseline"):
        assert k not in d, k
    files = {p.name: np.load(p) for p in tmp_path.glob("*.npy")}
    assert set(files) == {"tokens.npy", "log_probs.npy", "logits.npy"}, set(files)
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert sum(p.stat().st_size for p in tmp_path.glob("*.npy")) <= 64 << 20
    t = files["tokens.npy"]
    assert t.shape == (1, 1, tokens) and np.array_equal(t, np.round(t)) and t.min() >= 0 and t.max() < 128263
    assert np.isfinite(files["log_probs.npy"]).all()
    assert files["logits.npy"].shape == (1 << 22,) and np.isfinite(files["logits.npy"]).all()
