"""The split-key decode attention on shared-prefix caches (pcy_attn_decode_split, pcy_llama_decode_split, pcy_llama_beam_steps_split,
pcy_llama_decode_gemm_split): the beams of a prompt share ONE pass over its K / V, the softmax statistics are kept per key chunk
and folded in a fixed-order combine -- two launches per layer, no score rows in memory.

Operator level, on the shapes of tests/test_gpu_attn_mq.py: the kernel against an emulation that states its rounding points
(tests/attn_split_ref.py, fed the library's own chunk length) at the bars test_attn_decode_shared_vs_oracle uses against its reference, plus what
the header promises -- the appended K / V bits, an untouched prefix and suffix, repeatable bits, bits that do not depend on the tile slot or the
prompt mates, slots above *pos never read into a result, the mask rules and a fully masked chunk, a position outside the suffix, argument
errors that launch nothing.  Engine level: forced-token steps of decode_split and decode_gemm(shared_attn="split") against the teacher-forced
oracle, generate(method="beam", shared_attn="split") against the oracle's beam search, the replayed chain against the four-call body, captures
that are never shared with the default chain, the refusals."""
import functools

import pytest
import torch

from attn_split_ref import rel64, split_reference, truth64
from beam_oracle import assert_beam_matches_oracle
from conftest import assert_bf16_close, pcy_disable, rel_err
from test_gpu_attn_mq import SHAPES, _caches, _fair_half_mask, _forced, _inputs, _prompt_batch
from test_gpu_decode_gemm import _gen_inputs, _geo, _oracle_embeds, _prompts, small  # noqa: F401  (small: the module's fixture)
from test_gpu_kernels import _attn_decode_mask

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
IDS = lambda s: "-".join(map(str, s))


@pytest.fixture(scope="module")
def ctx():
    from procyon_amd.engine import Context
    return Context.get()


def _counts():
    from procyon_amd import _lib
    lib = _lib.load()
    return int(lib.pcy_debug_attn_split_count()), int(lib.pcy_debug_decode_gemm_count()), int(lib.pcy_debug_attn_mq_count())


def _logical(shape, x):
    """roped q [B,H,1,dh] and K / V [B,H,t+1,dh] over the logical slots, the new token last"""
    H, Hkv = shape[0], shape[1]
    G = H // Hkv
    return x["qr"], torch.cat([x["kc"], x["kr"]], 2).repeat_interleave(G, 1), torch.cat([x["vc"], x["v"]], 2).repeat_interleave(G, 1)


def _reference(ctx, shape, mask=None):
    """the emulation on the logical rows with the library's chunk length (mask [B, t] over the cached slots; the new token is always kept)"""
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    qr, K, V = _logical(shape, _inputs(shape))
    full = None if mask is None else torch.cat([mask, torch.ones(B, 1, dtype=torch.uint8)], 1)
    chunk = ctx.attn_split_chunk_keys(B, rpp, H, Hkv, dh, Tp)
    assert chunk > 0 and chunk % 32 == 0
    return split_reference(qr, K, V, dh ** -0.5, full, chunk, Tp)


@functools.lru_cache(maxsize=None)
def _reference_unmasked(ctx, shape):
    return _reference(ctx, shape)


def _run(ctx, shape, x, keep=None, pos=None, qkv=None, **cache_kw):
    """one call on fresh copies -> (o, suffix K, suffix V, prefix K, prefix V) on the CPU"""
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    prefix, cache = _caches(shape, x, **cache_kw)
    posd = torch.tensor([x["t"] if pos is None else pos], dtype=torch.int32).cuda()
    o = ctx.attn_decode_split((x["qkv"] if qkv is None else qkv).cuda(), cache, 0, posd, x["cos"].cuda(), x["sin"].cuda(), H, Hkv, dh,
                              keep=None if keep is None else keep.cuda().contiguous(), B=B)
    return o.cpu(), cache.k[0].cpu(), cache.v[0].cpu(), prefix.k[0].cpu(), prefix.v[0].cpu()


def _bars(out, ref, what):
    assert rel_err(out, ref) < 1e-3, (what, rel_err(out, ref))
    assert_bf16_close(out, ref, what, max_frac=0.03, inter=torch.full_like(ref, 0.05))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_attn_decode_split_vs_emulation(ctx, shape):
    """against split_reference at the bars of test_attn_decode_shared_vs_oracle (the error against float64 printed beside it); the appended
    K / V are the oracle's roped key and the V bit for bit; the prefix and every other suffix slot are untouched; a second call on fresh copies
    gives the same bits; NaN in the suffix slots above `own` never reaches the result."""
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    x, ref = _inputs(shape), _reference_unmasked(ctx, shape)
    n0 = _counts()
    out, sk, sv, pk, pv = _run(ctx, shape, x)
    assert _counts() == n0                                      # (the operator is no step: no counter moves)
    truth = truth64(*_logical(shape, x), dh ** -0.5, None)
    print(f"attn_decode_split {shape}: rel. err vs the emulation {rel_err(out, ref):.3e}; vs float64: kernel {rel64(out, truth):.3e}, "
          f"emulation {rel64(ref, truth):.3e}")
    _bars(out, ref, "attn decode split")
    assert torch.equal(sk[:, :, own], x["kr"][:, :, 0]) and torch.equal(sv[:, :, own], x["v"][:, :, 0])
    assert torch.equal(pk, x["pk"]) and torch.equal(pv, x["pv"]), "the prefix panels were written"
    rest = [j for j in range(x["Tsfx"]) if j != own]
    assert torch.equal(sk[:, :, rest], x["sk"][:, :, rest]) and torch.equal(sv[:, :, rest], x["sv"][:, :, rest]), "a suffix slot other than the appended one was written"
    again = _run(ctx, shape, x)
    for a, b in zip((out, sk, sv), again):
        assert torch.equal(a, b), "a repeated call gives other bits"
    tails = []
    for fill in (0.0, float("nan")):
        sk2, sv2 = x["sk"].clone(), x["sv"].clone()
        sk2[:, :, own:] = fill; sv2[:, :, own:] = fill
        tails.append(_run(ctx, shape, x, sk=sk2, sv=sv2)[0])
    assert torch.isfinite(tails[1].float()).all(), "a slot above *pos reached the result"
    assert torch.equal(tails[0], tails[1]) and torch.equal(tails[0], out)


def test_equal_rows_give_equal_bits(ctx):
    """two rows of one prompt with the same qkv, suffix and mask -- in different query tiles -- and a row of ANOTHER prompt whose prefix is a
    copy: equal bits in o and in the appended K / V."""
    shape = (32, 8, 128, 64, 5, 20, 2, 33)
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    x = _inputs(shape)
    a, b, c = 3, 17, 20 + 9                                    # 3 and 17: tiles 0 and 1 of prompt 0 (4 queries per row); 29: prompt 1
    qkv, sk, sv, pk = x["qkv"].clone(), x["sk"].clone(), x["sv"].clone(), x["pk"].clone()
    pv = x["pv"].clone()
    pk[1], pv[1] = pk[0], pv[0]
    for r in (b, c):
        qkv[r], sk[r], sv[r] = qkv[a], sk[a], sv[a]
    keep = torch.ones(B, Tp + x["Tsfx"], dtype=torch.uint8)
    keep[:, :Tp + own] = _attn_decode_mask("leftpad", B, Tp + own, seed=5)
    for r in (b, c):
        keep[r] = keep[a]
    out, k2, v2, _, _ = _run(ctx, shape, dict(x, pv=pv), keep=keep, qkv=qkv, sk=sk, sv=sv, pk=pk)
    for r in (b, c):
        assert torch.equal(out[r], out[a]), (r, "o")
        assert torch.equal(k2[r, :, own], k2[a, :, own]) and torch.equal(v2[r, :, own], v2[a, :, own]), (r, "appended K / V")
    assert not torch.equal(out[a], out[a + 1])


@pytest.mark.parametrize("mode", ["leftpad", "half", "all_masked", "ones"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_attn_decode_split_key_mask(ctx, shape, mode):
    """the four modes of test_attn_decode_key_mask, another mask for every row, against the emulation under the same mask at the same bars (the
    random halves drawn by test_gpu_attn_mq's `_fair_half_mask`, which looks at the default kernel and the eager formulas only)."""
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    x, t, G = _inputs(shape), Tp + own, H // Hkv
    mask = _fair_half_mask(ctx, shape) if mode == "half" else _attn_decode_mask(mode, B, t, seed=H * 1000 + t + B)
    ref = _reference_unmasked(ctx, shape) if mode == "ones" else _reference(ctx, shape, mask)
    keep = torch.ones(B, Tp + x["Tsfx"], dtype=torch.uint8)
    keep[:, :t] = mask
    out, sk, sv, pk, pv = _run(ctx, shape, x, keep=keep)
    assert torch.isfinite(out.float()).all()
    _bars(out, ref, f"attn decode split, mask {mode}")
    assert torch.equal(sk[:, :, own], x["kr"][:, :, 0]) and torch.equal(sv[:, :, own], x["v"][:, :, 0])
    assert torch.equal(pk, x["pk"]) and torch.equal(pv, x["pv"])
    if mode == "all_masked":                                   # every chunk but the own one has w_c == 0, and the own one is one-hot
        assert torch.equal(out.view(B, H, dh), x["v"][:, :, 0].repeat_interleave(G, 1)), "o must be the new token's V row"
    if mode == "ones":
        assert torch.equal(out, _run(ctx, shape, x)[0]), "all ones differs from keep = NULL"
    other = keep.clone()
    other[:, 0::2] *= 2
    other[:, 1::2] *= 255
    assert torch.equal(_run(ctx, shape, x, keep=other)[0], out), "a non-zero byte other than 1 does not count as kept"
    tail0 = keep.clone()
    tail0[:, t:] = 0
    assert torch.equal(_run(ctx, shape, x, keep=tail0)[0], out), "keep[b][t:] is read"


@pytest.mark.parametrize("shape", [(32, 8, 128, 600, 33, 10, 4, 40), (32, 8, 128, 1030, 2, 10, 1, 10), (8, 2, 64, 70, 2, 1, 5, 5)], ids=IDS)
def test_fully_masked_chunk(ctx, shape):
    """every third row masks ONE whole key chunk of the prefix (the second one; the others a left pad): finite, at the bars against the
    emulation; and bit-equal to the call whose K / V in that chunk are garbage for those rows' prompt -- w_c == 0 exactly."""
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    x, t = _inputs(shape), Tp + own
    chunk = ctx.attn_split_chunk_keys(B, rpp, H, Hkv, dh, Tp)
    assert 2 * chunk <= Tp, (chunk, Tp)
    mask = torch.ones(B, t, dtype=torch.uint8)
    mask[::3, chunk:2 * chunk] = 0
    mask[1::3, :3] = 0
    keep = torch.ones(B, Tp + x["Tsfx"], dtype=torch.uint8)
    keep[:, :t] = mask
    out = _run(ctx, shape, x, keep=keep)[0]
    assert torch.isfinite(out.float()).all()
    _bars(out, _reference(ctx, shape, mask), "a fully masked chunk")
    pk = x["pk"].clone()
    pk[:, :, chunk:2 * chunk] = pk[:, :, chunk:2 * chunk].flip(2) * 3      # other finite keys in the masked chunk
    moved = _run(ctx, shape, x, keep=keep, pk=pk)[0]
    assert torch.equal(moved[::3], out[::3]), "a fully masked chunk reached the result"
    assert not torch.equal(moved[1::3], out[1::3])


def test_position_outside_the_suffix_writes_nothing(ctx):
    """*pos = Tp - 1 (inside the prefix) and *pos = Tp + Tmax (behind the suffix): o keeps its sentinel, the whole cache is untouched"""
    shape = (32, 8, 128, 37, 0, 10, 2, 20)
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    x = _inputs(shape)
    for pos in (Tp - 1, Tp + x["Tsfx"]):
        prefix, cache = _caches(shape, x)
        o = torch.full((B, H * dh), 7.0, dtype=BF, device="cuda")
        ctx.attn_decode_split(x["qkv"].cuda(), cache, 0, torch.tensor([pos], dtype=torch.int32).cuda(), x["cos"].cuda(), x["sin"].cuda(), H, Hkv, dh,
                              B=B, out=o)
        assert bool((o == 7.0).all()), pos
        assert torch.equal(cache.k[0].cpu(), x["sk"]) and torch.equal(cache.v[0].cpu(), x["sv"])
        assert torch.equal(prefix.k[0].cpu(), x["pk"]) and torch.equal(prefix.v[0].cpu(), x["pv"])


def test_argument_errors_launch_nothing(ctx):
    """a plain cache, a grouped cache, an incomplete shared cache, B outside [1, cache rows], head_dim 32, H / Hkv = 16: PcyError, o keeps its
    sentinel, the caches are untouched, the counters stand still"""
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import KVCache, LlamaConfig
    shape = (4, 2, 64, 5, 1, 5, 3, 15)
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    x = _inputs(shape)
    posd = torch.tensor([x["t"]], dtype=torch.int32).cuda()

    def refused(cache, rows, match, H=H, Hkv=Hkv, dh=dh, qkv=None):
        qkv = x["qkv"].cuda() if qkv is None else qkv
        k0, v0, n0 = cache.k.clone(), cache.v.clone(), _counts()
        o = torch.full((max(rows, 1), H * dh), 7.0, dtype=BF, device="cuda")
        with pytest.raises(PcyError, match=match):
            ctx.attn_decode_split(qkv, cache, 0, posd, x["cos"].cuda(), x["sin"].cuda(), H, Hkv, dh, B=rows, out=o)
        ctx.sync()
        assert _counts() == n0 and bool((o == 7.0).all())
        assert torch.equal(cache.k, k0) and torch.equal(cache.v, v0)

    prefix, cache = _caches(shape, x)
    cfg = LlamaConfig(vocab=8, d=H * dh, n_layers=1, n_heads=H, n_kv_heads=Hkv, ffn=64)
    refused(KVCache(cfg, B, Tp + x["Tsfx"], "cuda"), B, "no shared prefix")
    refused(KVCache.grouped(cfg, "cuda", prefix, [5, 5, 5], [Tp, Tp - 1, Tp], x["Tsfx"]), B, "grouped")
    refused(cache, B + 1, "cache rows")
    refused(cache, 0, "cache rows")
    broken = KVCache(cfg, B, x["Tsfx"], "cuda", prefix=prefix, rows_per_prefix=rpp)
    broken.c.prefix_v = None
    refused(broken, B, "shared-prefix cache needs")
    wide = torch.zeros(B, 4096, dtype=BF, device="cuda")
    refused(cache, B, "head_dim", H=4, Hkv=2, dh=32, qkv=wide)
    refused(cache, B, "H/Hkv", H=16, Hkv=1, dh=64, qkv=wide)


# ---------------------------------------------------------------------------------------------- engine level
N = 3          # forced decode steps per case
# (geometry, prompts, beam, T); (2, 10, 30): the appended slots 30..32 cross a 32-key block of the logical row
STEP_CASES = [("llama8b", 1, 10, 13), ("llama8b", 1, 20, 12), ("llama8b", 2, 10, 30), ("split", 1, 10, 13)]


def _forced_steps(eng, V, emb, mask, beam, step):
    """prefill the P prompts once, wrap with new_beam_cache, N steps of `step(cache, st, B)` on forced tokens with the clean keep mask
    -> logits [N, B, V], the appended K / V [L, B, Hkv, N, dh] (device tensors)"""
    from procyon_amd.engine import Context, GenState
    P, T = mask.shape
    B = P * beam
    prefix = eng.new_cache(P, T)
    eng.prefill(emb.cuda(), mask, prefix, "last")
    cache = eng.new_beam_cache(prefix, beam, N + 2)
    keep = torch.ones(B, T + N + 2, dtype=torch.uint8, device="cuda")
    keep[:, :T] = mask.repeat_interleave(beam, 0).to("cuda", torch.uint8)
    st = GenState(B, V, N + 2, "cuda", keep=keep)
    lg = []
    for s in range(N):
        st.pos.fill_(T + s)
        st.next_tok.copy_(_forced(B, V, s).to(torch.int32))
        step(cache, st, B)
        lg.append(st.logits.clone())
    Context.get().sync()
    return torch.stack(lg), cache.k[:, :, :, :N].clone(), cache.v[:, :, :, :N].clone()


def _check_forced_against_oracle(name, kw, sd, emb, mask, beam, logits, what):
    """the first, a middle and the last beam of the first and the last prompt against the teacher-forced oracle at every step: rel. err < 2e-2
    (the bar of test_decode_gemm_shared_attn_forced_steps; no argmax rule: the tokens are forced)"""
    from oracle import llama_ref as LR
    P, V = mask.shape[0], kw["vocab"]
    B = P * beam
    rows = sorted({p * beam + j for p in (0, P - 1) for j in (0, beam // 2, beam - 1)})
    pr = torch.tensor(rows) // beam
    geom = LR.LlamaGeom(**kw, max_pos=512)
    m = mask[pr]
    past = LR.llama_forward(sd, geom, inputs_embeds=emb[pr], attn_mask=m, logits_rows="last")["past_kv"]
    got, worst = logits[:, torch.tensor(rows, device="cuda")].float().cpu(), 0.0
    for s in range(N):
        m = torch.cat([m, torch.ones(len(rows), 1)], 1)
        r = LR.llama_forward(sd, geom, input_ids=_forced(B, V, s)[rows][:, None].long(), attn_mask=m, past_kv=past, logits_rows="last")
        past, ref = r["past_kv"], r["logits"][:, -1].float()
        for j, b in enumerate(rows):
            e = rel_err(got[s, j], ref[j])
            worst = max(worst, e)
            assert e < 2e-2, (what, name, b, s, e)
    print(f"{what} {name} {P}x{beam}: worst rel. err vs the oracle {worst:.3e} on rows {rows}")


@pytest.mark.parametrize("name,P,beam,T", STEP_CASES)
def test_decode_split_forced_steps(monkeypatch, name, P, beam, T):
    """N forced-token steps of decode_split on a beam cache: the counter says the step ran (and neither the GEMM step's nor the many-queries
    attention's moves); sampled rows against the teacher-forced oracle; a repeated run gives equal bits; layer 0's appended K / V of the first
    step are the default step's bits (its qkv are the same bits in both runs)."""
    kw, sd, eng = _geo(name)
    pcy_disable(monkeypatch)
    emb, mask = _prompt_batch(P, T, kw["d"], seed=P * 100 + T)
    n0 = _counts()
    logits, k, v = _forced_steps(eng, kw["vocab"], emb, mask, beam, eng.decode_split)
    n1 = _counts()
    assert (n1[0] - n0[0], n1[1] - n0[1], n1[2] - n0[2]) == (N, 0, 0)
    assert torch.isfinite(logits.float()).all()
    _check_forced_against_oracle(name, kw, sd, emb, mask, beam, logits, "decode_split")
    again = _forced_steps(eng, kw["vocab"], emb, mask, beam, eng.decode_split)
    for a, b_ in zip((logits, k, v), again):
        assert torch.equal(a, b_), (name, "repeat")
    n2 = _counts()
    _, k0, v0 = _forced_steps(eng, kw["vocab"], emb, mask, beam, eng.decode)
    assert _counts() == n2
    assert torch.equal(k[0, :, :, 0], k0[0, :, :, 0]) and torch.equal(v[0, :, :, 0], v0[0, :, :, 0]), "layer 0: the appended K / V of the first step"


@pytest.mark.parametrize("name", ["llama8b", "split"])
def test_decode_gemm_split_forced_steps(monkeypatch, name):
    """the same at 4 x 10 through decode_gemm(shared_attn="split"): both the GEMM step's counter and the split counter move, the many-queries one
    does not"""
    kw, sd, eng = _geo(name)
    pcy_disable(monkeypatch)
    P, beam, T = 4, 10, 13
    emb, mask = _prompt_batch(P, T, kw["d"], seed=P * 100 + T)
    step = lambda cache, st, B: eng.decode_gemm(cache, st, B, shared_attn="split")
    n0 = _counts()
    logits, k, v = _forced_steps(eng, kw["vocab"], emb, mask, beam, step)
    n1 = _counts()
    assert (n1[0] - n0[0], n1[1] - n0[1], n1[2] - n0[2]) == (N, N, 0)
    assert torch.isfinite(logits.float()).all()
    _check_forced_against_oracle(name, kw, sd, emb, mask, beam, logits, "decode_gemm split")
    again = _forced_steps(eng, kw["vocab"], emb, mask, beam, step)
    for a, b_ in zip((logits, k, v), again):
        assert torch.equal(a, b_), (name, "repeat")


@pytest.mark.parametrize("n", [1, 2])
def test_generate_beam_split_matches_oracle(small, n):
    """`generate(method="beam", shared_attn="split")`, beam 10 in groups of 2 (the reference's captioning call) on the replayed chain: 1 and 2
    prompts against the oracle's diverse beam search (the tie-aware rule of tests/beam_oracle.py)."""
    from oracle import llama_ref as LR
    m, w = small["model"], small["w"]
    instr, slots = _prompts(n, seed=n * 10 + 2)
    emb, mask = _oracle_embeds(small, _gen_inputs(small, instr, slots))
    enc = LR.make_text_encoder(w["llama"], small["lgeom"])
    trace = []
    kw = dict(max_len=6, beam_size=10, beam_group_size=2, diversity_penalty=0.8)
    t_ref, s_ref, lg_ref = LR.beam_search(enc, emb, mask, vocab_size=small["lgeom"].vocab, eos_id=m.tokenizer.eos_token_id, trace=trace, **kw)
    n0 = _counts()
    tokens, scores, logits, _ = m.generate(_gen_inputs(small, instr, slots), method="beam", shared_attn="split", **kw)
    n1 = _counts()
    assert n1[0] > n0[0] and n1[1:] == n0[1:]
    assert_beam_matches_oracle(tokens, scores, logits, t_ref, s_ref, lg_ref, trace)


def _beam_inputs(kw, P, T, seed):
    g = torch.Generator().manual_seed(seed)
    emb = (torch.randn(P, T, kw["d"], generator=g) * 0.02).to(BF).cuda()
    mask = torch.ones(P, T)
    if P > 1:
        mask[1, :3] = 0
    return emb, mask


@pytest.mark.parametrize("name,P", [("small", 1), ("small", 2), ("llama8b", 1)])
def test_chain_equals_the_four_call_body(monkeypatch, name, P):
    """generate_beam(shared_attn="split") on the replayed chain and, under PCY_DISABLE=beam_graph, as four calls per step: equal tokens, scores
    and logits records, bit for bit.  10 steps: more than one enqueue of the chain."""
    kw, sd, eng = _geo(name)
    emb, mask = _beam_inputs(kw, P, 13, seed=7 + P)
    res = []
    for off in ((), ("beam_graph",)):
        pcy_disable(monkeypatch, *off)
        n0 = _counts()
        res.append(eng.generate_beam(emb, mask, 10, 10, 2, 0.8, -1, 12, shared_attn="split"))
        n1 = _counts()
        assert (n1[0] - n0[0] == 9) if off else (n1[0] > n0[0]), (off, n0, n1)
        assert n1[1:] == n0[1:]
    assert torch.isfinite(res[0][2].float()).all() and res[0][2].shape[:2] == (P * 10, 10)
    for x, y in zip(res[0], res[1]):
        assert torch.equal(x, y), name


def test_split_and_default_chains_never_share_a_capture(monkeypatch):
    """default generate_beam, then "split", then default again on the same shapes: the two default runs are bit-identical, and the split counter
    moves in the middle run only"""
    kw, sd, eng = _geo("small")
    pcy_disable(monkeypatch)
    emb, mask = _beam_inputs(kw, 2, 13, seed=21)
    args = (6, 10, 2, 0.8, -1, 8)
    n0 = _counts()
    a = eng.generate_beam(emb, mask, *args)
    n1 = _counts()
    b = eng.generate_beam(emb, mask, *args, shared_attn="split")
    n2 = _counts()
    c = eng.generate_beam(emb, mask, *args)
    n3 = _counts()
    assert n1 == n0 and n2[0] > n1[0] and n2[1:] == n1[1:] and n3 == n2
    for x, y in zip(a, c):
        assert torch.equal(x, y)
    assert torch.isfinite(b[2].float()).all()


def test_generate_beam_refusals(monkeypatch):
    """"split" off the shared cache (1 prompt x beam 5, whose plan is the plain cache; PCY_DISABLE=beam_kv_shared) is a ValueError before anything
    is launched, with or without the GEMM step; a value that is none of False / True / "split" too; shared_attn=True without decode_gemm keeps
    its ValueError.  No counter moves."""
    from fulldepth_common import decode_counts
    kw, sd, eng = _geo("small")
    emb4, mask4 = _beam_inputs(kw, 4, 9, seed=3)

    def refused(emb, mask, beam, value, **opt):
        n0, d0 = _counts(), decode_counts()
        with pytest.raises(ValueError, match="shared_attn"):
            eng.generate_beam(emb, mask, 5, beam, beam // 5, 0.8, -1, 8, shared_attn=value, **opt)
        assert _counts() == n0 and decode_counts() == d0

    pcy_disable(monkeypatch, "beam_kv_shared")
    refused(emb4, mask4, 10, "split")
    refused(emb4, mask4, 10, "split", decode_gemm=True)
    pcy_disable(monkeypatch)
    refused(emb4[:1], mask4[:1], 5, "split")
    refused(emb4[:1], mask4[:1], 5, "split", decode_gemm=True)
    refused(emb4, mask4, 10, "auto")
    refused(emb4, mask4, 10, True)                             # (decode_gemm=False: the GEMM step is not in use -- today's rule)
    n0 = _counts()
    eng.generate_beam(emb4, mask4, 5, 10, 2, 0.8, -1, 8, decode_gemm=True, shared_attn="split")
    n1 = _counts()
    assert (n1[0] - n0[0], n1[1] - n0[1], n1[2] - n0[2]) == (4, 4, 0)


def test_decode_split_argument_errors_launch_nothing(monkeypatch):
    """pcy_llama_decode_split: a plain cache, a grouped cache, B beyond the cache's rows, a row count below the batched loop's and fp8 layers are
    argument errors that launch nothing"""
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import Context, GenState
    kw, sd, eng = _geo("small")
    pcy_disable(monkeypatch)
    P, beam, T, V = 2, 10, 10, kw["vocab"]
    B = P * beam
    emb, mask = _prompt_batch(P, T, kw["d"], seed=9)
    prefix = eng.new_cache(P, T)
    eng.prefill(emb.cuda(), None, prefix, "last")
    shared = eng.new_beam_cache(prefix, beam, 4)
    plain = eng.new_cache(B, T + 4)
    grouped = eng.new_grouped_cache(prefix, [10, 10], [T, T - 1], 4)
    st = GenState(64, V, 4, "cuda")
    st.pos.fill_(T)
    st.logits.fill_(1.0)
    Context.get().sync()

    def refused(c, rows, match):
        k0, v0, n0 = c.k.clone(), c.v.clone(), _counts()
        with pytest.raises(PcyError, match=match):
            eng.decode_split(c, st, rows)
        Context.get().sync()
        assert _counts() == n0
        assert torch.equal(c.k, k0) and torch.equal(c.v, v0) and bool((st.logits == 1.0).all())

    refused(plain, B, "no shared prefix")
    refused(grouped, B, "grouped")
    refused(shared, B + 1, "cache rows")
    refused(shared, 1, "batched decode loop")
    eng.quantize_fp8()
    try:
        refused(shared, B, "fp8")
    finally:
        eng.set_fp8(False)
    n0 = _counts()
    eng.decode_split(shared, st, B)                            # ... and the same call is served once the fp8 layers are off
    Context.get().sync()
    n1 = _counts()
    assert n1[0] - n0[0] == 1 and n1[1:] == n0[1:] and torch.isfinite(st.logits[:B].float()).all()
