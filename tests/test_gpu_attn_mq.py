"""The many-queries decode attention on shared-prefix caches (pcy_attn_decode_shared, pcy_llama_decode_gemm_mq): all rows of a
prompt are scored against ONE pass over the K / V they share, the prefix cut into key chunks whose fp32 partial sums are added in a fixed order.

Operator level: the eager formulas and bars of test_attn_decode / test_attn_decode_key_mask (tests/test_gpu_kernels.py) on the logical rows, plus
what the header promises -- the appended K / V bits, an untouched prefix and suffix, repeatable bits, bits that do not depend on the tile slot or
the prompt mates, slots above *pos never read into a result, the mask rules, a position outside the suffix, argument errors that launch nothing.
Engine level: forced-token steps of decode_gemm(shared_attn=True) against the oracle on sampled rows, generate(method="beam") against the
oracle's beam search, the refusals of generate_beam, counters that prove which step ran."""
import functools

import pytest
import torch
import torch.nn.functional as F

from beam_oracle import assert_beam_matches_oracle
from conftest import assert_bf16_close, pcy_disable, rel_err
from fulldepth_common import decode_counts
from test_gpu_decode_gemm import GEOMS, _gen_inputs, _geo, _oracle_embeds, _prompts, small  # noqa: F401  (small: the module's fixture)
from test_gpu_kernels import _attn_decode_mask, rnd

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# (H, Hkv, dh, Tp, own, rows_per_prefix, P, B): prefix slots, filled suffix slots per row, rows per prompt, prompts, rows of the call
SHAPES = [
    (32, 8, 128, 37, 0, 10, 2, 20),      # Tp no multiple of 32, empty suffix (the first step), 40 queries in a tile
    (32, 8, 128, 600, 33, 10, 4, 40),    # several key chunks, a suffix that crosses a 32-key block
    (32, 8, 128, 64, 5, 20, 2, 33),      # 80 queries = two query tiles; the last prompt is short (13 rows)
    (32, 32, 128, 45, 3, 10, 2, 20),     # G = 1: 10 queries in a tile
    (4, 2, 64, 5, 1, 5, 3, 15),          # Tp < 32, dh 64
    (8, 1, 128, 1, 0, 3, 1, 3),          # a one-slot prefix, G = 8
    (32, 8, 128, 1030, 2, 10, 1, 10),    # a long prefix with one prompt
    (8, 2, 64, 70, 2, 1, 5, 5),          # rows_per_prefix = 1: every row its own prompt
]
SPARE = 3      # suffix slots behind the appended one


@pytest.fixture(scope="module")
def ctx():
    from procyon_amd.engine import Context
    return Context.get()


def _counts():
    from procyon_amd import _lib
    lib = _lib.load()
    return int(lib.pcy_debug_attn_mq_count()), int(lib.pcy_debug_decode_gemm_count())


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """host tensors of a shape (built once, never modified): qkv, prefix K / V [P,Hkv,Tp,dh], suffix K / V [B,Hkv,Tsfx,dh], rope tables, the
    logical cached rows [B,Hkv,t,dh] and the oracle's roped q / k and v of the new token"""
    from oracle import llama_ref as LR
    from procyon_amd.engine import rope_tables
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    t, Tsfx = Tp + own, own + 1 + SPARE
    qkv = rnd(B, (H + 2 * Hkv) * dh, seed=1)
    pk, pv = rnd(P, Hkv, Tp, dh, seed=2), rnd(P, Hkv, Tp, dh, seed=3)
    sk, sv = rnd(B, Hkv, Tsfx, dh, seed=4), rnd(B, Hkv, Tsfx, dh, seed=5)
    cos, sin = rope_tables(dh, 10000.0, t + 2, "cpu")
    prow = torch.arange(B) // rpp
    kc, vc = torch.cat([pk[prow], sk[:, :, :own]], 2), torch.cat([pv[prow], sv[:, :, :own]], 2)
    q = qkv[:, :H * dh].view(B, 1, H, dh).transpose(1, 2)
    k = qkv[:, H * dh:(H + Hkv) * dh].view(B, 1, Hkv, dh).transpose(1, 2)
    v = qkv[:, (H + Hkv) * dh:].view(B, 1, Hkv, dh).transpose(1, 2)
    qr, kr = LR.apply_rope(q, k, cos[t][None, None].expand(B, 1, dh), sin[t][None, None].expand(B, 1, dh))
    return dict(qkv=qkv, pk=pk, pv=pv, sk=sk, sv=sv, cos=cos, sin=sin, kc=kc, vc=vc, qr=qr, kr=kr, v=v, t=t, Tsfx=Tsfx)


def _reference(shape, x, mask=None):
    """the eager formulas of test_attn_decode (mask: test_attn_decode_key_mask's, [B, t] over the cached slots) on the logical rows"""
    from oracle import llama_ref as LR
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    t, G = x["t"], H // Hkv
    K = torch.cat([x["kc"], x["kr"]], 2).repeat_interleave(G, 1)
    V = torch.cat([x["vc"], x["v"]], 2).repeat_interleave(G, 1)
    s = torch.matmul(x["qr"], K.transpose(2, 3)) * dh ** -0.5
    if mask is not None:
        s = s + LR.build_additive_mask(torch.cat([mask, torch.ones(B, 1, dtype=torch.uint8)], 1), B, 1, t, BF)
    p = F.softmax(s, dim=-1, dtype=torch.float32).to(BF)
    return torch.matmul(p, V).transpose(1, 2).reshape(B, H * dh)


@functools.lru_cache(maxsize=None)
def _reference_unmasked(shape):
    return _reference(shape, _inputs(shape))


def _caches(shape, x, sk=None, sv=None, pk=None):
    """fresh device copies: (prefix cache, shared-prefix cache of B rows)"""
    from procyon_amd.engine import KVCache, LlamaConfig
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    cfg = LlamaConfig(vocab=8, d=H * dh, n_layers=1, n_heads=H, n_kv_heads=Hkv, ffn=64)
    prefix = KVCache(cfg, P, Tp, "cuda")
    prefix.k[0].copy_(x["pk"] if pk is None else pk); prefix.v[0].copy_(x["pv"])
    cache = KVCache(cfg, B, x["Tsfx"], "cuda", prefix=prefix, rows_per_prefix=rpp)
    cache.k[0].copy_(x["sk"] if sk is None else sk); cache.v[0].copy_(x["sv"] if sv is None else sv)
    return prefix, cache


def _run(ctx, shape, x, keep=None, pos=None, qkv=None, **cache_kw):
    """one call on fresh copies -> (o, suffix K, suffix V, prefix K, prefix V) on the CPU"""
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    prefix, cache = _caches(shape, x, **cache_kw)
    posd = torch.tensor([x["t"] if pos is None else pos], dtype=torch.int32).cuda()
    o = ctx.attn_decode_shared((x["qkv"] if qkv is None else qkv).cuda(), cache, 0, posd, x["cos"].cuda(), x["sin"].cuda(), H, Hkv, dh,
                               keep=None if keep is None else keep.cuda().contiguous(), B=B)
    return o.cpu(), cache.k[0].cpu(), cache.v[0].cpu(), prefix.k[0].cpu(), prefix.v[0].cpu()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_attn_decode_shared_vs_oracle(ctx, shape):
    """bars of test_attn_decode; the appended K / V are the oracle's roped key and the V bit for bit; the prefix and every other suffix slot
    are untouched; a second call on fresh copies gives the same bits; NaN in the suffix slots above `own` never reaches the result."""
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    x, ref = _inputs(shape), _reference_unmasked(shape)
    n0 = _counts()
    out, sk, sv, pk, pv = _run(ctx, shape, x)
    assert _counts() == n0                                      # (the operator is no step: neither counter moves)
    print(f"attn_decode_shared {shape}: rel. err {rel_err(out, ref):.3e}")
    assert rel_err(out, ref) < 1e-3
    assert_bf16_close(out, ref, "attn decode shared", max_frac=0.03, inter=torch.full_like(ref, 0.05))
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
    y = dict(x, pv=pv)
    out, k2, v2, _, _ = _run(ctx, shape, y, keep=keep, qkv=qkv, sk=sk, sv=sv, pk=pk)
    for r in (b, c):
        assert torch.equal(out[r], out[a]), (r, "o")
        assert torch.equal(k2[r, :, own], k2[a, :, own]) and torch.equal(v2[r, :, own], v2[a, :, own]), (r, "appended K / V")
    assert not torch.equal(out[a], out[a + 1])


def _meets_bars(out, ref, what):
    try:
        assert_bf16_close(out, ref, what, max_frac=0.03, inter=torch.full_like(ref, 0.05))
    except AssertionError:
        return False
    return rel_err(out, ref) < 1e-3


def _fair_half_mask(ctx, shape):
    """The random-half mask of a shape: the first of the seeds H * 1000 + t + B (test_attn_decode_key_mask's), + 1, + 2 ... on which the project's
    own yardstick kernel -- pcy_attn_decode on a PLAIN cache holding the same logical rows -- meets the bars against the eager reference.
    Why: bf16(q.k) of a dominant key can flip by one ulp between the MFMA's and the CPU matmul's order of the fp32 sum, which moves a whole
    head's output by more than assert_bf16_close allows (measured at the first seed on (32, 8, 128, 1030, 2, 10, 1, 10): two elements 9 %
    beyond the tolerance, the same two with the same figures for pcy_attn_decode and for the kernel under test).  The choice depends on the
    reference and on the untouched default kernel only, never on the code under test, which is then held to the unchanged bars."""
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    x, t = _inputs(shape), Tp + own
    Tmax = Tp + x["Tsfx"]
    kc, vc = torch.zeros(B, Hkv, Tmax, dh, dtype=BF), torch.zeros(B, Hkv, Tmax, dh, dtype=BF)
    kc[:, :, :t], vc[:, :, :t] = x["kc"], x["vc"]
    pos = torch.tensor([t], dtype=torch.int32).cuda()
    for k in range(8):
        mask = _attn_decode_mask("half", B, t, seed=H * 1000 + t + B + k)
        keep = torch.ones(B, Tmax, dtype=torch.uint8)
        keep[:, :t] = mask
        out = ctx.attn_decode(x["qkv"].cuda(), kc.cuda(), vc.cuda(), pos, x["cos"].cuda(), x["sin"].cuda(), H, Hkv, dh, keep=keep.cuda()).cpu()
        if _meets_bars(out, _reference(shape, x, mask), "yardstick"):
            return mask
    pytest.fail(f"{shape}: pcy_attn_decode misses the bars on all 8 random halves")


@pytest.mark.parametrize("mode", ["leftpad", "half", "all_masked", "ones"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_attn_decode_shared_key_mask(ctx, shape, mode):
    """the modes and rules of test_attn_decode_key_mask, another mask for every row (two rows of one prompt with different left pads among them).
    The random halves are drawn by `_fair_half_mask`; the bars are test_attn_decode's, unchanged."""
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    x, t, G = _inputs(shape), Tp + own, H // Hkv
    mask = _fair_half_mask(ctx, shape) if mode == "half" else _attn_decode_mask(mode, B, t, seed=H * 1000 + t + B)
    if mode == "leftpad" and t >= 2 and rpp >= 2:
        assert int(mask[0].sum()) != int(mask[1].sum())        # rows 0 and 1 share prompt 0
    ref = _reference_unmasked(shape) if mode == "ones" else _reference(shape, x, mask)
    keep = torch.ones(B, Tp + x["Tsfx"], dtype=torch.uint8)
    keep[:, :t] = mask
    out, sk, sv, pk, pv = _run(ctx, shape, x, keep=keep)
    assert rel_err(out, ref) < 1e-3
    assert_bf16_close(out, ref, f"attn decode shared, mask {mode}", max_frac=0.03, inter=torch.full_like(ref, 0.05))
    assert torch.equal(sk[:, :, own], x["kr"][:, :, 0]) and torch.equal(sv[:, :, own], x["v"][:, :, 0])
    assert torch.equal(pk, x["pk"]) and torch.equal(pv, x["pv"])
    if mode == "all_masked":
        assert torch.equal(out.view(B, H, dh), x["v"][:, :, 0].repeat_interleave(G, 1)), "one-hot softmax: o must be the new token's V row"
    if mode == "ones":
        assert torch.equal(out, _run(ctx, shape, x)[0]), "all ones differs from keep = NULL"
    other = keep.clone()
    other[:, 0::2] *= 2
    other[:, 1::2] *= 255
    assert torch.equal(_run(ctx, shape, x, keep=other)[0], out), "a non-zero byte other than 1 does not count as kept"
    tail0 = keep.clone()
    tail0[:, t:] = 0
    assert torch.equal(_run(ctx, shape, x, keep=tail0)[0], out), "keep[b][t:] is read"


def test_position_outside_the_suffix_writes_nothing(ctx):
    """*pos = Tp - 1 (inside the prefix) and *pos = Tp + Tmax (behind the suffix): o keeps its sentinel, the whole cache is untouched"""
    shape = (32, 8, 128, 37, 0, 10, 2, 20)
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    x = _inputs(shape)
    for pos in (Tp - 1, Tp + x["Tsfx"]):
        prefix, cache = _caches(shape, x)
        o = torch.full((B, H * dh), 7.0, dtype=BF, device="cuda")
        ctx.attn_decode_shared(x["qkv"].cuda(), cache, 0, torch.tensor([pos], dtype=torch.int32).cuda(), x["cos"].cuda(), x["sin"].cuda(), H, Hkv, dh,
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
            ctx.attn_decode_shared(qkv, cache, 0, posd, x["cos"].cuda(), x["sin"].cuda(), H, Hkv, dh, B=rows, out=o)
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
    few = KVCache(cfg, B, x["Tsfx"], "cuda", prefix=prefix, rows_per_prefix=rpp)
    few.c.prefix_B = 2                                         # 15 rows of 5 need 3 prefix rows
    refused(few, B, "prefix rows")
    # geometry: the rows of qkv are wide enough for each of these readings of the same buffers
    wide = torch.zeros(B, 4096, dtype=BF, device="cuda")
    refused(cache, B, "head_dim", H=4, Hkv=2, dh=32, qkv=wide)
    refused(cache, B, "H/Hkv", H=16, Hkv=1, dh=64, qkv=wide)
    refused(cache, B, "H/Hkv", H=6, Hkv=2, dh=64, qkv=wide)


# ---------------------------------------------------------------------------------------------- engine level
N = 3          # forced decode steps per case
# (geometry, prompts, beam, T); (2, 20, 30): the appended slots 30..32 cross a 32-key block of the logical row; (33, 10, 9): 330 rows, two
# 256-row GEMM tiles
STEP_CASES = [(g, P, beam, T) for g in GEOMS for P, beam, T in ((4, 10, 13), (16, 10, 12), (2, 20, 30))] + [("small", 33, 10, 9)]


def _prompt_batch(P, T, d, seed):
    g = torch.Generator().manual_seed(seed)
    emb = (torch.randn(P, T, d, generator=g) * 0.02).to(BF)
    mask = torch.ones(P, T)
    for p in range(P):
        mask[p, :(p * 5) % 7 if p % 3 else 0] = 0               # ragged left pads
    return emb, mask


def _forced(B, V, s):
    return (7 * torch.arange(B) + 3 * s + 1) % V


def _forced_steps(eng, V, emb, mask, beam, shared_attn):
    """prefill the P prompts once, wrap with new_beam_cache, N steps of decode_gemm on forced tokens with the clean keep mask
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
        eng.decode_gemm(cache, st, B, shared_attn=shared_attn)
        lg.append(st.logits.clone())
    Context.get().sync()
    return torch.stack(lg), cache.k[:, :, :, :N].clone(), cache.v[:, :, :, :N].clone()


@pytest.mark.parametrize("name,P,beam,T", STEP_CASES)
def test_decode_gemm_shared_attn_forced_steps(monkeypatch, name, P, beam, T):
    """N forced-token steps of decode_gemm(shared_attn=True) on a beam cache: the counters say which step ran; the first, a middle and the last
    beam of the first and the last prompt against the teacher-forced oracle at every step (rel. err < 2e-2, fulldepth_common.check_oracle's
    bar; no argmax rule: the tokens are forced); a repeated run gives equal bits; the K / V appended in the first step against the run with
    shared_attn=False -- bit for bit in layer 0, whose qkv are the same bits in both runs.  (The deeper layers project another attention
    output: its bits are not those of the default kernel, so their K / V agree to rounding only -- held at the logits' bar.)"""
    from oracle import llama_ref as LR
    kw, sd, eng = _geo(name)
    pcy_disable(monkeypatch)
    V, B = kw["vocab"], P * beam
    emb, mask = _prompt_batch(P, T, kw["d"], seed=P * 100 + T)
    n0, d0 = _counts(), decode_counts()
    logits, k, v = _forced_steps(eng, V, emb, mask, beam, True)
    n1 = _counts()
    assert (n1[0] - n0[0], n1[1] - n0[1]) == (N, N) and decode_counts() == d0
    assert torch.isfinite(logits.float()).all()
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
            assert e < 2e-2, (name, b, s, e)
    print(f"decode_gemm shared_attn {name} {P}x{beam} T={T}: worst rel. err vs the oracle {worst:.3e} on rows {rows}")
    again = _forced_steps(eng, V, emb, mask, beam, True)
    for a, b_ in zip((logits, k, v), again):
        assert torch.equal(a, b_), (name, "repeat")
    n2 = _counts()
    _, k0, v0 = _forced_steps(eng, V, emb, mask, beam, False)
    n3 = _counts()
    assert (n3[0] - n2[0], n3[1] - n2[1]) == (0, N)
    assert torch.equal(k[0, :, :, 0], k0[0, :, :, 0]) and torch.equal(v[0, :, :, 0], v0[0, :, :, 0]), "layer 0: the appended K / V of the first step"
    for l in range(1, k.shape[0]):
        assert rel_err(k[l, :, :, 0].float().cpu(), k0[l, :, :, 0].float().cpu()) < 2e-2 and rel_err(v[l, :, :, 0].float().cpu(), v0[l, :, :, 0].float().cpu()) < 2e-2


@pytest.mark.parametrize("n,group", [(4, 2), (4, 5), (16, 2), (16, 5)])
def test_generate_beam_shared_attn_matches_oracle(small, n, group):
    """`generate(method="beam", decode_gemm=True, shared_attn=True)`, beam 10: the prompts, seeds and cases of
    test_generate_beam_decode_gemm_matches_oracle against the oracle's diverse beam search (the tie-aware rule of tests/beam_oracle.py)."""
    from oracle import llama_ref as LR
    m, w = small["model"], small["w"]
    instr, slots = _prompts(n, seed=n * 10 + group)
    emb, mask = _oracle_embeds(small, _gen_inputs(small, instr, slots))
    enc = LR.make_text_encoder(w["llama"], small["lgeom"])
    trace = []
    kw = dict(max_len=6, beam_size=10, beam_group_size=group, diversity_penalty=0.8)
    t_ref, s_ref, lg_ref = LR.beam_search(enc, emb, mask, vocab_size=small["lgeom"].vocab, eos_id=m.tokenizer.eos_token_id, trace=trace, **kw)
    n0, d0 = _counts(), decode_counts()
    tokens, scores, logits, _ = m.generate(_gen_inputs(small, instr, slots), method="beam", decode_gemm=True, shared_attn=True, **kw)
    n1 = _counts()
    assert (n1[0] - n0[0], n1[1] - n0[1]) == (kw["max_len"] - 1,) * 2 and decode_counts() == d0
    assert_beam_matches_oracle(tokens, scores, logits, t_ref, s_ref, lg_ref, trace)


def test_generate_beam_refuses_shared_attn_off_the_shared_cache(monkeypatch):
    """shared_attn without the shared cache (PCY_DISABLE=beam_kv_shared; 1 prompt x beam 5, whose plan is the plain cache) or without the GEMM
    step: ValueError before anything is launched.  A call without shared_attn raises neither counter."""
    kw, sd, eng = _geo("small")
    g = torch.Generator().manual_seed(3)
    emb4 = (torch.randn(4, 9, kw["d"], generator=g) * 0.02).to(BF).cuda()
    mask4 = torch.ones(4, 9)
    args = (5, 10, 2, 0.8, -1, 8)

    def refused(emb, mask, beam, **opt):
        n0, d0 = _counts(), decode_counts()
        with pytest.raises(ValueError, match="shared_attn"):
            eng.generate_beam(emb, mask, 5, beam, beam // 5, 0.8, -1, 8, shared_attn=True, **opt)
        assert _counts() == n0 and decode_counts() == d0

    pcy_disable(monkeypatch, "beam_kv_shared")
    refused(emb4, mask4, 10, decode_gemm=True)
    pcy_disable(monkeypatch)
    refused(emb4[:1], mask4[:1], 5, decode_gemm=True)
    refused(emb4, mask4, 10)                                   # (decode_gemm=False: the GEMM step is not in use)
    n0 = _counts()
    eng.generate_beam(emb4, mask4, *args)
    assert _counts() == n0
    eng.generate_beam(emb4, mask4, *args, decode_gemm=True)
    n1 = _counts()
    assert (n1[0] - n0[0], n1[1] - n0[1]) == (0, 4)
    eng.generate_beam(emb4, mask4, *args, decode_gemm=True, shared_attn=True)
    n2 = _counts()
    assert (n2[0] - n1[0], n2[1] - n1[1]) == (4, 4)


def test_decode_gemm_mq_refuses_fp8_and_plain_caches(monkeypatch):
    """pcy_llama_decode_gemm_mq: a plain cache, a grouped cache, B beyond the cache's rows and fp8 layers are argument errors that launch nothing"""
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import Context, GenState
    kw, sd, eng = _geo("small")
    pcy_disable(monkeypatch)
    P, beam, T, V = 4, 10, 10, kw["vocab"]
    B = P * beam
    emb, mask = _prompt_batch(P, T, kw["d"], seed=9)
    prefix = eng.new_cache(P, T)
    eng.prefill(emb.cuda(), None, prefix, "last")
    shared = eng.new_beam_cache(prefix, beam, 4)
    plain = eng.new_cache(B, T + 4)
    grouped = eng.new_grouped_cache(prefix, [10, 10, 10, 10], [T, T - 1, T, T - 2], 4)
    st = GenState(64, V, 4, "cuda")
    st.pos.fill_(T)
    st.logits.fill_(1.0)
    Context.get().sync()

    def refused(c, rows, match):
        k0, v0, n0, d0 = c.k.clone(), c.v.clone(), _counts(), decode_counts()
        with pytest.raises(PcyError, match=match):
            eng.decode_gemm(c, st, rows, shared_attn=True)
        Context.get().sync()
        assert _counts() == n0 and decode_counts() == d0
        assert torch.equal(c.k, k0) and torch.equal(c.v, v0) and bool((st.logits == 1.0).all())

    refused(plain, B, "no shared prefix")
    refused(grouped, B, "grouped")
    refused(shared, B + 1, "cache rows")
    eng.quantize_fp8()
    try:
        refused(shared, B, "fp8")
    finally:
        eng.set_fp8(False)
    n0 = _counts()
    eng.decode_gemm(shared, st, B, shared_attn=True)          # ... and the same call is served once the fp8 layers are off
    Context.get().sync()
    n1 = _counts()
    assert (n1[0] - n0[0], n1[1] - n0[1]) == (1, 1) and torch.isfinite(st.logits[:B].float()).all()
