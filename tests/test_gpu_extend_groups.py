"""GPU: the GROUPED extension (pcy_attn_extend_grouped / pcy_llama_extend_grouped): the rows of a call are groups, group g
reads the first len[g] slots of prefix row g and every row's own panel starts right behind its group's prefix.  Operator, engine
(LlamaEngine.new_grouped_cache / extend(own_past=...)), `forward(share_prefix="groups")` and `score_candidates(ragged=True)`.

The bit contract: packed == unpacked, and every row of a grouped call == that row ALONE through the uniform pcy_attn_extend on a one-row plain
cache with the same logical contents and t_past = len[g] + t_own.  The prefix slots at and above len[g] hold NaN in every operator case and
everything unwritten holds the poison value: a kernel that addresses either shows up in the output or in the cache comparison.
The oracle bars are those of tests/test_gpu_extend.py / test_gpu_extend_packed.py for the same arithmetic (restated, not widened)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import score_common as SC
from conftest import assert_bf16_close, record_parity, rel_err

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
POISON = 768.0      # (exact in bf16)
N_LAYERS, LAYER = 2, 1


def rnd(*shape, seed=0, std=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * std).to(BF)


def bits(x):
    return x.view(torch.int16)


@pytest.fixture(scope="module")
def ctx():
    from procyon_amd.engine import Context
    return Context.get()


# ---------------------------------------------------------------------------------------------------------------- the operator
#        H  Hkv  dh  prefix_T  [(rows, len) ...]            t_own  S  keep
CASES = [(8, 2, 128, 45, [(3, 45), (1, 7), (2, 33)], 0, 5, "none"),     # len == prefix_T; len < 32: no shared-phase block; one shared block + a straddling
                                                                        # one; a tile spanning several rows; a one-row group
         (4, 2, 64, 64, [(1, 64), (3, 32), (2, 1)], 0, 33, "none"),     # G*S = 66 > 64: a row's queries cut by a tile edge; len % 32 == 0; len = 1
         (8, 2, 128, 40, [(2, 40), (2, 12)], 10, 20, "none"),           # t_own > 0
         (4, 2, 64, 40, [(2, 7), (2, 40)], 0, 19, "pads"),              # masks that differ inside a group, pads in prefix and suffix, one row all 0
         (4, 4, 128, 1, [(1, 1), (1, 1)], 0, 1, "none"),                # the smallest shape
         (8, 2, 128, 45, [(5, 20)], 0, 5, "none")]                      # one group, len < prefix_T
IDS = lambda c: f"H{c[0]}kv{c[1]}dh{c[2]}-pre{c[3]}-" + "_".join(f"{r}x{n}" for r, n in c[4]) + f"-own{c[5]}-S{c[6]}-{c[7]}"


def _cfg(H, Hkv, dh):
    from procyon_amd.engine import LlamaConfig
    return LlamaConfig(vocab=16, d=H * dh, n_layers=N_LAYERS, n_heads=H, n_kv_heads=Hkv, ffn=64)


def _fill(cache, layer, k_rows, v_rows):
    """poison everything, then put k_rows / v_rows [rows, Hkv, t, dh] into slots [0, t) of `layer`"""
    cache.k.fill_(POISON)
    cache.v.fill_(POISON)
    t = k_rows.shape[2]
    if t:
        cache.k[layer, :, :, :t] = k_rows.cuda()
        cache.v[layer, :, :, :t] = v_rows.cuda()


def _rows_of(groups):
    return [g for g, (r, _) in enumerate(groups) for _ in range(r)]


def _make_cache(case):
    """-> (grouped cache, per-row logical K / V lists [Hkv, len + t_own, dh] on the CPU); deterministic: two calls give twins.
    Prefix slots at and above len[g] hold NaN, the other layer and every unwritten own slot the poison value."""
    from procyon_amd.engine import KVCache
    H, Hkv, dh, Tp, groups, t_own, S, _ = case
    cfg = _cfg(H, Hkv, dh)
    n, B = len(groups), sum(r for r, _ in groups)
    pre_k, pre_v = rnd(n, Hkv, Tp, dh, seed=13), rnd(n, Hkv, Tp, dh, seed=14)
    for g, (_, ln) in enumerate(groups):
        pre_k[g, :, ln:] = float("nan")
        pre_v[g, :, ln:] = float("nan")
    own_k, own_v = rnd(B, Hkv, t_own, dh, seed=11), rnd(B, Hkv, t_own, dh, seed=12)
    prefix = KVCache(cfg, n, Tp, "cuda")
    _fill(prefix, LAYER, pre_k, pre_v)
    cache = KVCache.grouped(cfg, "cuda", prefix, [r for r, _ in groups], [ln for _, ln in groups], t_own + S + 3)
    _fill(cache, LAYER, own_k, own_v)
    k_log = [torch.cat([pre_k[g, :, :groups[g][1]], own_k[b]], 1) for b, g in enumerate(_rows_of(groups))]
    v_log = [torch.cat([pre_v[g, :, :groups[g][1]], own_v[b]], 1) for b, g in enumerate(_rows_of(groups))]
    return cache, k_log, v_log


def _keep_for(case):
    """[B, prefix_T + Tmax] in every row's OWN logical slots (its len[g] prefix slots, then its own panel)"""
    H, Hkv, dh, Tp, groups, t_own, S, mode = case
    if mode == "none":
        return None
    B = sum(r for r, _ in groups)
    keep = torch.ones(B, Tp + t_own + S + 3, dtype=torch.uint8)
    assert groups == [(2, 7), (2, 40)]
    keep[0, :3] = 0                   # pads inside the (short) prefix ...
    keep[1, 7 + 15:] = 0              # ... right pads in the suffix of the group's other row: the masks differ inside a group
    keep[2, :33] = 0                  # beyond the first 32-key block of the long prefix
    keep[2, 40 + 10:] = 0
    keep[3, :] = 0                    # one row with every byte 0: every query of it has no allowed key
    return keep


def _reference_row(case, qkv_row, k_log, v_log, keep_row, t_past):
    """oracle formulas for ONE row: apply_rope at t_past + s, then layer_forward's eager attention under build_additive_mask"""
    from oracle import llama_ref as LR
    from procyon_amd.engine import rope_tables
    H, Hkv, dh, _, _, _, S, _ = case
    cos, sin = rope_tables(dh, 10000.0, t_past + S, "cpu")
    q = qkv_row[:, :H * dh].view(1, S, H, dh).transpose(1, 2)
    k = qkv_row[:, H * dh:(H + Hkv) * dh].view(1, S, Hkv, dh).transpose(1, 2)
    v = qkv_row[:, (H + Hkv) * dh:].view(1, S, Hkv, dh).transpose(1, 2)
    q, k = LR.apply_rope(q, k, cos[t_past:t_past + S][None], sin[t_past:t_past + S][None])
    kk, vv = torch.cat([k_log[None], k], 2), torch.cat([v_log[None], v], 2)
    g = H // Hkv
    ke = kk[:, :, None].expand(1, Hkv, g, t_past + S, dh).reshape(1, H, t_past + S, dh)
    ve = vv[:, :, None].expand(1, Hkv, g, t_past + S, dh).reshape(1, H, t_past + S, dh)
    sc = torch.matmul(q, ke.transpose(2, 3)) * (dh ** -0.5)
    sc = sc + LR.build_additive_mask(None if keep_row is None else keep_row[None, :t_past + S], 1, S, t_past, BF)
    p = F.softmax(sc, dim=-1, dtype=torch.float32).to(BF)
    return torch.matmul(p, ve).transpose(1, 2).contiguous().reshape(S, H * dh), k[0], v[0]


def _dev_keep(keep, cache):
    if keep is None:
        return None
    kd = torch.zeros(keep.shape[0], cache.capacity, dtype=torch.uint8)
    n = min(cache.capacity, keep.shape[1])
    kd[:, :n] = keep[:, :n]
    return kd.cuda()


def _run(ctx, case, cache, qkv, keep, packed):
    from procyon_amd.engine import rope_tables
    H, Hkv, dh, Tp, groups, t_own, S, _ = case
    cos, sin = rope_tables(dh, 10000.0, Tp + t_own + S + 8, "cuda")
    return ctx.attn_extend(qkv.cuda().clone(), cache, LAYER, t_own, cos, sin, H, Hkv, dh, keep=_dev_keep(keep, cache), packed=packed, groups=cache).cpu()


def _run_alone(ctx, case, qkv_row, k_log, v_log, keep_row, t_past, packed):
    """the row through today's pcy_attn_extend on a one-row PLAIN cache with the same logical contents"""
    from procyon_amd.engine import KVCache, rope_tables
    H, Hkv, dh, Tp, groups, t_own, S, _ = case
    one = KVCache(_cfg(H, Hkv, dh), 1, t_past + S + 3, "cuda")
    _fill(one, LAYER, k_log[None], v_log[None])
    cos, sin = rope_tables(dh, 10000.0, Tp + t_own + S + 8, "cuda")
    kd = None if keep_row is None else _dev_keep(keep_row[None], one)
    return ctx.attn_extend(qkv_row.cuda().clone(), one, LAYER, t_past, cos, sin, H, Hkv, dh, keep=kd, packed=packed).cpu()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_grouped_operator_bits_and_oracle(ctx, case):
    H, Hkv, dh, Tp, groups, t_own, S, mode = case
    row_grp = _rows_of(groups)
    B = len(row_grp)
    cache_u, k_log, v_log = _make_cache(case)
    cache_p, _, _ = _make_cache(case)
    assert torch.equal(bits(cache_u.prefix.k), bits(cache_p.prefix.k)) and torch.equal(cache_u.k, cache_p.k)            # twins
    assert any(ln < Tp for _, ln in groups) == bool(torch.isnan(cache_p.prefix.k[LAYER].float()).any())                  # the NaN slots exist
    qkv = rnd(B * S, (H + 2 * Hkv) * dh, seed=1)
    keep = _keep_for(case)
    pre_before = (cache_p.prefix.k.clone(), cache_p.prefix.v.clone())
    out_u = _run(ctx, case, cache_u, qkv, keep, False)
    out_p = _run(ctx, case, cache_p, qkv, keep, True)
    print(f"grouped attn_extend packed vs unpacked {IDS(case)}: {(out_p != out_u).float().mean().item():.4f} of elements differ")
    assert bool(torch.isfinite(out_u.float()).all()) and bool(torch.isfinite(out_p.float()).all())                       # no NaN slot was read
    assert torch.equal(out_p, out_u)
    assert torch.equal(cache_p.k, cache_u.k) and torch.equal(cache_p.v, cache_u.v)
    # every row alone, through the uniform operator (unpacked and packed) on a one-row plain cache with t_past = len[g] + t_own
    refs, k_new, v_new = [], [], []
    for b, g in enumerate(row_grp):
        t_past = groups[g][1] + t_own
        kb = None if keep is None else keep[b]
        q_row = qkv[b * S:(b + 1) * S]
        for packed in (False, True):
            alone = _run_alone(ctx, case, q_row, k_log[b], v_log[b], kb, t_past, packed)
            assert torch.equal(alone, out_p[b * S:(b + 1) * S]), f"row {b} (group {g}) alone, packed={packed}"
        r, kn, vn = _reference_row(case, q_row, k_log[b], v_log[b], kb, t_past)
        refs.append(r)
        k_new.append(kn)
        v_new.append(vn)
    # the oracle formulas, with the bars of the uniform operator's tests
    ref = torch.cat(refs, 0)
    err = rel_err(out_p, ref)
    print(f"grouped attn_extend {IDS(case)}: rel_err {err:.3e}, {(out_p != ref).float().mean().item():.4f} of elements differ")
    record_parity(f"extend_groups/operator/{IDS(case)}", rel_err=err)
    assert err < 1e-3
    assert_bf16_close(out_p, ref, "attn_extend grouped", max_frac=0.03, inter=torch.full_like(ref, 0.5 if mode == "none" else 0.03))
    # K / V: own slots [t_own, t_own + S) hold the roped reference, what was there stays, poison everywhere else, the other layer untouched
    s0 = t_own
    assert torch.equal(cache_p.k[LAYER, :, :, s0:s0 + S].cpu(), torch.stack(k_new)) and torch.equal(cache_p.v[LAYER, :, :, s0:s0 + S].cpu(), torch.stack(v_new))
    assert bool((cache_p.k[LAYER, :, :, s0 + S:] == POISON).all()) and bool((cache_p.v[LAYER, :, :, s0 + S:] == POISON).all())
    assert bool((cache_p.k[1 - LAYER] == POISON).all()) and bool((cache_p.v[1 - LAYER] == POISON).all())
    if t_own:
        own_k = torch.stack([k_log[b][:, groups[g][1]:] for b, g in enumerate(row_grp)])
        own_v = torch.stack([v_log[b][:, groups[g][1]:] for b, g in enumerate(row_grp)])
        assert torch.equal(cache_p.k[LAYER, :, :, :t_own].cpu(), own_k) and torch.equal(cache_p.v[LAYER, :, :, :t_own].cpu(), own_v)
    # the prefix cache is bit-unchanged, NaN included
    assert torch.equal(bits(cache_p.prefix.k), bits(pre_before[0])) and torch.equal(bits(cache_p.prefix.v), bits(pre_before[1]))
    if keep is None:                                                                                                     # keep all ones == keep None
        _fill(cache_p, LAYER, rnd(B, Hkv, t_own, dh, seed=11), rnd(B, Hkv, t_own, dh, seed=12))
        ones = torch.ones(B, cache_p.capacity, dtype=torch.uint8)
        assert torch.equal(_run(ctx, case, cache_p, qkv, ones, True), out_p), "keep all ones vs keep = None"


def test_uniform_table_equals_the_uniform_entries(ctx):
    """[(3, 45), (3, 45)] on the geometry of CASES[0]: the bits of pcy_attn_extend and pcy_attn_extend_packed on a `new_shared_cache` twin"""
    from procyon_amd.engine import KVCache, rope_tables
    H, Hkv, dh, Tp, _, _, S, _ = CASES[0]
    case = (H, Hkv, dh, Tp, [(3, 45), (3, 45)], 0, S, "none")
    qkv = rnd(6 * S, (H + 2 * Hkv) * dh, seed=1)
    cos, sin = rope_tables(dh, 10000.0, Tp + S + 8, "cuda")
    for packed in (False, True):
        grouped, _, _ = _make_cache(case)
        twin = KVCache(_cfg(H, Hkv, dh), 6, S + 3, "cuda", prefix=grouped.prefix, rows_per_prefix=3)
        twin.k.copy_(grouped.k)
        twin.v.copy_(grouped.v)
        out_g = _run(ctx, case, grouped, qkv, None, packed)
        out_t = ctx.attn_extend(qkv.cuda().clone(), twin, LAYER, Tp, cos, sin, H, Hkv, dh, packed=packed).cpu()
        assert torch.equal(out_g, out_t), f"packed={packed}"
        assert torch.equal(grouped.k, twin.k) and torch.equal(grouped.v, twin.v)


def _raw_groups(cache, rows, lens, t_own):
    """a pcy_prefix_groups with HOST arrays of the test's choosing (the device tables are the cache's own: nothing may be launched anyway)"""
    from procyon_amd import _lib
    h_rows, h_len = (C.c_int32 * max(len(rows), 1))(*rows), (C.c_int32 * max(len(lens), 1))(*lens)
    ga = _lib.PrefixGroups(len(rows), t_own, h_rows, h_len, cache.d_row0.data_ptr(), cache.d_len.data_ptr(), cache.d_row_grp.data_ptr())
    ga._hold = (h_rows, h_len)
    return ga


def test_grouped_operator_argument_errors(ctx):
    """every argument error of pcy_attn_extend_grouped, checked on the host arrays; nothing is written"""
    from procyon_amd import _lib
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import KVCache, rope_tables
    H, Hkv, dh, Tp, S = 8, 2, 128, 45, 5
    case = (H, Hkv, dh, Tp, [(3, 45), (3, 20)], 0, S, "none")
    cache, _, _ = _make_cache(case)                                                         # 6 rows, Tmax = S + 3, two prefix rows
    snap = (cache.k.clone(), cache.v.clone(), cache.prefix.k.clone(), cache.prefix.v.clone())
    cos, sin = rope_tables(dh, 10000.0, 128, "cuda")
    W = (H + 2 * Hkv) * dh
    qkv = rnd(8 * S, W, seed=1).cuda()
    o = torch.empty(8 * S, H * dh, dtype=BF, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(kv, rows, lens, t_own=0, B=6, S_=S, H_=H, Hkv_=Hkv, dh_=dh, ld=W, packed=0):
        ga = _raw_groups(cache, rows, lens, t_own)
        _lib.check(ctx.lib.pcy_attn_extend_grouped(ctx.h, p(qkv), ld, C.byref(kv.c), C.byref(ga), LAYER, p(o), H_ * dh_, p(cos), p(sin), None,
                                                   B, S_, H_, Hkv_, dh_, packed), "pcy_attn_extend_grouped")

    plain = KVCache(_cfg(H, Hkv, dh), 6, 64, "cuda")
    uniform = KVCache(_cfg(H, Hkv, dh), 6, S + 3, "cuda", prefix=cache.prefix, rows_per_prefix=3)
    errors = [("the groups hold 5 rows", lambda pk: call(cache, [3, 2], [45, 20], packed=pk)),               # sum(rows) != B
              ("exceeds cache rows", lambda pk: call(cache, [4, 3], [45, 20], B=7, packed=pk)),              # B beyond the cache's rows
              (r"rows=0", lambda pk: call(cache, [6, 0], [45, 20], packed=pk)),                              # a rows[g] < 1
              (r"len=0 outside", lambda pk: call(cache, [3, 3], [0, 20], packed=pk)),                        # a len[g] outside [1, prefix_T]
              (r"len=46 outside", lambda pk: call(cache, [3, 3], [45, 46], packed=pk)),
              ("suffix capacity", lambda pk: call(cache, [3, 3], [45, 20], t_own=4, packed=pk)),             # t_own + S > Tmax
              ("3 groups need more", lambda pk: call(cache, [2, 2, 2], [45, 20, 20], packed=pk)),            # n_groups > prefix_B
              ("rows_per_prefix == 0", lambda pk: call(plain, [3, 3], [45, 20], packed=pk)),                 # a plain cache
              ("rows_per_prefix == 0", lambda pk: call(uniform, [3, 3], [45, 20], packed=pk)),               # ... or one with rows_per_prefix != 0
              ("S=0", lambda pk: call(cache, [3, 3], [45, 20], S_=0, packed=pk)),                            # S < 1
              ("head_dim", lambda pk: call(cache, [3, 3], [45, 20], H_=8, Hkv_=2, dh_=32, ld=12 * 32, packed=pk))]
    for match, fn in errors:
        msgs = []
        for pk in (0, 1):
            with pytest.raises(PcyError, match=match) as ei:
                fn(pk)
            msgs.append(str(ei.value))
        assert msgs[0] == msgs[1]
    for a, b in zip(snap, (cache.k, cache.v, cache.prefix.k, cache.prefix.v)):
        assert torch.equal(bits(a), bits(b))
    assert bool((plain.k == 0).all()) and bool((uniform.k == 0).all())
    # the uniform operator refuses a grouped cache: never a fallback
    with pytest.raises(PcyError, match="shared-prefix cache needs"):
        ctx.attn_extend(qkv[:6 * S], cache, LAYER, Tp, cos, sin, H, Hkv, dh)
    with pytest.raises(PcyError, match="shared-prefix cache needs"):
        ctx.attn_extend(qkv[:6 * S], cache, LAYER, Tp, cos, sin, H, Hkv, dh, packed=True)
    assert torch.equal(cache.k, snap[0])


# ---------------------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def env():
    from oracle import esm_ref as ER
    from oracle import llama_ref as LR
    e = SC.build_env()
    g = e["w"]["geom"]
    e["lgeom"], e["egeom"] = LR.LlamaGeom(**g["llama"]), ER.EsmGeom(**g["esm"])
    return e


GROUPS = [(3, 13), (1, 5), (2, 9)]      # (rows, len)
TP_, S_, S2_ = 13, 9, 4
ROW_GRP = _rows_of(GROUPS)
ROW_LEN = [GROUPS[g][1] for g in ROW_GRP]


@pytest.fixture(scope="module")
def work(env):
    """three prompts of 13 / 5 / 9 tokens with 3 / 1 / 2 rows of S = 9 tokens (right pads in two rows) and S2 = 4 more: the oracle on the
    concatenated REAL rows, the existing prefill of the same rows, D and the bar (built as tests/test_gpu_extend.py builds its own) -- once"""
    from oracle import llama_ref as LR
    eng = env["model"].text_encoder.engine
    sd, geom = env["w"]["llama"], env["lgeom"]
    g = torch.Generator().manual_seed(31)
    B, n = len(ROW_GRP), len(GROUPS)
    pre_ids = torch.randint(0, 2000, (n, TP_), generator=g)
    pmask = (torch.arange(TP_)[None] < torch.tensor([ln for _, ln in GROUPS])[:, None]).long()      # RIGHT-padded prompts
    suf_ids = torch.randint(0, 2000, (B, S_ + S2_), generator=g)
    smask = torch.ones(B, S_ + S2_, dtype=torch.long)
    smask[1, 6:S_] = 0
    smask[5, 4:S_] = 0
    labels = torch.where(smask.bool(), suf_ids, torch.full_like(suf_ids, -100))[:, :S_].clone()
    labels[:, 0] = -100
    emb_w = sd["model.embed_tokens.weight"]
    pre_emb, suf_emb = F.embedding(pre_ids, emb_w), F.embedding(suf_ids, emb_w)
    T = TP_ + S_ + S2_
    cat_emb = torch.zeros(B, T, emb_w.shape[1], dtype=BF)
    cat_mask = torch.zeros(B, T, dtype=torch.long)
    lg_ref = []
    for b, gi in enumerate(ROW_GRP):
        ln = ROW_LEN[b]
        row = torch.cat([pre_emb[gi, :ln], suf_emb[b]], 0)
        m = torch.cat([torch.ones(ln, dtype=torch.long), smask[b]])
        lg_ref.append(LR.llama_forward(sd, geom, inputs_embeds=row[None], attn_mask=m[None])["logits"][0, ln:])
        cat_emb[b, :ln + S_ + S2_] = row
        cat_mask[b, :ln + S_ + S2_] = m
    lg_ref = torch.stack(lg_ref)                                                # [B, S + S2, V]
    V = lg_ref.shape[-1]
    ce = F.cross_entropy(lg_ref.float()[:, :S_ - 1].reshape(-1, V), labels[:, 1:].reshape(-1), ignore_index=-100, reduction="none").view(B, S_ - 1)
    # D: the EXISTING prefill on the same rows (right-padded to one length)
    own, _ = eng.prefill(cat_emb.cuda(), cat_mask, eng.new_cache(B, T), torch.arange(B * T, dtype=torch.int32))
    own = own.view(B, T, V).cpu()
    own = torch.stack([own[b, ROW_LEN[b]:ROW_LEN[b] + S_ + S2_] for b in range(B)])
    delta = float((own.float() - lg_ref.float()).abs().max())
    labelled = labels[:, 1:] != -100
    rows_ref = lg_ref[:, :S_ - 1][labelled].float()
    l64 = torch.logsumexp(rows_ref.double(), -1)
    nll64 = l64 - rows_ref.double().gather(1, labels[:, 1:][labelled][:, None])[:, 0]
    err_a = float((ce[labelled].double() - nll64).abs().max())
    big = torch.maximum(l64.abs(), rows_ref.max(-1).values.double().abs()).max()
    op_bar = 8 * max(err_a, 2.0 ** (math.floor(math.log2(float(big))) - 23))
    bar = 2 * delta + 2 * 2.0 ** -7 * float(lg_ref.float().abs().max()) + op_bar
    # keep in every row's OWN logical slots: [len real prefix slots][S + S2 suffix slots]
    keep = torch.zeros(B, TP_ + S_ + S2_, dtype=torch.long)
    for b in range(B):
        keep[b, :ROW_LEN[b]] = 1
        keep[b, ROW_LEN[b]:ROW_LEN[b] + S_ + S2_] = smask[b]
    return dict(pmask=pmask, labels=labels, keep=keep, pre_emb=pre_emb, suf_emb=suf_emb, lg_ref=lg_ref, ce=ce, labelled=labelled, delta=delta,
                op_bar=op_bar, bar=bar, B=B, V=V)


def _prefix(env, work):
    eng = env["model"].text_encoder.engine
    prefix = eng.new_cache(len(GROUPS), TP_)
    eng.prefill(work["pre_emb"].cuda(), work["pmask"], prefix, logit_rows=None)
    return prefix


def _extend_grouped(env, work, prefix=None, **kw):
    eng = env["model"].text_encoder.engine
    prefix = _prefix(env, work) if prefix is None else prefix
    cache = eng.new_grouped_cache(prefix, [r for r, _ in GROUPS], [ln for _, ln in GROUPS], S_ + S2_)
    return eng.extend(cache, work["suf_emb"][:, :S_].cuda(), keep=work["keep"][:, :TP_ + S_], **kw), cache


def _counts(lib):
    from procyon_amd import _lib
    return (lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND), lib.pcy_debug_dispatch_count(_lib.DISPATCH_EXTEND_PACKED),
            lib.pcy_debug_extend_grouped_count())


def test_engine_grouped_against_the_oracle_packed_equals_unpacked(env, work):
    eng = env["model"].text_encoder.engine
    lib = eng.ctx.lib
    kw = dict(logit_rows="all", labels=work["labels"], want_hidden=True)
    e0, p0, g0 = _counts(lib)
    (lg_u, hid_u, nll_u, n_u), cache_u = _extend_grouped(env, work, **kw)
    assert _counts(lib) == (e0 + 1, p0, g0 + 1)                           # a grouped call: the extension's count and the grouped one
    (lg_p, hid_p, nll_p, n_p), cache_p = _extend_grouped(env, work, packed=True, **kw)
    assert _counts(lib) == (e0 + 2, p0 + 1, g0 + 2)                       # ... and the packed one when packed
    B, V, bar, labelled = work["B"], work["V"], work["bar"], work["labelled"]
    assert lg_u.shape == (B * S_, V) and hid_u.shape == (B, S_, eng.cfg.d) and nll_u.shape == (B, S_)
    assert n_u == n_p == int(labelled.sum())
    assert torch.equal(lg_p, lg_u) and torch.equal(nll_p, nll_u) and torch.equal(hid_p, hid_u)
    assert torch.equal(cache_p.k, cache_u.k) and torch.equal(cache_p.v, cache_u.v)
    lg = lg_u.view(B, S_, V).cpu().float()
    tn = nll_u.cpu()
    err_lg = float((lg - work["lg_ref"][:, :S_].float()).abs().max())
    err_tok = float((tn[:, 1:][labelled] - work["ce"][labelled]).abs().max())
    print(f"grouped extend vs oracle: logits err {err_lg:.3e} token_nll err {err_tok:.3e} D {work['delta']:.3e} op_bar {work['op_bar']:.3e} bar {bar:.3e}")
    record_parity("extend_groups/vs_oracle", logits_err=err_lg, token_nll_err=err_tok, delta=work["delta"], bar=bar)
    assert bool((tn[:, 0] == 0).all()) and bool((tn[:, 1:][~labelled] == 0).all())
    assert err_lg <= bar and err_tok <= bar
    assert bar < 0.5
    # a second extension behind the first: own_past = S
    lg2, _, _, _ = eng.extend(cache_p, work["suf_emb"][:, S_:].cuda(), own_past=S_, keep=work["keep"], logit_rows="all", packed=True)
    lg2u, _, _, _ = eng.extend(cache_u, work["suf_emb"][:, S_:].cuda(), own_past=S_, keep=work["keep"], logit_rows="all")
    assert torch.equal(lg2, lg2u) and torch.equal(cache_p.k, cache_u.k)
    err2 = float((lg2.view(B, S2_, V).cpu().float() - work["lg_ref"][:, S_:].float()).abs().max())
    print(f"grouped extend, own_past = {S_}: logits err {err2:.3e} (bar {bar:.3e})")
    record_parity("extend_groups/second_extension_vs_oracle", logits_err=err2, bar=bar)
    assert err2 <= bar
    # KVCache.layer: the logical rows per row
    ks, _ = cache_p.layer(0, S_ + S2_)
    assert [k.shape[1] for k in ks] == [ln + S_ + S2_ for ln in ROW_LEN]


def test_engine_uniform_table_equals_the_shared_cache(env):
    """len == prefix_T in every group: the GEMM shapes are those of `extend` on `new_shared_cache`, so the bits must match (left pads in a prompt,
    right pads in two suffixes: the keep layouts coincide)"""
    eng = env["model"].text_encoder.engine
    sd = env["w"]["llama"]
    g = torch.Generator().manual_seed(21)
    P, N, TP, S = 2, 3, 13, 9
    pre_ids, suf_ids = torch.randint(0, 2000, (P, TP), generator=g), torch.randint(0, 2000, (P * N, S), generator=g)
    pmask = torch.ones(P, TP, dtype=torch.long)
    pmask[1, :5] = 0
    smask = torch.ones(P * N, S, dtype=torch.long)
    smask[1, 6:] = 0
    smask[5, 4:] = 0
    labels = torch.where(smask.bool(), suf_ids, torch.full_like(suf_ids, -100))
    labels[:, 0] = -100
    emb_w = sd["model.embed_tokens.weight"]
    prefix = eng.new_cache(P, TP)
    eng.prefill(F.embedding(pre_ids, emb_w).cuda(), pmask, prefix, logit_rows=None)
    suf = F.embedding(suf_ids, emb_w).cuda()
    keep = torch.cat([pmask.repeat_interleave(N, 0), smask], 1)
    for packed in (False, True):
        shared = eng.new_shared_cache(prefix, N, S)
        grouped = eng.new_grouped_cache(prefix, [N] * P, [TP] * P, S)
        a = eng.extend(shared, suf, TP, keep=keep, logit_rows="all", labels=labels, want_hidden=True, packed=packed)
        b = eng.extend(grouped, suf, keep=keep, logit_rows="all", labels=labels, want_hidden=True, packed=packed)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3], f"packed={packed}"
        assert torch.equal(shared.k, grouped.k) and torch.equal(shared.v, grouped.v)


def test_engine_grouped_argument_errors(env, work):
    from procyon_amd._lib import PcyError
    from procyon_amd.engine import GenState
    eng = env["model"].text_encoder.engine
    prefix = _prefix(env, work)
    rows, lens = [r for r, _ in GROUPS], [ln for _, ln in GROUPS]
    cache = eng.new_grouped_cache(prefix, rows, lens, S_)
    cache.k.fill_(POISON)
    cache.v.fill_(POISON)
    snap = (cache.k.clone(), cache.v.clone(), prefix.k.clone(), prefix.v.clone())
    emb = work["suf_emb"][:, :S_].cuda()
    # the host side
    with pytest.raises(ValueError, match="own_past"):
        eng.extend(cache, emb, TP_)                                               # t_past with a grouped cache
    with pytest.raises(ValueError, match="own_past"):
        eng.extend(eng.new_shared_cache(prefix, 2, S_), emb, TP_, own_past=0)     # own_past with any other cache
    with pytest.raises(ValueError, match="keep"):
        eng.extend(cache, emb, keep=torch.ones(6, TP_ + S_ - 1))                  # keep shorter than the longest row
    with pytest.raises(ValueError, match="outside"):
        eng.new_grouped_cache(prefix, rows, [14, 5, 9], S_)
    with pytest.raises(ValueError, match="groups on a prefix cache"):
        eng.new_grouped_cache(prefix, [1, 1, 1, 1], [5, 5, 5, 5], S_)
    # the library
    with pytest.raises(PcyError, match="suffix capacity"):
        eng.extend(cache, emb, own_past=1)                                        # t_own + S > Tmax
    with pytest.raises(PcyError, match="S=0"):
        eng.extend(cache, emb[:, :0])                                             # S < 1
    big_prefix = eng.new_cache(1, 4090)
    big = eng.new_grouped_cache(big_prefix, [1], [4090], 16)
    with pytest.raises(PcyError, match="rope table"):
        eng.extend(big, emb[:1])                                                  # max(len) + t_own + S > max_pos
    assert bool((big.k == 0).all())
    eng.quantize_fp8()
    try:
        with pytest.raises(PcyError, match="fp8"):
            eng.extend(cache, emb)                                                # fp8 layers
    finally:
        eng.set_fp8(False)
    # every other entry refuses a grouped cache (rows_per_prefix == 0) with its present message
    cache.group_rows, saved = None, cache.group_rows                              # (hand the cache to the uniform entry as it is)
    try:
        for packed in (False, True):
            with pytest.raises(PcyError, match="shared-prefix cache needs"):
                eng.extend(cache, emb, TP_, packed=packed)
    finally:
        cache.group_rows = saved
    st = GenState(6, eng.cfg.vocab, 1, eng.device)
    st.pos.fill_(TP_)
    with pytest.raises(PcyError, match="shared-prefix cache needs"):
        eng.decode(cache, st, 6)
    with pytest.raises(PcyError, match="cannot be prefilled"):
        eng.prefill(emb, None, cache, logit_rows=None)
    for a, b in zip(snap, (cache.k, cache.v, prefix.k, prefix.v)):
        assert torch.equal(a, b)
    lg, _, _, _ = eng.extend(cache, emb, keep=work["keep"][:, :TP_ + S_], logit_rows="last")     # after the refusals the call still works
    assert lg.shape == (6, work["V"]) and bool(torch.isfinite(lg.float()).all())


# ---------------------------------------------------------------------------------------------------------------- the model
QA_HEAD = "w11 w12 w13 <|protein|> binds <|protein|> ? [ANSWER] yes w14 w15 w16 w17 w18 w19 w20 w21 <|protein|> binds"    # the construction of
TAILS_A, TAILS_B = ["", "w5", "w5 w6"], ["", "w7", "w8 w6"]                                                            # tests/test_gpu_extend_packed.py
_qa = lambda t: QA_HEAD + " <|protein|> " + (t + " " if t else "") + "? [ANSWER]"
# two receptors (the third slot: protein 0 / protein 1) x three tails, and a singleton; interleaved A0 B0 ONE A1 B1 A2 B2
MIX_INSTR = [_qa(TAILS_A[0]), _qa(TAILS_B[0]), "w30 w31 <|protein|> ? [ANSWER]", _qa(TAILS_A[1]), _qa(TAILS_B[1]), _qa(TAILS_A[2]), _qa(TAILS_B[2])]
MIX_SLOTS = [[0, 1, 0, 2], [0, 1, 1, 3], [4], [0, 1, 0, 5], [0, 1, 1, 6], [0, 1, 0, 7], [0, 1, 1, 2]]
ONE_INSTR = [_qa(t) for t in TAILS_A + TAILS_B]                                            # the six rows of one receptor of the packed test
ONE_SLOTS = [[0, 1, 0, 2 + i] for i in range(6)]


@pytest.fixture(scope="module")
def prot():
    from procyon_amd import synth
    return synth.protein_tokens([90, 41, 30, 35, 52, 47, 33, 61], seed=3)


def _inputs(prot, instr, slots):
    return {"data": {"seq": prot, "seq_idx": torch.arange(prot.shape[0]), "text": [], "drug": None},
            "input": {"seq": [list(s) for s in slots], "text": [[] for _ in instr], "drug": None},
            "target": {"seq": None, "text": None, "drug": None}, "instructions": list(instr)}


@pytest.fixture(scope="module")
def mix(env, prot):
    """the seven mixed rows: the oracle on the full rows' embeddings and the EXISTING forward, computed once; bar = 2 D + 2 * 2^-7 * max|ref|"""
    from oracle import llama_ref as LR
    m = env["model"]
    emb, ids, am, *_ = m._preprocessing(_inputs(prot, MIX_INSTR, MIX_SLOTS), crop_off=False)
    real = int(am.sum(1).max())
    B = len(MIX_INSTR)
    pos = torch.tensor([int((ids[i] == m.answer_idx).nonzero()[:, 0].max()) for i in range(B)])
    ref = LR.llama_forward(env["w"]["llama"], env["lgeom"], inputs_embeds=emb[:, :real].cpu(), attn_mask=am[:, :real])["logits"]
    ref = ref[torch.arange(B), pos].float()
    own = m.forward(_inputs(prot, MIX_INSTR, MIX_SLOTS))
    D = float((own["outputs"].answer_logits[:, 0].cpu().float() - ref).abs().max())
    return dict(ids=ids, pos=pos, ref=ref, D=D, bar=2 * D + 2 * 2.0 ** -7 * float(ref.abs().max()), B=B, real=real)


def test_forward_groups_against_the_oracle(env, prot, mix):
    m = env["model"]
    eng = m.text_encoder.engine
    lib = eng.ctx.lib
    B, pos = mix["B"], mix["pos"]
    seen = []
    real_prefill = eng.prefill
    eng.prefill = lambda emb, *a, **k: (seen.append(tuple(emb.shape)), real_prefill(emb, *a, **k))[1]
    try:
        e0, p0, g0 = _counts(lib)
        out = m.forward(_inputs(prot, MIX_INSTR, MIX_SLOTS), share_prefix="groups")                     # packed=True is the default of this path
        assert _counts(lib) == (e0 + 1, p0 + 1, g0 + 1)                                                 # ONE extension, grouped and packed
    finally:
        del eng.prefill
    plan = out["prefix_plan"]
    assert plan["n_groups"] == 3 and plan["group_rows"] == [3, 3, 1] and plan["order"].tolist() == [0, 3, 5, 1, 4, 6, 2]
    assert len(seen) == 1 and seen[0][:2] == (3, plan["prefix_T"])                                      # ONE prefill of n_groups rows
    slot3 = int((mix["ids"][0] == m.prot_replacement_idx).nonzero()[3, 0])
    assert plan["group_len"] == [slot3, slot3, int(pos[2])] and plan["group_len"][2] < slot3            # the singleton's prefix is right-padded
    assert torch.equal(out["answer_positions"], pos) and torch.equal(out["text_toks"], mix["ids"])
    out_u = m.forward(_inputs(prot, MIX_INSTR, MIX_SLOTS), share_prefix="groups", packed=False)
    lg, lg_u = out["outputs"].answer_logits, out_u["outputs"].answer_logits
    assert lg.shape == (B, 1, mix["ref"].shape[-1]) and lg.dtype == BF
    assert torch.equal(lg, lg_u), "packed and unpacked grouped extension"
    # the answer logits in the CALLER's row order, against the oracle
    err = float((lg[:, 0].cpu().float() - mix["ref"]).abs().max())
    per_row = (lg[:, 0].cpu().float() - mix["ref"]).abs().max(1).values
    print(f"forward(share_prefix='groups') vs oracle: {err:.3e} (per row {[f'{x:.2e}' for x in per_row.tolist()]}); D {mix['D']:.3e} bar {mix['bar']:.3e}")
    record_parity("extend_groups/forward_vs_oracle", logits_err=err, delta=mix["D"], bar=mix["bar"])
    assert err <= mix["bar"]
    assert mix["bar"] < 0.5
    # the dictionary of share_prefix=True (the ordinary one + the plan), the lazy rest as there
    assert set(out) == set(m.forward(_inputs(prot, MIX_INSTR, MIX_SLOTS))) | {"prefix_plan"}
    lz = out["outputs"].logits
    assert lz.shape == (B, mix["real"], mix["ref"].shape[-1])
    assert torch.equal(lz[torch.arange(B), pos], lg[:, 0]) and lz._full_t is None


def test_forward_groups_with_one_receptor_equals_share_prefix_true(env, prot):
    m = env["model"]
    a = m.forward(_inputs(prot, ONE_INSTR, ONE_SLOTS), share_prefix=True)
    b = m.forward(_inputs(prot, ONE_INSTR, ONE_SLOTS), share_prefix="groups")
    assert b["prefix_plan"]["n_groups"] == 1 and b["prefix_plan"]["group_len"] == [a["prefix_plan"]["Tp"]] and b["prefix_plan"]["S"] == a["prefix_plan"]["S"]
    assert torch.equal(a["outputs"].answer_logits, b["outputs"].answer_logits)
    assert set(a) == set(b)
    with pytest.raises(ValueError, match="retrieval"):
        m.forward(_inputs(prot, ONE_INSTR, ONE_SLOTS), share_prefix="groups", retrieval=True)
    with pytest.raises(ValueError, match="compute_loss"):
        m.forward(_inputs(prot, ONE_INSTR, ONE_SLOTS), share_prefix="groups", compute_loss=True)
    with pytest.raises(ValueError, match="share_prefix="):
        m.forward(_inputs(prot, ONE_INSTR, ONE_SLOTS), share_prefix="group")


def _split(instr):
    head, tail = instr.split("[ANSWER]")
    return head + "[ANSWER]", tail.strip()


def test_every_shared_prefix_call_is_one_extension(env, prot):
    """The one-call-per-batch property of every driver over `LlamaEngine.extend`: the extension counters advance by ONE per call -- the packed
    one only when asked for, the grouped one only on the two grouped paths -- and `generate_lookahead` by one plain extension per pass.
    (Expected values read off the drivers: each makes exactly one `extend` call, the lookahead loop one pcy_llama_extend per pass.)  A second,
    identical call returns the same bits."""
    m = env["model"]
    eng = m.text_encoder.engine
    lib = eng.ctx.lib
    prompts = [_split(i)[0] for i in SC.INSTR]
    two = [i for i in range(len(MIX_INSTR)) if i != 2]                                           # 2 receptors x 3 rows, tails of 0 / 1 / 2 words
    qa = lambda instr, slots, **kw: m.forward(_inputs(prot, instr, slots), **kw)["outputs"].answer_logits
    cand = lambda n, lists, **kw: m.score_candidates(SC.make_inputs(env, instr=prompts[:n], slots=SC.SLOTS[:n]), lists, **kw)["token_nll"]
    #        name                         the call                                                                            grouped
    calls = [("forward(share_prefix=True)", lambda pk: qa(ONE_INSTR[:4], ONE_SLOTS[:4], share_prefix=True, packed=pk), 0),     # 4 rows, one receptor
             ("forward(share_prefix='groups')", lambda pk: qa([MIX_INSTR[i] for i in two], [MIX_SLOTS[i] for i in two], share_prefix="groups", packed=pk), 1),
             ("score_candidates", lambda pk: cand(2, [["yes", "w3 w4", "no w5 w6"], ["alpha", "beta gamma", "w7"]], packed=pk), 0),
             ("score_candidates(ragged)", lambda pk: cand(3, [["yes"], ["alpha", "w7 w8", "beta gamma delta"], ["q r", "w9"]], ragged=True, packed=pk), 1)]
    for name, call, grouped in calls:
        for packed in (False, True):
            e0, p0, g0 = _counts(lib)
            first = call(packed)
            assert _counts(lib) == (e0 + 1, p0 + int(packed), g0 + grouped), f"{name}, packed={packed}"
            assert torch.equal(call(packed), first), f"{name}, packed={packed}: a second call"
    emb, ids, *_ = m._preprocessing(_inputs(prot, [MIX_INSTR[0]], [MIX_SLOTS[0]]), aaseq_type="protein", crop_off=True, no_pad=True, left_pad=True)
    hist = ids[0].clone()
    hist[hist == m.prot_replacement_idx] = -1
    runs = []
    for _ in range(2):
        e0, p0, g0 = _counts(lib)
        tok, lp, lg, (_, _, look) = eng.generate_lookahead(emb, hist, 6, 4, keep_logits=True)
        passes = look.stats()["passes"]
        assert 2 <= passes <= 5                                                                  # 5 tokens behind the prefill's, 1 to 4 per pass
        assert _counts(lib) == (e0 + passes, p0, g0), "generate_lookahead: one plain extension per pass"
        runs.append((tok.cpu(), lp.cpu(), lg.cpu().clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_score_candidates_ragged_against_score_text(env, work):
    m = env["model"]
    lib = m.text_encoder.engine.ctx.lib
    prompts, tails = zip(*[_split(i) for i in SC.INSTR])
    long = "alpha beta gamma delta epsilon zeta eta theta iota"
    cands = [[tails[0]], [tails[1], "w7 w8", long], [tails[2], "w7 w8"]]                     # lists of 1 / 3 / 2
    e0, p0, g0 = _counts(lib)
    res = m.score_candidates(SC.make_inputs(env, instr=list(prompts)), cands, ragged=True)
    assert _counts(lib) == (e0 + 1, p0, g0 + 1)
    assert res["cache"].prefix.B == 3 and res["cache"].B == 6 and res["cache"].group_rows == [1, 3, 2]      # the prompts were prefilled ONCE each
    plan, S = res["plan"], res["plan"]["S"]
    assert len(set(plan["group_len"])) > 1 and plan["prefix_mask"].sum(1).tolist() == plan["group_len"]
    assert bool((plan["prefix_mask"][:, 0] == 1).all())                                      # right-aligned at position 0
    assert res["token_nll"].shape == (3, 3, S) and res["seq_nll"].shape == res["n_tokens"].shape == res["mean_nll"].shape == res["order"].shape == (3, 3)
    assert res["n_candidates"].tolist() == [1, 3, 2]
    real = torch.tensor([[True, False, False], [True, True, True], [True, True, False]])
    # score_text of the 6 concatenated rows
    rows = [p + " " + c for p, cs in zip(prompts, cands) for c in cs]
    slots = [s for s, cs in zip(SC.SLOTS, cands) for _ in cs]
    st = m.score_text(SC.make_inputs(env, instr=rows, slots=slots))
    n_ref = st["n_tokens"].cpu()
    assert torch.equal(res["n_tokens"].cpu()[real], n_ref)
    diff = (res["seq_nll"].cpu()[real] - st["seq_nll"].cpu()).abs()
    print(f"score_candidates(ragged) vs score_text: seq_nll diff {diff.max().item():.3e}, per token {(diff / n_ref).max().item():.3e} (bar {work['bar']:.3e})")
    record_parity("extend_groups/score_candidates_vs_score_text", seq_nll_diff=float(diff.max()), per_token=float((diff / n_ref).max()), bar=work["bar"])
    assert bool((diff <= work["bar"] * n_ref).all())
    # the padding: token_nll 0, n_tokens 0, seq_nll / mean_nll +inf, sorted last
    pad = ~real
    assert bool((res["token_nll"].cpu()[pad] == 0).all()) and bool((res["n_tokens"].cpu()[pad] == 0).all())
    assert bool((res["seq_nll"].cpu()[pad] == float("inf")).all()) and bool((res["mean_nll"].cpu()[pad] == float("inf")).all())
    assert torch.equal(res["mean_nll"].cpu()[real], (res["seq_nll"] / res["n_tokens"]).cpu()[real])
    assert torch.equal(res["order"], torch.argsort(res["mean_nll"], dim=1, stable=True))
    assert res["order"][0].tolist() == [0, 1, 2] and int(res["order"][2, 2]) == 2
    # packed: the same bits
    res_p = m.score_candidates(SC.make_inputs(env, instr=list(prompts)), cands, ragged=True, packed=True)
    for k in ("token_nll", "seq_nll", "mean_nll", "order", "n_tokens"):
        assert torch.equal(res_p[k], res[k]), k
    # the uniform planner keeps its refusal
    with pytest.raises(ValueError, match="same number of candidates"):
        m.score_candidates(SC.make_inputs(env, instr=list(prompts)), cands)
    with pytest.raises(ValueError, match="same number of candidates"):
        m.score_candidates(SC.make_inputs(env, instr=list(prompts)), cands, ragged=False)
