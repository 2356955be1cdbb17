"""CPU: the references of tests/glue_ref.py, which tests/test_gpu_glue_ops.py compares the bf16 glue kernels against, held to what the
project already trusts -- torch's own bf16 operators and the oracle -- on every input set the GPU test uses and at the GPU test's own
bars.  An input set on which two correct evaluations cannot meet the bar would fail here first."""
import pytest
import torch
import torch.nn.functional as F

import glue_ref as G
from conftest import assert_bf16_close
from oracle import esm_ref as ER
from oracle import llama_ref as LR
from oracle import procyon_ref as PR

BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("rows,d", G.NORM_SHAPES)
def test_layernorm_ref(rows, d):
    c = G.norm_case(rows, d, "ln")
    ref = G.layernorm(c["x"], c["w"], c["b"])
    assert_bf16_close(F.layer_norm(c["x"], (d,), c["w"], c["b"], G.EPS), ref, f"ln {rows}x{d}", max_frac=G.NORM_MAX_FRAC)
    if rows >= 4:
        assert torch.equal(G.bits(ref[G.ROW_ZERO]), G.bits(c["b"]))
        if d & (d - 1) == 0:
            assert bool((c["x"][G.ROW_CONST] == 1.5).all()) and torch.equal(G.bits(ref[G.ROW_CONST]), G.bits(c["b"]))


@pytest.mark.parametrize("rows,d", G.NORM_SHAPES + G.NORM_INPLACE)
def test_rmsnorm_ref(rows, d):
    c = G.norm_case(rows, d, "rms")
    assert G.settle_rms_ties(c["x"].clone()) == 0          # the case is settled: no intermediate within 2^-20 of a rounding boundary
    for cast, nm in ((0, "hf5"), (1, "hf431")):
        ref = G.rmsnorm(c["x"], c["w"], G.EPS, cast)
        assert_bf16_close(LR.rms_norm(c["x"], c["w"], G.EPS, nm), ref, f"rms {nm} {rows}x{d}", max_frac=G.NORM_MAX_FRAC)
        if rows >= 4:
            assert bool((ref[G.ROW_ZERO] == 0).all())
            assert bool((c["x"][G.ROW_SPIKE] == 64.0).sum() == 1)
            if d & (d - 1) == 0:
                assert bool((c["x"][G.ROW_CONST] == 1.5).all())
    if rows * d >= 64 * 1280:                                # the two casts are different operators on these inputs
        assert not torch.equal(G.rmsnorm(c["x"], c["w"], G.EPS, 0), G.rmsnorm(c["x"], c["w"], G.EPS, 1))


def test_tie_distance():
    y = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -30, -3.0 - 2.0 ** -7, 0.0, 0.75], dtype=torch.float64)
    t = G.tie_distance(y)
    assert float(t[0]) == pytest.approx(2.0 ** -8) and float(t[1]) == 0.0 and float(t[2]) == pytest.approx(2.0 ** -30, rel=1e-2)
    assert float(t[3]) == 0.0 and float(t[4]) == float("inf") and float(t[5]) == pytest.approx(2.0 ** -9 / 0.75)


# ------------------------------------------------------------------------------------------------ rotary
@pytest.mark.parametrize("nh,dh,ld,col0", G.ROPE_GEOMS)
@pytest.mark.parametrize("mode,scaled", G.ROPE_VARIANTS)
def test_rope_ref(nh, dh, ld, col0, mode, scaled):
    c = G.rope_case(nh, dh, ld, col0)
    cos, sin = G.rope_tables(dh)
    geom = LR.LlamaGeom(vocab=1, d=nh * dh, n_layers=1, n_heads=nh, n_kv_heads=nh, ffn=1)
    cos_o, sin_o = LR.rope_tables(geom, BF, G.ROPE_NPOS)
    assert torch.equal(cos, cos_o) and torch.equal(sin, sin_o)
    T, w = len(G.ROPE_POS), slice(col0, col0 + nh * dh)
    ref = G.rope(c["buf"], col0, nh, dh, c["pos"], cos, sin, mode, dh ** -0.5 if scaled else 0.0)
    x = c["buf"][:, w].reshape(T, nh, dh).transpose(0, 1)[None]
    ct, st = cos[c["pos"].long()], sin[c["pos"].long()]
    if mode == 0:
        orc, _ = LR.apply_rope(x, x, ct[None], st[None])
    else:
        orc, _ = ER.apply_rope(x * dh ** -0.5 if scaled else x, x, ct, st, "fp32_once")
    assert torch.equal(G.bits(orc[0].transpose(0, 1).reshape(T, nh * dh)), G.bits(ref[:, w]))
    keep = torch.ones(ld, dtype=torch.bool)
    keep[w] = False
    assert torch.equal(G.bits(ref[:, keep]), G.bits(c["buf"][:, keep]))
    assert not torch.equal(G.bits(ref[1:, w]), G.bits(c["buf"][1:, w]))
    if not scaled:                                            # position 0: cos 1, sin 0
        assert torch.equal(G.bits(ref[0]), G.bits(c["buf"][0]))


# ------------------------------------------------------------------------------------------------ pooler
def test_pool_layout():
    seg, rng, nrows = G.pool_layout()
    assert [sum(ln for _, ln in rng[seg[p]:seg[p + 1]]) for p in range(len(seg) - 1)] == [1, 2, 3, 4, 31, 32, 33, 34, 65, 130]
    assert sorted({seg[p + 1] - seg[p] for p in range(len(seg) - 1)}) == [1, 2, 3]
    starts = [st for st, _ in rng]
    assert starts != sorted(starts) and starts != sorted(starts, reverse=True)
    assert any(rng[seg[p]][1] == 1 and seg[p + 1] - seg[p] > 1 for p in range(10)) and any(rng[seg[p + 1] - 1][1] == 1 and seg[p + 1] - seg[p] > 1 for p in range(10))
    assert min(starts) >= 1 and max(st + ln for st, ln in rng) < nrows           # an unused row at both ends


@pytest.mark.parametrize("d", G.POOL_DIMS)
@pytest.mark.parametrize("mode,nan", [(0, False), (0, True), (1, False), (1, True), (2, False)])
def test_pool_ref(d, mode, nan):
    c = G.pool_case(d, nan)
    h, seg, rng = c["h"], c["seg"], c["rng"]
    ref = G.pool(h, seg, rng, mode)
    rows = [torch.cat([h[st:st + ln] for st, ln in rng[seg[p]:seg[p + 1]]]) for p in range(len(seg) - 1)]
    assert all(bool((r.float().abs() < 8).all() or nan) for r in rows)           # no row of POOL_GAP inside a range
    if mode == 2:
        orc = torch.stack([r.max(0)[0] for r in rows])
        assert torch.equal(G.bits(orc), G.bits(ref))
        return
    orc = torch.stack([(r[1:-1] if mode == 1 else r).nanmean(0) for r in rows])
    want_nan = torch.zeros(len(rows), d, dtype=torch.bool)
    if mode == 1:
        want_nan[:2] = True                                  # one and two tokens: nothing between the ends
    if nan:
        want_nan[G.POOL_NAN_PROTEIN, d - 1] = True
    assert torch.equal(ref.isnan(), want_nan) and torch.equal(orc.isnan(), want_nan)
    assert_bf16_close(orc[~want_nan], ref[~want_nan], f"pool {d} mode {mode} nan {nan}", max_frac=G.POOL_MAX_FRAC)
    if mode == 1:
        assert torch.equal(G.bits(ref[2]), G.bits(rows[2][1]))
    if nan:
        assert int(h.isnan().sum()) > d // 8 + 33


# ------------------------------------------------------------------------------------------------ splice
@pytest.mark.parametrize("d", G.SPLICE_DIMS)
@pytest.mark.parametrize("which", G.SPLICE_MAPS)
def test_splice_ref(d, which):
    c = G.splice_case(d, which)
    table, soft, ids, sm = c["table"], c["soft"], c["ids"], c["soft_map"]
    both = torch.cat((table, soft))
    assert bool(both.float().isfinite().all())
    assert all(len(set(G.bits(row).tolist())) == d for row in both[::9])                 # distinct along a row
    assert all(len(set(G.bits(both)[:, k].tolist())) == both.shape[0] for k in (0, d // 2, d - 1))      # and down a column
    assert {0, G.SPLICE_VOCAB - 1} <= set(ids.tolist()) and len(set(ids.tolist())) < ids.numel()
    ref = G.splice(table, ids, soft, sm)
    # the oracle splices soft rows in order at the rows that hold a placeholder id: give it the placeholder and the rows in map order
    ph = G.SPLICE_VOCAB
    m = torch.zeros(ids.numel(), dtype=torch.bool) if sm is None else sm >= 0
    ids_o = torch.where(m, torch.full_like(ids, ph), ids).long()[None]
    orc, _ = PR.prepare_input_embeddings(torch.cat((table, torch.zeros(1, d, dtype=BF))), ids_o, ph, soft[sm[m].long()] if bool(m.any()) else None)
    assert torch.equal(G.bits(orc[0]), G.bits(ref))
    assert int(m.sum()) == {"null": 0, "none_soft": 0, "mixed": 18, "all_soft": G.SPLICE_ROWS}[which]
