"""GPU: the fused lm_head x cross-entropy operator (pcy_lm_head_xent, procyon_amd/csrc/pcy_xent.hip) against `Context.gemm` logits.

The rounded logit of every (m, n) must be the bits pcy_gemm stores, so `label_logit` and `row_max` -- both free of any summation order --
are compared EXACTLY; `lse` / `nll` are compared with a float64 logsumexp / gather on those same logits under the bar

    8 x max( (a) the error of torch's own fp32 cross_entropy / logsumexp against that float64 value, on the CPU, same logits,
             (b) one fp32 ulp at max(|lse|, |row_max|) )

(8: two fp32 summation trees carry independent errors of the same size).  Three planted weight sets at d = 256 make the faults a row
reduction over a ragged vocabulary can have visible (measured on the CPU at M = 257, V = 128 263: dropping the 7 tail columns moves the
peaked LSE by 3.9, including 121 zero pad columns moves the negative LSE by 13.4; on random data the same faults move it by 4e-5 / 6e-4):
  random    logits ~ N(0, 1)
  negative  every logit in [-22, -18]: a zero from a padded column would dominate
  peaked    logits of 85-92 planted at the tile edges and in the ragged tail: exp overflows without the max, a dropped tail shows
V = 128 263 = 1002 x 128 + 7 and 2 311 = 18 x 128 + 7: the last column tile holds 7 columns."""
import math

import pytest
import torch

from conftest import record_parity

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
D = 256
MS = [1, 63, 64, 65, 129, 257]
VS = [128263, 2311]
SETS = ["random", "negative", "peaked"]
_CACHE = {}


def _planted_targets(V):
    return [0, 127, 128, 255, 256, V - 8, V - 7, V - 1]


def _make(V, kind):
    g = torch.Generator().manual_seed(1000 + V % 977 + SETS.index(kind))
    M = 257
    x0 = torch.randn(D, generator=g)
    x = (x0[None] + 0.1 * torch.randn(M, D, generator=g)).to(BF)
    n2 = float(x0.pow(2).sum())
    if kind == "random":
        W = torch.randn(V, D, generator=g) / 16
    elif kind == "negative":
        W = -(20 / n2) * x0[None] + 0.02 * torch.randn(V, D, generator=g)
    else:
        W = torch.randn(V, D, generator=g) / 16
        W[V - 1] = (90 / n2) * x0
        W[V - 7] = (88 / n2) * x0
        for k in (127, 128, 255, 256, 128255, 128256):
            if k < V - 7:
                W[k] = (85 / n2) * x0
    tg = torch.randint(0, V, (M,), generator=g)
    tg[:8] = torch.tensor(_planted_targets(V))
    return x, W.to(BF), tg


def _ulp32(v):
    """one fp32 ulp at |v| (float64 tensor in, float64 out)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 23)


def _reference(G):
    """G [M, V] bf16 logits (device) -> float64 lse / row max on the host + bar term (a): torch's own fp32 error on these logits"""
    lg = G.cpu()
    l64 = torch.logsumexp(lg.double(), -1)
    l32 = torch.logsumexp(lg.float(), -1).double()
    return lg, l64, float((l32 - l64).abs().max())


def _case(V, kind):
    """per (V, set), once: inputs on the device, the M = 257 `Context.gemm` logits, their float64 reference and bar term (a)"""
    key = (V, kind)
    if key not in _CACHE:
        from procyon_amd.engine import Context
        ctx = Context.get()
        x, W, tg = _make(V, kind)
        xd, Wd, tgd = x.cuda(), W.cuda(), tg.cuda()
        G = ctx.gemm(xd, Wd)
        lg, l64, err_lse = _reference(G)
        lab64 = lg.double().gather(1, tg[:, None])[:, 0]
        nll64 = l64 - lab64
        ce32 = torch.nn.functional.cross_entropy(lg.float(), tg, reduction="none").double()
        err_a = max(err_lse, float((ce32 - nll64).abs().max()))
        rmax = lg.float().max(-1).values.double()
        _CACHE[key] = dict(ctx=ctx, x=xd, W=Wd, tg=tgd, G=G, l64=l64, nll64=nll64, rmax=rmax, err_a=err_a)
    return _CACHE[key]


def _check_against_gemm(c, M, nll, lse, row_max, label, key):
    """the assertions of the header for rows [0, M) of case c"""
    G = c["ctx"].gemm(c["x"][:M].contiguous(), c["W"])
    assert torch.equal(G, c["G"][:M]), "Context.gemm is not row-invariant here: the shared reference does not apply"
    tg = c["tg"][:M]
    assert torch.equal(label, G.float().gather(1, tg[:, None].long())[:, 0]), "label_logit is not the bits Context.gemm stores"
    assert torch.equal(row_max, G.float().max(-1).values), "row_max is not the max of the Context.gemm row"
    l64, nll64, rmax = c["l64"][:M], c["nll64"][:M], c["rmax"][:M]
    ulp = _ulp32(torch.maximum(l64.abs(), rmax.abs()))
    bar = 8 * torch.clamp(ulp, min=c["err_a"])
    e_lse, e_nll = (lse.cpu().double() - l64).abs(), (nll.cpu().double() - nll64).abs()
    print(f"{key}: lse err {float(e_lse.max()):.3e} nll err {float(e_nll.max()):.3e} torch-fp32 err {c['err_a']:.3e} "
          f"ulp {float(ulp.max()):.3e} bar {float(bar.min()):.3e}")
    record_parity(key, lse_err=float(e_lse.max()), nll_err=float(e_nll.max()), torch_fp32_err=c["err_a"], ulp=float(ulp.max()),
                  bar=float(bar.min()))
    assert bool((e_lse <= bar).all()) and bool((e_nll <= bar).all()), (key, float(e_lse.max()), float(e_nll.max()), float(bar.min()))


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("V", VS)
@pytest.mark.parametrize("M", MS)
def test_xent_matches_gemm_logits(M, V, kind):
    from procyon_amd import _lib
    c = _case(V, kind)
    ctx = c["ctx"]
    n0 = ctx.lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT)
    nll, lse, row_max, label = ctx.lm_head_xent(c["x"][:M].contiguous(), c["W"], c["tg"][:M], want_parts=True)
    assert ctx.lib.pcy_debug_dispatch_count(_lib.DISPATCH_XENT) == n0 + 1
    assert nll.dtype == torch.float32 and nll.shape == (M,)
    _check_against_gemm(c, M, nll, lse, row_max, label, f"score/xent_{kind}_V{V}_M{M}")
    # nll alone (no optional outputs) and a second call: the same bits
    assert torch.equal(ctx.lm_head_xent(c["x"][:M].contiguous(), c["W"], c["tg"][:M]), nll)
    again = ctx.lm_head_xent(c["x"][:M].contiguous(), c["W"], c["tg"][:M], want_parts=True)
    assert all(torch.equal(a, b) for a, b in zip(again, (nll, lse, row_max, label)))


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("V", VS)
def test_xent_row_invariance(V, kind):
    """a row's nll / lse / label_logit bits depend neither on M nor on which other rows are scored"""
    c = _case(V, kind)
    ctx, x, W, tg = c["ctx"], c["x"], c["W"], c["tg"]
    whole = ctx.lm_head_xent(x, W, tg, want_parts=True)
    a = ctx.lm_head_xent(x[:65].contiguous(), W, tg[:65], want_parts=True)
    b = ctx.lm_head_xent(x[65:].contiguous(), W, tg[65:], want_parts=True)
    for i in (0, 1, 3):      # nll, lse, label_logit
        assert torch.equal(torch.cat([a[i], b[i]]), whole[i]), i
    for r in (0, 5, 7, 64, 65, 128, 200, 256):
        one = ctx.lm_head_xent(x[r:r + 1].contiguous(), W, tg[r:r + 1], want_parts=True)
        for i in (0, 1, 3):
            assert torch.equal(one[i], whole[i][r:r + 1]), (r, i)


def test_xent_edge_arguments():
    from procyon_amd._lib import PcyError
    c = _case(2311, "random")
    ctx, x, W, tg = c["ctx"], c["x"], c["W"], c["tg"]
    assert ctx.lm_head_xent(x[:0].contiguous(), W, tg[:0]).shape == (0,)          # M == 0: nothing to do
    bad = tg[:4].clone()
    bad[1], bad[2] = 2311, -1                                                     # no such column: NaN, the other rows untouched
    nll = ctx.lm_head_xent(x[:4].contiguous(), W, bad)
    good = ctx.lm_head_xent(x[:4].contiguous(), W, tg[:4])
    assert math.isnan(float(nll[1])) and math.isnan(float(nll[2])) and torch.equal(nll[[0, 3]], good[[0, 3]])
    with pytest.raises(PcyError):
        ctx.lm_head_xent(x[:4, :160].contiguous(), W[:, :160].contiguous(), tg[:4])   # d % 64 != 0


def test_xent_full_width_lm_head():
    """the lm_head of the full geometry (V = 128 263, d = 4096) once, M = 130 random normed rows, the same two bars"""
    from procyon_amd import synthetic_model as SM
    from procyon_amd.engine import Context
    model = SM.build("full", llama_layers=1, esm_layers=1)
    eng = model.text_encoder.engine
    W = eng.lm_head
    V, d = W.shape
    assert (V, d) == (128263, 4096)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(130, d, generator=g)
    x = (x / x.pow(2).mean(-1, keepdim=True).sqrt()).to(BF).cuda()
    tg = torch.randint(0, V, (130,), generator=g)
    tg[:8] = torch.tensor(_planted_targets(V))
    ctx = Context.get()
    G = ctx.gemm(x, W)
    lg, l64, err_lse = _reference(G)
    nll64 = l64 - lg.double().gather(1, tg[:, None])[:, 0]
    ce32 = torch.nn.functional.cross_entropy(lg.float(), tg, reduction="none").double()
    c = dict(ctx=ctx, x=x, W=W, tg=tg.cuda(), G=G, l64=l64, nll64=nll64, rmax=lg.float().max(-1).values.double(),
             err_a=max(err_lse, float((ce32 - nll64).abs().max())))
    nll, lse, row_max, label = ctx.lm_head_xent(x, W, c["tg"], want_parts=True)
    _check_against_gemm(c, 130, nll, lse, row_max, label, "score/xent_full_lm_head_M130")
