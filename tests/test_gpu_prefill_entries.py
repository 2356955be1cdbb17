"""GPU: pcy_llama_prefill and pcy_llama_prefill_all are one request in two shapes -- the last hidden state, the logits and the sum over the
L + 1 hidden states agree between them, on the bf16 path and on the fp8 path (the per-layer tail behind the fp8 projections: acc_rows and
the hidden_all copy together, which no other test asks for at once)."""
import pytest
import torch

from conftest import assert_bf16_close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
KW = dict(vocab=128263 - 128000 + 2048, d=256, n_layers=2, n_heads=4, n_kv_heads=2, ffn=512)   # the "small" synthetic geometry
B, T = 2, 12
SUM_ROWS = [3, 17]


@pytest.fixture(scope="module")
def eng():
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    e = LlamaEngine(synth.llama_state_dict(**KW), LlamaConfig(**KW, max_pos=64))
    e.quantize_fp8()
    e.set_fp8(False)
    return e


@pytest.mark.parametrize("fp8", [True, False])
def test_prefill_and_prefill_all_agree(eng, fp8):
    torch.manual_seed(11)
    emb = (torch.randn(B, T, KW["d"]) * 0.02).to(BF).cuda()
    mask = torch.ones(B, T)
    mask[1, :4] = 0
    rows = torch.arange(B * T, dtype=torch.int32)                          # 24 rows: both entries take the GEMV tail (<= 64)
    try:
        eng.set_fp8(fp8)
        c1, c2 = eng.new_cache(B, T), eng.new_cache(B, T)
        logits, hidden, hsum = eng.prefill(emb, mask, c1, rows, want_hidden=True, sum_rows=torch.tensor(SUM_ROWS, dtype=torch.int32))
        logits_all, hall = eng.prefill_all(emb, mask, c2, rows)
    finally:
        eng.set_fp8(False)
    assert hall.shape == (KW["n_layers"] + 1, B, T, KW["d"]) and hsum.shape == (len(SUM_ROWS), KW["d"])
    assert torch.equal(hidden, hall[-1]), "last hidden state"
    assert torch.equal(logits, logits_all), "logits of the same rows"
    assert torch.equal(c1.k, c2.k) and torch.equal(c1.v, c2.v)
    # the sum over all L + 1 states: fp32, in layer order, rounded once
    acc = torch.zeros(len(SUM_ROWS), KW["d"], dtype=torch.float32, device=hall.device)
    for l in range(KW["n_layers"] + 1):
        acc += hall[l].view(B * T, -1)[SUM_ROWS].float()
    assert_bf16_close(hsum.cpu(), acc.to(BF).cpu(), "hidden_sum", ulps=1)
    assert bool(hsum.float().abs().max() > 0)
    if fp8:   # ... and the fp8 projections really ran
        _, hidden16 = eng.prefill(emb, mask, eng.new_cache(B, T), None, want_hidden=True)
        assert not torch.equal(hidden, hidden16)


def test_logit_rows_spec_is_refused_by_name(eng):
    """prefill refuses "all" (prefill_all and extend take it); an unknown string names the accepted forms"""
    emb = torch.zeros(B, T, KW["d"], dtype=BF, device="cuda")
    with pytest.raises(ValueError, match=r'logit_rows=\'all\': expected "last", None'):
        eng.prefill(emb, None, eng.new_cache(B, T), "all")
    with pytest.raises(ValueError, match=r'logit_rows=\'first\': expected "all", "last", None'):
        eng.extend(eng.new_cache(B, 2 * T), emb, T, logit_rows="first")
