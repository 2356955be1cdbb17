"""ProCyon-Split's decoder (Llama-2-7B geometry: 32 heads = 32 kv heads, ffn 11008, vocabulary 32007) at FULL DEPTH in bf16 against the CPU
oracle and an fp32 evaluation of the same weights -- what tests/test_gpu_fulldepth.py does for ProCyon-Full's decoder, at the same bars:

    per step (and row)   err(HIP, fp32) <= 1.25 x err(oracle_bf16, fp32)
    argmax               HIP == oracle == fp32 on every step whose fp32 top-2 margin clears 4 x the bf16 logit noise
    gross-error guard    err(HIP, oracle_bf16) < 0.15 per (row, step)

Fixtures (tests/golden/make_fulldepth.py split1 split_rows20): s1_llama2_7b_T{128,704}_N128 -- one row, 128 teacher-forced cached steps, the
T = 704 run growing its cache 704 -> 832 across the decode attention's 768-key split; s2_llama2_7b_rows20_T64 -- twenty ragged left-padded rows
in the reference's compat mode (mask in the prefill only, positions arange(T), every cached slot attended afterwards), 16 cached steps.  The
number of clear-margin steps is a property of the fixture alone (25 of 129 in each one-row file; 8 / 11 / 14 / 40 / 80 pairs in the first
2 / 3 / 4 / 10 / 20 rows) and every test asserts a minimum of it.

Every test also asserts WHICH decode step served it (fulldepth_common.served_by, the PCY_DISPATCH_DEC_* counters): the one-launch multi-head
step may decline at launch time and the launches then compute the same bits, so without the counters the oracle result would not say which of
the two it holds for.  All steps here are eager (a replayed graph does not pass through the counters)."""
import pytest
import torch

from conftest import pcy_disable, record_parity, rel_err
from fulldepth_common import SLACK, llama_stats, llama_steps, margin_conditioned, rows_compat_check, rows_compat_run, served_by

pytestmark = pytest.mark.gpu
SPLIT = dict(vocab=32007, d=4096, n_layers=32, n_heads=32, n_kv_heads=32, ffn=11008)
NDEC = 128     # cached steps of the one-row fixtures


@pytest.fixture(scope="module")
def split():
    """Llama-2-7B geometry on the CPU-seeded weights of the fixtures"""
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig, LlamaEngine
    return LlamaEngine(synth.llama_state_dict(**SPLIT, workers=16), LlamaConfig(**SPLIT, max_pos=4096), free_source=True)


_DEFAULT_RUN = {}


def _default_run(split, golden, monkeypatch, T):
    """the one-row run at default switches (once per module): logits [129, V], prefill hidden row; every cached step on the multi-head
    one-launch step"""
    if T not in _DEFAULT_RUN:
        pcy_disable(monkeypatch)
        monkeypatch.delenv("PCY_AO_XMIN", raising=False)
        g = golden(f"s1_llama2_7b_T{T}_N{NDEC}")
        with served_by("step_mha", steps=NDEC) as delta:
            got, hid = llama_steps(split, g, T, SPLIT["vocab"])
        _DEFAULT_RUN[T] = (got, hid, dict(delta))
    return _DEFAULT_RUN[T]


@pytest.mark.parametrize("T", [128, 704])
def test_llama2_7b_full_depth_one_row_128_steps(split, golden, monkeypatch, T):
    """One row, prefill + 128 teacher-forced cached steps at default switches (decode_step_mha_kernel: all 32 layers in one launch; T = 704
    crosses the key split at 768 cached keys in the middle of the run).  Per step the truth-distance bar, argmax on EVERY clear-margin step (at
    least 16 of them), agreement rates as test_llama8b_full_depth_256_steps (2 of 65 scaled to 129: 4), the prefill's final-normed hidden row;
    every cached step served by the multi-head one-launch step, none by a fallback."""
    g = golden(f"s1_llama2_7b_T{T}_N{NDEC}")
    got, h_hip, delta = _default_run(split, golden, monkeypatch, T)
    st = llama_stats(got, g)
    nstep = st["nstep"]
    mean = lambda v: sum(v) / len(v)
    clear, ao, at = margin_conditioned(st, g)
    worst = max(a / b for a, b in zip(st["e_hip_truth"], st["e_ref_truth"]))
    e_hid, e_hid_ref = rel_err(h_hip, g["hidden_fp32"][0]), rel_err(g["hidden_bf16"][0].float(), g["hidden_fp32"][0])
    for s in range(nstep):
        if s < 4 or s % 16 == 0 or st["rows"][s][0] != st["rows"][s][1]:
            print(f"T={T} step {s}: err(HIP,fp32) {st['e_hip_truth'][s]:.3e}  err(oracle_bf16,fp32) {st['e_ref_truth'][s]:.3e}  err(HIP,oracle_bf16) "
                  f"{st['e_hip_ref'][s]:.3e}  argmax HIP {st['rows'][s][0]} / fp32 {st['rows'][s][1]} / oracle {st['rows'][s][2]}  fp32 top-2 margin {st['rows'][s][3]:.3e}")
    print(f"T={T} prefill hidden row: err(HIP,fp32) {e_hid:.3e}  err(oracle_bf16,fp32) {e_hid_ref:.3e}; clear-margin steps {clear} (HIP == oracle on {ao}, "
          f"== fp32 on {at}); worst ratio {worst:.3f}; decode steps served by {delta}")
    record_parity(f"fulldepth/llama2_7b_random_init_T{T}_128_steps", steps=nstep, err_hip_fp32_mean=mean(st["e_hip_truth"]), err_oracle_fp32_mean=mean(st["e_ref_truth"]),
                  err_hip_oracle_mean=mean(st["e_hip_ref"]), err_hip_oracle_max=max(st["e_hip_ref"]), worst_ratio_hip_over_oracle=worst,
                  agree_hip_fp32=st["agree_hip_truth"], agree_oracle_fp32=st["agree_ref_truth"], agree_hip_oracle=st["agree_hip_ref"],
                  clear_margin_steps=clear, clear_agree_hip_oracle=ao, clear_agree_hip_fp32=at, hidden_err_hip_fp32=e_hid, hidden_err_oracle_fp32=e_hid_ref,
                  steps_on_decode_step_mha=delta["step_mha"])
    assert nstep == NDEC + 1
    for s in range(nstep):
        assert st["e_hip_truth"][s] <= SLACK * st["e_ref_truth"][s], (s, st["e_hip_truth"][s], st["e_ref_truth"][s])
    assert clear >= 16, clear
    assert ao == clear and at == clear, (clear, ao, at)
    assert st["agree_hip_truth"] >= st["agree_ref_truth"] - 4 and st["agree_hip_ref"] >= st["agree_ref_truth"] - 4   # (2 of 65 scaled to 129)
    assert max(st["e_hip_ref"]) < 0.15        # a wrong position / a dropped key range gives O(1)
    assert e_hid <= SLACK * e_hid_ref


@pytest.mark.parametrize("off,kind", [("decode_step", "layer"), ("decode_step,decode_layer", "loop_stream")])
def test_llama2_7b_full_depth_twins_bit_identical_across_the_key_split(split, golden, monkeypatch, off, kind):
    """The T = 704 run again with the one-launch step switched off -- PCY_DISABLE=decode_step: one launch per layer (decode_layer_mha_kernel);
    decode_step,decode_layer: launch by launch -- the logits of all 129 positions BIT-identical to the default run's, at 32 layers and across
    the 768-key split (so far shown at 2 layers).  This is what carries the oracle result of the default run over to the twins; the counters
    say that each side ran what it names."""
    T = 704
    g = golden(f"s1_llama2_7b_T{T}_N{NDEC}")
    ref, _, _ = _default_run(split, golden, monkeypatch, T)
    pcy_disable(monkeypatch, *off.split(","))
    with served_by(kind, steps=NDEC) as delta:
        got, _ = llama_steps(split, g, T, SPLIT["vocab"])
    differ = [s for s in range(ref.shape[0]) if not torch.equal(got[s], ref[s])]
    record_parity(f"fulldepth/llama2_7b_T704_twin_{kind}", steps=ref.shape[0], positions_not_bit_identical=len(differ), **{f"steps_on_{kind}": delta[kind]})
    assert not differ, (off, differ[:8])


@pytest.mark.parametrize("nrows,kind", [(2, "loop_stream"), (3, "loop_stream"), (4, "loop_mfma"), (10, "loop_mfma"), (20, "loop_mfma")])
def test_llama2_7b_full_depth_ragged_rows_compat_mode(split, golden, monkeypatch, nrows, kind):
    """Fixture s2: twenty ragged left-padded rows (0 .. 27 pad slots of 64) in the reference's compat mode, 16 teacher-forced cached steps, as
    batches of the first 2 / 3 rows (streaming GEMVs, below pcy_mfma_min_batch()), 4 (the first batch on the skinny-MFMA GEMVs, K = 11008 =
    86 x 128), 10 and 20 rows (the beam sizes of the reference's callers).  Per (row, step) the truth-distance bar, argmax on every clear-margin
    (row, step) -- at least `nrows` of them --, agreement rates, the gross-error guard; the counters say which GEMV family served the batch."""
    pcy_disable(monkeypatch)
    monkeypatch.delenv("PCY_MB_MAX", raising=False)
    g = golden("s2_llama2_7b_rows20_T64")
    ids, mask, toks = g["ids"].long()[:nrows], g["mask"].float()[:nrows], g["tokens"].long()[:, :nrows]
    with served_by(kind, steps=toks.shape[0] - 1) as delta:
        got = rows_compat_run(split, ids, mask, toks, nrows, list(range(nrows)), SPLIT["vocab"])
    rows_compat_check(f"fulldepth/llama2_7b_ragged_rows_compat_B{nrows}", got, g, list(range(nrows)), min_clear=nrows, **{f"steps_on_{kind}": delta[kind]})


# the s2 rows tiled into batches of more than 32 rows: row i holds s2 row (i - s) % 20, so rows [s, s + 20) -- the copies held to the oracle --
# straddle the 31 / 32 boundary (40 = 2 prompts x beam 20: s2 rows 14 .. 19 of the checked copies sit in the 8-row remainder pass)
_OVER_32 = {40: 18, 160: 23}


@pytest.mark.parametrize("B", sorted(_OVER_32))
def test_llama2_7b_full_depth_rows_over_32(split, golden, monkeypatch, B):
    """Decode steps above 32 rows at full depth: s2's twenty rows tiled into a B-row batch, every row teacher-forced with its s2 row's tokens.
    The copies in rows [s, s + 20) against the bf16 oracle and the fp32 truth at the bars of the 20-row test; every other copy of an s2 row --
    in another 32-row pass or in the remainder pass -- BIT-identical to the first one (logits of every step, the whole K / V cache)."""
    pcy_disable(monkeypatch)
    g = golden("s2_llama2_7b_rows20_T64")
    s = _OVER_32[B]
    perm = [(i - s) % 20 for i in range(B)]
    first = {}
    copy_of = [first.setdefault(p, i) for i, p in enumerate(perm)]
    ids, mask, toks = g["ids"].long()[perm], g["mask"].float()[perm], g["tokens"].long()[:, perm]
    rows = list(range(s, s + 20))
    with served_by("loop_mfma", steps=toks.shape[0] - 1) as delta:
        got = rows_compat_run(split, ids, mask, toks, B, list(range(B)), SPLIT["vocab"], keep_rows=rows, copy_of=copy_of)
    rows_compat_check(f"fulldepth/llama2_7b_rows_over_32_B{B}", got, g, [perm[i] for i in rows], min_clear=20, steps_on_loop_mfma=delta["loop_mfma"])
