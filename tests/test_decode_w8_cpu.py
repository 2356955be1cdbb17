"""Host side of the cached decode that streams e4m3 weights (pcy_gemv_w8, pcy_llama_decode_w8, pcy_llama_greedy_w8): the four
symbols are declared, exported and bound; the counter reads 0 with nothing run; the option's defaults and generate()'s refusals; and the
property the GPU tests' design rests on -- per-row e4m3 quantisation with a power-of-two scale is value-idempotent and its dequantised values are
bf16 numbers, so a model whose bf16 projection weights were first put on the e4m3 grid IS its own weight-only fp8 model.  No GPU."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcy_gemv_w8", "pcy_llama_decode_w8", "pcy_llama_greedy_w8", "pcy_debug_decode_w8_count")


def test_new_symbols_declared_exported_and_bound():
    from procyon_amd import _lib
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "pcy.h")).read())
    assert ("int pcy_gemv_w8(pcy_ctx*, const void* W8, const float* scale, const void* x, int ldx, const void* resid, void* y, int ldy, "
            "const void* rms_w, float rms_eps, int rms_cast, int N, int K, int B, int epi);") in header
    assert ("int pcy_llama_decode_w8(pcy_ctx*, const pcy_llama_desc*, const pcy_llama_layer_fp8* w8, const pcy_kv_cache*, const pcy_gen_state*, "
            "int B);") in header
    assert ("int pcy_llama_greedy_w8(pcy_ctx*, const pcy_llama_desc*, const pcy_llama_layer_fp8* w8, const pcy_kv_cache*, const pcy_gen_state*, "
            "int B, int n_steps, int use_graph);") in header
    assert "unsigned long long pcy_debug_decode_w8_count(void);" in header
    for name in NEW:
        assert name in _lib.SIGNATURES
    # pcy_llama_decode's / pcy_llama_greedy's arguments with the e4m3 layers behind the descriptor
    for new, old in (("pcy_llama_decode_w8", "pcy_llama_decode"), ("pcy_llama_greedy_w8", "pcy_llama_greedy")):
        res, args = _lib.SIGNATURES[old]
        assert _lib.SIGNATURES[new] == (res, args[:2] + [ctypes.POINTER(_lib.LlamaLayerFp8)] + args[2:])
    assert _lib.SIGNATURES["pcy_debug_decode_w8_count"] == (ctypes.c_ulonglong, [])
    assert len(_lib.SIGNATURES["pcy_gemv_w8"][1]) == 15
    lib = _lib.load()                                                                           # (raises on a symbol that is not exported)
    for name in NEW:
        assert getattr(lib, name) is not None
    # additions only: the ABI number, the dispatch kinds and the decode kinds stay where the suite pins them
    assert _lib.ABI_VERSION == 13 and "#define PCY_ABI_VERSION 13 " in header and lib.pcy_abi_version() == 13
    assert len([k for k in vars(_lib) if k.startswith("DISPATCH_") and isinstance(getattr(_lib, k), int)]) == 20 and len(_lib.DISPATCH_DECODE) == 7


def test_counter_reads_zero_with_nothing_run():
    """in a process of its own: other tests of this session may have run the step"""
    import subprocess
    import sys
    code = "from procyon_amd import _lib; print(int(_lib.load().pcy_debug_decode_w8_count()))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == "0"


def _bare_model(dtype):
    """a UnifiedProCyon with nothing but the dtype its caller asked for: generate() decides its refusals before it touches the inputs"""
    from procyon_amd.model.model_unified import UnifiedProCyon
    m = UnifiedProCyon.__new__(UnifiedProCyon)
    m.dtype = dtype
    return m


def test_option_defaults_to_false_and_engine_refusals():
    from procyon_amd.engine import LlamaEngine
    from procyon_amd.model.model_unified import UnifiedProCyon
    for fn in (LlamaEngine.generate_greedy, LlamaEngine.generate_sampling, UnifiedProCyon.generate):
        assert inspect.signature(fn).parameters["decode_w8"].default is False, fn
    assert callable(LlamaEngine.decode_w8) and callable(LlamaEngine.greedy_steps_w8) and callable(LlamaEngine._ensure_fp8_copies)
    use = LlamaEngine._use_decode_w8
    assert use(False, 40) is False and use(True, 1) is True and use(True, 8) is True
    with pytest.raises(ValueError, match="1..8 rows"):
        use(True, 9)
    for bad in ("auto", 1, None):
        with pytest.raises(ValueError, match="decode_w8"):
            use(bad, 1)
    for gemm in (True, "auto"):
        with pytest.raises(ValueError, match="decode_gemm"):
            use(True, 4, gemm)


def test_generate_refusals_on_a_bare_model():
    m = _bare_model(torch.bfloat16)
    with pytest.raises(ValueError, match="lookahead"):
        m.generate({}, method="greedy", lookahead=4, decode_w8=True)
    for gemm in (True, "auto"):
        with pytest.raises(ValueError, match="decode_gemm"):
            m.generate({}, method="greedy", decode_gemm=gemm, decode_w8=True)
    with pytest.raises(ValueError, match="beam"):
        m.generate({}, method="beam", decode_w8=True)
    with pytest.raises(ValueError, match="1..8 rows"):
        m.generate({"instructions": ["w1 [ANSWER]"] * 9}, method="greedy", decode_w8=True)
    for bad in ("auto", 1, None, "yes"):
        with pytest.raises(ValueError, match="decode_w8"):
            m.generate({}, method="greedy", decode_w8=bad)
    with pytest.raises(NotImplementedError, match="bf16"):
        _bare_model(torch.float32).generate({}, method="greedy", decode_w8=True)


def _matrices():
    """20 random matrices whose rows spread over six decades, then the edge rows: all zero, at the 2^-126 scale floor, and a row whose maximum
    rounds DOWN to 224 so that requantising halves its scale"""
    g = torch.Generator().manual_seed(8)
    out = []
    for i in range(20):
        rows, K = 24 + i, 64 + 16 * (i % 5)
        mag = 10.0 ** (torch.rand(rows, 1, generator=g) * 6 - 4)
        out.append((torch.randn(rows, K, generator=g) * mag).to(torch.bfloat16))
    edge = torch.zeros(4, 64)
    edge[1] = torch.randn(64, generator=g) * 2.0 ** -130                 # amax / 2^-126 far below 448: the scale sits on its floor
    edge[2] = torch.randn(64, generator=g).clamp(-1, 1) * 100.0
    edge[2, 0] = 231.0                                                   # scale 1: 231 lies between the codes 224 and 240 and rounds to 224,
    edge[3] = torch.randn(64, generator=g).clamp(-1, 1)                  # so the dequantised row has amax 224 and requantises at scale 0.5
    edge[3, 5] = 1.0
    out.append(edge.to(torch.bfloat16))
    return out


def test_quantisation_is_value_idempotent_and_bf16_exact():
    from oracle import fp8_ref as FR
    halved = 0
    for w in _matrices():
        q, s = FR.quant_rows(w)
        deq = FR.dequant(q, s)
        assert torch.isfinite(deq).all()
        assert torch.equal(deq.to(torch.bfloat16).float(), deq), "dequant(quant_rows(w)) must be representable in bf16"
        q2, s2 = FR.quant_rows(deq.to(torch.bfloat16))
        assert torch.equal(FR.dequant(q2, s2), deq), "quantising the dequantised matrix must give the same VALUES"
        halved += int((s2 < s).sum())
        zero = w.float().abs().amax(-1) == 0
        assert torch.equal(s[zero], torch.ones(int(zero.sum()))) and not bool(deq[zero].any())
    assert halved >= 1, "the row that rounds down to 224 must change its scale (codes and scales may change, values may not)"
