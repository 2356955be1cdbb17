"""Host side of the many-queries decode attention on shared-prefix caches (pcy_attn_decode_shared / pcy_llama_decode_gemm_mq):
the three symbols are declared, exported and bound; the counter reads 0 with nothing run; `shared_attn` exists with default False on every
driver; generate()'s refusals; the caption plugin forwards the key.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcy_attn_decode_shared", "pcy_llama_decode_gemm_mq", "pcy_debug_attn_mq_count")


def test_new_symbols_declared_exported_and_bound():
    from procyon_amd import _lib
    header = open(os.path.join(ROOT, "include", "pcy.h")).read()
    assert re.search(r"\bint\s+pcy_attn_decode_shared\s*\(\s*pcy_ctx\*\s*,\s*void\* qkv\s*,\s*int ld\s*,\s*const pcy_kv_cache\* kv\s*,\s*int layer\s*,\s*void\* o\s*,"
                     r"\s*int ldo\s*,\s*const int32_t\* pos\s*,\s*const void\* cos_t\s*,\s*const void\* sin_t\s*,\s*const uint8_t\* keep\s*,\s*int B\s*,\s*int H\s*,"
                     r"\s*int Hkv\s*,\s*int dh\s*\)\s*;", header)
    assert re.search(r"\bint\s+pcy_llama_decode_gemm_mq\s*\(\s*pcy_ctx\*\s*,\s*const pcy_llama_desc\*\s*,\s*const pcy_kv_cache\*\s*,\s*const pcy_gen_state\*\s*,\s*int B\s*\)\s*;", header)
    assert re.search(r"\bunsigned long long\s+pcy_debug_attn_mq_count\s*\(\s*void\s*\)\s*;", header)
    for name in NEW:
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["pcy_llama_decode_gemm_mq"] == _lib.SIGNATURES["pcy_llama_decode_gemm"]
    assert _lib.SIGNATURES["pcy_debug_attn_mq_count"] == (ctypes.c_ulonglong, [])
    vp, ci = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["pcy_attn_decode_shared"] == (ci, [vp, vp, ci, ctypes.POINTER(_lib.KvCache), ci, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci])
    lib = _lib.load()                                                                           # (raises on a symbol that is not exported)
    for name in NEW:
        assert getattr(lib, name) is not None
    # additions only: the ABI number, the dispatch kinds and the decode kinds stay where the suite pins them
    assert _lib.ABI_VERSION == 13 and re.search(r"#define PCY_ABI_VERSION 13\b", header)
    assert len([k for k in vars(_lib) if k.startswith("DISPATCH_") and isinstance(getattr(_lib, k), int)]) == 20 and len(_lib.DISPATCH_DECODE) == 7


def test_counter_reads_zero_with_nothing_run():
    """in a process of its own: other tests of this session may have run the step"""
    import subprocess
    import sys
    code = "from procyon_amd import _lib; print(int(_lib.load().pcy_debug_attn_mq_count()))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == "0"


def test_drivers_and_callers_take_the_option():
    import inspect
    from procyon_amd import pipelines
    from procyon_amd.engine import Context, LlamaEngine
    from procyon_amd.model.model_unified import UnifiedProCyon
    for fn in (LlamaEngine.decode_gemm, LlamaEngine.generate_beam, UnifiedProCyon.generate, pipelines.caption_bulk):
        assert inspect.signature(fn).parameters["shared_attn"].default is False, fn
    names = list(inspect.signature(Context.attn_decode_shared).parameters)
    assert names == ["self", "qkv", "cache", "layer", "pos", "cos_t", "sin_t", "H", "Hkv", "dh", "keep", "B", "out"]


def _bare_model(dtype):
    """a UnifiedProCyon with nothing but the dtype its caller asked for: generate() decides its refusals before it touches the inputs"""
    from procyon_amd.model.model_unified import UnifiedProCyon
    m = UnifiedProCyon.__new__(UnifiedProCyon)
    m.dtype = dtype
    return m


def test_generate_refuses_shared_attn_off_the_beam_search_with_lookahead_and_on_fp32():
    m = _bare_model(torch.bfloat16)
    for method in ("greedy", "sampling", "nucleus", "temperature"):
        with pytest.raises(ValueError, match="shared_attn"):
            m.generate({}, method=method, decode_gemm=True, shared_attn=True)
    with pytest.raises(ValueError, match="lookahead"):
        m.generate({}, method="greedy", lookahead=4, shared_attn=True)
    with pytest.raises(NotImplementedError, match="bf16"):
        _bare_model(torch.float32).generate({}, method="beam", shared_attn=True)


def test_caption_plugin_reads_shared_attn_from_model_config():
    from types import SimpleNamespace
    from procyon_amd.evaluate import ProcyonCaptionEval
    seen = []

    class Model:
        device = "cpu"

        def eval(self):
            return self

        def bfloat16(self):
            return self

        def generate(self, inputs, **kw):
            seen.append(kw)
            return None, None, None, [["a"] * 10]

    batch = {"reference_indices": {"input": {"seq": [[7]]}}}

    class Loader:
        dataset = SimpleNamespace(aaseq_type="protein")

        def __iter__(self):
            return iter([batch])

    for cfg, want in (({}, None), ({"decode_gemm": True}, None), ({"decode_gemm": True, "shared_attn": True}, True)):
        ev = ProcyonCaptionEval.from_model(Model(), cfg, SimpleNamespace(caption_max_len=4))
        assert ev.shared_attn == (want or False)
        ev.get_predictions(Loader())
        assert seen[-1].get("shared_attn") == want      # (absent by default: the call is today's)
        assert seen[-1].get("decode_gemm") == cfg.get("decode_gemm")
