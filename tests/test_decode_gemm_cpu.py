"""Host side of the decode step for more than 32 rows (pcy_llama_decode_gemm): the two symbols are declared, exported and bound;
the counter reads 0 with nothing run; the plan behind decode_gemm="auto"; generate()'s refusals.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcy_llama_decode_gemm", "pcy_debug_decode_gemm_count")


def test_new_symbols_declared_exported_and_bound():
    from procyon_amd import _lib
    header = open(os.path.join(ROOT, "include", "pcy.h")).read()
    assert re.search(r"\bint\s+pcy_llama_decode_gemm\s*\(\s*pcy_ctx\*\s*,\s*const pcy_llama_desc\*\s*,\s*const pcy_kv_cache\*\s*,\s*const pcy_gen_state\*\s*,\s*int B\s*\)\s*;", header)
    assert re.search(r"\bunsigned long long\s+pcy_debug_decode_gemm_count\s*\(\s*void\s*\)\s*;", header)
    for name in NEW:
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["pcy_llama_decode_gemm"] == _lib.SIGNATURES["pcy_llama_decode"]      # the contract of pcy_llama_decode, also in its arguments
    assert _lib.SIGNATURES["pcy_debug_decode_gemm_count"] == (ctypes.c_ulonglong, [])
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
    code = "from procyon_amd import _lib; print(int(_lib.load().pcy_debug_decode_gemm_count()))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == "0"


def test_decode_gemm_plan():
    from procyon_amd.engine import DECODE_GEMM_MIN_ROWS, decode_gemm_plan
    assert DECODE_GEMM_MIN_ROWS >= 33
    classes = [(s, m) for s in (False, True) for m in (False, True)]
    for shared, mha in classes:
        got = [decode_gemm_plan(rows, shared, mha) for rows in range(0, 300)]
        assert all(isinstance(g, bool) for g in got)
        assert not any(got[:33]), "never at or below 32 rows"
        assert got == sorted(got), "monotone in rows"
        assert got[160] and decode_gemm_plan(4096, shared, mha)
    assert decode_gemm_plan(DECODE_GEMM_MIN_ROWS) and not decode_gemm_plan(DECODE_GEMM_MIN_ROWS - 1)


def _bare_model(dtype):
    """a UnifiedProCyon with nothing but the dtype its caller asked for: generate() decides its refusals before it touches the inputs"""
    from procyon_amd.model.model_unified import UnifiedProCyon
    m = UnifiedProCyon.__new__(UnifiedProCyon)
    m.dtype = dtype
    return m


def test_generate_refuses_decode_gemm_with_lookahead_and_on_fp32():
    m = _bare_model(torch.bfloat16)
    for opt in (True, "auto"):
        with pytest.raises(ValueError, match="lookahead"):
            m.generate({}, method="greedy", lookahead=4, decode_gemm=opt)
    with pytest.raises(ValueError, match="decode_gemm"):
        m.generate({}, method="greedy", decode_gemm="yes")
    with pytest.raises(NotImplementedError, match="bf16"):
        _bare_model(torch.float32).generate({}, method="beam", decode_gemm=True)


def test_drivers_and_callers_take_the_option():
    import inspect
    from procyon_amd import pipelines
    from procyon_amd.engine import LlamaEngine
    from procyon_amd.model.model_unified import UnifiedProCyon
    for fn in (LlamaEngine.generate_greedy, LlamaEngine.generate_sampling, LlamaEngine.generate_beam, UnifiedProCyon.generate, pipelines.caption_bulk):
        assert inspect.signature(fn).parameters["decode_gemm"].default is False, fn
    assert callable(LlamaEngine.decode_gemm)
    eng = LlamaEngine.__new__(LlamaEngine)
    with pytest.raises(ValueError, match="decode_gemm"):
        eng._use_decode_gemm("always", 160)
    assert eng._use_decode_gemm(False, 160) is False and eng._use_decode_gemm(True, 1) is True


def test_caption_plugin_reads_decode_gemm_from_model_config():
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

    for cfg, want in (({}, None), ({"decode_gemm": "auto"}, "auto"), ({"decode_gemm": True}, True)):
        ev = ProcyonCaptionEval.from_model(Model(), cfg, SimpleNamespace(caption_max_len=4))
        assert ev.decode_gemm == (want or False)
        ev.get_predictions(Loader())
        assert seen[-1].get("decode_gemm") == want      # (absent by default: the call is today's)
