"""CPU: the binding of the lookahead pass on the decode loop -- pcy_attn_window, pcy_llama_decode_window and their counter in
the header, the library and `_lib.SIGNATURES`, one ABI number in all three -- and the refusals of `generate_lookahead(step=...)` /
`generate(lookahead_step=...)` that need no device.  The device side is held in tests/test_gpu_look_window.py."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pcy_attn_window", "pcy_llama_decode_window", "pcy_debug_decode_window_count", "pcy_attn_window_chunk")


def test_entry_points_in_header_library_and_signatures():
    from procyon_amd import _lib
    header = open(os.path.join(ROOT, "include", "pcy.h")).read()
    lib = _lib.load()
    for name in SYMBOLS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    # one ABI number in the header, the binding and the library
    m = re.search(r"#define PCY_ABI_VERSION (\d+)\b", header)
    assert m and int(m.group(1)) == _lib.ABI_VERSION == lib.pcy_abi_version()
    # the argument lists the binding declares are the header's: 14 and 7 arguments
    assert len(_lib.SIGNATURES["pcy_attn_window"][1]) == 14 and len(_lib.SIGNATURES["pcy_llama_decode_window"][1]) == 7
    assert _lib.SIGNATURES["pcy_debug_decode_window_count"][1] == []


def test_chunk_length_is_a_multiple_of_32_and_the_counter_starts_readable():
    from procyon_amd import _lib
    lib = _lib.load()
    c = lib.pcy_attn_window_chunk()
    assert c >= 32 and c % 32 == 0
    assert lib.pcy_debug_decode_window_count() >= 0


def test_defaults_are_extend():
    from procyon_amd.engine import LlamaEngine
    from procyon_amd.model.model_unified import UnifiedProCyon
    assert inspect.signature(LlamaEngine.generate_lookahead).parameters["step"].default == "extend"
    assert inspect.signature(UnifiedProCyon.generate).parameters["lookahead_step"].default == "extend"
    assert inspect.signature(UnifiedProCyon.generate).parameters["lookahead"].default == 0


def test_generate_lookahead_refuses_an_unknown_step_before_anything_else():
    from procyon_amd.engine import LlamaEngine
    eng = object.__new__(LlamaEngine)          # no device, no weights: the check comes first
    emb = torch.zeros(1, 5, 8, dtype=torch.bfloat16)
    for bad in ("decode", "", None, "Window", 1):
        with pytest.raises(ValueError, match="step="):
            LlamaEngine.generate_lookahead(eng, emb, torch.arange(5), 4, 4, step=bad)


def test_generate_refuses_lookahead_step_without_a_device():
    from procyon_amd.model.model_unified import UnifiedProCyon
    m = object.__new__(UnifiedProCyon)
    m.dtype = torch.bfloat16
    with pytest.raises(ValueError, match="lookahead_step"):
        m.generate({}, method="greedy", lookahead=4, lookahead_step="decode")
    with pytest.raises(ValueError, match="lookahead_step"):
        m.generate({}, method="greedy", lookahead_step="decode")
    with pytest.raises(ValueError, match="lookahead_step"):      # "window" chooses the pass of a lookahead run: not without one
        m.generate({}, method="greedy", lookahead_step="window")
    m.dtype = torch.float32                                          # the fp32 family refuses it as it refuses lookahead
    with pytest.raises(NotImplementedError, match="bf16 engine"):
        m.generate({}, method="greedy", lookahead=4, lookahead_step="window")
    with pytest.raises(NotImplementedError, match="bf16 engine"):
        m.generate({}, method="greedy", lookahead_step="window")
