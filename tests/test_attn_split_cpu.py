"""Host side of the split-key decode attention on shared-prefix caches (pcy_attn_decode_split, pcy_llama_decode_split, pcy_llama_beam_steps_split,
pcy_llama_decode_gemm_split): the symbols are declared, exported and bound while the ABI pins stay; the chunk query is host
arithmetic on its six arguments; the emulation of the kernel's arithmetic (tests/attn_split_ref.py) is no further from float64 than the
reference's bf16 formulas; a fully masked chunk drops out exactly; the refusals of the Python layer.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

from attn_split_ref import eager_reference, rel64, split_reference, truth64
from test_gpu_attn_mq import SHAPES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pcy_attn_decode_split", "pcy_attn_split_chunk_keys", "pcy_llama_decode_split", "pcy_llama_beam_steps_split", "pcy_llama_decode_gemm_split",
       "pcy_debug_attn_split_count")


def test_new_symbols_declared_exported_and_bound():
    from procyon_amd import _lib
    header = open(os.path.join(ROOT, "include", "pcy.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    S = _lib.SIGNATURES
    ci = ctypes.c_int
    assert S["pcy_attn_decode_split"] == S["pcy_attn_decode_shared"] and len(S["pcy_attn_decode_split"][1]) == 15
    assert S["pcy_attn_split_chunk_keys"] == (ci, [ci] * 6)
    assert S["pcy_llama_decode_split"] == S["pcy_llama_decode"] and len(S["pcy_llama_decode_split"][1]) == 5
    assert S["pcy_llama_beam_steps_split"] == S["pcy_llama_beam_steps"] and len(S["pcy_llama_beam_steps_split"][1]) == 12
    assert S["pcy_llama_decode_gemm_split"] == S["pcy_llama_decode_gemm_mq"]
    assert S["pcy_debug_attn_split_count"] == (ctypes.c_ulonglong, [])
    lib = _lib.load()                                                                           # (raises on a symbol that is not exported)
    for name in NEW:
        assert getattr(lib, name) is not None
    # additions only: the ABI number, the dispatch kinds and the decode kinds stay where the suite pins them
    assert _lib.ABI_VERSION == 13 and re.search(r"#define PCY_ABI_VERSION 13\b", header) and lib.pcy_abi_version() == 13
    assert len([k for k in vars(_lib) if k.startswith("DISPATCH_") and isinstance(getattr(_lib, k), int)]) == 20 and len(_lib.DISPATCH_DECODE) == 7


def test_counter_reads_zero_with_nothing_run():
    """in a process of its own: other tests of this session may have run the step"""
    import subprocess
    import sys
    code = "from procyon_amd import _lib; print(int(_lib.load().pcy_debug_attn_split_count()))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip().splitlines()[-1] == "0"


def _chunk(B, rpp, H, Hkv, dh, Tp):
    from procyon_amd import _lib
    return int(_lib.load().pcy_attn_split_chunk_keys(B, rpp, H, Hkv, dh, Tp))


def test_chunk_query_is_host_arithmetic_on_its_six_arguments(monkeypatch):
    """positive multiples of 32 on the operator shapes and the benchmark's geometries; the same answer when asked again, in another order, and
    under environment switches; a longer prefix never gets more than 128 keys per chunk (the chunk's scores wait in registers)"""
    asks = [(B, rpp, H, Hkv, dh, Tp) for H, Hkv, dh, Tp, own, rpp, P, B in SHAPES]
    asks += [(10, 10, 32, 8, 128, 512), (20, 20, 32, 8, 128, 512), (20, 10, 32, 32, 128, 704), (32, 32, 32, 32, 128, 704), (160, 10, 32, 8, 128, 4096)]
    first = [_chunk(*a) for a in asks]
    for c in first:
        assert c > 0 and c % 32 == 0 and c <= 128, first
    monkeypatch.setenv("PCY_DISABLE", "beam_graph,attn_o,decode_nb")
    monkeypatch.setenv("PCY_AO_XMIN", "384")
    assert [_chunk(*a) for a in reversed(asks)] == first[::-1]
    assert _chunk(0, 10, 32, 8, 128, 512) == 0 and _chunk(10, 0, 32, 8, 128, 512) == 0 and _chunk(10, 10, 32, 8, 128, 0) == 0


def _cpu_inputs(shape, seed):
    """the recipe of tests/test_gpu_attn_mq.py::_inputs with seeds of its own -> roped q [B,H,1,dh], K / V [B,H,t+1,dh] over the logical slots"""
    from oracle import llama_ref as LR
    from procyon_amd.engine import rope_tables
    from test_gpu_kernels import rnd
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    t, G = Tp + own, H // Hkv
    qkv = rnd(B, (H + 2 * Hkv) * dh, seed=seed * 10 + 1)
    pk, pv = rnd(P, Hkv, Tp, dh, seed=seed * 10 + 2), rnd(P, Hkv, Tp, dh, seed=seed * 10 + 3)
    sk, sv = rnd(B, Hkv, own + 1, dh, seed=seed * 10 + 4), rnd(B, Hkv, own + 1, dh, seed=seed * 10 + 5)
    cos, sin = rope_tables(dh, 10000.0, t + 2, "cpu")
    prow = torch.arange(B) // rpp
    q = qkv[:, :H * dh].view(B, 1, H, dh).transpose(1, 2)
    k = qkv[:, H * dh:(H + Hkv) * dh].view(B, 1, Hkv, dh).transpose(1, 2)
    v = qkv[:, (H + Hkv) * dh:].view(B, 1, Hkv, dh).transpose(1, 2)
    qr, kr = LR.apply_rope(q, k, cos[t][None, None].expand(B, 1, dh), sin[t][None, None].expand(B, 1, dh))
    K = torch.cat([pk[prow], sk[:, :, :own], kr], 2).repeat_interleave(G, 1)
    V = torch.cat([pv[prow], sv[:, :, :own], v], 2).repeat_interleave(G, 1)
    return qr, K, V


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_emulation_is_no_further_from_float64_than_the_eager_formulas(shape):
    """rel64(split_reference, truth) <= 1.25 x rel64(eager bf16 formulas, truth) on every operator shape and 3 seeds, the chunk length the
    library's own; 1.25 is the factor of tests/test_gpu_fulldepth.py."""
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    chunk = _chunk(B, rpp, H, Hkv, dh, Tp)
    for seed in (1, 2, 3):
        qr, K, V = _cpu_inputs(shape, seed)
        truth = truth64(qr, K, V, dh ** -0.5, None)
        e_split = rel64(split_reference(qr, K, V, dh ** -0.5, None, chunk, Tp), truth)
        e_eager = rel64(eager_reference(qr, K, V, dh ** -0.5, None), truth)
        print(f"{shape} seed {seed} chunk {chunk}: split {e_split:.3e}  eager {e_eager:.3e}  ratio {e_split / e_eager:.3f}")
        assert e_split <= 1.25 * e_eager, (shape, seed, e_split, e_eager)


def test_fully_masked_chunk_drops_out_exactly():
    """rows whose mask blanks one whole prefix chunk (the last one, so that cutting it out moves no other boundary): finite, and bit-equal to
    the result with that chunk's keys removed; rows that keep the chunk do change"""
    shape = (8, 2, 64, 256, 3, 5, 2, 10)
    H, Hkv, dh, Tp, own, rpp, P, B = shape
    chunk = 64
    qr, K, V = _cpu_inputs(shape, 4)
    n = K.shape[2]
    mask = torch.ones(B, n, dtype=torch.uint8)
    mask[::3, Tp - chunk:Tp] = 0
    mask[1::3, :7] = 0
    out = split_reference(qr, K, V, dh ** -0.5, mask, chunk, Tp)
    assert torch.isfinite(out.float()).all()
    rest = torch.cat([torch.arange(0, Tp - chunk), torch.arange(Tp, n)])
    cut = split_reference(qr, K[:, :, rest], V[:, :, rest], dh ** -0.5, mask[:, rest], chunk, Tp - chunk)
    assert torch.equal(out[::3], cut[::3])
    assert not torch.equal(out[1::3], cut[1::3])


def _bare_model(dtype):
    """a UnifiedProCyon with nothing but the dtype its caller asked for: generate() decides its refusals before it touches the inputs"""
    from procyon_amd.model.model_unified import UnifiedProCyon
    m = UnifiedProCyon.__new__(UnifiedProCyon)
    m.dtype = dtype
    return m


def test_python_layer_refusals():
    from procyon_amd.engine import check_shared_attn
    assert check_shared_attn(False) is False and check_shared_attn(True) is True and check_shared_attn("split") == "split"
    m = _bare_model(torch.bfloat16)
    for bad in ("auto", "Split", 1, 0, None, "true"):
        with pytest.raises(ValueError, match="shared_attn"):
            check_shared_attn(bad)
        with pytest.raises(ValueError, match="shared_attn"):
            m.generate({}, method="beam", shared_attn=bad)
    for method in ("greedy", "sampling", "nucleus", "temperature"):
        with pytest.raises(ValueError, match="shared_attn"):
            m.generate({}, method=method, shared_attn="split")
    with pytest.raises(ValueError, match="lookahead"):
        m.generate({}, method="greedy", lookahead=4, shared_attn="split")
    for method in ("greedy", "beam"):
        with pytest.raises(ValueError, match="decode_w8"):
            m.generate({}, method=method, decode_w8=True, shared_attn="split")
    with pytest.raises(NotImplementedError, match="bf16"):
        _bare_model(torch.float32).generate({}, method="beam", shared_attn="split")


def test_drivers_take_the_option():
    import inspect
    from procyon_amd.engine import Context, LlamaEngine
    assert inspect.signature(LlamaEngine.beam_steps).parameters["split"].default is False
    assert list(inspect.signature(LlamaEngine.decode_split).parameters) == ["self", "cache", "st", "B"]
    assert list(inspect.signature(Context.attn_decode_split).parameters) == list(inspect.signature(Context.attn_decode_shared).parameters)


def test_caption_plugin_passes_split_through():
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

    class Loader:
        dataset = SimpleNamespace(aaseq_type="protein")

        def __iter__(self):
            return iter([{"reference_indices": {"input": {"seq": [[7]]}}}])

    ev = ProcyonCaptionEval.from_model(Model(), {"shared_attn": "split"}, SimpleNamespace(caption_max_len=4))
    assert ev.shared_attn == "split"
    ev.get_predictions(Loader())
    assert seen[-1].get("shared_attn") == "split" and seen[-1].get("decode_gemm") is None
