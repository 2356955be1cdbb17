"""GPU: what the decode, beam-search and sampling entries of the C ABI refuse, through the shared checks of procyon_amd/csrc/pcy_engine.hip
(check_step_args / decode_prologue, check_beam_args, check_sample_args, f32_stream_check): every refusal is code 1 with a text that names the
entry that was called, moves no dispatch or selection counter, and leaves the context as it was -- a valid 3-step greedy run behind the
refusals equals the same run on a fresh context bit for bit, tokens and logits, bf16 and fp32.

The engines are the tiny ones of tests/test_gpu_select.py (vocab 50, d 64, one layer, 2 heads, 1 KV head, ffn 128, max_pos 64) on a cache of
2 rows x 16 slots.  The fp32 engine has 4 heads instead of 2: head_dim 32 is not one the fp32 step serves (16 / 64 / 128), so with 2 heads
every fp32 chain entry would be refused for its geometry before it looks at the argument under test, and no valid fp32 step could follow.

B = 0 and B = cache rows + 1 go to the entries that run a decode step and to the fp32 picks.  pcy_greedy_pick and pcy_sample_pick (bf16) take
a row count that they do not compare with the cache -- the selection tests call them with caches of any size -- and the single beam steps
take no cache: they get the cases that apply to them.  Nothing here launches more than the six valid steps at the end."""
import ctypes as C
import re

import pytest
import torch

from test_gpu_select import _engine

pytestmark = pytest.mark.gpu
BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
GEO = dict(vocab=50, d=64, n_layers=1, n_heads=2, n_kv_heads=1, ffn=128)
GEO_F32 = dict(GEO, n_heads=4)
V, ROWS, SLOTS, STEPS, T0 = GEO["vocab"], 2, 16, 3, 4
NAN = float("nan")


def _lib():
    from procyon_amd import _lib as L
    return L.load()


def _counters():
    """every dispatch, route and step counter of the library"""
    lib = _lib()
    return ([int(lib.pcy_debug_dispatch_count(k)) for k in range(20)], [int(lib.pcy_debug_attn_route_count(k)) for k in range(4)],
            [int(lib.pcy_debug_gemv_route_count(k)) for k in range(6)],
            [int(lib.pcy_debug_f32_select_count(k)) for k in range(2)], [int(lib.pcy_debug_look_count(k)) for k in range(2)],
            int(lib.pcy_debug_f32_stream_count()), int(lib.pcy_debug_attn_split_count()), int(lib.pcy_debug_decode_gemm_count()),
            int(lib.pcy_debug_attn_mq_count()), int(lib.pcy_debug_decode_w8_count()), int(lib.pcy_debug_decode_window_count()),
            int(lib.pcy_debug_extend_grouped_count()))


def _refused(entry, call, text=None):
    """`call` raises PcyError with code 1 and the LIBRARY's text (behind the wrapper's own prefix) naming `entry`; no counter moves"""
    from procyon_amd._lib import PcyError
    n0 = _counters()
    with pytest.raises(PcyError, match=r"\(code 1\): " + re.escape(entry) + ": .*" + (text or "")):
        call()
    assert _counters() == n0, entry


def _engine_f32(ctx=None):
    from procyon_amd import synth
    from procyon_amd.engine import LlamaConfig
    from procyon_amd.engine_f32 import LlamaEngineF32
    return LlamaEngineF32(synth.llama_state_dict(**GEO_F32, dtype=F32), LlamaConfig(**GEO_F32, max_pos=64), ctx=ctx)


def _beam_state(B, beam, call_B=None):
    """a complete beam state of B x beam rows; call_B: the B the wrappers pass instead (the arrays stay valid)"""
    from procyon_amd.engine import BeamState
    bs = BeamState(B, beam, STEPS, 2, T0, "cuda")
    if call_B is not None:
        bs.B = call_B
    return bs


BEAM_CASES = (("beam", lambda: _beam_state(1, 33), 3), ("group_size", lambda: _beam_state(1, 4), 3), ("B=0", lambda: _beam_state(1, 1, call_B=0), 1))


# ---------------------------------------------------------------------------------------------- bf16
def test_bf16_entries_refuse_and_the_context_is_untouched():
    from procyon_amd import synth
    from procyon_amd.engine import Context, GenState, LlamaConfig, LlamaEngine
    eng = _engine(V)
    cache = eng.new_cache(ROWS, SLOTS)
    st = GenState(ROWS, V, STEPS, "cuda")
    u = torch.full((STEPS * (ROWS + 1),), 0.5, device="cuda")

    # beam = 33, beam = 4 with group_size = 3, B = 0: the single step and both chains; B * beam = cache rows + 1: the chains
    for text, make, group in BEAM_CASES:
        bs = make()
        lg = torch.zeros(bs.BB, V, dtype=BF, device="cuda")
        _refused("pcy_beam_step", lambda: eng.beam_step(lg, bs, group, 0.8), text)
        for split in (False, True):
            name = "pcy_llama_beam_steps_split" if split else "pcy_llama_beam_steps"
            rec = torch.zeros(STEPS, bs.BB, V, dtype=BF, device="cuda")
            _refused(name, lambda: eng.beam_steps(cache, bs.gen_state(V), bs, group, 0.8, rec, STEPS, split=split), text)
    bs = _beam_state(ROWS + 1, 1)
    for split in (False, True):
        name = "pcy_llama_beam_steps_split" if split else "pcy_llama_beam_steps"
        rec = torch.zeros(STEPS, bs.BB, V, dtype=BF, device="cuda")
        _refused(name, lambda: eng.beam_steps(cache, bs.gen_state(V), bs, 1, 0.8, rec, STEPS, split=split), "cache rows")

    # temperature = 0, nucleus_prob = 1, nucleus_prob = NaN: the pick and the loop
    for kw, text in ((dict(temperature=0.0), "temperature"), (dict(nucleus_prob=1.0), "nucleus_prob"), (dict(nucleus_prob=NAN), "nucleus_prob")):
        _refused("pcy_sample_pick", lambda: eng.sample_pick(cache, st, ROWS, True, u, **kw), text)
        _refused("pcy_llama_sample", lambda: eng.sample_steps(cache, st, ROWS, STEPS, u, **kw), text)

    # B = 0, B = cache rows + 1: every entry that runs the step
    for rows in (0, ROWS + 1):
        text = f"B={rows}"
        _refused("pcy_llama_decode", lambda: eng.decode(cache, st, rows), text)
        _refused("pcy_llama_decode_layers", lambda: eng.decode_layers(cache, st, rows, 2), text)
        _refused("pcy_llama_decode_graph", lambda: eng.decode_graph(cache, st, rows), text)
        _refused("pcy_llama_decode_split", lambda: eng.decode_split(cache, st, rows), text)
        _refused("pcy_llama_sample", lambda: eng.sample_steps(cache, st, rows, STEPS, u), text)
        for graph in (False, True):
            _refused("pcy_llama_greedy", lambda: eng.greedy_steps(cache, st, rows, STEPS, use_graph=graph), text)

    # a NULL model, cache or state (a NULL struct pointer: nothing to dereference): code 1, not a host crash
    lib, h, bs = eng.ctx.lib, eng.ctx.h, _beam_state(1, 2)
    rec = torch.zeros(STEPS, 2, V, dtype=BF, device="cuda")
    full = (C.byref(eng.desc), C.byref(cache.c), C.byref(st.c))
    tails = {"pcy_llama_decode": (ROWS,), "pcy_llama_decode_layers": (ROWS, 1), "pcy_llama_decode_graph": (ROWS,), "pcy_llama_greedy": (ROWS, STEPS, 1),
             "pcy_llama_decode_split": (ROWS,), "pcy_llama_sample": (ROWS, STEPS, 1.0, -1.0, u.data_ptr()),
             "pcy_llama_beam_steps": (1, 2, 1, 0.8, C.byref(bs.c), rec.data_ptr(), STEPS, 0),
             "pcy_llama_beam_steps_split": (1, 2, 1, 0.8, C.byref(bs.c), rec.data_ptr(), STEPS, 0)}
    for name, tail in tails.items():
        for missing in range(3):
            n0 = _counters()
            rc = getattr(lib, name)(h, *[None if i == missing else a for i, a in enumerate(full)], *tail)
            msg = lib.pcy_last_error().decode()
            assert rc == 1 and msg.startswith(name + ": ") and "incomplete" in msg, (name, missing, rc, msg)
            assert _counters() == n0, name

    # behind the refusals the shared context runs what a fresh one runs, bit for bit
    def greedy(e):
        c, s = e.new_cache(ROWS, SLOTS), GenState(ROWS, V, STEPS, "cuda", keep_logits=True)
        g = torch.Generator().manual_seed(5)
        c.k.copy_((torch.randn(c.k.shape, generator=g) * 0.5).to(BF))
        c.v.copy_((torch.randn(c.v.shape, generator=g) * 0.5).to(BF))
        s.pos.fill_(T0)
        s.next_tok.copy_(torch.tensor([3, 7], dtype=I32))
        e.greedy_steps(c, s, ROWS, STEPS)
        e.ctx.sync()
        return s.tokens_out.cpu(), s.logits_all.contiguous().view(torch.int16), s.logprob.cpu().view(I32), int(s.pos), int(s.step)

    fresh = Context()
    other = LlamaEngine(synth.llama_state_dict(**GEO), LlamaConfig(**GEO, max_pos=64), ctx=fresh)
    got, want = greedy(eng), greedy(other)
    lib.pcy_ctx_destroy(fresh.h)
    assert got[3:] == (T0 + STEPS, STEPS) and got[3:] == want[3:]
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(got[1].view(BF).float()).all())


# ---------------------------------------------------------------------------------------------- fp32
def test_f32_entries_refuse_and_the_context_is_untouched():
    from procyon_amd.engine import Context
    from procyon_amd.engine_f32 import GenStateF32
    eng = _engine_f32()
    cache, st = eng.new_cache(ROWS, SLOTS), eng.new_gen_state(ROWS, STEPS)
    u = torch.full((STEPS * (ROWS + 1),), 0.5, device="cuda")

    for text, make, group in BEAM_CASES:
        bs = make()
        lg, rec = torch.zeros(bs.BB, V, device="cuda"), torch.zeros(STEPS, bs.BB, V, device="cuda")
        gs = GenStateF32(bs.BB, V, 1, "cuda", pos=bs.pos, next_tok=bs.next_tok)
        _refused("pcy_f32_beam_step", lambda: eng.beam_step(lg, bs, group, 0.8), text)
        _refused("pcy_f32_llama_beam_steps", lambda: eng.beam_steps(cache, gs, bs, group, 0.8, rec, STEPS), text)
    bs = _beam_state(ROWS + 1, 1)
    _refused("pcy_f32_llama_beam_steps", lambda: eng.beam_steps(cache, eng.new_gen_state(bs.BB, 1), bs, 1, 0.8, torch.zeros(STEPS, bs.BB, V, device="cuda"), STEPS),
             f"B={ROWS + 1}")

    for kw, text in ((dict(temperature=0.0), "temperature"), (dict(nucleus_prob=1.0), "nucleus_prob"), (dict(nucleus_prob=NAN), "nucleus_prob")):
        _refused("pcy_f32_sample_pick", lambda: eng.sample_pick(cache, st, ROWS, True, u, **kw), text)
        for graph in (False, True):
            _refused("pcy_f32_llama_sample", lambda: eng.sample_steps(cache, st, ROWS, STEPS, u, graph=graph, **kw), text)

    for rows in (0, ROWS + 1):
        text = f"B={rows}"
        for graph in (False, True):
            _refused("pcy_f32_llama_decode_graph" if graph else "pcy_f32_llama_decode", lambda: eng.decode_stream(cache, st, rows, graph=graph), text)
            _refused("pcy_f32_llama_greedy", lambda: eng.greedy_steps(cache, st, rows, STEPS, graph=graph), text)
            _refused("pcy_f32_llama_sample", lambda: eng.sample_steps(cache, st, rows, STEPS, u, graph=graph), text)
        _refused("pcy_f32_greedy_pick", lambda: eng.greedy_pick(cache, st, rows), text)
        _refused("pcy_f32_sample_pick", lambda: eng.sample_pick(cache, st, rows, True, u), text)

    def greedy(e):
        c, s = e.new_cache(ROWS, SLOTS), e.new_gen_state(ROWS, STEPS, keep_logits=True)
        g = torch.Generator().manual_seed(6)
        c.k.copy_(torch.randn(c.k.shape, generator=g) * 0.5)
        c.v.copy_(torch.randn(c.v.shape, generator=g) * 0.5)
        s.set(pos=T0, next_tok=torch.tensor([3, 7]))
        e.greedy_steps(c, s, ROWS, STEPS)
        e.ops.ctx.sync()
        return s.tokens_out.cpu(), s.logits_all.cpu().view(I32), s.logprob.cpu().view(I32), int(s.pos), int(s.step)

    fresh = Context()
    got, want = greedy(eng), greedy(_engine_f32(fresh))
    eng.ops.lib.pcy_ctx_destroy(fresh.h)
    assert got[3:] == (T0 + STEPS, STEPS) and got[3:] == want[3:]
    for a, b in zip(got[:3], want[:3]):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(got[1].view(F32)).all()) and bool(torch.isfinite(got[2].view(F32)).all())
