"""No GPU: the EOS stop of greedy and sampling generation -- the trailing fields of the generation state, the refusals and
defaults of the Python layers, and the plain-Python restatement of the stop rule (tests/stop_eos_ref.py) that tests/test_gpu_stop_eos.py holds
the kernels to."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import stop_eos_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the state
def test_gen_state_ends_with_the_stop_fields():
    from procyon_amd import _lib
    names = [f[0] for f in _lib.GenState._fields_]
    assert names[-4:] == ["finished", "done", "n_steps_run", "eos_id"], names
    assert names[:10] == ["pos", "step", "next_tok", "tokens_out", "logprob", "logits", "logits_all", "keep", "max_steps", "logits_all_ld"]
    kinds = dict(_lib.GenState._fields_)
    assert kinds["finished"] is ctypes.c_void_p and kinds["done"] is ctypes.c_void_p and kinds["n_steps_run"] is ctypes.c_void_p
    assert kinds["eos_id"] is ctypes.c_int32
    # the positional constructions of engine.py / engine_f32.py from before the fields: ten arguments, the new fields zero
    st = _lib.GenState(1, 2, 3, 4, 5, 6, 7, None, 9, 10)
    assert (st.finished, st.done, st.n_steps_run, st.eos_id) == (None, None, None, 0)
    assert st.max_steps == 9 and st.logits_all_ld == 10
    st = _lib.GenState(1, 2, 3, 4, 5, 6, 7, None, 9, 10, 11, 12, 13, 14)
    assert (st.finished, st.done, st.n_steps_run, st.eos_id) == (11, 12, 13, 14)


def test_header_declares_the_fields_behind_the_old_ones_and_no_new_function():
    header = open(os.path.join(ROOT, "include", "pcy.h")).read()
    body = header[:header.index("} pcy_gen_state;")]
    body = body[body.rindex("typedef struct {"):]
    order = [body.index(w) for w in ("int32_t logits_all_ld;", "int32_t* finished;", "int32_t* done;", "int32_t* n_steps_run;", "int32_t eos_id;")]
    assert order == sorted(order), order
    assert re.search(r"#define\s+PCY_ABI_VERSION\s+13\b", header)
    assert len(set(re.findall(r"\b(pcy_[a-z0-9_]+)\s*\(", header))) == 108


# ------------------------------------------------------------------------------------------------ refusals and defaults
def _bare_model(dtype):
    """a UnifiedProCyon with nothing but the dtype its caller asked for: generate() decides its refusals before it touches the inputs"""
    from procyon_amd.model.model_unified import UnifiedProCyon
    m = UnifiedProCyon.__new__(UnifiedProCyon)
    m.dtype = dtype
    return m


def test_generate_refusals():
    for dtype in (torch.bfloat16, torch.float32):
        m = _bare_model(dtype)
        for bad in (None, 1, 0, "yes", "True", 2.0):
            with pytest.raises(ValueError, match="stop_on_eos"):
                m.generate({}, method="greedy", stop_on_eos=bad)
        with pytest.raises(ValueError, match="stop_on_eos"):
            m.generate({}, method="beam", stop_on_eos=True)
    # the beam refusal comes before anything the beam search itself refuses
    with pytest.raises(ValueError, match="stop_on_eos"):
        _bare_model(torch.bfloat16).generate({}, method="beam", stop_on_eos=True, shared_attn="split")
    # off is off: beam with stop_on_eos=False gets as far as the inputs
    with pytest.raises((KeyError, TypeError, AttributeError)):
        _bare_model(torch.bfloat16).generate({}, method="beam", stop_on_eos=False)


def test_engine_argument_check():
    from procyon_amd.engine import check_stop_arg
    assert check_stop_arg(None, 10, "x") is None and check_stop_arg(0, 10, "x") == 0 and check_stop_arg(9, 10, "x") == 9
    for bad in (10, -1, True, False, 2.0, "2"):
        with pytest.raises(ValueError, match="stop_on_eos"):
            check_stop_arg(bad, 10, "x")


def test_drivers_default_to_off():
    from procyon_amd.engine import GenState, LlamaEngine
    from procyon_amd.engine_f32 import GenStateF32, LlamaEngineF32
    from procyon_amd.model.model_unified import UnifiedProCyon
    from procyon_amd.pipelines import caption_bulk
    for fn in (LlamaEngine.generate_greedy, LlamaEngine.generate_sampling, LlamaEngine.generate_lookahead, LlamaEngineF32.generate_greedy,
               LlamaEngineF32.generate_sampling):
        assert inspect.signature(fn).parameters["stop_on_eos"].default is None, fn
    for cls in (GenState, GenStateF32):
        assert inspect.signature(cls.__init__).parameters["eos_id"].default is None, cls
    assert inspect.signature(LlamaEngineF32.new_gen_state).parameters["eos_id"].default is None
    assert inspect.signature(UnifiedProCyon.generate).parameters["stop_on_eos"].default is False
    assert inspect.signature(caption_bulk).parameters["stop_on_eos"].default is False
    assert list(inspect.signature(caption_bulk).parameters)[-1] == "stop_on_eos"
    with pytest.raises(ValueError, match="stop_on_eos"):
        caption_bulk(None, None, None, [], stop_on_eos="yes")
    src = open(os.path.join(ROOT, "scripts", "caption_bulk.py")).read()
    assert '"--stop_on_eos", action="store_true"' in src


def test_caption_plugin_takes_the_option():
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

    args = SimpleNamespace(caption_max_len=4)
    ev = ProcyonCaptionEval.from_model(Model(), {}, args)
    assert ev.stop_on_eos is False
    ev.get_predictions(Loader())
    assert "stop_on_eos" not in seen[-1]
    ev = ProcyonCaptionEval.from_model(Model(), {"stop_on_eos": True, "generation_method": "greedy", "num_captions": 1, "beam_group_size": 1}, args)
    ev.get_predictions(Loader())
    assert seen[-1].get("stop_on_eos") is True and seen[-1]["method"] == "greedy"
    # beam search has its own stop: nothing is passed on, generate() would refuse it
    ev = ProcyonCaptionEval.from_model(Model(), {"stop_on_eos": True}, args)
    ev.get_predictions(Loader())
    assert "stop_on_eos" not in seen[-1] and seen[-1]["method"] == "beam"
    with pytest.raises(ValueError, match="stop_on_eos"):
        ProcyonCaptionEval.from_model(Model(), {"stop_on_eos": 1}, args)


# ------------------------------------------------------------------------------------------------ the restatement's own edge cases
E = 7


def test_ref_rows_finish_independently():
    tokens = [[1, 2, E], [E, 3, 4], [5, 6, 5], [5, E, 5], [9, 9, 9]]
    gains = [[-1.0, -2.0, -4.0], [-8.0, -16.0, -32.0], [-64.0, -128.0, -256.0], [-512.0, -1024.0, -2048.0], [-1.5, -1.5, -1.5]]
    r = R.stop_eos(tokens, E, gains)
    assert r["tokens"] == [[1, 2, E], [E, 3, E], [E, 6, E], [E, E, E]]
    assert r["logprob"] == [-9.0, -2.0 - 16.0 - 128.0 - 1024.0, -4.0]      # the EOS itself is added, nothing behind it
    assert r["done"] and r["done_step"] == 3 and r["steps_run"] == 4 and r["finished"] == [True] * 3
    assert R.padded_tokens(r, E, 6) == [[1, E, E, E, E, E], [2, 3, 6, E, E, E], [E] * 6]


def test_ref_edges():
    # EOS at step 0 of one row
    r = R.stop_eos([[E], [3]], E, [[-0.5], [-0.25]])
    assert r["tokens"] == [[E]] and r["logprob"] == [-0.5] and r["done_step"] == 0 and r["steps_run"] == 1
    # all rows in one step
    r = R.stop_eos([[1, 2], [E, E], [3, 3]], E)
    assert r["done_step"] == 1 and r["tokens"] == [[1, 2], [E, E]] and r["logprob"] is None
    # never
    t = [[1, 2], [3, 4]]
    r = R.stop_eos(t, E, [[-1.0, -1.0], [-2.0, -2.0]])
    assert not r["done"] and r["done_step"] is None and r["steps_run"] == 2 and r["tokens"] == t and r["logprob"] == [-3.0, -3.0]
    assert r["finished"] == [False, False]
    # a row finished on entry never emits a token of its own and adds nothing
    r = R.stop_eos([[1, 2], [3, E]], E, [[-1.0, -1.0], [-2.0, -2.0]], finished0=[True, False])
    assert r["tokens"] == [[E, 2], [E, E]] and r["logprob"] == [0.0, -3.0] and r["done_step"] == 1
    # every row finished on entry: the first step raises done, having emitted only EOS
    r = R.stop_eos([[1], [2]], E, finished0=[True])
    assert r["tokens"] == [[E]] and r["done_step"] == 0
    # no steps
    r = R.stop_eos([], E, finished0=[False, False])
    assert r["tokens"] == [] and not r["done"] and r["steps_run"] == 0
    # a second EOS of a finished row's table is never looked at; a step behind done changes nothing
    r = R.stop_eos([[E], [E], [E]], E, [[-1.0], [-1.0], [-1.0]])
    assert r["steps_run"] == 1 and r["logprob"] == [-1.0]


def test_ref_helpers():
    assert R.first_eos([1, 2, E, E], E) == 2 and R.first_eos([1, 2], E) is None and R.first_eos([], E) is None
    from procyon_amd.engine import STOP_CHUNK
    assert STOP_CHUNK == 8 and R.enqueued_bound(0, STOP_CHUNK) == 15 and R.enqueued_bound(10, STOP_CHUNK) == 25


def test_chunked_driver_on_a_scripted_state():
    """`steps_until_done` with a state whose flag is scripted: it enqueues chunks of STOP_CHUNK, reads the look of the chunk BEFORE the latest,
    and so stops within enqueued_bound of the finishing step -- for every finishing step of a 40-step run and for none"""
    from procyon_amd.engine import STOP_CHUNK, steps_until_done

    class St:
        def __init__(self, finish):
            self.finish, self.enq = finish, 0

        def look_at_done(self):
            seen = self.finish is not None and self.enq >= self.finish      # the flag as of what is enqueued NOW
            return lambda: seen

    for total in (1, 7, 8, 9, 39):
        for finish in [None] + list(range(0, total + 1)):      # finish = decode steps after which done is up (0: the prefill's pick)
            st = St(finish)
            sizes = []

            def enqueue(n):
                sizes.append(n)
                st.enq += n
            got = steps_until_done(st, total, enqueue, st.look_at_done())
            assert got == st.enq == sum(sizes) and all(1 <= n <= STOP_CHUNK for n in sizes) and all(n == STOP_CHUNK for n in sizes[:-1])
            if finish is None:
                assert got == total
            else:
                assert got >= min(finish, total) and got <= min(total, max(finish, 1) + 2 * STOP_CHUNK - 1), (total, finish, got)


def test_caption_bulk_with_the_option_gives_the_same_table(monkeypatch):
    """caption_bulk generates with beam search, which ends on the device once every beam holds an EOS: the option is accepted, nothing is
    passed on to generate (which would refuse it with method="beam"), and the table is the one without it"""
    import procyon.data.inference_utils as IU
    from procyon_amd.pipelines import caption_bulk
    seen = []

    class Model:
        def eval(self):
            return self

        def bfloat16(self):
            return self

        def generate(self, inputs, **kw):
            seen.append(kw)
            return None, None, None, [[f"c{i} of {s}<|end_of_text|> tail" for i in range(kw["beam_size"])] for s in inputs["input"]["seq"]]

    monkeypatch.setattr(IU, "create_caption_input_simple", lambda **kw: {
        "data": {"seq": torch.tensor(kw["input_aaseq_ids"]), "text": []}, "input": {"seq": [[0]], "text": [[]]}, "instructions": ["i"]})
    monkeypatch.setattr(IU, "uniprot_id_to_index", lambda u: int(u[1:]))
    ids = ["P1", "P2", "P3"]
    off = caption_bulk(Model(), None, None, ids, beam_size=4, batch_size=2)
    on = caption_bulk(Model(), None, None, ids, beam_size=4, batch_size=2, stop_on_eos=True)
    assert off.equals(on) and off.shape == (3, 3) and off["response1"].tolist()[0] == "c2 of [0]"
    assert len(seen) == 4 and all(kw["method"] == "beam" and "stop_on_eos" not in kw for kw in seen)
