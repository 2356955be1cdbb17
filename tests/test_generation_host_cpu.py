"""No GPU: the host side of the generation drivers (procyon_amd/engine.py: `run_generation`, `hand_out`, `sampling_variates`,
`beam_parent_index`, `beam_steps_until_done`) on scripted states -- what is enqueued, in which order, where the host looks, and what is handed
out.  The drivers of both engine families are these functions plus their own `enqueue`; tests/test_gpu_*.py hold the drivers to the oracle."""
import pytest
import torch

from procyon_amd.engine import (STOP_CHUNK, beam_parent_index, beam_steps_until_done, hand_out, run_generation, sampling_variates,
                                steps_until_done)

EOS = 7


class State:
    """a generation state without a device: the fields `hand_out` reads, and a `done` flag scripted as in
    test_stop_eos_cpu.test_chunked_driver_on_a_scripted_state (finish = decode steps after which it is up, 0: the first pick, None: never)"""

    def __init__(self, B=2, max_steps=8, V=5, eos_id=None, steps_run=None, finish=None, keep_logits=True):
        self.tokens_out = torch.arange(B * max_steps, dtype=torch.int32).view(B, max_steps) + 100
        self.logprob = -torch.arange(B, dtype=torch.float32)
        self._record = torch.arange(max_steps * B * V, dtype=torch.float32).view(max_steps, B, V) if keep_logits else None
        self.eos_id, self.steps_run, self.finish = eos_id, steps_run, finish
        self.enq, self.picked, self.log = 0, False, []

    @property
    def logits_all(self):
        if self.log[-1:] != ["hand_out"]:
            self.log.append("hand_out")
        return self._record

    def look_at_done(self):
        self.log.append("look")
        seen = self.finish is not None and self.picked and self.enq >= self.finish      # the flag as of what is enqueued NOW
        return lambda: seen

    def callables(self):
        def first_pick():
            self.log.append("pick")
            self.picked = True

        def enqueue(n):
            self.log.append(n)
            self.enq += n
        return first_pick, enqueue, lambda: self.log.append("sync")


# ------------------------------------------------------------------------------------------------ the runner
def test_runner_without_a_stop():
    st = State(max_steps=1)
    tok, lp, la = run_generation(st, 1, *st.callables())
    assert st.log == ["pick", "sync", "hand_out"]                      # enqueue never, sync once
    assert tok.shape == (2, 1) and la.shape == (2, 1, 5) and lp is st.logprob
    st = State(max_steps=9)
    run_generation(st, 9, *st.callables())
    assert st.log == ["pick", 8, "sync", "hand_out"]                   # all steps in one enqueue, no look


@pytest.mark.parametrize("finish", [0, 11, None])      # raised by the first pick, in the middle of a chunk, never
def test_runner_with_a_stop_chunks_like_steps_until_done(finish):
    max_len = 40
    ref = State(eos_id=EOS, finish=finish)
    ref.picked = True
    ref_total = steps_until_done(ref, max_len - 1, ref.callables()[1], ref.look_at_done())
    ref_sizes = [e for e in ref.log if isinstance(e, int)]
    st = State(max_steps=max_len, eos_id=EOS, finish=finish, steps_run=max_len)
    run_generation(st, max_len, *st.callables())
    sizes = [e for e in st.log if isinstance(e, int)]
    assert sizes == ref_sizes and st.enq == ref_total
    if finish is None:
        assert st.enq == max_len - 1
    else:
        assert st.enq < max_len - 1 and st.enq <= max(finish, 1) + 2 * STOP_CHUNK - 1
    # pick, the look behind it, then chunk + look alternating, the sync, the hand-out
    assert st.log[:2] == ["pick", "look"] and st.log[-2:] == ["sync", "hand_out"]
    body = st.log[2:-2]
    assert body[0::2] == sizes and body[1::2] == ["look"] * len(sizes)


def test_runner_with_a_stop_and_one_token():
    st = State(max_steps=1, eos_id=EOS, finish=0, steps_run=1)
    run_generation(st, 1, *st.callables())
    assert st.log == ["pick", "sync", "hand_out"]


# ------------------------------------------------------------------------------------------------ the hand-out
def test_hand_out_without_a_stop():
    st = State(B=3, max_steps=8, V=5)
    tok, lp, la = hand_out(st)
    assert tok.dtype == torch.int64 and torch.equal(tok, st.tokens_out.long())
    assert lp is st.logprob
    assert la.shape == (3, 8, 5) and torch.equal(la, st._record.transpose(0, 1))
    tok, lp, la = hand_out(State(keep_logits=False))
    assert la is None and tok.shape == (2, 8)


def test_hand_out_with_a_stop():
    st = State(B=3, max_steps=8, V=5, eos_id=EOS, steps_run=3)
    tok, lp, la = hand_out(st)
    assert tok.dtype == torch.int64 and torch.equal(tok[:, :3], st.tokens_out[:, :3].long()) and bool((tok[:, 3:] == EOS).all())
    assert lp is st.logprob
    assert la.shape == (3, 3, 5) and torch.equal(la, st._record.transpose(0, 1)[:, :3])
    assert int(st.tokens_out[0, 3]) != EOS                             # (the state itself is left as it was)


# ------------------------------------------------------------------------------------------------ the variates
def test_variates_drawn():
    torch.manual_seed(3)
    u = sampling_variates(None, 4, 2, "cpu")
    torch.manual_seed(3)
    assert u.dtype == torch.float32 and u.shape == (8,) and torch.equal(u, torch.rand(8, dtype=torch.float32))      # ONE draw of that size


def test_variates_given():
    given = torch.rand(6, 2, dtype=torch.float64)[:, 0]                # float64, not contiguous
    assert not given.is_contiguous()
    for max_len, B in ((3, 2), (2, 2), (5, 1)):                        # exactly as many, and more
        u = sampling_variates(given, max_len, B, "cpu")
        assert u.dtype == torch.float32 and u.is_contiguous() and torch.equal(u, given.float())
    with pytest.raises(ValueError, match=r"\b7 uniform variates\b.*\b8\b"):
        sampling_variates(torch.rand(7), 4, 2, "cpu")


# ------------------------------------------------------------------------------------------------ the parent chain
@pytest.mark.parametrize("steps", [1, 2, 7])
def test_parent_index_against_reindexing_the_history_every_step(steps):
    BB, V = 6, 5
    g = torch.Generator().manual_seed(steps)
    anc = torch.randint(0, BB, (steps, BB), generator=g, dtype=torch.int32)
    rec = torch.randn(steps, BB, V, generator=g)
    # the reference's way (the host loop of _generate_beam_search_f32: `rec[g0:g1] = rec[parents]`): after every step the whole history,
    # the step's own record included, follows the step's parents
    hist = rec[:0]
    for s in range(steps):
        hist = torch.cat([hist, rec[s:s + 1]])[:, anc[s].long()]
    idx = beam_parent_index(anc)
    assert idx.shape == (steps, BB) and idx.dtype == torch.int64
    assert torch.equal(rec.gather(1, idx[:, :, None].expand(steps, BB, V)), hist)


# ------------------------------------------------------------------------------------------------ the beam look loop
class Beams:
    """`done` scripted: up once `raised_at` steps are enqueued; every read is recorded with the step it happened at"""

    def __init__(self, raised_at=None):
        self.raised_at, self.i, self.reads, self.offered = raised_at, 1, [], []

    @property
    def done(self):
        self.reads.append(self.i)
        return self.raised_at is not None and self.i > self.raised_at

    def advance(self, take):
        def advance(i, n_max):
            assert i == self.i
            self.offered.append(n_max)
            n = take(n_max)
            self.i += n
            return n
        return advance


def test_beam_loop_chunks_and_looks():
    bs = Beams()
    assert beam_steps_until_done(bs, 30, bs.advance(lambda n: n)) == 30
    assert bs.offered == [7, 8, 8, 6] and bs.reads == [8, 16, 24]
    bs = Beams()
    assert beam_steps_until_done(bs, 16, bs.advance(lambda n: n)) == 16
    assert bs.offered == [7, 8] and bs.reads == [8]                    # (no look at max_len itself)


def test_beam_loop_one_step_at_a_time():
    bs = Beams()
    assert beam_steps_until_done(bs, 20, bs.advance(lambda n: 1)) == 20
    assert bs.offered == [7, 6, 5, 4, 3, 2, 1, 8, 7, 6, 5, 4, 3, 2, 1, 4, 3, 2, 1] and bs.reads == [8, 16]


@pytest.mark.parametrize("take", [lambda n: n, lambda n: 1])
def test_beam_loop_ends_at_the_look_behind_the_flag(take):
    bs = Beams(raised_at=3)
    assert beam_steps_until_done(bs, 30, bs.advance(take)) == 8 and bs.reads == [8]
    bs = Beams(raised_at=3)
    assert beam_steps_until_done(bs, 5, bs.advance(take)) == 5 and bs.reads == []
    bs = Beams(raised_at=8)                                            # raised by a step of the second chunk: seen at 16
    assert beam_steps_until_done(bs, 30, bs.advance(take)) == 16 and bs.reads == [8, 16]


def test_beam_loop_of_one_step_runs_nothing():
    bs = Beams()
    assert beam_steps_until_done(bs, 1, bs.advance(lambda n: n)) == 1 and bs.offered == [] and bs.reads == []
