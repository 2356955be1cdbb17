"""beam_cache_plan (procyon_amd/engine.py): the rule that decides whether the beams of a prompt share ONE copy of its K / V (a KVCache with a
prefix) and the slot counts of the two layouts; the names it is given (disabled_switches) and the decode state a beam search runs on
(BeamState.gen_state).  Pure arithmetic and descriptors, no GPU."""
import pytest

from procyon_amd.engine import BeamState, beam_cache_plan, disabled_switches

SWITCHES = ("beam_kv_shared", "beam_prefill_once", "beam_kv_suffix")


@pytest.mark.parametrize("B,beam,shared", [
    (1, 1, False), (4, 1, False), (16, 1, False), (40, 1, False),      # beam 1: nothing to share, whatever the row count
    (1, 5, False), (1, 8, False), (2, 4, False),                       # <= 8 rows: the small-batch step's range (PCY_NB_MAX clamps at 8)
    (1, 10, True), (4, 10, True), (16, 10, True), (1, 9, True), (3, 3, True), (1, 20, True),
])
def test_beam_cache_plan_truth_table(B, beam, shared):
    assert beam_cache_plan(B, beam, 512, 64, ())["shared"] is shared
    assert beam_cache_plan(B, beam, 512, 64, ["attn_o", "beam_graph", ""])["shared"] is shared      # other names do not matter


@pytest.mark.parametrize("name", SWITCHES)
def test_each_switch_turns_the_shared_cache_off(name):
    for B, beam in ((1, 10), (4, 10), (16, 10)):
        assert beam_cache_plan(B, beam, 704, 64, ())["shared"] is True
        assert beam_cache_plan(B, beam, 704, 64, [name])["shared"] is False
        assert beam_cache_plan(B, beam, 704, 64, ["beam_graph", name])["shared"] is False
        assert beam_cache_plan(B, beam, 704, 64, name.split(","))["shared"] is False
    assert beam_cache_plan(4, 10, 704, 64, ["x" + name, name + "x"])["shared"] is True      # whole names only


@pytest.mark.parametrize("B,beam,T,max_new", [(1, 10, 512, 64), (16, 10, 704, 64), (1, 20, 704, 128), (4, 10, 21, 8), (1, 5, 100, 32)])
def test_beam_cache_plan_slot_counts(B, beam, T, max_new):
    """slots per layer and kv head: B*T + B*beam*max_new shared against B*beam*(T + max_new) plain -- reported for both layouts whatever the
    decision, so that a caller can print the saving it gives up"""
    p = beam_cache_plan(B, beam, T, max_new, ())
    assert p["rows"] == B * beam and p["prefix_rows"] == B and p["prefix_slots"] == T and p["suffix_slots"] == max_new
    assert p["slots_shared"] == B * T + B * beam * max_new
    assert p["slots_plain"] == B * beam * (T + max_new)
    assert p["slots_plain"] - p["slots_shared"] == B * (beam - 1) * T
    assert p["slots_shared"] <= p["slots_plain"]


def test_evaluation_default_saving():
    """16 prompts x beam 10 on ProCyon-Split (32 layers, 32 kv heads of 128, T = 704, 64 new tokens): 64 GB of K + V plain, 59 GB of it the
    prompts' rows ten times over; shared, the prompts' rows exist once: 11 GB"""
    p = beam_cache_plan(16, 10, 704, 64, ())
    per_slot = 2 * 32 * 32 * 128 * 2          # K and V, layers, kv heads, head_dim, bf16
    assert p["shared"]
    assert round(p["slots_plain"] * per_slot / 1e9) == 64
    assert round(160 * 704 * per_slot / 1e9) == 59
    assert round(p["slots_shared"] * per_slot / 1e9) == 11


def test_gen_state_of_a_beam_state_is_built_on_its_arrays():
    """the decode step reads the position and the next tokens where the beam step writes them: same tensors, same addresses in the descriptor"""
    bs = BeamState(2, 3, 4, 7, prompt_len=5, device="cpu")
    gs = bs.gen_state(11)
    assert gs.pos is bs.pos and gs.next_tok is bs.next_tok and gs.pos.data_ptr() == bs.pos.data_ptr() and gs.next_tok.data_ptr() == bs.next_tok.data_ptr()
    assert gs.c.pos == bs.pos.data_ptr() == bs.c.pos and gs.c.next_tok == bs.next_tok.data_ptr() == bs.c.next_tok
    assert gs.logits.shape == (6, 11) and gs.c.max_steps == 1 and gs.tokens_out.shape == (6, 1)
    assert gs.c.logits_all_ld == 11 and not gs.c.logits_all and not gs.c.keep and int(gs.pos) == 5


def test_disabled_switches(monkeypatch):
    monkeypatch.delenv("PCY_DISABLE", raising=False)
    assert disabled_switches() == frozenset()
    monkeypatch.setenv("PCY_DISABLE", "a,,b , a")
    assert disabled_switches() == {"a", "b"} and isinstance(disabled_switches(), frozenset)
    monkeypatch.setenv("PCY_DISABLE", "xbeam_graph")
    assert "beam_graph" not in disabled_switches()
