"""CPU: the host twins of greedy decoding with lookahead (procyon_amd.engine.lookup_draft / lookahead_passes; the device side is held to them
in tests/test_gpu_lookahead.py) on hand-made histories, and the binding of the new entry points."""
import math

import pytest

from procyon_amd.engine import lookahead_passes, lookup_draft

# (history, window, ngram_max, ngram_min, expected drafts, what the case is about): shared with the GPU operator test
DRAFT_CASES = [
    # the 3-gram (1 2 3) occurs early, the 1-gram (3) again later: the longest n-gram wins over the more recent shorter one
    ([1, 2, 3, 7, 8, 9, 3, 5, 1, 2, 3], 4, 3, 1, [7, 8, 9], "longest wins"),
    # (1 2) occurs at 0 and at 4: the most recent occurrence wins among equal lengths
    ([1, 2, 7, 7, 1, 2, 8, 8, 1, 2], 3, 2, 1, [8, 8], "most recent wins"),
    # the continuation runs into the end of the history: filled up with the filler h[n-1]
    ([5, 6, 9, 5, 6], 5, 2, 1, [9, 5, 6, 6], "runs into the end"),
    # ... or into a negative entry
    ([5, 6, 9, -1, 4, 4, 5, 6], 5, 2, 1, [9, 6, 6, 6], "runs into a negative entry"),
    # negative entries never match: the suffix (-1 3) is skipped as a 2-gram, the 1-gram (3) matches at 1
    ([-1, 3, 8, -1, 3], 3, 2, 1, [8, 3], "negative suffix entry"),
    # ... and a negative entry inside the history never equals a token: (2 -1) is no occurrence of (2 4)
    ([2, -1, 9, 2, 4, 7, 2, 4], 2, 2, 2, [7], "window 2"),
    ([1, 2, 3, 4, 5], 4, 3, 1, [5, 5, 5], "no match: all filler"),
    ([7], 3, 3, 1, [7, 7], "a history of one token"),
    # the match may overlap the suffix: i + g < n is all that is asked
    ([4, 4, 4, 4], 3, 3, 1, [4, 4], "overlapping match"),
    ([9, 1, 2, 3, 1, 2], 2, 3, 1, [3], "window 2 takes one draft"),
]


@pytest.mark.parametrize("case", DRAFT_CASES, ids=lambda c: c[5].replace(" ", "_"))
def test_lookup_draft(case):
    hist, W, gmax, gmin, want, _ = case
    got = lookup_draft(hist, W, gmax, gmin)
    assert got == want and len(got) == W - 1


def test_lookup_draft_most_recent_is_the_largest_start():
    # three occurrences of (1 2); the drafts come from behind the last one that is not the suffix itself
    assert lookup_draft([1, 2, 10, 1, 2, 20, 1, 2, 30, 1, 2], 2, 2, 2) == [30]


def test_lookup_draft_argument_errors():
    with pytest.raises(ValueError):
        lookup_draft([], 4, 3, 1)
    with pytest.raises(ValueError):
        lookup_draft([1, 2], 1, 3, 1)


@pytest.mark.parametrize("W", [2, 4, 5, 8])
@pytest.mark.parametrize("max_len", [1, 2, 12, 24])
def test_passes_all_right_and_all_wrong(W, max_len):
    toks = [(7 * i + 3) % 50 for i in range(max_len)]
    prompt = [60, 61, 62]
    right = [-1] + toks[1:]
    p, acc = lookahead_passes(toks, prompt, W, (3, 1), forced=right)
    assert p == math.ceil((max_len - 1) / W)
    assert sum((k + 1) * a for k, a in enumerate(acc)) == max_len - 1 and sum(acc) == p
    wrong = [(t + 1) % 50 for t in toks]
    p, acc = lookahead_passes(toks, prompt, W, (3, 1), forced=wrong)
    assert p == max_len - 1 and acc == [max_len - 1] + [0] * (W - 1)


def test_passes_known_pattern():
    # the prompt holds (1 2 3 4 5 6); the text repeats it.  Token 0 = 1 comes from the prefill.  Window 4, 1-grams only:
    #   pass 1: hist ...6 | 1      -> (1) found at 0, drafts 2 3 4: all right, commits 2 3 4 5
    #   pass 2: hist ... 1 2 3 4 5 -> (5) found at 4, drafts 6 1 2: 6 right, then the text says 9: commits 6 9
    #   pass 3: hist ... 6 9       -> (9) nowhere: filler 9 9 9, the text says 1: commits 1
    #   pass 4: hist ... 9 1       -> (1) most recent at 6, drafts 2 3 4: the text ends with 2: commits 2 (clamped)
    prompt, toks = [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6, 9, 1, 2]
    p, acc = lookahead_passes(toks, prompt, 4, (1, 1))
    assert (p, acc) == (4, [2, 1, 0, 1])
    # the same with the third pass's drafts dictated: forced[7] = 1 and forced[8] = 2 are right -> it commits 1 2 and the text is complete
    p, acc = lookahead_passes(toks, prompt, 4, (1, 1), forced=[-1] * 7 + [1, 2])
    assert (p, acc) == (3, [0, 2, 0, 1])


def test_new_entry_points_are_bound():
    from procyon_amd import _lib
    for name in ("pcy_look_draft", "pcy_look_verify", "pcy_debug_look_count"):
        assert name in _lib.SIGNATURES
    assert _lib.ABI_VERSION == 13 and len([k for k in vars(_lib) if k.startswith("DISPATCH_") and isinstance(getattr(_lib, k), int)]) == 20
    want = ["hist", "n_hist", "window", "forced", "counters", "last", "cap", "W", "ngram_max", "ngram_min"]
    assert [f[0] for f in _lib.LookState._fields_] == want
