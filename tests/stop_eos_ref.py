"""The EOS stop of the greedy and sampling picks (include/pcy.h, the trailing fields of pcy_gen_state) restated in plain
Python on a table of what the picks WITHOUT a stop would emit.

    tokens [steps][B]   token row b would pick at step s (its selection does not depend on the other rows)
    gains  [steps][B]   the log-probability increment of that pick (optional; any numbers)

Rules: an unfinished row emits its token and adds its gain, and is finished from the next step on when the token is eos_id; a finished row
emits eos_id and adds nothing; the step in which the last unfinished row of [0, B) finishes raises `done`; a step behind `done` changes
nothing.  Rows that are finished before the first step (`finished0`) never emit a token of their own.
"""


def stop_eos(tokens, eos_id, gains=None, finished0=None):
    """-> dict(tokens [steps_run][B], logprob [B] (python floats added in step order; None without gains), finished [B] bools,
    done (bool), steps_run (the steps whose picks changed anything == the step that raised done + 1, or len(tokens) when none did),
    done_step (index of the step that raised done, None when none did))"""
    steps = len(tokens)
    B = len(tokens[0]) if steps else (len(finished0) if finished0 is not None else 0)
    fin = [bool(f) for f in finished0] if finished0 is not None else [False] * B
    lp = [0.0] * B if gains is not None else None
    out, done, done_step = [], False, None
    for s in range(steps):
        if done:
            break
        row = []
        for b in range(B):
            if fin[b]:
                row.append(eos_id)
                continue
            t = tokens[s][b]
            row.append(t)
            if lp is not None:
                lp[b] += gains[s][b]
            if t == eos_id:
                fin[b] = True
        out.append(row)
        if all(fin):
            done, done_step = True, s
    return dict(tokens=out, logprob=lp, finished=fin, done=done, steps_run=len(out), done_step=done_step)


def padded_tokens(ref, eos_id, max_len):
    """[B][max_len]: what a driver hands out -- the rows of `ref` transposed, eos_id in every slot behind steps_run"""
    B = len(ref["finished"])
    return [[ref["tokens"][s][b] if s < ref["steps_run"] else eos_id for s in range(max_len)] for b in range(B)]


def first_eos(row, eos_id):
    """index of the first eos_id in a token row, None when it holds none"""
    for i, t in enumerate(row):
        if t == eos_id:
            return i
    return None


def enqueued_bound(done_step, chunk):
    """decode steps a chunked driver may have enqueued when `done` was raised by the pick of generated token `done_step` (token 0 comes from
    the prefill's logits and costs no decode step): the flag of a chunk is read after the NEXT chunk was enqueued, so at most the rest of the
    finishing chunk and one more chunk -- 2 * chunk - 1 steps behind the finishing one"""
    return done_step + 2 * chunk - 1
