"""What the full-depth GPU tests of the two decoders share (tests/test_gpu_fulldepth.py: Llama-3-8B geometry; tests/test_gpu_fulldepth_split.py:
Llama-2-7B geometry): the teacher-forced runs, the comparison against a fixture's bf16 oracle and fp32 truth at the project's bars, and the
decode-step dispatch counters (`served_by`) with which a test asserts WHICH decode step it compared; and `check_oracle`, the two-layer
oracle comparison on sampled rows of a ragged batch with the clean decode mask (tests/test_gpu_decode_wide.py, tests/test_gpu_decode_mask.py).
Not a test module."""
from contextlib import contextmanager

import torch

from conftest import record_parity, rel_err

SLACK = 1.25


def decode_counts():
    """decode steps enqueued so far, by what served them (pcy_debug_dispatch_count, procyon_amd/_lib.py DISPATCH_DECODE): step_gqa / step_mha
    (one row, all layers in one launch), layer (one row, a launch per layer), step_nb / step_mb (small- / mid-batch step), loop_stream /
    loop_mfma (launch per stage).  One count per step that passes through the engine's enqueue -- an eager step, or the CAPTURE of a graph;
    a replayed graph counts nothing."""
    from procyon_amd import _lib as L
    lib = L.load()
    return {k: int(lib.pcy_debug_dispatch_count(v)) for k, v in L.DISPATCH_DECODE.items()}


@contextmanager
def served_by(kind, steps=None):
    """Around EAGER decode steps: exactly `steps` of them were served by `kind` and none by anything else -- a fused step that declines at
    launch time (LDS size for the cache length, co-residency, a missing buffer) falls back to the launches with the same bits, and a
    bit-identity test would then compare the launches with themselves.  steps = None (runs that replay a captured graph: only the capture
    counts): any number by `kind`, still none by anything else.  Yields the dict that holds the deltas afterwards."""
    before, delta = decode_counts(), {}
    yield delta
    after = decode_counts()
    delta.update({k: after[k] - before[k] for k in after})
    others = {k: v for k, v in delta.items() if k != kind and v}
    assert not others, f"decode steps expected on '{kind}' were served by {others} ({delta[kind]} by '{kind}')"
    if steps is not None:
        assert delta[kind] == steps, f"{delta[kind]} of {steps} decode steps were served by '{kind}'"


def llama_steps(eng, g, T, vocab):
    """prefill + teacher-forced cached decode steps on the fixture's tokens -> logits [nstep, V] fp32 (CPU), prefill hidden row"""
    from procyon_amd.engine import GenState
    ids, toks = g["ids"].long(), g["tokens"].long()
    nstep = toks.numel()                          # prefill + the cached decode steps
    cache = eng.new_cache(1, T + nstep + 1)
    logits, hidden = eng.prefill(eng.embed_tokens(ids), None, cache, "last", want_hidden=True)
    got = [logits[0].cpu()]
    st = GenState(1, vocab, nstep + 1, "cuda")
    for s in range(1, nstep):                     # teacher-forced on the bf16 oracle's greedy tokens
        st.pos.fill_(T + s - 1)
        st.next_tok.copy_(toks[s - 1:s].to(torch.int32))
        eng.decode(cache, st, 1)
        got.append(st.logits[0].cpu())
    return torch.stack(got).float(), hidden[0, -1].cpu().float()



def llama_stats(got, g):
    """per-step errors and agreement counts of HIP logits [65, V] against the fixture's bf16 oracle and fp32 truth (column subset)"""
    cols = g["cols"].long()
    truth, ref = g["logits_fp32"], g["logits_bf16"].float()
    nstep = got.shape[0]
    out = dict(nstep=nstep, e_hip_truth=[], e_ref_truth=[], e_hip_ref=[], agree_hip_truth=0, agree_ref_truth=0, agree_hip_ref=0, rows=[])
    for s in range(nstep):
        out["e_hip_truth"].append(rel_err(got[s, cols], truth[s]))
        out["e_ref_truth"].append(rel_err(ref[s], truth[s]))
        out["e_hip_ref"].append(rel_err(got[s, cols], ref[s]))
        am, am_t, am_r = int(got[s].argmax()), int(g["top_ids_fp32"][s, 0]), int(g["top_ids_bf16"][s, 0])
        out["agree_hip_truth"] += am == am_t
        out["agree_ref_truth"] += am_r == am_t
        out["agree_hip_ref"] += am == am_r
        out["rows"].append((am, am_t, am_r, float(g["top_vals_fp32"][s, 0] - g["top_vals_fp32"][s, 1])))
    return out



def margin_conditioned(st, g):
    """Steps whose fp32 top-2 margin exceeds 4 x the per-logit noise of the bf16 pipeline (rms over the fixture's columns of
    oracle_bf16 - fp32 at that step): there two bf16 implementations MUST pick the same token (a flip needs a 2.8-sigma event on the
    difference of two logit errors).  Returns (n_clear, n_clear_agree_hip_oracle, n_clear_agree_hip_fp32)."""
    truth, ref = g["logits_fp32"], g["logits_bf16"].float()
    clear = agree_o = agree_t = 0
    for s_, (am, am_t, am_r, margin) in enumerate(st["rows"]):
        noise = float((ref[s_] - truth[s_]).pow(2).mean().sqrt())
        if margin >= 4.0 * noise:
            clear += 1
            agree_o += am == am_r
            agree_t += am == am_t
    return clear, agree_o, agree_t



def rows_compat_run(llama, ids, mask, toks, rows, teacher, vocab, keep_rows=None, copy_of=None):
    """prefill (left-padded rows, compat mode) + teacher-forced cached steps of a B-row batch; rows in `teacher` are fed the fixture's tokens
    (toks [nstep, len(teacher)]), every other row its own argmax.  -> logits [nstep, B, V] fp32 (CPU); with `keep_rows` only those rows
    [nstep, len(keep_rows), V] (the argmax of the others is taken on the device).  `copy_of` [B] (rows holding the same prompt and the same
    tokens): the logits of every step and the whole K / V cache of row b must be BIT-identical to those of row copy_of[b] (checked on the device)."""
    from procyon_amd.engine import GenState
    B, T = ids.shape
    nstep = toks.shape[0]
    cache = llama.new_cache(B, T + nstep + 1)
    logits, _ = llama.prefill(llama.embed_tokens(ids), mask, cache, "last")
    ksel = None if keep_rows is None else torch.tensor(keep_rows, device=logits.device)
    csel = None if copy_of is None else torch.tensor(copy_of, device=logits.device)
    host = lambda lg: lg.float().cpu() if ksel is None else lg[ksel].float().cpu()
    same = lambda lg: csel is None or torch.equal(lg, lg[csel])
    assert same(logits), "prefill logits of copies differ"
    got = [host(logits)]
    st = GenState(B, vocab, nstep + 1, "cuda")            # keep = None: compat mode (every cached slot is attended)
    tsel = torch.tensor(teacher)
    for s in range(1, nstep):
        if ksel is None:
            nxt = got[-1].argmax(-1).to(torch.int32)
        else:
            nxt = (logits if s == 1 else st.logits).float().argmax(-1).cpu().to(torch.int32)
        nxt[tsel] = toks[s - 1].to(torch.int32)
        st.pos.fill_(T + s - 1)
        st.next_tok.copy_(nxt)
        llama.decode(cache, st, B)
        assert same(st.logits), f"step {s}: logits of copies differ"
        got.append(host(st.logits))
    if csel is not None:
        assert torch.equal(cache.k, cache.k[:, csel]) and torch.equal(cache.v, cache.v[:, csel]), "K / V rows of copies differ"
    return torch.stack(got)



def rows_compat_check(name, got, g, sel, min_clear, **extra):
    """got [nstep, n, V] (the fixture's rows `sel` of the batch) against the fixture's bf16 oracle and fp32 truth: per (row, step) the truth
    distance bar, argmax on every clear-margin (row, step), agreement rates; one PARITY record."""
    allcols = g["cols"].long()
    nstep = got.shape[0]
    e_ht, e_rt, e_hr, clear, clear_ok, agree_hr, agree_rt = [], [], [], 0, 0, 0, 0
    for s in range(nstep):
        for j, b in enumerate(sel):
            cols = allcols if allcols.dim() == 1 else allcols[b]     # (a fixture may keep its own column subset for every row: cols [B, C])
            truth, ref = g["logits_fp32"][s, b], g["logits_bf16"][s, b].float()
            e_ht.append(rel_err(got[s, j, cols], truth)); e_rt.append(rel_err(ref, truth)); e_hr.append(rel_err(got[s, j, cols], ref))
            am, am_t, am_r = int(got[s, j].argmax()), int(g["top_ids_fp32"][s, b, 0]), int(g["top_ids_bf16"][s, b, 0])
            agree_hr += am == am_r
            agree_rt += am_r == am_t
            noise = float((ref - truth).pow(2).mean().sqrt())
            if float(g["top_vals_fp32"][s, b, 0] - g["top_vals_fp32"][s, b, 1]) >= 4.0 * noise:
                clear += 1
                clear_ok += (am == am_r) and (am == am_t)
    mean = lambda v: sum(v) / len(v)
    record_parity(name, rows_x_steps=len(e_ht), err_hip_fp32_mean=mean(e_ht), err_oracle_fp32_mean=mean(e_rt), err_hip_oracle_mean=mean(e_hr),
                  err_hip_oracle_max=max(e_hr), worst_ratio_hip_over_oracle=max(a / b for a, b in zip(e_ht, e_rt)), agree_hip_oracle=agree_hr,
                  agree_oracle_fp32=agree_rt, clear_margin=clear, clear_agree=clear_ok, **extra)
    for a, b in zip(e_ht, e_rt):
        assert a <= SLACK * b, (a, b)
    assert clear >= min_clear and clear_ok == clear, (clear, clear_ok)
    assert agree_hr >= agree_rt - max(2, len(e_ht) // 32), (agree_hr, agree_rt)
    assert max(e_hr) < 0.15        # a wrong position / a dropped pad slot / a stale hand-over gives O(1)



def check_oracle(sd, kw, emb, mask, got, rows, what, n_steps):
    """prefill + the HIP greedy tokens teacher-forced through the oracle on `rows` alone (clean decode mask); per (row, step) rel. err < 2e-2,
    and the HIP token is the oracle's argmax except on a near-tie (top-2 margin inside 4 x the logit noise of that row and step).
    `got`: the sampled rows' logits [n_steps + 1, len(rows), V] and tokens [len(rows), n_steps + 1] on the CPU.  -> the worst rel. err."""
    from oracle import llama_ref as LR
    geom = LR.LlamaGeom(**kw, max_pos=512)
    m = mask[rows]
    r = LR.llama_forward(sd, geom, inputs_embeds=emb[rows], attn_mask=m, logits_rows="last")
    tok = got["tokens"]
    worst = 0.0
    for s_ in range(n_steps + 1):
        if s_:
            m = torch.cat([m, torch.ones(len(rows), 1)], 1)
            r = LR.llama_forward(sd, geom, input_ids=tok[:, s_ - 1:s_].long(), attn_mask=m, past_kv=past, logits_rows="last")
        past = r["past_kv"]
        ref = r["logits"][:, -1].float()
        for j, b in enumerate(rows):
            hip = got["logits"][s_, j].float()
            worst = max(worst, rel_err(hip, ref[j]))
            assert rel_err(hip, ref[j]) < 2e-2, (what, b, s_, rel_err(hip, ref[j]))
            if int(tok[j, s_]) != int(ref[j].argmax()):
                top2 = ref[j].topk(2).values
                assert float(top2[0] - top2[1]) <= 4 * float((hip - ref[j]).abs().max()), (what, b, s_)
    return worst
