"""The decode key mask (`pcy_gen_state.keep`, [B, Tmax]: "clean" mode -- the left-pad slots of a ragged batch are not attended during the
cached steps) on EVERY decode path of the engine.  attn_args() hands `st->keep` to the attention of all of them and PcyMbArgs.keep carries
it into the mid-batch step; until this module only the launch-per-stage MFMA loop above 32 rows ran with a mask (tests/test_gpu_decode_wide.py).

Per (geometry, family of paths, batch, cache length) a left-padded ragged batch is prefilled with its mask and decoded for N cached greedy
steps with GenState(keep=keep), keep[:, :T] = mask, ones behind (what generate_greedy(clean_decode_mask=True) builds).  A family = the paths
that serve one batch size with ONE set of bits: the first is the default, the others its fused form / its launch-per-stage twins.  Held, for
every path of the family:
  (a) the dispatch counters: every eager step ran on the path the case names (served_by);
  (b) the oracle on sampled rows (fulldepth_common.check_oracle: teacher-forced on the HIP tokens, clean mask, rel. err < 2e-2) -- once per
      family on the first path, whose bits (c) pins on the others;
  (c) the same bits as the first path of the family, eager and replayed twice: logits of every step, tokens, log-probs, appended K / V;
  (d) on the unpadded batch, keep of all ones gives the bits of keep = None;
  (e) the one-pad row and the most padded row r give the bits they give in a batch of B copies of r (one mask row for every row: a mix-up
      of mask rows is invisible there and shows in the ragged batch).
Before the HIP result is looked at, the oracle ALONE says that the case can fail (the control): for every sampled row with an eighth or more
of its prompt padded, its compat-mode logits (no mask in the cached steps: the reference's quirk) lie 5 x the bar away from its clean-mode
logits at every cached step.  And once per geometry the HIP run with keep = None is itself beyond the bar from the clean oracle."""
import pytest
import torch

from conftest import pcy_disable, record_parity, rel_err
from fulldepth_common import check_oracle, served_by

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
GEOMS = {
    "full": dict(vocab=4096, d=4096, n_layers=2, n_heads=32, n_kv_heads=8, ffn=14336),        # Llama-3-8B (ProCyon-Full's decoder)
    "split": dict(vocab=2048, d=4096, n_layers=2, n_heads=32, n_kv_heads=32, ffn=11008),      # Llama-2-7B (ProCyon-Split's)
    "small": dict(vocab=128263 - 128000 + 2048, d=256, n_layers=2, n_heads=4, n_kv_heads=2, ffn=512),   # synthetic_model "small": no fused step
}
N = 3                      # cached decode steps per case
BAR = 2e-2                 # check_oracle's bar on the rel. error of a logits row
CONTROL = 5 * BAR          # ignoring the mask must move the oracle's logits by this much
XMIN = 384                 # PCY_AO_XMIN of the cases above the key-split threshold (T = 420)
ENV = ("PCY_NB_MAX", "PCY_MB_MAX", "PCY_AO_XMIN")


# ---------------------------------------------------------------------------------------------------------------- paths
def _family(geom, fam):
    """[(label, dispatch-counter kind, environment, PCY_DISABLE names)]: the first entry is the default of the batch size, the others give
    the same bits (procyon_amd/csrc/pcy_switch.h; plan_decode in pcy_engine.hip)."""
    nb, mb = {"PCY_NB_MAX": "8"}, {"PCY_MB_MAX": "32"}
    mfma = [("loop_mfma", "loop_mfma", {}, ()), ("loop_mfma/attn_qkv_finish off", "loop_mfma", {}, ("attn_qkv_finish",)),
            ("loop_mfma/finish_norm off", "loop_mfma", {}, ("finish_norm",))]
    step1 = "step_gqa" if geom == "full" else "step_mha"
    return {
        # one row: all layers in one launch; a launch per layer; launch per stage with the fused attention + o; with the plain attention
        "one": [(step1, step1, {}, ()), ("layer", "layer", {}, ("decode_step",)), ("loop_stream/attn_o", "loop_stream", {}, ("decode_layer",)),
                ("loop_stream/plain", "loop_stream", {}, ("attn_o",))],
        # 2..8 rows of the Llama-3-8B geometry: the small-batch step and its streaming twin
        "nb": [("step_nb", "step_nb", nb, ()), ("loop_stream/nb twin", "loop_stream", nb, ("decode_nb_step",))],
        # the MFMA loop (7..32 rows; from 4 rows on the other geometries) and its twins
        "mfma": mfma,
        # ... and 9..32 rows of the Llama-3-8B geometry on the opt-in mid-batch step
        "mb": mfma[:1] + [("step_mb", "step_mb", mb, ())] + mfma[1:],
        # no fused form: the streaming launches (2, 3 rows outside the Llama-3-8B geometry; one row of the small decoder, whose fused
        # launchers decline)
        "stream": [("loop_stream", "loop_stream", {}, ())],
        "stream1": [("loop_stream", "loop_stream", {}, ()), ("loop_stream/attn_o off", "loop_stream", {}, ("attn_o",))],
    }[fam]


# (geometry, family, B, T, layout of the pads)
CASES = []
for T_ in (24, 300):
    CASES += [("full", "one", 1, T_, "unpadded"), ("full", "one", 1, T_, "padded")]
    CASES += [("full", "nb", 2, T_, "a"), ("full", "nb", 2, T_, "b")] + [("full", "nb", B_, T_, "ragged") for B_ in (4, 5, 6, 8)]
    CASES += [("full", "mfma", 8, T_, "ragged")] + [("full", "mb", B_, T_, "ragged") for B_ in (10, 20, 32)]
    CASES += [("split", "one", 1, T_, "unpadded"), ("split", "one", 1, T_, "padded"), ("split", "stream", 2, T_, "a"), ("split", "stream", 2, T_, "b")]
    CASES += [("split", "mfma", B_, T_, "ragged") for B_ in (4, 10, 32)]
    CASES += [("small", "stream1", 1, T_, "padded"), ("small", "stream", 2, T_, "b"), ("small", "mfma", 5, T_, "ragged"), ("small", "mfma", 20, T_, "ragged")]
# above the key-split threshold (PCY_AO_XMIN = 384): the fused launches that split the keys and exchange the scores
CASES += [("full", "one", 1, 420, "unpadded"), ("full", "one", 1, 420, "padded"), ("split", "one", 1, 420, "unpadded"), ("split", "one", 1, 420, "padded"),
          ("full", "nb", 2, 420, "a"), ("full", "nb", 2, 420, "b"), ("full", "nb", 4, 420, "ragged"), ("full", "nb", 5, 420, "ragged")]


@pytest.fixture(scope="module")
def engines():
    """name -> (geometry, state dict, engine); built at first use, two layers each"""
    built = {}

    def get(name):
        if name not in built:
            from procyon_amd import synth
            from procyon_amd.engine import LlamaConfig, LlamaEngine
            kw = GEOMS[name]
            sd = synth.llama_state_dict(**kw)
            built[name] = (kw, sd, LlamaEngine(sd, LlamaConfig(**kw, max_pos=512)))
        return built[name]
    yield get
    built.clear()


# ---------------------------------------------------------------------------------------------------------------- inputs
def _pads(B, T, layout):
    """left-pad length of every row.  Batches of 4 and more: row 0 unpadded, row 1 ONE pad slot (an off-by-one in the slot index), row 2 the
    most padded (two thirds), the last row a sixth, the others up to a half -- at least two rows with an eighth or more (the control).  Two
    rows cannot hold all of that: layout "a" = (0, 1), layout "b" = two padded rows.  One row: unpadded, or a quarter padded."""
    if B == 1:
        return [0 if layout == "unpadded" else T // 4]
    if B == 2:
        return [0, 1] if layout == "a" else [T // 5 + 1, T // 2]
    pads = [0, 1, (2 * T) // 3] + [(b * 37) % (T // 2) for b in range(3, B)]
    pads[B - 1] = T // 6 + 1
    return pads


def _batch(B, T, d, layout, seed):
    g = torch.Generator().manual_seed(seed)
    emb = (torch.randn(B, T, d, generator=g) * 0.02).to(BF)
    pads = _pads(B, T, layout)
    mask = torch.ones(B, T)
    for b, p in enumerate(pads):
        mask[b, :p] = 0
    return emb, mask, pads


def _sampled(B, pads):
    """rows the oracle runs: all up to 5 rows; else row 0, the one-pad row, the most padded row, the last row"""
    return list(range(B)) if B <= 5 else sorted({0, pads.index(1), pads.index(max(pads)), B - 1})


# ---------------------------------------------------------------------------------------------------------------- oracle
def _oracle_chains(sd, kw, emb, mask, rows, tokens=None):
    """The oracle on `rows`: the masked prefill, then N cached steps twice from the same prefill -- clean (the mask grows by ones) and compat
    (attn_mask = None, the reference's quirk: the pad slots are attended), both fed `tokens` [n, >= N], or with tokens = None the clean
    chain's own greedy tokens.  -> clean, compat: logits [N + 1, n, V] fp32 (row 0, the prefill, is the same in both)."""
    from oracle import llama_ref as LR
    geom = LR.LlamaGeom(**kw, max_pos=512)
    m = mask[rows]
    r = LR.llama_forward(sd, geom, inputs_embeds=emb[rows], attn_mask=m, logits_rows="last")
    clean, compat = [r["logits"][:, -1].float()], [r["logits"][:, -1].float()]
    past_c = past_q = r["past_kv"]
    for s_ in range(N):
        tok = clean[-1].argmax(-1, keepdim=True) if tokens is None else tokens[:, s_:s_ + 1].long()
        m = torch.cat([m, torch.ones(len(rows), 1)], 1)
        rc = LR.llama_forward(sd, geom, input_ids=tok, attn_mask=m, past_kv=past_c, logits_rows="last")
        rq = LR.llama_forward(sd, geom, input_ids=tok, attn_mask=None, past_kv=past_q, logits_rows="last")
        past_c, past_q = rc["past_kv"], rq["past_kv"]
        clean.append(rc["logits"][:, -1].float()); compat.append(rq["logits"][:, -1].float())
    return torch.stack(clean), torch.stack(compat)


def _control(sd, kw, emb, mask, pads, rows, what):
    """The inputs can fail the case: on the oracle alone, every sampled row with an eighth or more of its prompt padded moves by CONTROL or
    more at every cached step when the mask is ignored.  -> the smallest distance seen (None: no such row)."""
    T = mask.shape[1]
    ctl = [b for b in rows if pads[b] * 8 >= T]
    if not ctl:
        return None
    clean, compat = _oracle_chains(sd, kw, emb, mask, ctl)
    dist = [rel_err(compat[s_, j], clean[s_, j]) for s_ in range(1, N + 1) for j in range(len(ctl))]
    print(f"control {what}: rows {ctl} pads {[pads[b] for b in ctl]}: compat vs clean, min over rows and steps {min(dist):.3f}")
    assert min(dist) >= CONTROL, (f"mis-built case {what}: ignoring the mask moves the oracle's logits of a padded row by {min(dist):.3f} only "
                                  f"(< {CONTROL}); lengthen the pads")
    return min(dist)


# ---------------------------------------------------------------------------------------------------------------- the HIP side
def _prefill(eng, emb, mask):
    """the masked prefill under the default switches -> (K, V, logits) of a cache with room for the N steps"""
    cache = eng.new_cache(emb.shape[0], emb.shape[1] + N + 2)
    logits, _ = eng.prefill(emb.cuda(), mask, cache, "last")
    return cache.k.clone(), cache.v.clone(), logits.clone()


def _copies(snap, r):
    """the post-prefill state of a batch made of copies of row r"""
    k, v, logits = snap
    B = logits.shape[0]
    return k[:, r:r + 1].expand(-1, B, -1, -1, -1).contiguous(), v[:, r:r + 1].expand(-1, B, -1, -1, -1).contiguous(), logits[r:r + 1].expand(B, -1).contiguous()


def _decode(monkeypatch, eng, V, snap, mask, keep, variant, xmin, use_graph):
    """N greedy cached steps from the post-prefill state `snap` on the path `variant` names.  keep: "mask" (keep[:, :T] = mask, ones behind),
    "ones" or None.  Every eager step must be served by the variant's kind (a replayed run: its capture).  -> dict of device tensors:
    logits [N + 1, n, V], tokens [n, N + 1], logprob [n], the appended K / V slots."""
    from procyon_amd.engine import Context, GenState
    label, kind, env, off = variant
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    if xmin:
        monkeypatch.setenv("PCY_AO_XMIN", str(xmin))
    pcy_disable(monkeypatch, *off)
    n, T = mask.shape
    Tmax = T + N + 2
    cache = eng.new_cache(n, Tmax)
    kp = None
    if keep is not None:
        kp = torch.ones(n, Tmax, dtype=torch.uint8, device="cuda")
        if keep == "mask":
            kp[:, :T] = mask.to("cuda", torch.uint8)
    st = GenState(n, V, N + 2, "cuda", keep=kp)
    cache.k.copy_(snap[0]); cache.v.copy_(snap[1])
    st.logits.copy_(snap[2]); st.pos.fill_(T)
    eng.pick(cache, st, n, advance_pos=False)
    lg = [snap[2].clone()]
    with served_by(kind, None if use_graph else N):
        for _ in range(N):
            eng.greedy_steps(cache, st, n, 1, use_graph=use_graph)
            lg.append(st.logits.clone())
    Context.get().sync()
    return dict(logits=torch.stack(lg), tokens=st.tokens_out[:, :N + 1].clone(), logprob=st.logprob.clone(),
                k=cache.k[:, :, :, T:T + N].clone(), v=cache.v[:, :, :, T:T + N].clone())


def _rows(out, rows):
    """the sampled rows of the logits and tokens, on the CPU"""
    r = torch.tensor(rows, device="cuda")
    return dict(logits=out["logits"][:, r].cpu(), tokens=out["tokens"][r].cpu())


def _same(a, b, what, row=None):
    sel = {"logits": lambda x: x[:, row], "tokens": lambda x: x[row], "logprob": lambda x: x[row], "k": lambda x: x[:, row], "v": lambda x: x[:, row]}
    for key in a:
        x, y = (a[key], b[key]) if row is None else (sel[key](a[key]), sel[key](b[key]))
        assert torch.equal(x, y), (what, key)


WORST = {}      # worst HIP-vs-oracle error per (geometry, path label), over the cases run so far -> the parity report


@pytest.mark.parametrize("geom,fam,B,T,layout", CASES)
def test_masked_decode_path(engines, monkeypatch, geom, fam, B, T, layout):
    """(a)-(e) of the module's docstring and the control, for every path of the family."""
    kw, sd, eng = engines(geom)
    V, xmin = kw["vocab"], XMIN if T > XMIN else 0
    what = (geom, fam, B, T, layout)
    emb, mask, pads = _batch(B, T, kw["d"], layout, seed=B * 1000 + T)
    rows = _sampled(B, pads)
    # the control, on the oracle alone and before any HIP result: ignoring the mask would be seen
    dist = _control(sd, kw, emb, mask, pads, rows, what)
    assert dist is not None or layout in ("unpadded", "a"), "every other layout has rows that carry the control"
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    pcy_disable(monkeypatch)
    snap = _prefill(eng, emb, mask)
    snap_ones = _prefill(eng, emb, torch.ones(B, T))                           # (d): the same batch unpadded
    e_rows = sorted({b for b in range(B) if pads[b] == 1} | {pads.index(max(pads))}) if B > 1 else []
    ref = None
    for variant in _family(geom, fam):
        label = variant[0]
        run = lambda snap_, mask_, keep, use_graph=False: _decode(monkeypatch, eng, V, snap_, mask_, keep, variant, xmin, use_graph)
        out = run(snap, mask, "mask")                                          # (a) inside: served_by
        assert torch.isfinite(out["logits"].float()).all(), (what, label)
        if ref is not None:                                                    # (c) the bits of the family's first path
            _same(out, ref, what + (label, "twin"))
        # (e) a row takes ITS row of the mask: the same bits as in a batch of copies of it  (the exact checks come before the oracle: they
        # name what is wrong, e.g. a mix-up of mask rows, where the oracle only says that something is)
        for r in e_rows:
            cp = run(_copies(snap, r), mask[r:r + 1].expand(B, -1).contiguous(), "mask")
            _same(out, cp, what + (label, "row vs its copies", r), row=r)
        # (d) all ones == no mask
        _same(run(snap_ones, torch.ones(B, T), "ones"), run(snap_ones, torch.ones(B, T), None), what + (label, "all ones vs None"))
        for i in range(2):                                                     # (c) replayed, twice: the second starts from the tag / flag state of the first
            _same(run(snap, mask, "mask", use_graph=True), out, what + (label, "replay", i))
        if ref is None:                                                        # (b) the oracle, on the first path of the family -- whose bits (c) pins on the others
            ref = out
            worst = check_oracle(sd, kw, emb, mask, _rows(out, rows), rows, what + (label,), N)
        key = f"decode_mask/{geom}/{label}"
        w = WORST.setdefault(key, dict(err_hip_oracle_max=0.0, cases=0, control_min=None))
        w["err_hip_oracle_max"] = max(w["err_hip_oracle_max"], worst)
        w["cases"] += 1
        if dist is not None:
            w["control_min"] = dist if w["control_min"] is None else min(w["control_min"], dist)
        record_parity(key, **w)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_dropping_the_mask_on_the_hip_side_is_beyond_the_bar(engines, monkeypatch, geom):
    """The other half of the control: the HIP run of a ragged batch with keep = None (every cached slot attended) is farther than the bar
    from the CLEAN oracle on every padded row and cached step -- the mask handed to the HIP path does something, and (b) would see it gone.
    (Teacher-forced on this run's own tokens.  The default path of 4 rows: step_nb / loop_mfma / loop_mfma.)"""
    kw, sd, eng = engines(geom)
    B, T = 4, 24
    emb, mask, pads = _batch(B, T, kw["d"], "ragged", seed=77)
    for var in ENV:
        monkeypatch.delenv(var, raising=False)
    pcy_disable(monkeypatch)
    variant = ("step_nb", "step_nb", {}, ()) if geom == "full" else _family(geom, "mfma")[0]      # (4 rows: inside the default PCY_NB_MAX)
    out = _decode(monkeypatch, eng, kw["vocab"], _prefill(eng, emb, mask), mask, None, variant, 0, False)
    padded = [b for b in range(B) if pads[b] * 8 >= T]
    assert len(padded) >= 2
    got = _rows(out, padded)
    clean, _ = _oracle_chains(sd, kw, emb, mask, padded, tokens=got["tokens"])
    for j, b in enumerate(padded):
        assert rel_err(got["logits"][0, j], clean[0, j]) < BAR, (geom, b, "prefill")
        for s_ in range(1, N + 1):
            e = rel_err(got["logits"][s_, j], clean[s_, j])
            print(f"{geom} row {b} ({pads[b]} pads of {T}) step {s_}: HIP without the mask vs clean oracle {e:.3f}")
            assert e > BAR, (geom, b, s_, e)


def test_generate_greedy_clean_mask_matches_oracle(engines):
    """`LlamaEngine.generate_greedy(clean_decode_mask=True)` end to end against `oracle.llama_ref.greedy_generate(clean_decode_mask=True)` on
    the small decoder, 3 ragged rows (0, 1 and 7 pads of 20), free running: tokens equal up to a near-tie of the oracle, per-step logits at
    the bar of test_llama_greedy_matches_oracle (tests/test_gpu_models.py), which holds the compat form of the call; replay == eager."""
    from oracle import llama_ref as LR
    kw, sd, eng = engines("small")
    geom = LR.LlamaGeom(**kw, max_pos=512)
    B, T, L_ = 3, 20, 16
    emb = (torch.randn(B, T, kw["d"], generator=torch.Generator().manual_seed(13)) * 0.05).to(BF)
    mask = torch.ones(B, T)
    mask[1, :1] = 0
    mask[2, :7] = 0
    tok_ref, lg_ref, lp_ref = LR.greedy_generate(sd, geom, emb, mask, L_, clean_decode_mask=True)
    _, lg_compat, _ = LR.greedy_generate(sd, geom, emb, mask, L_, clean_decode_mask=False)
    assert rel_err(lg_compat[2, 1], lg_ref[2, 1]) >= CONTROL      # (the control: the compat form of the call is another result)
    tok, lp, lg, _ = eng.generate_greedy(emb.cuda(), mask, L_, keep_logits=True, clean_decode_mask=True, use_graph=False)
    tok2, _, _, _ = eng.generate_greedy(emb.cuda(), mask, L_, keep_logits=False, clean_decode_mask=True, use_graph=True)
    assert torch.equal(tok.cpu(), tok2.cpu()), "graph replay differs from eager launches"
    tok, lg = tok.cpu(), lg.cpu()
    for b in range(B):
        for s_ in range(L_):
            # (the same tokens up to here: comparable logits.  The bar comes BEFORE the near-tie rule: logits of a run that ignores the mask are
            # so far off that their "noise" would excuse any token)
            assert rel_err(lg[b, s_], lg_ref[b, s_]) < 1e-2, (b, s_, rel_err(lg[b, s_], lg_ref[b, s_]))
            if tok[b, s_] != tok_ref[b, s_]:
                top2 = lg_ref[b, s_].float().topk(2).values
                noise = float((lg[b, s_].float() - lg_ref[b, s_].float()).abs().max())
                assert float(top2[0] - top2[1]) <= 4 * noise, (b, s_)
                break
        assert s_ >= 1, (b, "no cached step was compared")
    same = (tok == tok_ref).all(1)
    assert torch.allclose(lp.cpu()[same], lp_ref[same], atol=0.25)
