"""Float64 restatements and case tables of the fp32 stream step (include/pcy.h: the streaming fp32 GEMV, the decode attention that reads its
position on the device, the device-resident step), built on tests/f32_ref.py and written from the header, never from the kernels.  The
GPU tests (tests/test_gpu_f32_stream.py) and the CPU test (tests/test_f32_stream_cpu.py) read the same numbers."""
import torch
import torch.nn.functional as F

import f32_ref as R

F64 = torch.float64
EPI_STORE, EPI_RESID, EPI_SWIGLU = 0, 1, 4
EPIS = {"store": EPI_STORE, "resid": EPI_RESID, "swiglu": EPI_SWIGLU}

# ---- the GEMV's loop edges (procyon_amd/csrc/pcy_f32_gemv.hip): a k-step is one 16-byte load per lane of a 16-row group = 16 floats; the 8
# waves of a workgroup take 8 k-steps each per pass of its k loop, and all 8 split K (STORE / RESID) or 4 per matrix (SWIGLU: gate and up)
GEMV_KSTEP, GEMV_ROWS = 16, 16
GEMV_PASS = {"store": 8 * 8 * 16, "resid": 8 * 8 * 16, "swiglu": 4 * 8 * 16}      # floats of K per pass of a workgroup's k loop
GEMV_WIDEST = 32                                                                  # rows of x that share one pass over the weights


def gemv_cases(epi):
    """name -> (B, N, K): the smallest shapes that reach each loop edge of this epilogue's kernel"""
    P, S, G, W = GEMV_PASS[epi], GEMV_KSTEP, GEMV_ROWS, GEMV_WIDEST
    return {
        "kstep_b1": (1, G + 1, S),                    # a single k-step, one row, N % 4 != 0, one row group + 1
        "pass_b32": (W, G - 1, P),                    # exactly one pass of the k loop, the widest single pass, one row group - 1
        "pass1_b33": (W + 1, G + 1, P + S),           # one pass + one step, a second pass over the weights for the 33rd row
        "pass1_b16": (16, 50, P + S),                 # one x tile exactly
        "pass1_b17": (17, 50, P + S),                 # the second x tile begins
        "k20_b3": (3, 50, 20),                        # K % 16 != 0: the last k-step is cut
        "rot_b2": (2, 50, 4 * P),                     # four passes: row groups 0..3 walk them rotated by 0..3
        "window_b5": (5, G + 1, P + S),               # x, y, resid are column windows of wider buffers
        "alias_b5": (5, G + 1, P + S),                # resid is y (RESID only; the other epilogues run it as a plain call)
    }


def gemv_case(epi, name):
    B, N, K = gemv_cases(epi)[name]
    return dict(x=R.rnd(B, K, seed=201), W=R.rnd(N, K, seed=202, std=0.05), W2=R.rnd(N, K, seed=203, std=0.05), resid=R.rnd(B, N, seed=204))


def gemv(x, W, W2, resid, epi, dt=F64):
    """y = epi(x . W^T): STORE the product, RESID + resid, SWIGLU silu(x . W^T) * (x . W2^T)"""
    if epi == EPI_SWIGLU:
        return R.silu_mul(R.linear(x, W, dt=dt), R.linear(x, W2, dt=dt), dt=dt)
    return R.linear(x, W, resid=resid if epi == EPI_RESID else None, dt=dt)


# ---- decode attention at a device position: rope q and the new k at t, append K / V at slot t, exact softmax over slots [0, t]
ATTN_POS = (0, 62, 63, 64, 199)
ATTN_POS_LONG = 600            # beyond the 512 keys the threads of a workgroup take in one round (one geometry)


def attn_pos_case(t, H, Hkv, dh):
    """R.decode_case(t, ...): qkv [3, (H + 2 Hkv) dh] un-roped, caches [3, t + 7, Hkv dh] with NaN in every slot >= t (slot t is the one the
    operator writes; the slots above must never reach a result) + the rotary tables"""
    c = R.decode_case(t, H, Hkv, dh)
    c["cos"], c["sin"] = R.rope_tables(dh, t + 7)
    return c


def attn_decode_pos(qkv, kc, vc, t, cos, sin, H, Hkv, dh, scale, dt=F64):
    """-> (o [B, H dh], K cache, V cache after the append) in dt"""
    B = qkv.shape[0]
    pos = torch.full((B,), t, dtype=torch.int32)
    r = R.rope(qkv, 0, H + Hkv, dh, pos, cos, sin, dt=dt)            # q heads and k heads are neighbours: one rotation
    kc2, vc2 = kc.to(dt).clone(), vc.to(dt).clone()
    kc2[:, t] = r[:, H * dh:(H + Hkv) * dh]
    vc2[:, t] = r[:, (H + Hkv) * dh:]
    return R.attn_decode(r[:, :H * dh], kc2, vc2, t + 1, H, Hkv, dh, scale, dt=dt), kc2, vc2


# ---- the step on the padded greedy fixture of tests/test_gpu_fp32.py (R.GEN_GEOM, 3 prompts, left pads {0, 5, 1}, 6 steps)
def gen_fixture():
    """state dict, oracle geometry, prompt ids / mask / embeddings and the oracle's greedy run: tokens [3, 6], logits [3, 6, V], summed
    log-probabilities [3]"""
    from oracle import llama_ref as LR
    from procyon_amd import synth
    sd = synth.llama_state_dict(**R.GEN_GEOM, dtype=torch.float32)
    geom = LR.LlamaGeom(**R.GEN_GEOM)
    ids, mask = R.gen_case()
    emb = F.embedding(ids, sd["model.embed_tokens.weight"])
    toks, logits, lp = LR.greedy_generate(sd, geom, emb, mask, R.GEN_STEPS, clean_decode_mask=False)
    return dict(sd=sd, geom=geom, ids=ids, mask=mask, emb=emb, toks=toks, logits=logits, logprob=lp, steps=R.GEN_STEPS)


def top2_margins(logits):
    """[..., V] -> (top-1 - top-2) / the row's norm"""
    top = logits.to(F64).topk(2, -1).values
    return (top[..., 0] - top[..., 1]) / logits.to(F64).norm(dim=-1)


TOKEN_MARGIN = 1e-3            # the fixture's smallest top-2 margin over the row norm must stay above this (10 x the 1e-4 bar)

# ---- beam search: the oracle's smallest gap between the last selected and the first rejected candidate, over the row norm
BEAM_KW = dict(max_len=5, beam_size=4, beam_group_size=2, diversity_penalty=0.8)
BEAM_GAP = 2e-4
BEAM_SEED = 306                # prompt ids of the engine-level beam case: the fixture's own first two prompts leave a gap of 1.3e-4 only


def beam_fixture(gen):
    """two prompts of R.GEN_T tokens on the greedy fixture's model, left pads {0, 5}: (embeddings, mask)"""
    ids = torch.randint(0, R.GEN_GEOM["vocab"], (2, R.GEN_T), generator=torch.Generator().manual_seed(BEAM_SEED))
    return F.embedding(ids, gen["sd"]["model.embed_tokens.weight"]), gen["mask"][:2]


def beam_oracle(sd, geom, emb, mask, eos_id, **kw):
    """LR.beam_search on the oracle's text encoder -> (tokens, scores, logits, smallest (gap / largest row norm of the step) over every
    selection of the search)"""
    from oracle import llama_ref as LR
    enc = LR.make_text_encoder(sd, geom)
    norms = []

    def enc_n(**a):
        logits, past = enc(**a)
        norms.append(float(logits[:, -1].to(F64).norm(dim=-1).max()))
        return logits, past

    trace = []
    t, s, lg = LR.beam_search(enc_n, emb, mask, vocab_size=geom.vocab, eos_id=eos_id, trace=trace, **kw)
    g = kw["beam_group_size"]
    rel = min(float(v[g - 1] - v[g]) / norms[i] for i, _, _, v in trace)
    return t, s, lg, rel
