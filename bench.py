#!/usr/bin/env python
"""bench.py -- ProCyon-Full phenotype generation on MI355X (BASELINE.json configs[1]).

Workload (one "step" = one whole job): ESM2-650M encodes one 1024-residue protein (S=1026) -> mean pool ->
3-layer token projector -> soft-token splice into a 512-token prompt (2 <|protein|> slots + [ANSWER]) ->
Llama-3-8B prefill -> 256 greedy tokens with KV-cached decode (no EOS stop), bf16, batch 1, through the
`UnifiedProCyon.generate(method="greedy")` mirror.  Synthetic random-init weights of the real architecture,
inputs resident in HBM.  value = generated tokens / wall time of the timed steps (end to end: encoder + prefill
+ decode), whole job over all ranks; N > 1 runs N independent replicas (generation rows are independent,
SURVEY.md section 8e: "replicas only") plus a DP-sharded retrieval leg with ONE RCCL all-gather.

A plain run sets up, warms up, times the steps and prints the headline line; nothing else.  With `--full` the JSON line also
carries `phases`, `roofline` (dominant kernel = the decode layer launch, algorithmic bytes / HIP-event time measured live),
`retrieval`, the `configs` block and `cpu_baseline` (the oracle on the host's cores, bounded sample), each measured after
the timed steps.  `--dump-outputs DIR` writes what the last timed step returned (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tokens", type=int, default=256)
    ap.add_argument("--residues", type=int, default=1024)
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--geometry", default="full")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-live-pmc", action="store_true", help="roofline.traffic from the committed profiles/ ratio instead of two rocprofv3 --pmc passes run now")
    ap.add_argument("--retrieval-proteins", type=int, default=750, help="proteins per rank in the retrieval leg (30 engine batches, ~1.2 s per pass -- a 0.4 s pass of 10 batches moved by a fifth with one host or clock event: the first batch's host packing is the only one the GPU waits for)")
    ap.add_argument("--no-configs", action="store_true", help="skip the BASELINE configs[3] / configs[4] block (batch-32 generation, pair scoring)")
    ap.add_argument("--full", action="store_true", help="after the timed steps also measure the phases, the roofline, the retrieval leg, the "
                                                        "configs block and the CPU baseline (the --no-* options above apply to this mode)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the arrays the last timed step returned to DIR/<name>.npy")
    return ap.parse_args()


DUMP_LOGITS_SAMPLE = 1 << 22   # elements of the logits record kept by --dump-outputs (16 MB of float32)


def dump_outputs(path, toks, lp, logits):
    """What `UnifiedProCyon.generate(method="greedy")` hands its caller, as .npy files: the generated token ids (float64, exact), their
    log-probabilities (float32) and the logits record (float32).  The record is [1, 1, tokens, vocab] (131 MB at the default size), so
    above DUMP_LOGITS_SAMPLE elements a fixed sample of them is written instead: the flat indices
    np.sort(np.random.default_rng(0).choice(numel, DUMP_LOGITS_SAMPLE, replace=False)), the same for every run of the same shape."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "tokens.npy"), toks.cpu().numpy().astype(np.float64))
    np.save(os.path.join(path, "log_probs.npy"), lp.float().cpu().numpy())
    flat = logits.float().cpu().reshape(-1).numpy()
    if flat.size > DUMP_LOGITS_SAMPLE:
        flat = flat[np.sort(np.random.default_rng(0).choice(flat.size, DUMP_LOGITS_SAMPLE, replace=False))]
    np.save(os.path.join(path, "logits.npy"), flat)


def relaunch_under_torchrun(a):
    """`python bench.py --gpus N` without a launcher: start N ranks (one per GPU, RCCL) under torch.distributed.run and pass
    every argument on; the child ranks find WORLD_SIZE set and run the bench."""
    import socket
    import subprocess
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.run(cmd, env=env).returncode)


def cpu_baseline(tokens, residues, prompt):
    """Oracle (oracle/, kind "port") on the host cores: 2 of 33 ESM2-650M layers at S=residues+2, 2 of 32 Llama-3-8B
    layers for prefill (T=prompt) and 4 cached decode steps + the lm_head, scaled to the full depth."""
    from oracle import esm_ref as ER
    from oracle import llama_ref as LR
    from procyon_amd import synth
    # torch-CPU bf16 is fastest at ~32 threads on the GPU box's EPYC host (tools/archive/cpu_threads_probe.py: 8/32/64/128/256
    # threads -> 11.7/9.4/29.9/35.2/3334 ms per decode layer), so the baseline is not handicapped by oversubscription
    torch.set_num_threads(min(32, os.cpu_count()))
    cores = torch.get_num_threads()
    ek = dict(d=1280, n_layers=2, n_heads=20, ffn=5120)
    esd = synth.esm_state_dict(**ek)
    toks = synth.protein_tokens([residues], seed=0)
    ER.esm_forward(esd, ER.EsmGeom(**ek), toks[:, :66])   # warm-up
    t0 = time.perf_counter()
    ER.esm_forward(esd, ER.EsmGeom(**ek), toks)
    t_esm = (time.perf_counter() - t0) * 33 / 2
    lk = dict(vocab=128263, d=4096, n_layers=2, n_heads=32, n_kv_heads=8, ffn=14336)
    lsd = synth.llama_state_dict(**lk)
    emb = (torch.randn(1, prompt, 4096) * 0.02).bfloat16()
    nd = 4

    def run(n_layers):
        geom = LR.LlamaGeom(**{**lk, "n_layers": n_layers})
        t0 = time.perf_counter()
        r = LR.llama_forward(lsd, geom, inputs_embeds=emb, attn_mask=torch.ones(1, prompt), logits_rows="last")
        tp = time.perf_counter() - t0
        past, tok = r["past_kv"], r["logits"][:, -1].argmax(-1, keepdim=True)
        t0 = time.perf_counter()
        for _ in range(nd):
            r = LR.llama_forward(lsd, geom, input_ids=tok, attn_mask=None, past_kv=past, logits_rows="last")
            past, tok = r["past_kv"], r["logits"][:, -1].argmax(-1, keepdim=True)
        return tp, (time.perf_counter() - t0) / nd

    run(1)                                   # warm the thread pool / allocator
    p1, d1 = run(1)
    p2, d2 = run(2)
    # one layer costs (t2 - t1); embedding + final norm + lm_head cost t1 minus one layer
    lay_p, lay_d = max(p2 - p1, 1e-6), max(d2 - d1, 1e-6)
    t_prefill = 32 * lay_p + max(p1 - lay_p, 0.0)
    t_step = 32 * lay_d + max(d1 - lay_d, 0.0)
    total = t_esm + t_prefill + (tokens - 1) * t_step
    cpu_model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                cpu_model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"value": round(tokens / total, 3), "unit": "tokens/s", "cores": cores, "kind": "port", "cpu_model": cpu_model,
            "host_logical_cpus": os.cpu_count(),
            "sample": f"oracle (torch-CPU bf16): 2/33 ESM2-650M layers S={residues + 2}, 2/32 Llama-3-8B layers (1- and 2-layer runs differenced) prefill T={prompt} "
                      f"+ {nd} decode steps + lm_head, scaled to 32 layers; esm {t_esm:.2f}s prefill {t_prefill:.2f}s "
                      f"decode {t_step * 1e3:.0f} ms/token"}


def live_pmc_traffic(kernel_sub, geometry):
    """HBM bytes per launch of the decode-step kernel from two rocprofv3 --pmc passes (separate passes, --kernel-trace only: MI355X_MICROARCH.md,
    HBM section) over tools/pmc_decode.py, run NOW on this box.  None when rocprofv3 is missing, this process is itself being profiled, or a pass
    fails / times out -- the committed ratio of profiles/ is used then."""
    import shutil, subprocess, tempfile
    if shutil.which("rocprofv3") is None or any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ):
        return None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from pmc_hbm_summary import summarise
        d = tempfile.mkdtemp(prefix="pcy_pmc_", dir="/tmp")
        env = dict(os.environ, TMPDIR="/tmp")
        if geometry == "split":
            env["GEO"] = "split"
        for c in ("FETCH_SIZE", "WRITE_SIZE"):
            subprocess.run(["rocprofv3", "--pmc", c, "--kernel-trace", "-d", os.path.join(d, c), "-o", "p", "--output-format", "csv", "--",
                            sys.executable, os.path.join(ROOT, "tools", "pmc_decode.py")], cwd="/tmp", env=env, timeout=300, check=True,
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        alg = 13227261952 if geometry == "split" else 14029094912   # 32 layers x (weights + cached K/V at t = 512..536), tools/r6_profiles.sh
        r = summarise(os.path.join(d, "FETCH_SIZE"), os.path.join(d, "WRITE_SIZE"), kernel_sub, alg, "live")
        shutil.rmtree(d, ignore_errors=True)
        v = next(iter(r["kernels"].values()))
        return v if v["launches"][0] >= 8 and 0.5 < v["ratio"] < 3.0 else None
    except Exception:
        return None


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(a)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != max(a.gpus, 1) and rank == 0:
        print(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}; reporting n_gpus={world}", file=sys.stderr)
    local = int(os.environ.get("LOCAL_RANK", "0"))
    dist = world > 1 or bool(os.environ.get("PCY_BENCH_FORCE_DIST"))   # the env switch exercises the RCCL path on one GPU
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if dist:
        import torch.distributed as td
        td.init_process_group(backend="nccl", device_id=dev)

    from procyon_amd import synth
    from procyon_amd import synthetic_model as SM
    from procyon_amd.engine import Context

    model = SM.build(a.geometry, device=dev, max_new_tokens=a.tokens)
    ctx = Context.get(dev)
    eng = model.text_encoder.engine
    cfg = eng.cfg
    prot = synth.protein_tokens([a.residues], seed=0)

    def barrier():
        if dist:
            td.barrier()
        torch.cuda.synchronize()

    phases = {}

    def one_step(record=False):
        inputs = SM.caption_inputs(model, prot, n_prompt_words=a.prompt - 2, n_slots=2, seed=0)
        if record:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            emb, ids, mask, *_ = model._preprocessing(inputs, crop_off=True, no_pad=True, left_pad=True)
            torch.cuda.synchronize(); t1 = time.perf_counter()
            assert emb.shape[1] == a.prompt, emb.shape
            cache = eng.new_cache(1, a.prompt + a.tokens)
            logits, _ = eng.prefill(emb, mask, cache, "last")
            torch.cuda.synchronize(); t2 = time.perf_counter()
            phases.update(encode_project_splice_ms=(t1 - t0) * 1e3, prefill_ms=(t2 - t1) * 1e3)
        toks, lp, logits, text = model.generate(inputs, max_len=a.tokens, method="greedy")
        assert toks.shape == (1, 1, a.tokens)
        return toks, lp, logits

    for _ in range(a.warmup):
        one_step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        # the previous step's logits record (pinned host memory, one per call) goes back to the allocator before the next step needs one
        result = None
        result = one_step()
    barrier()
    dt = time.perf_counter() - t0
    if dist:
        t = torch.tensor([dt], device=dev)
        td.all_reduce(t, op=td.ReduceOp.MAX)
        dt = float(t)
    value = world * a.tokens * a.steps / dt
    ctx.sync()   # raises if a cross-workgroup hand-over of the fused decode launches ever hit its watchdog (results would be invalid)
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, *result)
    out = {"metric": f"phenotype-gen tokens/sec ({'ProCyon-Split' if a.geometry == 'split' else 'ProCyon-Full'} greedy generation, end to end)", "value": round(value, 2),
           "unit": "tokens/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 2),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
           "config": {"workload": (f"configs[1]: ProCyon-Full (ESM2-650M + Llama-3-8B geometry={a.geometry}) bf16 batch=1, " if a.geometry != "split" else
                                   "configs[0] shape on the GPU: ProCyon-Split (ESM2-150M + Llama-2-7B geometry) bf16 batch=1, ") +
                                  f"{a.residues}-residue protein, {a.prompt}-token prompt, {a.tokens}-token greedy generation",
                      "parallelism": f"replicas x{world}" if world > 1 else "single GPU"}}
    if not a.full:
        if rank == 0:
            print(json.dumps(out))
        if dist:
            td.destroy_process_group()
        return

    # ---- phases + decode-only rate (outside the timed region) --------------------------------------
    one_step(record=True)
    inputs = SM.caption_inputs(model, prot, n_prompt_words=a.prompt - 2, n_slots=2, seed=0)
    emb, ids, mask, *_ = model._preprocessing(inputs, crop_off=True, no_pad=True, left_pad=True)
    from procyon_amd.engine import GenState
    cache = eng.new_cache(1, a.prompt + a.tokens)
    st = GenState(1, cfg.vocab, a.tokens, dev)
    logits, _ = eng.prefill(emb, mask, cache, "last")
    st.logits.copy_(logits); st.pos.fill_(a.prompt)
    eng.pick(cache, st, 1, advance_pos=False)
    prefill_flop = 2 * cfg.n_layers * (cfg.d * (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim + cfg.n_heads * cfg.head_dim * cfg.d
                                       + 3 * cfg.d * cfg.ffn) * a.prompt + 4 * cfg.n_layers * cfg.n_heads * cfg.head_dim * a.prompt * a.prompt / 2 \
        + 2 * cfg.vocab * cfg.d
    # prefill alone, HIP events (the wall-clock phase above includes the host side of the call)
    eng.prefill(emb, mask, cache, "last")
    ctx.timer_start()
    for _ in range(5):
        eng.prefill(emb, mask, cache, "last")
    pre_ms = ctx.timer_stop() / 5
    phases.update(prefill_kernels_ms=pre_ms, prefill_TFLOPs=prefill_flop / 1e12 / (pre_ms / 1e3),
                  prefill_mfma_frac_of_2500TF=prefill_flop / 1e12 / (pre_ms / 1e3) / 2500.0)
    # the encoder alone, HIP events (ESM2 over the one protein + pooling; `encode_project_splice_ms` above is wall clock and includes the
    # host side: tokenising, packing, the projector and the splice)
    esm_eng = model.protein_seq_encoder.engine
    for _ in range(3):
        esm_eng.forward(prot)
    # one call per timed region: replays of ONE captured launch chain queued back to back wait for each other on the host side (10 ms per call
    # in some runs against 4.5 ms of kernels, tools/t_esm_graph_count.py) -- the generation loop issues one call per protein, never a queue
    enc_ms = 0.0
    for _ in range(5):
        ctx.timer_start()
        esm_eng.forward(prot)
        enc_ms += ctx.timer_stop() / 5
    S_ = a.residues + 2
    enc_flop = (2 * 648806400 * S_ + 168960 * S_ * S_) if a.geometry == "full" else None
    phases.update(encode_kernels_ms=enc_ms)
    if enc_flop:
        phases.update(encode_TFLOPs=enc_flop / 1e12 / (enc_ms / 1e3), encode_mfma_frac_of_2500TF=enc_flop / 1e12 / (enc_ms / 1e3) / 2500.0)
    logits, _ = eng.prefill(emb, mask, cache, "last")
    st.logits.copy_(logits); st.pos.fill_(a.prompt)
    eng.pick(cache, st, 1, advance_pos=False)
    eng.greedy_steps(cache, st, 1, 8)          # warm the graph
    ctx.timer_start()
    nsteps = a.tokens - 16
    eng.greedy_steps(cache, st, 1, nsteps)
    dec_ms = ctx.timer_stop() / nsteps
    step_bytes = 2 * (cfg.n_layers * (cfg.d * (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim + cfg.n_heads * cfg.head_dim * cfg.d
                                      + 3 * cfg.d * cfg.ffn + 2 * cfg.d) + cfg.d + cfg.vocab * cfg.d)
    kv_bytes = 2 * cfg.n_layers * cfg.n_kv_heads * cfg.head_dim * 2 * (a.prompt + a.tokens // 2)
    phases.update(decode_ms_per_token=dec_ms, decode_tokens_per_s=1e3 / dec_ms,
                  decode_step_algorithmic_GB=(step_bytes + kv_bytes) / 1e9,
                  decode_step_GBps=(step_bytes + kv_bytes) / 1e9 / (dec_ms / 1e3))

    off = set(os.environ.get("PCY_DISABLE", "").split(","))   # procyon_amd/csrc/pcy_switch.h
    # ---- roofline of the dominant kernel: the decode LAYER launch (qkv + attention + o + gate/up + down of one layer, one per layer per token)
    mha = cfg.n_kv_heads == cfg.n_heads == 32 and cfg.ffn == 11008   # ProCyon-Split (Llama-2-7B): decode_step_mha_kernel, pcy_decode_mha.hip
    one_launch = (cfg.d == 4096 and (cfg.ffn == 14336 or mha) and cfg.n_heads * cfg.head_dim == 4096 and
                  not (off & {"decode_layer", "attn_o"}))
    all_layers = one_launch and "decode_step" not in off   # decode_step_kernel: the 32 layers in ONE launch
    t_mid = int(st.pos.item())                     # cache length of the measured launches (the timed decode ended here)
    reps = 8
    eng.decode_layers(cache, st, 1, 2)
    ctx.timer_start()
    eng.decode_layers(cache, st, 1, reps)          # reps x n_layers layer launches (+ 2 one-thread counter launches per pass)
    k_ms = ctx.timer_stop() / (reps * (1 if all_layers else cfg.n_layers))
    qkvw = (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim
    # weight bytes of one layer per token (Wqkv, Wo, Wgu, Wdown, two norm vectors) + the cached K/V rows it reads
    k_bytes = 2 * (cfg.d * qkvw + cfg.n_heads * cfg.head_dim * cfg.d + 3 * cfg.d * cfg.ffn + 2 * cfg.d) + 2 * cfg.n_kv_heads * cfg.head_dim * 2 * t_mid
    if all_layers:
        k_bytes *= cfg.n_layers
    traffic, traffic_source = None, None
    # HBM bytes per launch cannot be read inside the timed process: they come from separate `rocprofv3 --pmc FETCH_SIZE` /
    # `--pmc WRITE_SIZE` passes over tools/bench_decode.py (the same kernel, the same shapes), committed under profiles/
    traffic_ratio = None
    # (the live counter passes run at the very END of the bench, behind every timed leg -- see live_traffic below: run here, in front of the
    # retrieval leg, they cost its single timed pass 5-20 % on two of three boxes; the committed ratio is the value until then)
    want_live = all_layers and rank == 0 and world == 1 and not a.no_live_pmc and a.geometry in ("full", "split")
    try:
        pname = next(n for n in ((("r06_pmc_decode_step_mha.json",) if mha else ("r06_pmc_decode_step.json", "archive/r05_pmc_decode_step.json")) if all_layers
                                 else ("archive/r02_pmc_decode_layer.json",))
                     if os.path.exists(os.path.join(ROOT, "profiles", n)))
        pm = json.load(open(os.path.join(ROOT, "profiles", pname)))["kernels"]
        if one_launch and (a.geometry == "full" or (mha and all_layers)):
            v = [v for k, v in pm.items() if "decode_step_kernel" in k or "decode_step_mha_kernel" in k or "decode_layer_kernel" in k or "attn_block_kernel" in k][0]
            # the counters were taken at another cache length (t = 512..536) than this run's timed region: the measured / algorithmic
            # RATIO carries over, the byte count is scaled to this run's launch (review, round 4: not two numbers from different lengths)
            traffic_ratio = v["hbm_bytes_per_launch"] / v["algorithmic_bytes"]
            traffic = int(round(traffic_ratio * k_bytes))
            traffic_source = (f"profiles/{pname}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes at t = 512..536 (FETCH_SIZE doubled per MI355X_MICROARCH.md) measured "
                              f"{v['hbm_bytes_per_launch']} B against {v['algorithmic_bytes']} algorithmic; that ratio x this launch's algorithmic bytes")
    except Exception:
        pass
    kname = ("decode_step_mha_kernel", "decode_layer_mha_kernel") if mha else ("decode_step_kernel<128,4>", "decode_layer_kernel<128,4>")
    roofline = {"bound": "hbm", "kernel": (f"{kname[0]} (all {cfg.n_layers} Llama decoder layers of a decode step in one launch: per layer qkv, attention, o, gate/up, down)"
                                           if all_layers else f"{kname[1]} (one Llama decoder layer per launch; {cfg.n_layers} launches/token)"
                                           if one_launch else "decoder layer as separate launches (average per layer)"),
                "achieved": round(k_bytes / 1e9 / (k_ms / 1e3), 1), "peak": 8000.0, "unit": "GB/s",
                "frac": round(k_bytes / 1e9 / (k_ms / 1e3) / 8000.0, 4), "traffic": traffic, "traffic_over_algorithmic": None if traffic_ratio is None else round(traffic_ratio, 4),
                "traffic_source": traffic_source,
                "bytes_per_launch": k_bytes, "avg_launch_us": round(k_ms * 1e3, 2), "cache_len": t_mid}

    # ---- retrieval leg (config 3 shape): DP-sharded forward_sequences + ONE all-gather --------------
    from procyon_amd.distributed import embed_sharded
    nprot = a.retrieval_proteins * world
    plen = a.residues if a.geometry == "full" else 100
    # proteins per engine call: "batch size chosen by the engine" (BASELINE configs[2]) -> EsmEngine.preferred_batch
    rb = model.protein_seq_encoder.engine.preferred_batch(plen + 2)
    tok_fn = lambda idx: synth.protein_tokens([plen] * len(idx), seed=1000 + (idx[0] if len(idx) else 0))
    embed_sharded(model, tok_fn, 3 * rb * world, batch_size=rb)   # untimed: workspace growth, first-launch effects, the capture of the batch's launch chain (second sight)
    # ONE timed pass (review, round 4: no best-of-2); a second, untimed-for-the-record pass is reported beside it so that a box that lost part
    # of the first one shows (`second_pass_proteins_per_s`)
    barrier(); t0 = time.perf_counter()
    allz = embed_sharded(model, tok_fn, nprot, batch_size=rb)
    barrier(); rt = time.perf_counter() - t0
    barrier(); t0 = time.perf_counter()
    embed_sharded(model, tok_fn, nprot, batch_size=rb)
    barrier(); rt2 = time.perf_counter() - t0
    assert allz.shape[0] == nprot
    # the same leg with the exact-rounding two-pass attention (PCY_ESM_ATTN=exact: the reference's bf16 rounding points op for op;
    # the default is the single-pass kernel, held to the fp32 evaluation instead -- DESIGN.md section 4)
    rt_exact = None
    if os.environ.get("PCY_ESM_ATTN", "fast")[0] != "e":
        os.environ["PCY_ESM_ATTN"] = "exact"
        embed_sharded(model, tok_fn, 3 * rb * world, batch_size=rb)
        barrier(); t0 = time.perf_counter()
        embed_sharded(model, tok_fn, nprot, batch_size=rb)
        barrier(); rt_exact = time.perf_counter() - t0
        os.environ["PCY_ESM_ATTN"] = "fast"
    # the gathered [N_total, D] matrix against single-rank embeddings of a sample of its rows (first / middle / last protein:
    # the last one lives on the last rank): a protein's embedding does not depend on its batch mates, so the rows must be EQUAL
    per = -(-nprot // world)                                   # shard size (distributed.shard_indices)
    for i in sorted({0, nprot // 2, nprot - 1}):
        b0 = (i // per) * per + ((i % per) // rb) * rb           # first protein of the engine call that embedded protein i
        idx = list(range(b0, min(b0 + rb, (i // per + 1) * per, nprot)))
        ref_row = model.forward_sequences(tok_fn(idx))["shared"][i - b0]
        assert torch.equal(ref_row, allz[i]), f"gathered embedding of protein {i} differs from the single-rank result"
    # the encoder of one retrieval batch alone, HIP events on the engine's stream (the leg above is wall clock: host packing, pooling,
    # projector, the gather; on a busy host it loses up to 15 % to the launch rate)
    btoks = tok_fn(list(range(rb)))
    for _ in range(2):
        esm_eng.forward(btoks)
    ctx.timer_start()
    for _ in range(4):
        esm_eng.forward(btoks)
    enc_b_ms = ctx.timer_stop() / 4
    retrieval = {"proteins_per_s": round(nprot / rt, 2), "n_proteins": nprot, "residues": plen, "batch": rb, "timing": "single pass", "second_pass_proteins_per_s": round(nprot / rt2, 2),
                 "mfma_frac_of_2500TF": round(nprot / rt * (2 * 648806400 * (plen + 2) + 168960 * (plen + 2) ** 2) / 2.5e15, 4) if a.geometry == "full" else None,
                 "encoder_ms_per_batch": round(enc_b_ms, 3), "encoder_proteins_per_s": round(rb / enc_b_ms * 1e3, 1),
                 "encoder_mfma_frac_of_2500TF": round(rb / enc_b_ms * 1e3 * (2 * 648806400 * (plen + 2) + 168960 * (plen + 2) ** 2) / 2.5e15, 4) if a.geometry == "full" else None,
                 "attention": "single-pass (PCY_ESM_ATTN=fast, default)" if rt_exact is not None else "exact two-pass (PCY_ESM_ATTN=exact)",
                 "proteins_per_s_exact_attention": round(nprot / rt_exact, 2) if rt_exact is not None else None,
                 "collective": "one RCCL all-gather through pcy_allgather" if dist else "none (single rank)", "gather_checked_rows": 3}

    # ---- BASELINE configs[3] (batch-32 mixed-length generation, 4a equal and 4b ragged prompts) and configs[4] (pair scoring) ----
    # At N > 1 (or PCY_BENCH_FORCE_DIST=1) the 32 rows / the 256 pairs are SPLIT across the ranks (contiguous
    # chunks in rank order, one final all-gather of the token ids / probabilities) -- the 1 -> 8 GPU scaling curve of configs[3].
    configs = None
    batched_roofline = None
    decode_curve = None
    if not a.no_configs and a.geometry == "full":
        from procyon_amd import workloads as WL
        model.text_encoder.max_new_tokens = 512
        if not dist:
            batched_roofline = WL.batched_decode_roofline(model, rows=32, prompt=512, new_tokens=512)
        configs = {"config3_4a_batch32_mixed_residues_T512": WL.run_config4(model, new_tokens=512, ragged=False),
                   "config3_4b_batch32_ragged_prompts": WL.run_config4(model, new_tokens=512, ragged=True),
                   "config4_pair_scoring_256": WL.run_config5(model, pairs=256, chunk=64, fp8=True)}
        if not dist:
            # per-batch decode curve (beam search = batch beam_size; the N-GPU points of configs[3] run 32 / N rows per GPU) and the 1 -> 8 GPU
            # curve of configs[3] projected from single-GPU runs of every rank's chunk (replicas, no traffic inside the loop)
            decode_curve = WL.decode_batch_curve(model)
            configs["config3_projected_scaling"] = WL.config3_projected_scaling(model, new_tokens=512, single_gpu=configs["config3_4a_batch32_mixed_residues_T512"])
            # the reference's own generation method (model_unified.py:702-842; scripts/caption_bulk.py:121-132 hard-codes it): beam search on the
            # headline's inputs -- ms per beam step from the slope over max_len (decode of beam rows + record + bookkeeping + KV reorder)
            binp = SM.caption_inputs(model, prot, n_prompt_words=a.prompt - 2, n_slots=2, seed=0)
            beams = {}
            # beam 5 / 5: the signature default (model_unified.py:924-940); beam 10 / 2: scripts/caption_bulk.py:193-194 + :130 and the evaluation
            # plugin (evaluate/framework/procyon.py:72-76); beam 20 / 2 at max_len 200: examples/phenotype_generation.ipynb cell 14
            for (bsz, grp, n_hi) in ((5, 5, 88), (10, 2, 88), (20, 2, 200)):
                tms = {}
                model.generate(binp, max_len=4, method="beam", beam_size=bsz, beam_group_size=grp)
                for n in (24, n_hi):
                    torch.cuda.synchronize(); tb = time.perf_counter()
                    model.generate(binp, max_len=n, method="beam", beam_size=bsz, beam_group_size=grp)
                    torch.cuda.synchronize(); tms[n] = (time.perf_counter() - tb) * 1e3
                beams[f"beam{bsz}_group{grp}"] = {"ms_per_step": round((tms[n_hi] - tms[24]) / (n_hi - 24), 3), f"ms_generate_{n_hi}_steps": round(tms[n_hi], 1),
                                                 "prompt_tokens": a.prompt, "mean_cache_len": a.prompt + (24 + n_hi) // 2,
                                                 "prefill": "one per prompt, K / V rows broadcast to the beams"}
            configs["beam_search_caption"] = beams
        if not dist:
            # fp8 accuracy where it can be judged: the same model with its residual branches damped to a quarter (a trained-like
            # regime instead of the chaotic random-init one), LAST because it rewrites the decoder's weights in place
            WL.damp_residual_branches(model, 0.25)
            acc = WL.run_config5(model, pairs=128, chunk=64, fp8=True)
            configs["config4_fp8_accuracy_damped_model"] = {k: acc[k] for k in ("pairs", "answer_logits_rel_err_fp8_vs_bf16",
                                                                                  "yes_no_agreement_fp8_vs_bf16", "mean_abs_dP_yes")}
            configs["config4_fp8_accuracy_damped_model"]["residual_branch_scale"] = 0.25

    if rank == 0:
        out.update(phases={k: round(v, 3) for k, v in phases.items()}, roofline=roofline, retrieval=retrieval)
        if configs is not None:
            out["configs"] = configs
        if decode_curve is not None:
            out["batched_decode_curve"] = decode_curve
        if batched_roofline is not None:
            out["batched_decode_roofline"] = batched_roofline
        if not a.no_cpu_baseline and a.geometry == "full" and world == 1:   # reported at N = 1 only
            out["cpu_baseline"] = cpu_baseline(a.tokens, a.residues, a.prompt)
        if want_live:   # roofline.traffic from two rocprofv3 --pmc passes run NOW (nothing timed is left to disturb)
            live = live_pmc_traffic("decode_step_mha_kernel" if mha else "decode_step_kernel", a.geometry)
            if live is not None:
                ratio = live["hbm_bytes_per_launch"] / live["algorithmic_bytes"]
                roofline["traffic"] = int(round(ratio * roofline["bytes_per_launch"]))
                roofline["traffic_over_algorithmic"] = round(ratio, 4)
                roofline["traffic_source"] = (
                    f"LIVE: two rocprofv3 passes (--pmc FETCH_SIZE, --pmc WRITE_SIZE; --kernel-trace only) over tools/pmc_decode.py run by this bench.py "
                    f"invocation on this box behind its timed legs, 24 launches of the same kernel at t = 512..536: (2 x FETCH_SIZE + WRITE_SIZE) x 1024 = "
                    f"{live['hbm_bytes_per_launch']} B against {live['algorithmic_bytes']} algorithmic (FETCH_SIZE doubled per MI355X_MICROARCH.md); "
                    f"that ratio x this launch's algorithmic bytes")
        print(json.dumps(out))
    if dist:
        td.destroy_process_group()


if __name__ == "__main__":
    main()
