"""ctypes binding of libpcy.so (include/pcy.h).  The product path has NO fallback: if the HIP
library is missing or fails to load, importing the engine raises."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PCY_LIB") or os.path.join(_HERE, "libpcy.so")   # PCY_LIB: A/B of experimental builds

EPI_STORE, EPI_RESID, EPI_GELU_ERF, EPI_GELU_ESM, EPI_SWIGLU = range(5)
POOL_MEAN, POOL_MEAN_CORRECTED, POOL_MAX = range(3)
ABI_VERSION = 13
# pcy_debug_dispatch_count kinds
(DISPATCH_GEMM_128, DISPATCH_GEMM_64, DISPATCH_GEMM_BIG, DISPATCH_GEMM_BIG_PERSIST, DISPATCH_GEMM_SPLITK, DISPATCH_GEMM_FP8, DISPATCH_ATTN_FAST,
 DISPATCH_DEC_STEP_GQA, DISPATCH_GEMM_MID, DISPATCH_ESM_GRAPH, DISPATCH_DEC_STEP_MHA, DISPATCH_DEC_LAYER, DISPATCH_DEC_STEP_NB, DISPATCH_DEC_STEP_MB,
 DISPATCH_DEC_LOOP_STREAM, DISPATCH_DEC_LOOP_MFMA, DISPATCH_SHARED_PREFIX, DISPATCH_XENT, DISPATCH_EXTEND,
 DISPATCH_EXTEND_PACKED) = range(20)
# which way a decode step was served (one count per step enqueued outside a graph replay; pcy_internal.h PCY_DISPATCH_DEC_*)
DISPATCH_DECODE = dict(step_gqa=DISPATCH_DEC_STEP_GQA, step_mha=DISPATCH_DEC_STEP_MHA, layer=DISPATCH_DEC_LAYER, step_nb=DISPATCH_DEC_STEP_NB,
                       step_mb=DISPATCH_DEC_STEP_MB, loop_stream=DISPATCH_DEC_LOOP_STREAM, loop_mfma=DISPATCH_DEC_LOOP_MFMA)
# pcy_debug_attn_route_count words: which two-pass prefill attention kernel the launcher chose
ATTN_ROUTE_DH32, ATTN_ROUTE_DH64, ATTN_ROUTE_LDS128_1, ATTN_ROUTE_LDS128_2 = range(4)
# pcy_debug_gemv_route_count words: which kernel pcy_launch_gemv chose
GEMV_ROUTE_STREAM2, GEMV_ROUTE_STREAM4, GEMV_ROUTE_CHUNKED, GEMV_ROUTE_MFMA2, GEMV_ROUTE_MFMA3, GEMV_ROUTE_MFMA4 = range(6)

vp = C.c_void_p
i32 = C.c_int32
ci = C.c_int


class MlpDesc(C.Structure):
    _fields_ = [("n_layers", i32), ("dims", i32 * 9), ("w", vp * 8), ("b", vp * 8)]


class EsmLayer(C.Structure):
    _fields_ = [(n, vp) for n in ("wqkv", "bqkv", "wo", "bo", "ln1_w", "ln1_b", "w1", "b1", "w2", "b2", "ln2_w", "ln2_b")]


class EsmDesc(C.Structure):
    _fields_ = [("d", i32), ("n_layers", i32), ("n_heads", i32), ("ffn", i32), ("vocab", i32), ("ln_eps", C.c_float),
                ("rope_mode", i32), ("embed", vp), ("final_ln_w", vp), ("final_ln_b", vp), ("rope_cos", vp),
                ("rope_sin", vp), ("layers", C.POINTER(EsmLayer))]


class LlamaLayer(C.Structure):
    _fields_ = [(n, vp) for n in ("wqkv", "wo", "wgu", "wdown", "ln1", "ln2")]


class LlamaLayerFp8(C.Structure):
    _fields_ = [(n, vp) for n in ("wqkv", "wo", "wgu", "wdown", "sqkv", "so", "sgu", "sdown")]


class LlamaDesc(C.Structure):
    _fields_ = [("vocab", i32), ("d", i32), ("n_layers", i32), ("n_heads", i32), ("n_kv_heads", i32), ("head_dim", i32),
                ("ffn", i32), ("max_pos", i32), ("rms_eps", C.c_float), ("rms_cast", i32), ("embed", vp),
                ("final_norm", vp), ("lm_head", vp), ("rope_cos", vp), ("rope_sin", vp), ("layers", C.POINTER(LlamaLayer)),
                ("layers_fp8", C.POINTER(LlamaLayerFp8))]


class LlamaLayerF32(C.Structure):
    # (pcy_f32_llama_layer: the fp32 decoder layer of the stream step; gate and up stay separate matrices)
    _fields_ = [(n, vp) for n in ("wqkv", "wo", "wg", "wu", "wd", "ln1", "ln2")]


class LlamaDescF32(C.Structure):
    _fields_ = [("vocab", i32), ("d", i32), ("n_layers", i32), ("n_heads", i32), ("n_kv_heads", i32), ("head_dim", i32), ("ffn", i32),
                ("max_pos", i32), ("rms_eps", C.c_float), ("embed", vp), ("final_norm", vp), ("lm_head", vp), ("rope_cos", vp), ("rope_sin", vp),
                ("layers", C.POINTER(LlamaLayerF32))]


class KvCacheF32(C.Structure):
    _fields_ = [("k", vp), ("v", vp), ("B", i32), ("Tmax", i32)]


class KvCache(C.Structure):
    # (the trailing fields: an optional shared prefix, all zero = a plain cache -- include/pcy.h)
    _fields_ = [("k", vp), ("v", vp), ("B", i32), ("Tmax", i32), ("prefix_k", vp), ("prefix_v", vp), ("prefix_B", i32), ("prefix_T", i32),
                ("rows_per_prefix", i32)]


class PrefixGroups(C.Structure):
    # (pcy_prefix_groups: rows / len are HOST arrays, the d_* tables live on the device)
    _fields_ = [("n_groups", i32), ("t_own", i32), ("rows", C.POINTER(i32)), ("len", C.POINTER(i32)), ("d_row0", vp), ("d_len", vp), ("d_row_grp", vp)]


class GenState(C.Structure):
    _fields_ = [("pos", vp), ("step", vp), ("next_tok", vp), ("tokens_out", vp), ("logprob", vp), ("logits", vp),
                ("logits_all", vp), ("keep", vp), ("max_steps", i32), ("logits_all_ld", i32),
                # (the trailing fields: the EOS stop of the greedy and sampling picks, all zero = no stop -- include/pcy.h)
                ("finished", vp), ("done", vp), ("n_steps_run", vp), ("eos_id", i32)]


class LookState(C.Structure):
    # (pcy_look_state: the device-side state of greedy decoding with lookahead, beside a one-row GenState)
    _fields_ = [("hist", vp), ("n_hist", vp), ("window", vp), ("forced", vp), ("counters", vp), ("last", vp), ("cap", i32), ("W", i32),
                ("ngram_max", i32), ("ngram_min", i32)]


class BeamState(C.Structure):
    _fields_ = [("out", vp), ("max_len", i32), ("cur", vp), ("cur_new", vp), ("next_tok", vp), ("src", vp), ("anc", vp),
                ("has_eos", vp), ("blk_eos", vp), ("ticket", vp), ("pos", vp), ("step", vp), ("done", vp), ("eos_id", i32)]


# name -> (restype, argtypes); every symbol include/pcy.h declares
SIGNATURES = {
    "pcy_abi_version": (ci, []),
    "pcy_debug_dispatch_count": (C.c_ulonglong, [ci]),
    "pcy_last_error": (C.c_char_p, []),
    "pcy_ctx_create": (ci, [ci, vp, C.POINTER(vp)]),
    "pcy_ctx_destroy": (None, [vp]),
    "pcy_ctx_sync": (ci, [vp]),
    "pcy_timer_start": (ci, [vp]),
    "pcy_timer_stop": (ci, [vp, C.POINTER(C.c_float)]),
    "pcy_gemm": (ci, [vp, vp, ci, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci]),
    "pcy_gemv": (ci, [vp, vp, vp, ci, vp, vp, vp, ci, vp, C.c_float, ci, ci, ci, ci, ci]),
    "pcy_lm_head_xent": (ci, [vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp]),
    "pcy_lm_head_xent_ws_bytes": (C.c_size_t, [ci, ci]),
    "pcy_llama_score": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), vp, vp, vp, vp, vp, ci, ci, vp, vp, ci, vp, vp, ci, vp]),
    "pcy_decode_mlp": (ci, [vp, vp, vp, vp, vp, ci, ci, C.c_float, ci]),
    "pcy_rmsnorm": (ci, [vp, vp, vp, vp, ci, ci, C.c_float, ci]),
    "pcy_layernorm": (ci, [vp, vp, vp, vp, vp, ci, ci, C.c_float]),
    "pcy_embed_splice": (ci, [vp, vp, vp, vp, vp, vp, ci, ci]),
    "pcy_rope": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, vp, ci, ci, C.c_float]),
    "pcy_attention": (ci, [vp, vp, ci, ci, vp, ci, ci, vp, ci, ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, C.c_float]),
    "pcy_debug_attn_route_count": (C.c_ulonglong, [ci]),
    "pcy_debug_gemv_route_count": (C.c_ulonglong, [ci]),
    "pcy_attn_decode": (ci, [vp, vp, ci, vp, vp, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci, ci]),
    "pcy_attn_extend": (ci, [vp, vp, ci, C.POINTER(KvCache), ci, vp, ci, ci, vp, vp, vp, ci, ci, ci, ci, ci]),
    "pcy_attn_extend_packed": (ci, [vp, vp, ci, C.POINTER(KvCache), ci, vp, ci, ci, vp, vp, vp, ci, ci, ci, ci, ci]),
    "pcy_attn_extend_grouped": (ci, [vp, vp, ci, C.POINTER(KvCache), C.POINTER(PrefixGroups), ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci]),
    "pcy_pool": (ci, [vp, vp, ci, vp, vp, ci, ci, vp]),
    "pcy_retrieval_scores": (ci, [vp, vp, ci, vp, ci, ci, vp]),
    "pcy_comm_unique_id": (ci, [vp]),
    "pcy_comm_init": (ci, [vp, ci, ci, vp, C.POINTER(vp)]),
    "pcy_comm_destroy": (None, [vp]),
    "pcy_allgather": (ci, [vp, vp, vp, vp, C.c_size_t]),
    "pcy_retrieval_topk": (ci, [vp, vp, ci, vp, ci, ci, ci, vp, vp]),
    "pcy_retrieval_scores_f32": (ci, [vp, vp, ci, vp, ci, ci, ci, vp]),
    "pcy_retrieval_topk_f32": (ci, [vp, vp, ci, vp, ci, ci, ci, ci, vp, vp]),
    "pcy_qa_probs": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]),
    # fp32 operator family (include/pcy.h: callers that never call .bfloat16())
    "pcy_f32_linear": (ci, [vp, vp, ci, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci]),
    "pcy_f32_layernorm": (ci, [vp, vp, vp, vp, vp, ci, ci, C.c_float]),
    "pcy_f32_rmsnorm": (ci, [vp, vp, vp, vp, ci, ci, C.c_float]),
    "pcy_f32_rope": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, vp, ci, C.c_float]),
    "pcy_f32_embed": (ci, [vp, vp, vp, vp, vp, vp, ci, ci]),
    "pcy_f32_esm_embed": (ci, [vp, vp, vp, vp, ci, ci, vp, ci, ci]),
    "pcy_f32_silu_mul": (ci, [vp, vp, vp, vp, C.c_size_t]),
    "pcy_f32_acc_rows": (ci, [vp, vp, ci, vp, vp, ci, ci]),
    "pcy_f32_pool": (ci, [vp, vp, ci, vp, vp, ci, ci, vp]),
    "pcy_f32_attention": (ci, [vp, vp, ci, ci, vp, ci, ci, vp, ci, ci, vp, ci, vp, vp, ci, ci, ci, ci, ci, ci, C.c_float]),
    "pcy_f32_attn_decode": (ci, [vp, vp, ci, vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, ci, C.c_float]),
    "pcy_f32_attn_extend": (ci, [vp, vp, ci, vp, vp, ci, ci, vp, vp, ci, vp, ci, ci, ci, ci, ci, ci, ci, C.c_float]),
    "pcy_f32_lm_head_xent": (ci, [vp, vp, ci, vp, ci, ci, ci, vp, vp, vp, vp, vp]),
    "pcy_f32_lm_head_xent_ws_bytes": (C.c_size_t, [ci, ci]),
    # fp32 generation on the streaming GEMV (include/pcy.h)
    "pcy_f32_gemv": (ci, [vp, vp, vp, vp, ci, vp, ci, vp, ci, ci, ci, ci, ci]),
    "pcy_f32_attn_decode_pos": (ci, [vp, vp, ci, vp, vp, ci, ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, C.c_float]),
    "pcy_f32_llama_decode": (ci, [vp, C.POINTER(LlamaDescF32), C.POINTER(KvCacheF32), C.POINTER(GenState), ci]),
    "pcy_f32_llama_decode_graph": (ci, [vp, C.POINTER(LlamaDescF32), C.POINTER(KvCacheF32), C.POINTER(GenState), ci]),
    "pcy_f32_greedy_pick": (ci, [vp, C.POINTER(LlamaDescF32), C.POINTER(KvCacheF32), C.POINTER(GenState), ci, ci]),
    "pcy_f32_llama_greedy": (ci, [vp, C.POINTER(LlamaDescF32), C.POINTER(KvCacheF32), C.POINTER(GenState), ci, ci, ci]),
    "pcy_debug_f32_stream_count": (C.c_ulonglong, []),
    # fp32 selection on the device (include/pcy.h)
    "pcy_f32_beam_step": (ci, [vp, vp, ci, ci, ci, ci, C.c_float, C.POINTER(BeamState)]),
    "pcy_f32_kv_reorder_range": (ci, [vp, C.POINTER(LlamaDescF32), C.POINTER(KvCacheF32), vp, ci, ci, ci]),
    "pcy_f32_kv_copy_rows": (ci, [vp, C.POINTER(LlamaDescF32), C.POINTER(KvCacheF32), C.POINTER(KvCacheF32), vp, ci, ci]),
    "pcy_f32_llama_beam_steps": (ci, [vp, C.POINTER(LlamaDescF32), C.POINTER(KvCacheF32), C.POINTER(GenState), ci, ci, ci, C.c_float,
                                      C.POINTER(BeamState), vp, ci, ci]),
    "pcy_f32_sample_pick": (ci, [vp, C.POINTER(LlamaDescF32), C.POINTER(KvCacheF32), C.POINTER(GenState), ci, ci, C.c_float, C.c_float, vp, vp]),
    "pcy_f32_llama_sample": (ci, [vp, C.POINTER(LlamaDescF32), C.POINTER(KvCacheF32), C.POINTER(GenState), ci, ci, C.c_float, C.c_float, vp, ci]),
    "pcy_debug_f32_select_count": (C.c_ulonglong, [ci]),
    "pcy_quant_rows_fp8": (ci, [vp, vp, ci, ci, ci, vp, vp]),
    "pcy_gemm_fp8": (ci, [vp, vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci]),
    "pcy_mlp_forward": (ci, [vp, C.POINTER(MlpDesc), vp, ci, vp]),
    "pcy_esm_encode": (ci, [vp, C.POINTER(EsmDesc), vp, vp, vp, vp, ci, ci, ci, ci, ci, vp]),
    "pcy_llama_prefill": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), vp, vp, vp, vp, vp, ci, ci, vp, ci, vp, vp, vp, ci, vp]),
    "pcy_llama_prefill_all": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), vp, vp, vp, vp, vp, ci, ci, vp, ci, vp, vp]),
    "pcy_llama_extend": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), vp, vp, ci, ci, ci, vp, ci, vp, vp, vp, vp, ci, vp]),
    "pcy_llama_extend_packed": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), vp, vp, ci, ci, ci, vp, ci, vp, vp, vp, vp, ci, vp]),
    "pcy_llama_extend_grouped": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(PrefixGroups), vp, vp, ci, ci, ci, vp, ci, vp, vp, vp, vp,
                                      ci, vp]),
    "pcy_debug_extend_grouped_count": (C.c_ulonglong, []),
    "pcy_llama_extend_ws_bytes": (C.c_size_t, [C.POINTER(LlamaDesc), ci, ci, ci, ci]),
    "pcy_llama_decode": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci]),
    "pcy_debug_mc_trace": (ci, [vp, ci]),
    "pcy_llama_decode_layers": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci, ci]),
    "pcy_llama_decode_graph": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci]),
    "pcy_llama_decode_gemm": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci]),
    "pcy_debug_decode_gemm_count": (C.c_ulonglong, []),
    "pcy_attn_decode_shared": (ci, [vp, vp, ci, C.POINTER(KvCache), ci, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci]),
    "pcy_llama_decode_gemm_mq": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci]),
    "pcy_debug_attn_mq_count": (C.c_ulonglong, []),
    "pcy_attn_decode_split": (ci, [vp, vp, ci, C.POINTER(KvCache), ci, vp, ci, vp, vp, vp, vp, ci, ci, ci, ci]),
    "pcy_attn_split_chunk_keys": (ci, [ci, ci, ci, ci, ci, ci]),
    "pcy_llama_decode_split": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci]),
    "pcy_llama_decode_gemm_split": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci]),
    "pcy_debug_attn_split_count": (C.c_ulonglong, []),
    "pcy_gemv_w8": (ci, [vp, vp, vp, vp, ci, vp, vp, ci, vp, C.c_float, ci, ci, ci, ci, ci]),
    "pcy_llama_decode_w8": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(LlamaLayerFp8), C.POINTER(KvCache), C.POINTER(GenState), ci]),
    "pcy_llama_greedy_w8": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(LlamaLayerFp8), C.POINTER(KvCache), C.POINTER(GenState), ci, ci, ci]),
    "pcy_debug_decode_w8_count": (C.c_ulonglong, []),
    "pcy_greedy_pick": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci, ci]),
    "pcy_look_draft": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(LookState), C.POINTER(GenState), vp]),
    "pcy_look_verify": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(LookState), C.POINTER(GenState), vp]),
    "pcy_debug_look_count": (C.c_ulonglong, [ci]),
    "pcy_attn_window": (ci, [vp, vp, ci, C.POINTER(KvCache), ci, vp, ci, vp, vp, vp, ci, ci, ci, ci]),
    "pcy_attn_window_chunk": (ci, []),
    "pcy_llama_decode_window": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), vp, ci, vp]),
    "pcy_debug_decode_window_count": (C.c_ulonglong, []),
    "pcy_llama_greedy": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci, ci, ci]),
    "pcy_sample_pick": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci, ci, C.c_float, C.c_float, vp, vp]),
    "pcy_llama_sample": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci, ci, C.c_float, C.c_float, vp]),
    "pcy_beam_step": (ci, [vp, vp, ci, ci, ci, ci, C.c_float, C.POINTER(BeamState)]),
    "pcy_kv_reorder": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), vp, ci, ci]),
    "pcy_kv_reorder_range": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), vp, ci, ci, ci]),
    "pcy_llama_beam_steps": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci, ci, ci, C.c_float, C.POINTER(BeamState), vp, ci, ci]),
    "pcy_llama_beam_steps_split": (ci, [vp, C.POINTER(LlamaDesc), C.POINTER(KvCache), C.POINTER(GenState), ci, ci, ci, C.c_float, C.POINTER(BeamState), vp, ci, ci]),
}

_lib = None


class PcyError(RuntimeError):
    pass


def load():
    """dlopen libpcy.so and type every entry point.  Raises if the library or a symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PcyError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(the ProCyon engine has no CPU/torch fallback)")
    # torch first: it ships its own libamdhip64; loading libpcy.so before it binds the engine to /opt/rocm's copy and the
    # process ends up with two HIP runtimes (the second one then reports "no ROCm-capable device")
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.pcy_abi_version() != ABI_VERSION:
        raise PcyError("libpcy.so ABI version mismatch")
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().pcy_last_error()
        raise PcyError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")
