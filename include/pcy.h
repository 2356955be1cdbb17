/* pcy.h -- C ABI of the MI355X-native ProCyon forward/generation engine (libpcy.so).
 *
 * The reference (mims-harvard/ProCyon) is pure Python and has no FFI; this ABI is the boundary
 * the build introduces BELOW the reference's sub-module waist:
 *
 *   LlamaPostTokenization.forward   procyon/model/pmc_llama.py:546-596     -> pcy_llama_prefill / pcy_llama_decode*
 *   ESM_PLM.forward                 procyon/model/esm.py:504-558           -> pcy_esm_encode + pcy_pool
 *   ProteinPooler.forward           procyon/model/esm.py:131-173           -> pcy_pool
 *   create_mlp stacks               procyon/model/model_utils.py:13-41     -> pcy_mlp_forward
 *   _prepare_input_embeddings       procyon/model/model_unified.py:1135    -> pcy_embed_splice
 *   _generate_sampling (greedy)     procyon/model/model_unified.py:861-921 -> pcy_llama_greedy
 *
 * Conventions: plain pointers and sizes only.  Every `const void*` / `void*` tensor argument is a
 * DEVICE pointer to bf16 (raw 16-bit) data unless stated; int32 index arrays are device pointers
 * too.  The caller owns all tensors (the engine never frees them); the engine owns only its
 * scratch workspace.  Every call enqueues on the context's HIP stream and returns without
 * synchronising.  Return value 0 = ok, otherwise an error code with text in pcy_last_error()
 * (thread-local).  Nothing throws across the ABI.  One context per device/stream; a context is
 * not thread-safe.
 */
#ifndef PCY_H
#define PCY_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCY_ABI_VERSION 13

typedef struct pcy_ctx pcy_ctx;

/* epilogue selectors of pcy_gemm / pcy_gemv (bf16 rounding points in procyon_amd/csrc/pcy_common.h) */
enum { PCY_EPI_STORE = 0, PCY_EPI_RESID = 1, PCY_EPI_GELU_ERF = 2, PCY_EPI_GELU_ESM = 3, PCY_EPI_SWIGLU = 4 };
/* pooling modes of ProteinPooler (esm.py:138-149) */
enum { PCY_POOL_MEAN = 0, PCY_POOL_MEAN_CORRECTED = 1, PCY_POOL_MAX = 2 };

int pcy_abi_version(void);
/* Test instrumentation: number of launches that went to kernel family `kind` since the library was loaded.  GEMMs -- 0: 128x128 tiles,
 * 1: 64x64, 2: 256x256, 3: 256x256 persistent (ESM fc1 + GELU), 4: split-K, 5: fp8 256x256, 8: mid tiles; 6: single-pass ESM attention;
 * 9: ESM layers through a captured graph.  Decode steps, ONE count per step enqueued outside a graph replay, by what served it --
 * 7: one row, all layers in one launch, grouped-query geometry; 10: the same, multi-head geometry; 11: one row, a launch per layer;
 * 12: small-batch step (2..8 rows); 13: mid-batch step (9..32 rows, PCY_MB_MAX); 14: launch per stage, streaming GEMVs;
 * 15: launch per stage, MFMA GEMVs; 16: a step served from a shared-prefix cache (pcy_kv_cache.prefix_k), counted in addition to 14 / 15.
 * 17: calls of the fused lm_head x cross-entropy operator (pcy_lm_head_xent, also inside pcy_llama_score / pcy_llama_extend).
 * 18: calls of pcy_llama_extend (S more tokens per row against a filled cache).
 * 19: calls of pcy_llama_extend_packed (each also counts as kind 18).  A pcy_llama_extend_grouped call counts as kind 18, as kind 19 when
 * packed, and in pcy_debug_extend_grouped_count() below.
 * A fused step may decline at launch time (LDS size for the cache length, co-residency) and the step
 * then runs launch by launch with the same bits.  Parity tests use the counters to assert that they reach the kernel they claim to test. */
unsigned long long pcy_debug_dispatch_count(int kind);
/* calls of pcy_llama_extend_grouped (each also counts as kind 18, and as kind 19 when packed) */
unsigned long long pcy_debug_extend_grouped_count(void);
const char* pcy_last_error(void);
/* stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) or NULL for the default stream */
int pcy_ctx_create(int device_id, void* stream, pcy_ctx** out);
void pcy_ctx_destroy(pcy_ctx* ctx);
int pcy_ctx_sync(pcy_ctx* ctx);
/* HIP-event timer on the context's stream (bench.py roofline leg): start, stop -> elapsed ms */
int pcy_timer_start(pcy_ctx* ctx);
int pcy_timer_stop(pcy_ctx* ctx, float* ms_out);

/* ---- primitive ops (unit parity tests; also what the host composes for odd shapes) ---------- */
/* C[M,N] = epi(A[M,K] . W[N,K]^T + bias); EPI_SWIGLU: W is [N,K] with 16-row gate/up interleave, C is [M,N/2] (bias and resid are not read).
 * Rounding points: bf16(acc + bias), then bf16(. + resid) (EPI_RESID) or the bf16 -> bf16 activation; SwiGLU bf16(bf16(silu(bf16 g)) * bf16 u).
 * Operands (all bf16; lda / ldr / ldc = elements between rows):
 *   A [M, K] at stride lda, W [N, K] contiguous: read as 16-byte pieces of a row by LDS-DMA -- A and W 16-byte aligned, lda % 8 == 0,
 *     lda >= K, K a positive multiple of 64.  Rows M.. of A and N.. of W are never read, nor columns K.. of a row of A.
 *   C [M, N] at stride ldc >= N (N/2 for SwiGLU), resid [M, N] at stride ldr >= N (EPI_RESID only), bias [N] or NULL: any 2-byte aligned
 *     address and any stride.  The kernels move them as 8- or 16-byte pieces where strides, N and the three addresses allow it and element
 *     by element otherwise, with the same bits; only columns [0, N) of rows [0, M) are read or written.
 *   resid may be C itself with ldr == ldc (in place: every element is read before it is written, by the same lane); any other overlap of
 *     C with an input is outside the contract.
 *   EPI_SWIGLU: N % 32 == 0, and the store is one 8-byte piece per four features with no element-wise form: C 8-byte aligned, ldc % 4 == 0.
 * M == 0 or N == 0 returns 0 without a launch.  Refused with code 1 before any launch (C untouched): anything else -- an unknown epi, a NULL A /
 * W / C, EPI_RESID without resid, a negative size, K, lda, ldc, ldr or an alignment outside the above. */
int pcy_gemm(pcy_ctx*, const void* A, int lda, const void* W, const void* bias, const void* resid, int ldr,
             void* C, int ldc, int M, int N, int K, int epi);
/* y[B,N] = epi(x[B,K] . W[N,K]^T + bias); rms_w != NULL fuses RMSNorm(x)*rms_w in front (rms_cast 0: >=4.32, 1: 4.31; STORE / SWIGLU only,
 * min(B, 4) rows of x within 64 KiB).  EPI_SWIGLU: N = features, W is [2N, K] in the 16-row gate/up interleave, bias and resid are not read.
 * Operands (bf16): W [N, K] contiguous, x [B, K] at stride ldx, rms_w [K]: read as 16-byte pieces -- W, x, rms_w 16-byte aligned, K > 0,
 *   K % 8 == 0, ldx % 8 == 0, ldx >= K.  y [B, N] and resid [B, N] (EPI_RESID only) BOTH at stride ldy >= N, bias [N] or NULL: any 2-byte
 *   aligned address; 8-byte stores are used where ldy and y allow them, single elements otherwise, same bits.  resid may be y itself.
 *   EPI_SWIGLU: N % 16 == 0, y 8-byte aligned and ldy % 4 == 0 (the MFMA kernels store four features as one piece, no other form).
 * Only columns [0, N) of rows [0, B) of y are written.  N == 0 or B == 0 returns 0 without a launch; everything outside the above is refused
 * with code 1 before any launch (y untouched).  A row's bits depend neither on the other rows nor, among calls served by one kernel
 * (pcy_debug_gemv_route_count), on B; the streaming and the MFMA kernels add in different orders. */
int pcy_gemv(pcy_ctx*, const void* W, const void* x, int ldx, const void* bias, const void* resid, void* y, int ldy,
             const void* rms_w, float rms_eps, int rms_cast, int N, int K, int B, int epi);
/* One token through a Llama MLP, in place: x[d] += (silu(g) * u) . Wdown^T with [g; u] = (RMSNorm(x) * ln2) . Wgu^T
   (transformers LlamaDecoderLayer.forward: post_attention_layernorm -> LlamaMLP -> residual, as run per generated token by
   model_unified.py:883-915).  wgu: [2*ffn, d] in the 16-row gate/up interleave of pcy_gemv(EPI_SWIGLU); wdown: [d, ffn].
   Llama-3-8B geometry runs as ONE launch (the decode step's MLP chain kernel), anything else as the two pcy_gemv launches;
   same bits either way. */
int pcy_decode_mlp(pcy_ctx*, void* x, const void* ln2, const void* wgu, const void* wdown, int d, int ffn, float rms_eps, int rms_cast);
int pcy_rmsnorm(pcy_ctx*, const void* x, const void* w, void* y, int rows, int d, float eps, int cast);
int pcy_layernorm(pcy_ctx*, const void* x, const void* w, const void* b, void* y, int rows, int d, float eps);
/* out[r] = soft_map[r] >= 0 ? soft[soft_map[r]] : table[ids[r]]   (model_unified.py:1146-1167) */
int pcy_embed_splice(pcy_ctx*, const void* table, const int32_t* ids, const void* soft, const int32_t* soft_map,
                     void* out, int rows, int d);
/* In-place rotary on heads [0,nh) at column col0 of a token-major buffer [ntok, ld]; pos[tok] = position.
 * mode 0: (x*cos)+(rotate_half(x)*sin) with every op rounded to bf16 (HF Llama); mode 1: fp32, rounded once
 * (HF Esm).  prescale != 0 multiplies (and rounds) first: ESM's q * head_dim^-0.5.
 * Refused with code 1 before any launch (buf untouched): dh % 16 != 0 (the kernel moves 8-element chunks of each half head),
 * ld % 8 != 0 or col0 % 8 != 0 (16-byte accesses; buf, cos_t, sin_t 16-byte aligned), col0 + nh*dh > ld. */
int pcy_rope(pcy_ctx*, void* buf, int ld, int col0, int nh, int dh, const int32_t* pos, const void* cos_t,
             const void* sin_t, int ntok, int mode, float prescale);
/* Exact-rounding eager attention over packed sequences (cu/vt_cu as in pcy_esm_encode): q,k,v token-major with
 * head h at column col0 + h*dh; O = bf16( bf16(softmax_fp32( bf16(bf16(QK^T)*scale) + mask )) . V ).
 * keep: per-token key mask (attention_mask) or NULL; causal != 0 adds the causal mask; GQA when Hkv < H. */
int pcy_attention(pcy_ctx*, const void* q, int ldq, int qcol0, const void* k, int ldk, int kcol0, const void* v, int ldv,
                  int vcol0, void* o, int ldo, const int32_t* cu, const int32_t* vt_cu, const uint8_t* keep, int nseq,
                  int max_len, int vt_total, int H, int Hkv, int dh, int causal, float scale);
/* Test instrumentation: launches of the two-pass prefill attention since the library was loaded, by the kernel that the launcher chose
 * (pcy_attention, pcy_esm_encode, pcy_llama_prefill and every other caller of it) -- 0: head_dim 32; 1: head_dim 64; 2: head_dim 128, one
 * 16-row query tile per wave; 3: head_dim 128, two query tiles per wave (large grids); anything else reads 0.  The single-pass ESM kernel
 * counts as kind 6 of pcy_debug_dispatch_count and under none of these.  Words of their own, as pcy_debug_look_count: the kinds of
 * pcy_debug_dispatch_count are pinned.  Kernels 2 and 3 give one sequence the same bits (same key-block order, same rounding points). */
unsigned long long pcy_debug_attn_route_count(int which);
/* Test instrumentation: launches of pcy_gemv (and of every other caller of its launcher: the launch-per-stage decode steps) since the library
 * was loaded, by the kernel chosen, counted where the launch is decided -- 0: streaming, 2-row units; 1: streaming, 4-row units (N >= 8189);
 * 2: chunked (min(B, 4) rows of x exceed 64 KiB of LDS); 3: MFMA, weights through registers (PCY_DISABLE=gemv_lds); 4: MFMA, weights by
 * LDS-DMA, x one chunk ahead (PCY_DISABLE=gemv_mfma4); 5: MFMA, x and weights as pairs (B >= 4, K % 128 == 0, no fused norm); anything else
 * reads 0.  One count per launch: a batch is served in passes of 4 rows (0 - 2) or 32 rows (3 - 5).  Words of their own, as
 * pcy_debug_attn_route_count.  Kernels 3, 4 and 5 issue the same MFMAs in the same order (same bits); the streaming kernels add in another
 * order. */
unsigned long long pcy_debug_gemv_route_count(int which);
/* Decode attention of ONE new token per row against the [B,Hkv,Tmax,dh] cache: ropes q and the new k at position
 * *pos (device scalar = cache length), appends K,V at slot *pos, attends slots [0,*pos] (keep: optional [B,Tmax]
 * key mask, NULL = the reference's unmasked decode, quirk Q1).  qkv [B,(H+2Hkv)*dh] un-roped projections.
 * keep[b*Tmax + j] != 0 (any non-zero byte): row b attends cached slot j < *pos.  Slot *pos itself (the new token) is always
 * attended; bytes at and above *pos are not read. */
int pcy_attn_decode(pcy_ctx*, void* qkv, int ld, void* kcache, void* vcache, void* o, int ldo, const int32_t* pos,
                    const void* cos_t, const void* sin_t, const uint8_t* keep, int B, int H, int Hkv, int dh, int Tmax);
/* pooled[i] over the token ranges rng[2*r],rng[2*r+1] = (start,len), r in [seg[i], seg[i+1])  (esm.py:131-173) */
int pcy_pool(pcy_ctx*, const void* hidden, int d, const int32_t* seg, const int32_t* rng, int nprot, int mode, void* out);

/* Retrieval scoring (evaluate/framework/procyon.py:400-406, data/inference_utils.py:955-960):
 * sims[Q,N] = F.normalize(query) @ F.normalize(targets)^T in bf16 (norm rounded to bf16, then the division, then an
 * fp32-accumulating matmul rounded once).  D must be a multiple of 64. */
int pcy_retrieval_scores(pcy_ctx*, const void* query, int Q, const void* targets, int N, int D, void* sims_out);

/* ---- the one collective of the path: all-gather of the per-rank embedding blocks over RCCL / xGMI --------------------------
 * (reference pattern: training/trainIT.py:1594-1610, torch.distributed.all_gather of the shards of SequentialDistributedSampler).
 * One rank calls pcy_comm_unique_id (128 bytes) and distributes the id by any host channel (torch.distributed's store, MPI,
 * a file); every rank then calls pcy_comm_init.  pcy_allgather: recvbuf [nranks * bytes] = every rank's sendbuf [bytes] in
 * rank order, enqueued on the context's stream.  RCCL is dlopen'ed at first use (no link-time dependency). */
int pcy_comm_unique_id(void* id128);
int pcy_comm_init(pcy_ctx*, int nranks, int rank, const void* id128, void** comm_out);
void pcy_comm_destroy(void* comm);
int pcy_allgather(pcy_ctx*, void* comm, const void* sendbuf, void* recvbuf, size_t bytes);

/* Retrieval ranking (data/inference_utils.py:921-978 `get_proteins_from_embedding`): the same similarities, then per query the
 * k best targets in stable descending order (ties: the lower index first; torch.argsort leaves them open) -> idx_out [Q,k]
 * int32, score_out [Q,k] bf16.  1 <= k <= N; k == N is the full ranking (top_k=None). */
int pcy_retrieval_topk(pcy_ctx*, const void* query, int Q, const void* targets, int N, int D, int k, int32_t* idx_out, void* score_out);

/* The same two operations with fp32 similarities (the shim's `get_proteins_from_embedding` / `get_proteins_from_batched_embeddings`,
 * data/inference_utils.py:921-999: cached target matrices are fp32 and the batched form returns `.float()` scores):
 * sims[q][n] = (q / max(|q|, 1e-12)) . (t_n / max(|t_n|, 1e-12)), fp32 accumulation, fp32 result; query [Q,D] fp32, targets [N,D]
 * fp32 (targets_bf16 = 0) or bf16 (1); D % 4 == 0.  topk: idx_out [Q,k] int32, score_out [Q,k] fp32, stable descending order
 * (ties, incl. -0.0 vs +0.0: the lower index first). */
int pcy_retrieval_scores_f32(pcy_ctx*, const float* query, int Q, const void* targets, int targets_bf16, int N, int D, float* sims_out);
int pcy_retrieval_topk_f32(pcy_ctx*, const float* query, int Q, const void* targets, int targets_bf16, int N, int D, int k, int32_t* idx_out,
                           float* score_out);

/* QA read-out (reference: procyon/data/inference_utils.py:582-604, procyon/training/train_utils.py:1048-1070: `preds = logits.softmax(dim=-1)`
 * at the answer row, then the yes / no columns or the argmax).  logits [rows, V] bf16 (is_f32 = 0: fp32 statistics, ONE rounding of
 * exp(x - max) / sum, torch.softmax on a bf16 tensor) or fp32 (is_f32 = 1).  Optional outputs (NULL = not wanted): probs_out [rows, V] in
 * the logits' dtype; yes_no_out [rows, 2] fp32 = the stored probabilities of yes_id / no_id; argmax_out [rows] int32 = argmax of the stored
 * probabilities, lowest index on ties.  -inf logits are allowed and mean "never chosen" (stored probability exactly 0); a row must hold
 * at least one finite logit; NaN logits are outside the contract. */
int pcy_qa_probs(pcy_ctx*, const void* logits, int is_f32, int rows, int V, int yes_id, int no_id, void* probs_out, float* yes_no_out,
                 int32_t* argmax_out);

/* Teacher-forced scoring: lm_head x cross-entropy WITHOUT the [M, V] logits in memory.  x [M, d] bf16 (ldx elements between rows, ldx % 8
 * == 0), already final-normed; W [V, d] bf16 = lm_head in natural row order; targets [M] int32 in [0, V).  Per row, HF's causal-LM loss
 * term (`logits = bf16(acc)`, `logits.float()`, fp32 cross_entropy):
 *   nll_out[m] = lse - label,  lse = max + log(sum_n exp(l[n] - max)) in fp32 over the bf16-ROUNDED logits l[n] = bf16(x[m] . W[n]),
 *   label = l[targets[m]].  Every l[n] is bit-equal to what pcy_gemm(x, W, EPI_STORE) stores.
 * Optional outputs (NULL = not wanted), [M] fp32: lse_out, row_max_out, label_logit_out (the last two hold bf16 values).  A target outside
 * [0, V) gives NaN.  Deterministic (no atomics) and row-invariant: a row's bits depend neither on M nor on the other rows.  d % 64 == 0;
 * M == 0 returns 0 without a launch.  Scratch: pcy_lm_head_xent_ws_bytes(M, V) of the context's workspace (host arithmetic only, callable
 * without a device): min(M, 1024) x (column blocks x 8 + 4) bytes, a few thousand times smaller than the logits it replaces. */
int pcy_lm_head_xent(pcy_ctx*, const void* x, int ldx, const void* W, int M, int V, int d, const int32_t* targets, float* nll_out,
                     float* lse_out, float* row_max_out, float* label_logit_out);
size_t pcy_lm_head_xent_ws_bytes(int M, int V);

/* ---- fp8 weight path (BASELINE.json configs[4]: "fp8 MFMA weight path"; the reference has no fp8 counterpart) ----
 * Per-row symmetric OCP e4m3 quantisation of a bf16 matrix x[rows,K] (ldx elements between rows, K % 8 == 0):
 * scale_out[r] = the smallest power of two >= 2^-126 with amax|x[r,:]| / scale <= 448 (1 for an all-zero row),
 * q_out[r,k] = e4m3_rne(x / scale) (exact division), q_out [rows,K] bytes.  Used once per weight matrix (per output
 * channel) and per call on activations (per token). */
int pcy_quant_rows_fp8(pcy_ctx*, const void* x, int ldx, int rows, int K, void* q_out, float* scale_out);
/* C[M,N] = epi( ((A8[M,K] . W8[N,K]^T) * sa[m]) * sw[n] ) on the MX-scaled 16x16x128 fp8 MFMA (unit block scales), fp32
 * accumulation, then the same bf16 rounding points as pcy_gemm.  epi in {STORE, RESID, SWIGLU}; K a positive multiple of 128.
 * Operands: A8 [M, K] and W8 [N, K] contiguous e4m3 bytes, 16-byte aligned; sa [M], sw [N] fp32, 4-byte aligned (sw is read as 16-byte
 * pieces where its address allows); C, resid, ldc, ldr, the in-place residual and the SwiGLU rule exactly as pcy_gemm; no bias.
 * Refused with code 1 before any launch (C untouched): everything outside that, as pcy_gemm. */
int pcy_gemm_fp8(pcy_ctx*, const void* A8, const float* sa, const void* W8, const float* sw, const void* resid, int ldr,
                 void* C, int ldc, int M, int N, int K, int epi);

/* ---- create_mlp projector (model_utils.py:13-41) -------------------------------------------- */
typedef struct {
  int32_t n_layers;          /* 1 (bias-free Linear) or >= 2 (Linear+bias -> GELU ... -> Linear+bias) */
  int32_t dims[9];           /* dims[0]=in, dims[i+1]=out of layer i */
  const void* w[8];          /* [dims[i+1], dims[i]] */
  const void* b[8];          /* [dims[i+1]] or NULL */
} pcy_mlp_desc;
int pcy_mlp_forward(pcy_ctx*, const pcy_mlp_desc*, const void* x, int M, void* out);

/* ---- ESM2 encoder (esm.py:504-538 -> fair-esm ESM2 / HF EsmModel) ---------------------------- */
typedef struct {
  const void *wqkv, *bqkv;   /* [3d,d],[3d]: query,key,value rows stacked */
  const void *wo, *bo;       /* [d,d],[d] */
  const void *ln1_w, *ln1_b; /* attention LayerNorm */
  const void *w1, *b1;       /* [F,d],[F] */
  const void *w2, *b2;       /* [d,F],[d] */
  const void *ln2_w, *ln2_b; /* FFN LayerNorm */
} pcy_esm_layer;
typedef struct {
  int32_t d, n_layers, n_heads, ffn, vocab;
  float ln_eps;
  int32_t rope_mode;         /* 1: fp32, rounded once (HF Esm) ; 0: three bf16 roundings (fair-esm) */
  const void* embed;         /* [vocab,d] */
  const void *final_ln_w, *final_ln_b;
  const void *rope_cos, *rope_sin; /* [max_len, d/n_heads] bf16 */
  const pcy_esm_layer* layers;     /* host array [n_layers] */
} pcy_esm_desc;
/* Packed varlen batch: tokens[ntok], sequence q = tokens[cu[q]..cu[q+1]); pos[tok] = index inside its
 * sequence; vt_cu[q] = sum over earlier sequences of roundup(len,32), vt_total = vt_cu[nseq].
 * mask_pads=1: fair-esm semantics (callers pack WITHOUT pad tokens); mask_pads=0: the HF-"official"
 * call without attention_mask (esm.py:533): pack the padded rows, pads take part as ordinary tokens.
 * hidden_out [ntok,d] = representations[repr_layer] (post final LayerNorm). */
int pcy_esm_encode(pcy_ctx*, const pcy_esm_desc*, const int32_t* tokens, const int32_t* pos, const int32_t* cu,
                   const int32_t* vt_cu, int ntok, int nseq, int max_len, int vt_total, int mask_pads, void* hidden_out);

/* ---- Llama decoder (pmc_llama.py:546-596 -> HF LlamaForCausalLM) ----------------------------- */
typedef struct {
  const void* wqkv;          /* [(H+2Hkv)*dh, d]: q,k,v rows stacked */
  const void* wo;            /* [d, H*dh] */
  const void* wgu;           /* [2F, d]: gate/up interleaved in blocks of 16 rows */
  const void* wdown;         /* [d, F] */
  const void *ln1, *ln2;     /* [d] */
} pcy_llama_layer;
/* optional e4m3 copies of the four projection matrices (same row order / interleave as the bf16 ones) and their per-row
 * scales (pcy_quant_rows_fp8).  When pcy_llama_desc.layers_fp8 != NULL, pcy_llama_prefill quantises the input of every
 * projection per token and runs it through pcy_gemm_fp8; norms, rope, attention, residuals, lm_head and the whole
 * decode path stay bf16.  (The opt-in step pcy_llama_decode_w8 below streams the same copies in cached decode; it takes them as an
 * argument of its own and does not look at layers_fp8.) */
typedef struct {
  const void *wqkv, *wo, *wgu, *wdown;
  const float *sqkv, *so, *sgu, *sdown;
} pcy_llama_layer_fp8;
typedef struct {
  int32_t vocab, d, n_layers, n_heads, n_kv_heads, head_dim, ffn, max_pos;
  float rms_eps;
  int32_t rms_cast;          /* 0: w*bf16(x_hat) ; 1: bf16(w*x_hat) (transformers 4.31, SURVEY App.B Q11) */
  const void* embed;         /* [vocab,d] */
  const void* final_norm;    /* [d] */
  const void* lm_head;       /* [vocab,d] */
  const void *rope_cos, *rope_sin; /* [max_pos, head_dim] bf16 (table precision is the caller's choice, Q9/Q10) */
  const pcy_llama_layer* layers;   /* host array [n_layers] */
  const pcy_llama_layer_fp8* layers_fp8; /* host array [n_layers] or NULL (bf16 weights everywhere) */
} pcy_llama_desc;
typedef struct {
  void* k;                   /* [L,B,Hkv,Tmax,dh] bf16: layer l rows = past_key_values[l][0] */
  void* v;                   /* same for values */
  int32_t B, Tmax;
  /* Optional shared prefix (all zero = the plain cache above, exactly).  prefix_k / prefix_v [L,prefix_B,Hkv,prefix_T,dh] bf16: an ordinary
   * prefill cache of prefix_B prompts with Tmax == prefix_T.  Row b of the decode batch reads prefix row b / rows_per_prefix (the beams of a
   * prompt share ONE copy of its K/V), and k / v above then hold only the SUFFIX: logical key slot j < prefix_T of row b is
   * prefix[b / rows_per_prefix][j], slot j >= prefix_T is k[b][j - prefix_T]; the logical capacity is prefix_T + Tmax.  *pos, the rotary
   * position and the `keep` mask (row stride = the logical capacity) stay in logical slots; a decode step appends at k[b][*pos - prefix_T] and
   * never writes the prefix.  Served by the launch-per-stage batched decode loop only (pcy_llama_decode / _decode_graph / _beam_steps /
   * _greedy / _sample with >= 4 rows on a geometry that loop covers): anything else is an argument error, never a fallback.
   * pcy_kv_reorder* move suffix slots only; the prefill entries reject such a cache. */
  void* prefix_k;
  void* prefix_v;
  int32_t prefix_B, prefix_T, rows_per_prefix;
} pcy_kv_cache;
/* Prefill: embeds [B,T,d]; keep [B*T] uint8 attention_mask or NULL; pos[B*T] rotary positions
 * (reference: arange(T) per row, Q2); cu/vt_cu [B+1] = b*T / b*roundup(T,32).
 * logit_rows[n_logit_rows] = token rows (b*T+t) whose logits are wanted -> logits_out [n_logit_rows, vocab];
 * hidden_out (optional) [B*T,d] = hidden_states[-1] (final-normed). K/V of slots [0,T) are written.
 * sum_rows[n_sum_rows] (optional) -> hidden_sum_out [n_sum_rows, d] = sum over ALL L+1 hidden states of those token rows
 * (ret_token_access='all', model_unified.py:560-563: fp32 accumulation, rounded once). */
int pcy_llama_prefill(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const void* embeds, const uint8_t* keep,
                      const int32_t* pos, const int32_t* cu, const int32_t* vt_cu, int B, int T,
                      const int32_t* logit_rows, int n_logit_rows, void* logits_out, void* hidden_out,
                      const int32_t* sum_rows, int n_sum_rows, void* hidden_sum_out);
/* The same prefill that additionally materialises what `LlamaPostTokenization.forward` hands back besides the logits
 * (pmc_llama.py:575-596, `output_hidden_states=True`): hidden_all_out [L+1][B*T][d] bf16 = the embeddings, the output of layers
 * 0..L-2 and the final-normed output of layer L-1.  logit_rows may name every row (the reference's [B,T,V] logits): more than 64
 * rows take the lm_head as an MFMA GEMM -- on THIS entry point only; pcy_llama_prefill always uses the fused-norm GEMV, so a row's
 * logits there do not depend on the number of rows requested. */
int pcy_llama_prefill_all(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const void* embeds, const uint8_t* keep,
                          const int32_t* pos, const int32_t* cu, const int32_t* vt_cu, int B, int T, const int32_t* logit_rows,
                          int n_logit_rows, void* logits_out, void* hidden_all_out);
/* The prefill of pcy_llama_prefill (same launches, K/V of slots [0,T) written) followed by teacher-forced scoring: the token rows
 * score_rows[n_score] (flat b*T + t) are gathered, final-normed (rms_cast honoured) and handed to pcy_lm_head_xent against
 * targets[n_score] -> nll_out [n_score] fp32.  logit_rows / logits_out as in pcy_llama_prefill (the GEMV path, same bits), so a QA batch gets
 * its answer logits and its loss from ONE pass.  layers_fp8: the projections run fp8 as in the prefill, the lm_head stays bf16.  A cache with
 * a shared prefix is rejected. */
int pcy_llama_score(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const void* embeds, const uint8_t* keep, const int32_t* pos,
                    const int32_t* cu, const int32_t* vt_cu, int B, int T, const int32_t* score_rows, const int32_t* targets, int n_score,
                    float* nll_out, const int32_t* logit_rows, int n_logit_rows, void* logits_out);
/* S new tokens per row against a filled cache.  qkv [B*S, ld] un-roped projections (row b*S+s = token s of row b).  Ropes q and k at
 * position t_past + s (every row: quirk Q2), writes K/V of token s to LOGICAL slot t_past + s of row b in layer `layer` of the cache,
 * then O[b*S+s] = attention of that query over logical slots [0, t_past + s] (causal), HF eager rounding points.
 * kv: plain cache (t_past + S <= Tmax) or shared-prefix cache (t_past >= prefix_T, t_past + S <= prefix_T + Tmax; slots < prefix_T are
 * read from prefix row b / rows_per_prefix and never written).  keep: optional [B, capacity] bytes in logical slots (row stride = the
 * logical capacity, as pcy_gen_state.keep), non-zero = kept; it applies to old AND new key slots; bytes at and above t_past + S are
 * not read; NULL = every slot kept.  A query with no kept key gets the reference's uniform softmax over all t_past + S slots.
 * head_dim 64 or 128, any H / Hkv.  The same logical contents in a shared-prefix cache and in a plain cache give the same bits, and a
 * row's bits do not depend on the other rows of the call. */
int pcy_attn_extend(pcy_ctx*, void* qkv, int ld, const pcy_kv_cache* kv, int layer, void* o, int ldo, int t_past,
                    const void* cos_t, const void* sin_t, const uint8_t* keep, int B, int S, int H, int Hkv, int dh);
/* pcy_attn_extend with another work split: the 64 query slots of a workgroup are packed over the rows of one prompt (rows b with the same
 * b / rows_per_prefix; a plain cache: one row) and the H / Hkv query heads of one kv head, so that the whole 32-key blocks of the shared prefix
 * are staged once per 64 packed queries instead of once per (row, head).  Same arguments, same argument errors, and the same bits in `o` and in
 * the cache as pcy_attn_extend for every input (tests/test_gpu_extend_packed.py). */
int pcy_attn_extend_packed(pcy_ctx*, void* qkv, int ld, const pcy_kv_cache* kv, int layer, void* o, int ldo, int t_past,
                           const void* cos_t, const void* sin_t, const uint8_t* keep, int B, int S, int H, int Hkv, int dh);
/* S more tokens per row through all layers against a filled cache (HF: forward(inputs_embeds [B,S], past_key_values)).  embeds [B,S,d];
 * t_past = tokens every row already holds; keep as pcy_attn_extend.  K/V of logical slots [t_past, t_past+S) are written.
 * logit_rows / logits_out / hidden_out as pcy_llama_prefill, rows counted b*S + s.  score_rows / targets / nll_out as pcy_llama_score
 * (n_score = 0: no scoring).  layers_fp8 != NULL is an argument error in this version.  The layer loop is the prefill's (same projections,
 * norms and tails); the attention is pcy_attn_extend's, so no transposed copy of V is made and pcy_llama_extend_ws_bytes depends on
 * B, S and the row counts only, never on t_past or the cache's size.  Argument errors (nothing is launched, the cache stays as it was):
 * t_past + S beyond the logical capacity or max_pos, a shared cache with t_past < prefix_T, B beyond the cache's rows or beyond
 * prefix_B * rows_per_prefix, S < 1, fp8 layers, a head_dim other than 64 / 128. */
int pcy_llama_extend(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const void* embeds, const uint8_t* keep, int B, int S, int t_past,
                     const int32_t* logit_rows, int n_logit_rows, void* logits_out, void* hidden_out,
                     const int32_t* score_rows, const int32_t* targets, int n_score, float* nll_out);
size_t pcy_llama_extend_ws_bytes(const pcy_llama_desc*, int B, int S, int n_logit_rows, int n_score);   /* host arithmetic only */
/* pcy_llama_extend with the attention of pcy_attn_extend_packed in every layer: same arguments, errors, workspace and bits. */
int pcy_llama_extend_packed(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const void* embeds, const uint8_t* keep, int B, int S,
                            int t_past, const int32_t* logit_rows, int n_logit_rows, void* logits_out, void* hidden_out,
                            const int32_t* score_rows, const int32_t* targets, int n_score, float* nll_out);
/* Grouped extension: the B rows of the call are n_groups contiguous groups.  Group g holds rows[g] rows (in order) that read prefix row g of the
 * cache, whose first len[g] <= prefix_T slots are real and start at position 0; slots at and above len[g] of that prefix row are never addressed.
 * A row's own panel starts right behind its group's prefix: logical slot j < len[g] is prefix[g][j] (panel stride prefix_T), slot j >= len[g] is
 * k[b][j - len[g]].  t_own >= 0 tokens already sit in every row's own panel; query s of a row of group g sits at logical slot (= rotary position)
 * len[g] + t_own + s and attends logical slots [0, len[g] + t_own + s]; K / V of the new tokens go to own slots [t_own, t_own + S) of every row.
 * keep: optional [B, prefix_T + Tmax] bytes in logical slots (so a row's bytes are packed against ITS len[g]); bytes at and above
 * len[g] + t_own + S are not read; a query without a kept key gets the uniform softmax over the row's len[g] + t_own + S keys.
 * The cache: prefix_k, prefix_v, prefix_B >= n_groups, prefix_T, a suffix capacity Tmax and rows_per_prefix == 0 (every other entry refuses such a
 * cache).  rows / len are HOST arrays (the argument checks read them); d_row0 [n_groups + 1] (prefix sums of rows), d_len [n_groups] and
 * d_row_grp [B] (row -> group) are DEVICE copies that the caller keeps equal to them and alive until the stream has run the call.
 * Bits: every row gets what it gets ALONE from pcy_attn_extend on a one-row plain cache with the same logical contents and
 * t_past = len[g] + t_own; packed != 0 (the work split of pcy_attn_extend_packed, a workgroup per (tile, kv head, group)) gives the same bits.
 * Argument errors (nothing is launched, the caches stay as they were): sum(rows) != B, B beyond the cache's rows, a rows[g] < 1, a len[g] outside
 * [1, prefix_T], t_own + S > Tmax, max(len) + t_own + S > max_pos (pcy_llama_extend_grouped), n_groups > prefix_B, a plain cache or one with
 * rows_per_prefix != 0, S < 1, fp8 layers, a head_dim other than 64 / 128. */
typedef struct {
  int32_t n_groups, t_own;
  const int32_t* rows;       /* HOST [n_groups], >= 1 */
  const int32_t* len;        /* HOST [n_groups], 1 <= len[g] <= prefix_T */
  const int32_t* d_row0;     /* DEVICE [n_groups + 1] */
  const int32_t* d_len;      /* DEVICE [n_groups] */
  const int32_t* d_row_grp;  /* DEVICE [B] */
} pcy_prefix_groups;
int pcy_attn_extend_grouped(pcy_ctx*, void* qkv, int ld, const pcy_kv_cache* kv, const pcy_prefix_groups* groups, int layer, void* o, int ldo,
                            const void* cos_t, const void* sin_t, const uint8_t* keep, int B, int S, int H, int Hkv, int dh, int packed);
/* pcy_llama_extend on groups: logit_rows .. nll_out and the workspace (pcy_llama_extend_ws_bytes) exactly as there */
int pcy_llama_extend_grouped(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_prefix_groups* groups, const void* embeds,
                             const uint8_t* keep, int B, int S, int packed, const int32_t* logit_rows, int n_logit_rows, void* logits_out,
                             void* hidden_out, const int32_t* score_rows, const int32_t* targets, int n_score, float* nll_out);
typedef struct {
  int32_t* pos;              /* device scalar: cache length == rotary position of the next token (Q2) */
  int32_t* step;             /* device scalar: index of the next generated token */
  int32_t* next_tok;         /* [B] token fed to the next decode step */
  int32_t* tokens_out;       /* [B, max_steps] */
  float* logprob;            /* [B] running sum of log_softmax(logits)[token] */
  void* logits;              /* [B, vocab] logits of the latest step */
  void* logits_all;          /* optional record [max_steps, B, logits_all_ld] of every step's logits; may be PINNED HOST memory
                              * (hipHostMalloc): the rows then cross PCIe during the following decode steps */
  const uint8_t* keep;       /* optional [B, Tmax] decode key mask ("clean" mode; Tmax = the cache's), non-zero = kept; NULL = reference
                              * quirk Q1.  Every decode step hands it to its attention as pcy_attn_decode takes it: slot *pos itself is
                              * always attended; bytes at and above *pos are not read */
  int32_t max_steps;
  int32_t logits_all_ld;     /* row stride of logits_all in elements; 0 = vocab.  A multiple of 8 enables 16-byte stores */
  /* ---- EOS stop of the greedy and sampling picks; all zero / NULL = no stop: every entry launches what it
   * launched without these fields and gives the same bits.  With finished != NULL the four picks (pcy_greedy_pick, pcy_sample_pick,
   * pcy_f32_greedy_pick, pcy_f32_sample_pick, alone or inside pcy_llama_greedy / _sample / _greedy_w8 / pcy_f32_llama_greedy / _sample):
   *   unfinished row: the selection, logprob increment, tokens_out[b][*step] and next_tok[b] of the entry without a stop, bit for bit; a
   *     token equal to eos_id sets finished[b] (the EOS itself is emitted and its log-probability added);
   *   finished row: tokens_out[b][*step] = next_tok[b] = eos_id, logprob[b] unchanged; its logits are not read for a selection (they may
   *     hold anything, NaN included) and a sampling pick skips its histogram / radix passes unless a probs_out record is asked for; its
   *     variate stays uniforms[step * B + b], so no other row's draw moves; the logits_all / probs_out rows are written as without a stop;
   *   the launch that finishes the last unfinished row of [0, B) raises *done (and writes *n_steps_run) -- a count of the unfinished rows
   *     behind the picks of a launch, no floating-point atomics;
   *   a launch that finds *done set changes nothing: not *step, *pos, tokens_out, next_tok, logprob, finished nor the logits_all /
   *     probs_out record (pcy_beam_step's rule).  The decode launches in front of it still run and rewrite K / V at slot *pos, which no
   *     result anyone reads attends: steps enqueued past *done are harmless.
   * Rows finish independently: a row's tokens up to and including its EOS and its logprob are bit-equal to the same call without a stop.
   * Argument errors of every entry named above (code 1, nothing launched): finished != NULL with done == NULL; finished != NULL with eos_id
   * outside [0, vocab).  A captured chain is keyed on all four fields: a state with a stop and one without never share a graph. */
  int32_t* finished;         /* optional [B] device, zero-initialised: non-zero = the row has emitted eos_id.  NULL = no EOS stop */
  int32_t* done;             /* device scalar, zero-initialised: raised by the pick that finishes the last unfinished row of [0, B).
                              * Required when finished != NULL */
  int32_t* n_steps_run;      /* optional device scalar: *step behind the pick that raised *done == the number of real rows of
                              * tokens_out / logits_all (untouched while *done is 0) */
  int32_t eos_id;            /* read only when finished != NULL */
} pcy_gen_state;
/* one decode step: next_tok -> logits (and K/V appended at slot *pos); does not pick or advance */
int pcy_llama_decode(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B);
/* Measurement aid (tools/bench_decode.py with PCY_MC_TRACE=1 in the environment): copies the in-kernel time stamps of the last
 * fused decode launches ([2][128 layers][256 workgroups][16] ticks of 10 ns) to `out` (n words); returns n, or 0 when no stamps
 * were taken. */
int pcy_debug_mc_trace(unsigned long long* out, int n);
/* Measurement aid (bench.py roofline leg): `reps` passes over the decoder layers of a decode step -- no token embedding (the
 * residual stream is whatever the workspace holds), no lm_head, no pick; K/V of slot *pos are rewritten each pass.  With HIP
 * events around it: time per layer launch = elapsed / (reps * n_layers). */
int pcy_llama_decode_layers(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B, int reps);
/* the same step as ONE replayed hipGraph (captured on first use per model / cache / state / batch): for host-driven loops that
 * do their own selection between steps (sampling, diverse beam search).  next_tok and *pos are read from device memory. */
int pcy_llama_decode_graph(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B);
/* ---- the decode step for more than 32 rows: one pass over the weights whatever B ----
 * Opt-in, beside pcy_llama_decode, whose step above 32 rows streams every weight matrix once per 32 rows.  Here every projection and lm_head
 * is ONE MFMA GEMM over all B rows (the dispatcher of the prefill and of the cache extension); the attention is the default loop's launch.
 * Contract -- pcy_llama_decode's: next_tok -> logits in state->logits, K / V of the new token appended at logical slot *pos of every row;
 * does not pick, does not advance.  next_tok, *pos and keep are read from DEVICE memory: no host read, no synchronisation.  keep has the
 * decode meaning (slot *pos always attended, bytes at and above *pos not read; NULL = quirk Q1).  Plain caches and shared-prefix caches
 * (prefix_k / prefix_v, rows_per_prefix >= 1).  1 <= B <= the cache's rows, no other upper limit; meant for B >= 33.  One launch per stage
 * on the context's stream, never captured; the workspace is the context's (sized by B, the geometry and the cache capacity).
 * Argument errors (nothing launched, nothing written): a grouped cache (rows_per_prefix == 0 with a prefix), a model with fp8 layers,
 * B outside [1, cache rows], a geometry the GEMMs / the attention do not cover (d, ffn, H*dh, Hkv*dh % 64; head_dim 32 / 64 / 128;
 * H / Hkv in 1, 2, 4, 8).
 * NOT promised: the bits of pcy_llama_decode.  The GEMMs add up in another order than the default step's GEMVs, and a row's bits may depend
 * on B: tile shapes and K splits are chosen by the row count.  Tokens may therefore part from the default path's where two logits tie
 * within bf16 noise.
 * Promised: within ONE call a row's logits and appended K / V depend on that row's inputs alone -- not on the M tile it sits in nor on what
 * its batch mates hold (equal rows give equal bits); the same call repeated gives the same bits; plain and shared-prefix caches of equal
 * contents give equal bits; every row meets the oracle within the project's bar (tests/test_gpu_decode_gemm.py). */
int pcy_llama_decode_gemm(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B);
/* steps enqueued by pcy_llama_decode_gemm since the library was loaded.  A word of its own, as pcy_debug_look_count: the kinds of
 * pcy_debug_dispatch_count are pinned, and this step counts under none of the decode kinds. */
unsigned long long pcy_debug_decode_gemm_count(void);
/* Decode attention of ONE new token per row on layer `layer` of a shared-prefix cache, all rows of a prompt against ONE pass over its prefix
 * (DESIGN.md 4.3d).  The operator is pcy_attn_decode's: ropes q and the new k at *pos (device scalar = LOGICAL cache length t), appends K, V
 * at suffix slot t - prefix_T of the row's own panel, attends logical slots [0, t] -- slot j < prefix_T from prefix row b / rows_per_prefix,
 * slot j >= prefix_T from the row's own panel -- with pcy_attn_decode's rounding points.  keep: optional [B, prefix_T + Tmax] bytes in logical
 * slots read through the query's own row, non-zero = kept; slot t is always attended, bytes at and above t are not read.  The cache is passed
 * as to pcy_attn_extend, everything else as to pcy_attn_decode.  head_dim 64 or 128, H / Hkv in 1, 2, 4, 8, rows_per_prefix >= 1.
 * Work split: the K and V tiles of a (prompt, kv head) are staged once per 64 packed queries (rows x H / Hkv) and used by MFMA; the prefix is
 * cut into key chunks whose count is a function of (B, rows_per_prefix, prefix_T, geometry); the chunks' fp32 partial sums are added in chunk
 * order, the row's own slots last, and rounded once.  No atomics.
 * Promised: a query's bits depend on its own row's logical contents and on the call's shape (B, prefix_T, t, geometry) only; equal calls give
 * equal bits; the appended K / V have the bits pcy_attn_decode writes; the prefix is never written and of the suffix only slot t - prefix_T;
 * slots above t never reach a result.  NOT promised: the bits of pcy_attn_decode's output (another order of the sums).
 * t < prefix_T or t >= prefix_T + Tmax: nothing is written.  Argument errors (nothing launched, nothing written, no fallback): a plain cache,
 * a grouped cache (rows_per_prefix == 0), an incomplete shared cache, B outside [1, cache rows], an unsupported head_dim or H / Hkv, rows of
 * qkv / o that are not 16-byte aligned.  Workspace: the context's. */
int pcy_attn_decode_shared(pcy_ctx*, void* qkv, int ld, const pcy_kv_cache* kv, int layer, void* o, int ldo, const int32_t* pos,
                           const void* cos_t, const void* sin_t, const uint8_t* keep, int B, int H, int Hkv, int dh);
/* pcy_llama_decode_gemm with the attention of every layer served by pcy_attn_decode_shared's kernels: the same contract word for word, on
 * shared-prefix caches with rows_per_prefix >= 1 only (a plain cache, head_dim 32: argument errors as above).  The decode workspace keeps its
 * carve; the attention's score rows and partial sums lie behind it.  NOT promised: the bits of pcy_llama_decode_gemm. */
int pcy_llama_decode_gemm_mq(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B);
/* steps enqueued by pcy_llama_decode_gemm_mq since the library was loaded (each also counts in pcy_debug_decode_gemm_count, none under a
 * decode kind of pcy_debug_dispatch_count). */
unsigned long long pcy_debug_attn_mq_count(void);
/* ---- split-key decode attention on a shared-prefix cache ----
 * pcy_attn_decode_shared's operator, arguments, coverage and argument errors word for word; another arithmetic and another work split.
 * Arithmetic: s_j = bf16(bf16(q.k) * scale), a masked s_j = the bf16 minimum.  The prefix is cut into chunks of pcy_attn_split_chunk_keys()
 * keys; the row's own slots [prefix_T, t] are the last chunk.  Per chunk c: m_c = max s_j, e_j = exp(s_j - m_c) in fp32, l_c = sum e_j in fp32,
 * p_j = bf16(e_j), o_c = sum p_j * v_j in fp32.  Then m = max_c m_c, w_c = exp(m_c - m), o = bf16((sum_c w_c * o_c) / (sum_c w_c * l_c)),
 * both sums in chunk order, rounded once.  A chunk whose keys are all masked for a query has w_c == 0 exactly (slot t is never masked).
 * This gives up the reference's rounding point p = bf16(exp(s - m) / l) under the global (m, l); against float64 it is no worse.
 * Work split: two launches.  The first holds row workgroups (kv head, row: rope, append, the own slots) and prefix workgroups (key chunk x 64
 * packed queries, kv head, prompt: each K and each V tile staged once, S and P.V by MFMA, S never leaves the chip) and writes o_c and
 * (m_c, l_c); the second combines.  No atomics, no waiting between workgroups, no score rows in memory; the plan never depends on t.
 * Promised: a query's bits depend on its own row's logical contents and on the call's shape (B, rows_per_prefix, prefix_T, geometry) only;
 * equal calls give equal bits, equal rows in other tiles or prompts give equal bits; the appended K / V have the bits pcy_attn_decode writes;
 * the prefix is never written and of the suffix only slot t - prefix_T; slots above t never reach a result.  NOT promised: the bits of
 * pcy_attn_decode or of pcy_attn_decode_shared.  t < prefix_T or t >= prefix_T + Tmax: nothing is written.  Workspace: the context's. */
int pcy_attn_decode_split(pcy_ctx*, void* qkv, int ld, const pcy_kv_cache* kv, int layer, void* o, int ldo, const int32_t* pos,
                          const void* cos_t, const void* sin_t, const uint8_t* keep, int B, int H, int Hkv, int dh);
/* host arithmetic only: the keys per prefix chunk of pcy_attn_decode_split's plan for this shape (a positive multiple of 32; 0 for arguments
 * below 1).  A function of these six values and nothing else. */
int pcy_attn_split_chunk_keys(int B, int rows_per_prefix, int H, int Hkv, int dh, int prefix_T);
/* pcy_llama_decode's contract on the default batched loop, with the attention of every layer served by pcy_attn_decode_split's launches
 * (qkv projection with its own K-split finish -> attention -> o projection).  Eager.  Shared-prefix caches with rows_per_prefix >= 1 and a
 * row count the batched loop serves only; a plain or grouped cache, an uncovered geometry, fp8 layers: argument errors before any launch.
 * The attention's partial sums lie behind the decode carve and the K/V reorder scratch of pcy_llama_beam_steps.  NOT promised: the bits of
 * pcy_llama_decode. */
int pcy_llama_decode_split(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B);
/* pcy_llama_decode_gemm_mq with pcy_attn_decode_split's two launches in place of the four. */
int pcy_llama_decode_gemm_split(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B);
/* steps enqueued with the split-key attention since the library was loaded: by pcy_llama_decode_split, by pcy_llama_decode_gemm_split (which
 * also counts in pcy_debug_decode_gemm_count) and, once per captured chain, by pcy_llama_beam_steps_split. */
unsigned long long pcy_debug_attn_split_count(void);
/* ---- cached decode that streams e4m3 weights: weight-only fp8 projections for 1..8 rows ----
 * The operator.  y[b][n] = epi( (sum_k x[b][k] * f32(W8[n][k])) * scale[n] ): W8 [N,K] OCP e4m3 codes and scale [N] fp32 as pcy_quant_rows_fp8
 * makes them per output channel (EPI_SWIGLU: [2N,K] / [2N] in the 16-row gate/up interleave, y is [B,N]); x, resid, y, rms_w bf16.  The
 * activations stay bf16 and nothing is quantised per call.  fp32 accumulation, the scale ONCE on the finished sum, then pcy_gemv's rounding
 * points: STORE bf16(v); RESID bf16(bf16(v) + resid) (resid may alias y); SWIGLU bf16(bf16(silu(bf16(g))) * bf16(u)); rms_w != NULL fuses
 * RMSNorm(x) * rms_w in front (STORE / SWIGLU; rms_cast as pcy_gemv).  Up to 4 rows share a pass over the matrix, 5..8 rows take two.
 * The order of a (row, output) sum is a function of the output row and K alone: row b of a B-row call has the bits of the one-row call on it.
 * Argument errors (nothing launched): epi outside STORE / RESID / SWIGLU, B outside [1, 8], K % 16, ldx % 8, W8 / x not 16-byte aligned,
 * SWIGLU with N % 16, RESID without resid or with rms_w, a NULL tensor, a K whose x row does not fit the LDS of a CU. */
int pcy_gemv_w8(pcy_ctx*, const void* W8, const float* scale, const void* x, int ldx, const void* resid, void* y, int ldy, const void* rms_w,
                float rms_eps, int rms_cast, int N, int K, int B, int epi);
/* One decode step on the e4m3 copies of the projections.  Opt-in, beside pcy_llama_decode, with its contract: next_tok -> logits in
 * state->logits, K / V of the new token appended at slot *pos of every row; does not pick, does not advance; next_tok, *pos and keep are read
 * from device memory.  w8: HOST array [n_layers] of the e4m3 matrices and their per-row scales (same row order / interleave as the bf16 ones),
 * passed explicitly: desc->layers_fp8 keeps meaning "fp8 prefill" and is not read here.  One launch per stage on the context's stream: per
 * layer qkv (ln1 fused) -> the stand-alone decode attention -> o (+ residual) -> gate/up (ln2 fused, SwiGLU) -> down (+ residual), each a
 * pcy_gemv_w8 launch; norms, rope, attention, residuals stay bf16, and lm_head stays bf16 on the streaming GEMV with the final norm fused.
 * The workspace is the decode carve.  A model whose bf16 projection weights ARE dequant(w8) computes here what pcy_llama_decode computes, up
 * to the order of the sums.
 * Argument errors (nothing launched, nothing written): w8 NULL or a layer with a NULL pointer; B outside [1, min(8, cache rows)]; a
 * shared-prefix or grouped cache; d, ffn, H*dh or (H+2Hkv)*dh not multiples of 16; head_dim outside 32 / 64 / 128 or H / Hkv outside
 * 1, 2, 4, 8; d > 8192.
 * Promised: a row's logits and appended K / V depend on that row's inputs alone, not on B (1..8) nor on its batch mates; equal calls give
 * equal bits; pcy_llama_greedy_w8's graph replay and its eager loop give equal bits.  NOT promised: the bits of pcy_llama_decode. */
int pcy_llama_decode_w8(pcy_ctx*, const pcy_llama_desc*, const pcy_llama_layer_fp8* w8, const pcy_kv_cache*, const pcy_gen_state*, int B);
/* n_steps x (pcy_llama_decode_w8 + greedy pick) with no host synchronisation; use_graph != 0 replays ONE captured hipGraph per step (about
 * 160 launches per step of a 32-layer model make the eager loop host-bound at one row). */
int pcy_llama_greedy_w8(pcy_ctx*, const pcy_llama_desc*, const pcy_llama_layer_fp8* w8, const pcy_kv_cache*, const pcy_gen_state*, int B,
                        int n_steps, int use_graph);
/* steps enqueued by pcy_llama_decode_w8 / pcy_llama_greedy_w8 outside a graph replay (an eager step, or the capture of a graph).  A word of
 * its own, as pcy_debug_decode_gemm_count: this step counts under none of the decode kinds of pcy_debug_dispatch_count. */
unsigned long long pcy_debug_decode_w8_count(void);
/* argmax of state->logits (lowest index on ties) -> next_tok / tokens_out[step], logprob, ++pos? no: ++step only
 * when advance_pos == 0 (used on the prefill logits), ++pos and ++step otherwise.  logprob += bf16 log_softmax(logits)[token]: fp32
 * statistics, one rounding.  -inf logits are allowed and mean "never chosen" (banned tokens, also whole runs of them); a row must hold
 * at least one finite logit; NaN logits are outside the contract. */
int pcy_greedy_pick(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B, int advance_pos);
/* ---- greedy decoding with lookahead: several drafted tokens checked per pass over the weights ----
 * One prompt.  A pass is pcy_llama_extend with S = W rows at t_past = *pos: row 0 is the last committed token, rows 1..W-1 are drafts of
 * the tokens behind it.  Between two passes, on the device: pcy_look_verify (pick every row, count the leading drafts that were right, commit)
 * and pcy_look_draft (draft again, gather the W embedding rows).  A pass ALWAYS has W rows, also when fewer tokens remain: the projections'
 * tile and K-split choices depend on the row count, so only a fixed count keeps a token's bits independent of the drafts.
 * The state below works beside an ordinary one-row pcy_gen_state, of which pos, step, next_tok, tokens_out, logprob, logits_all and max_steps
 * are used; every pointer is device memory.
 *   hist     [cap] the prompt's token ids followed by every committed token; a negative entry is a slot that is no text token (soft-token
 *            slots, anything the caller wants kept out of the lookup): it never matches and ends a draft
 *   n_hist   device scalar, 1 <= *n_hist <= cap (appends beyond cap are dropped)
 *   window   [W] row 0 = the last committed token (the caller sets it once, before the first draft), rows 1..W-1 = the drafts
 *   forced   optional [max_steps] (NULL: none): forced[i] >= 0 replaces the draft of output token i -- how tests and measurements dictate
 *            the acceptance
 *   counters [2 + W] zero-initialised: [0] passes, [1] committed tokens, [2 + k] passes that committed k drafts (k + 1 tokens)
 *   last     [4] of the latest pcy_look_verify: leading drafts that were right, tokens committed, *step and *pos before the commit
 * Draft rule: with h = hist[0, n), for g = ngram_max down to ngram_min take the LARGEST i with i + g < n, h[i..i+g) == h[n-g..n) and every
 * compared entry >= 0; draft j = h[i+g+j], j = 0, 1, ... until the history ends, an entry is negative or W-1 drafts are filled; every draft
 * not filled that way (all of them when no g matches) is h[n-1].  (procyon_amd.engine.lookup_draft restates it on the host.) */
typedef struct {
  int32_t* hist;
  int32_t* n_hist;
  int32_t* window;
  const int32_t* forced;
  int32_t* counters;
  int32_t* last;
  int32_t cap, W;            /* 2 <= W <= 32 */
  int32_t ngram_max, ngram_min;   /* 1 <= ngram_min <= ngram_max <= 16 */
} pcy_look_state;
/* window[1..W) by the rule above, then embeds_out [W, d] bf16 = embed[window[r]] (bit copies of the table's rows).  d % 8 == 0. */
int pcy_look_draft(pcy_ctx*, const pcy_llama_desc*, const pcy_look_state*, const pcy_gen_state*, void* embeds_out);
/* logits [W, vocab] bf16 of the pass.  Per row the argmax and bf16 log_softmax(logits)[argmax] with the selection rule and the bits of
 * pcy_greedy_pick (lowest index on ties, -inf = never chosen, fp32 statistics, one rounding; the same device code).  a = the number of leading
 * drafts j with window[j+1] == argmax(row j); n = min(a + 1, max_steps - *step) tokens are committed: the argmaxes of rows 0..n-1 go to
 * tokens_out[*step..] and hist, their log-probabilities are added to logprob[0] in row order, rows 0..n-1 of the logits to rows *step.. of
 * logits_all (when kept; pinned host memory works), next_tok[0] = window[0] = the last of them, *pos += n, *step += n.  Deterministic.
 * The K / V of rejected rows stay in slots [*pos, ...) behind the new *pos; the next W-row pass rewrites them before any query reads them.
 * With the EOS stop of the state (finished != NULL, see pcy_gen_state; argument errors as there): the commit ends with the first committed
 * token that equals eos_id -- n is cut there, the rows behind it count as rejected drafts, nothing of them reaches tokens_out, logprob, hist
 * or the record -- and that launch sets finished[0], *done and *n_steps_run = the new *step; a launch that finds *done set commits nothing
 * (last[1] = 0). */
int pcy_look_verify(pcy_ctx*, const pcy_llama_desc*, const pcy_look_state*, const pcy_gen_state*, const void* logits);
/* calls since the library was loaded -- 0: pcy_look_draft, 1: pcy_look_verify (= passes); anything else reads 0.  Words of their own, as
 * pcy_debug_extend_grouped_count: the kinds of pcy_debug_dispatch_count are pinned. */
unsigned long long pcy_debug_look_count(int which);
/* ---- the lookahead pass on the decode loop ----
 * Window attention: W consecutive tokens of cache row 0 on layer `layer` of a PLAIN cache with kv->B == 1.  The operator is pcy_attn_extend's
 * with B = 1, S = W, t_past = *pos and no keep mask, *pos (device scalar) being read on the device: qkv [W, ld] holds the un-roped projections
 * (read only: the roped queries go to the workspace); q and k of row i are roped at position *pos + i, K / V of row i are written to slot
 * *pos + i, o[i] is the causal attention of query i over slots [0, *pos + i], with pcy_attn_extend's rounding points (bf16 scores, the scale
 * on the rounded score, probabilities normalised in fp32 before their rounding, fp32 P.V rounded once).  cos_t / sin_t hold at least Tmax
 * rows.  head_dim 64 or 128, H / Hkv in 1, 2, 4, 8, 2 <= W <= 32.
 * Work split: the W x H / Hkv queries of a kv head are packed into 16-wide MFMA tiles; the keys are cut into chunks of
 * pcy_attn_window_chunk() keys, one workgroup per (chunk, kv head, 64 packed queries), the grid sized from the capacity; a launch writes the
 * chunks' (max, sum), a second one their fp32 P.V under the query's global (max, sum), a third adds the chunks in chunk order.  No atomics.
 * Promised: query i's bits depend on the logical contents of slots [0, *pos + i], on i, *pos, W and the geometry only -- not on rows > i of
 * qkv (NaN included), not on what slots above *pos + i held, not on Tmax; a masked key contributes exactly 0 (select, not multiply); equal
 * calls give equal bits; the appended K / V have the bits pcy_attn_extend writes; slots below *pos and above *pos + W - 1 are never written.
 * *pos < 0 or *pos + W > Tmax: nothing is written.  NOT promised: the bits of pcy_attn_extend's or pcy_attn_decode's output.
 * Argument errors (nothing launched, nothing written): a shared-prefix or grouped cache, kv->B != 1, W outside [2, 32], Tmax < W, an
 * unsupported head_dim or H / Hkv, rows of qkv / o that are not 16-byte aligned.  Workspace: the context's. */
int pcy_attn_window(pcy_ctx*, void* qkv, int ld, const pcy_kv_cache* kv, int layer, void* o, int ldo, const int32_t* pos, const void* cos_t,
                    const void* sin_t, int W, int H, int Hkv, int dh);
/* keys per chunk of pcy_attn_window: a constant of the library, a multiple of 32 */
int pcy_attn_window_chunk(void);
/* One lookahead pass on the batched decode loop.  embeds [W, d] bf16 (what pcy_look_draft writes) -> logits_out [W, vocab] bf16; K / V of
 * row i appended at slot *pos + i of the one cache row.  Reads state->pos on the device and does not advance it (pcy_look_verify does); of
 * the state only pos and keep are read.  One launch per stage, always: per layer qkv -> pcy_attn_window -> o (+ residual) -> gate/up
 * (SwiGLU) -> down (+ residual), then the final norm and the lm_head GEMV for all W rows -- the launch-per-stage loop of pcy_llama_decode at
 * B = W (skinny-MFMA GEMVs with the RMSNorm fused into the K-split finish from W = the MFMA GEMVs' smallest batch on when d % 128 == 0 and
 * ffn % 128 == 0, the streaming GEMVs otherwise), never a fused one-launch step whatever the switches say, and with the GEMV's own finish
 * launch behind the qkv projection.  The decode workspace keeps its carve; the attention's buffers lie behind it.
 * Promised: row i's logits and appended K / V depend on rows <= i of embeds, on *pos, W and the cache below *pos only; equal calls give equal
 * bits.  NOT promised: the bits of pcy_llama_extend or pcy_llama_decode.
 * Argument errors (nothing launched, nothing written): state->keep != NULL, fp8 layers (desc->layers_fp8), everything pcy_attn_window
 * refuses, d, ffn, H*dh or (H+2Hkv)*dh not multiples of 16. */
int pcy_llama_decode_window(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, const void* embeds, int W,
                            void* logits_out);
/* calls of pcy_llama_decode_window since the library was loaded: a word of its own, as pcy_debug_decode_gemm_count */
unsigned long long pcy_debug_decode_window_count(void);
/* n_steps x (decode + pick) with no host synchronisation; use_graph != 0 replays a captured hipGraph */
int pcy_llama_greedy(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B, int n_steps,
                     int use_graph);
/* Sampling / nucleus selection (`_generate_sampling` without greedy, model_unified.py:896-906) on state->logits:
 *   probs = bf16 softmax(logits / temperature); nucleus_prob in (0,1): probs = softmax(logits) * mask of the tokens whose ascending
 *   cumulative probability has reached 1 - nucleus_prob (`_get_nucleus_mask`, not renormalised); nucleus_prob <= 0: no mask;
 *   token = first index whose cumulative masked probability exceeds uniforms[step * B + b] * total (inverse CDF with the CALLER's
 *   uniform variates in [0,1): torch's multinomial stream is not reproducible, the probability vector and the draw for a given u
 *   are); logprob += bf16 log_softmax(unscaled logits)[token]; then next_tok / tokens_out / ++step (/ ++pos) like pcy_greedy_pick.
 * probs_out: optional [B, vocab] bf16 record of the pre-sampling probability vector.  uniforms: device fp32 [max_steps * B].
 * -inf logits are allowed and mean "never chosen" (probability exactly 0); a row must hold at least one finite logit; NaN logits are
 * outside the contract. */
int pcy_sample_pick(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B, int advance_pos,
                    float temperature, float nucleus_prob, const float* uniforms, void* probs_out);
/* n_steps x (decode + sample) with no host synchronisation */
int pcy_llama_sample(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B, int n_steps,
                     float temperature, float nucleus_prob, const float* uniforms);
/* Diverse beam search bookkeeping of ONE step on the device (`_generate_beam_search`, model_unified.py:782-833): per prompt
 * and beam group, top-`group_size` of  log_softmax(logits) (model dtype) + running score - diversity_penalty * (count of the
 * token among the picks of the earlier groups at this step);  at step 0 only the first beam of a group is expanded.  Updates
 * the token histories, the running scores, `src` (parent slot of every slot: feed it to pcy_kv_reorder), `next_tok`, ++*step,
 * ++*pos (from step 1 on) and raises *done once every row holds `eos_id`; a launch with *done set changes nothing.
 * logits [B*beam, vocab] bf16.  All pointers are device memory; state layout in the struct below (BB = B * beam).
 * Equal candidate scores go to the lowest flat index row * vocab + token.  -inf logits are allowed and mean "never chosen" as long as a
 * group has group_size finite candidates left; a row must hold at least one finite logit; NaN logits are outside the contract (a
 * selection that finds no candidate then commits the group's first row and token 0: wrong, but inside the state arrays). */
typedef struct {
  int32_t* out; int32_t max_len;   /* [2][BB][max_len] token histories; buffer (*step & 1) is current; zero-initialised */
  float* cur; float* cur_new;      /* [BB] running scores (zero-initialised) + scratch */
  int32_t* next_tok;               /* [BB] */
  int32_t* src;                    /* [BB] */
  int32_t* anc;                    /* optional [max_len][BB]: src of every step (to permute a per-slot logits record afterwards) */
  uint8_t* has_eos;                /* [2][BB] zero-initialised */
  int32_t* blk_eos; int32_t* ticket;   /* [B], [1] zero-initialised */
  int32_t* pos; int32_t* step; int32_t* done;   /* device scalars */
  int32_t eos_id;
} pcy_beam_state;
int pcy_beam_step(pcy_ctx*, const void* logits, int vocab, int B, int beam, int group_size, float diversity_penalty,
                  const pcy_beam_state* state);
/* KV rows gather for beam search: cache[:, dst] = cache[:, src[dst]] over slots [0,t) (model_unified.py:830-832) */
int pcy_kv_reorder(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const int32_t* src_rows, int B, int t);
/* ... over slots [t0, t) only: for callers that know the rows hold the same contents below t0 -- the beams of a prompt share its prefix (the
 * reference moves the whole history of every row in every group of every step, model_unified.py:830-832; moving equal bytes changes nothing).
 * src_rows[b] may be any row of the cache (rows >= B are read straight from memory). */
int pcy_kv_reorder_range(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const int32_t* src_rows, int B, int t0, int t);
/* n_steps iterations (steps >= 1) of the loop body of `_generate_beam_search` (model_unified.py:751-842): decode step for the B * beam
 * rows -> logits_rec[step][row][vocab] = the step's logits (NULL: no record) -> pcy_beam_step -> pcy_kv_reorder over the slots the state's
 * position counter names, from slot kv_t0 on (0: all of them; the prompt length when the beams of a prompt share its prefix rows: see
 * pcy_kv_reorder_range); each iteration is ONE replayed launch chain.  gen_state->pos / next_tok must be the beam state's arrays.  Same
 * results as pcy_llama_decode_graph + a copy + pcy_beam_step + pcy_kv_reorder per step. */
int pcy_llama_beam_steps(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B, int beam, int group_size,
                         float diversity_penalty, const pcy_beam_state* state, void* logits_rec, int n_steps, int kv_t0);
/* ... with pcy_llama_decode_split's step inside (its cache rules; the same bits as the four calls around pcy_llama_decode_split).  A chain
 * captured with this attention and one without never share a graph. */
int pcy_llama_beam_steps_split(pcy_ctx*, const pcy_llama_desc*, const pcy_kv_cache*, const pcy_gen_state*, int B, int beam, int group_size,
                               float diversity_penalty, const pcy_beam_state* state, void* logits_rec, int n_steps, int kv_t0);

/* ---- fp32 operator family: the arithmetic of the reference's callers that never call `.bfloat16()` ----
 * /root/reference/examples/paper_analyses/protpep_qa_scores.py:55-58 (`model.eval().to(device)`: fp32 weights, every torch op in
 * fp32 -- the loop that defines BASELINE configs[4]), /root/reference/scripts/qa_filter_captions.py:17-18 and
 * /root/reference/scripts/caption_bulk.py:72-73.  Every pointer is a DEVICE pointer to fp32 (ids / pos / cu: int32, keep: uint8);
 * calls enqueue on the context's stream.  The host side (procyon_amd/engine_f32.py) strings these together op for op like the fp32
 * evaluation of the reference's modules: ESM2 encoder (esm.py:504-538) -> ProteinPooler (:131-173) -> create_mlp projectors
 * (model_utils.py:13-41) -> splice (model_unified.py:1135-1175) -> Llama prefill (pmc_llama.py:546-596) -> cached decode steps
 * of an fp32 generation (pcy_f32_attn_decode below). */
/* C[M,N] = act(A[M,K] . W[N,K]^T + bias[N]) (+ resid[M,N]); W is nn.Linear's [out, in]; act 0 = none, 1 = gelu
 * x * 0.5 * (1 + erf(x / sqrt 2)) (nn.GELU and the ESM gelu coincide in fp32).  bias / resid may be NULL; resid may alias C.
 * Matrix cores on exact fp32 products (v_mfma_f32_16x16x4_f32) when K % 16 == 0 and rows are 16-byte aligned, a plain kernel otherwise. */
int pcy_f32_linear(pcy_ctx*, const float* A, int lda, const float* W, const float* bias, const float* resid, int ldr, float* C, int ldc,
                   int M, int N, int K, int act);
/* torch.nn.functional.layer_norm / HF LlamaRMSNorm (w * (x * rsqrt(mean(x^2) + eps))) over rows of d */
int pcy_f32_layernorm(pcy_ctx*, const float* x, const float* w, const float* b, float* y, int rows, int d, float eps);
int pcy_f32_rmsnorm(pcy_ctx*, const float* x, const float* w, float* y, int rows, int d, float eps);
/* rotary embedding in place on heads [col0, col0 + nh*dh) of every row: x <- x' cos[pos] + rotate_half(x') sin[pos], x' = x * prescale
 * (prescale 0 = none; ESM scales q by dh^-1/2 BEFORE the rotation, esm2 multihead attention); cos / sin tables fp32 [n_pos, dh] */
int pcy_f32_rope(pcy_ctx*, float* buf, int ld, int col0, int nh, int dh, const int32_t* pos, const float* cos_t, const float* sin_t, int ntok,
                 float prescale);
/* out[r] = soft_map && soft_map[r] >= 0 ? soft[soft_map[r]] : table[ids[r]]: token embedding + soft-token splice as one gather */
int pcy_f32_embed(pcy_ctx*, const float* table, const int32_t* ids, const float* soft, const int32_t* soft_map, float* out, int rows, int d);
/* HF EsmEmbeddings with token_dropout over packed sequences (cu [nseq+1]): <mask> rows zero, x * 0.88 / (1 - mask ratio), pads zero */
int pcy_f32_esm_embed(pcy_ctx*, const float* table, const int32_t* tokens, const int32_t* cu, int nseq, int max_len, float* out, int d, int mask_pads);
int pcy_f32_silu_mul(pcy_ctx*, const float* gate, const float* up, float* out, size_t n);      /* out = silu(gate) * up */
int pcy_f32_acc_rows(pcy_ctx*, const float* src, int ld, const int32_t* rows, float* dst, int nrows, int d);   /* dst[r] += src[rows[r]] */
/* ProteinPooler over token ranges, arguments as pcy_pool (mode 0 mean, 1 mean of x[1:-1], 2 max) */
int pcy_f32_pool(pcy_ctx*, const float* hidden, int d, const int32_t* seg, const int32_t* rng, int nprot, int mode, float* out);
/* softmax((q . k) * scale + mask) . v over packed sequences (cu), grouped heads (Hkv | H), exact fp32 softmax; causal = 1: keys <= query;
 * keep (may be NULL): one byte per packed token, 0 = the key is masked out.  q / k / v are column windows of row-major buffers.
 * A query row without any kept key (a left-pad row) gets the reference's value, the softmax of a row that is finfo.min throughout:
 * the plain average of V over ALL keys of its sequence, causal or not, masked and later keys included.  The cached decode reads what
 * the next layers make of such rows (no mask after the prefill), so the value is part of the contract. */
int pcy_f32_attention(pcy_ctx*, const float* q, int ldq, int qcol0, const float* k, int ldk, int kcol0, const float* v, int ldv, int vcol0,
                      float* o, int ldo, const int32_t* cu, const uint8_t* keep, int nseq, int max_len, int H, int Hkv, int dh, int causal,
                      float scale);

/* fp32 decode attention (callers that never call .bfloat16() and generate: /root/reference/scripts/caption_bulk.py:70-73, 123-132): the new
 * token's q [B, H*dh] (roped) against slots [0, nkeys) of token-major caches [B][Tmax][Hkv*dh] (row stride ldkv floats); every slot is
 * attended (/root/reference/procyon/model/model_unified.py:769, :887 pass no mask after the prefill). */
int pcy_f32_attn_decode(pcy_ctx*, const float* q, int ldq, const float* kcache, const float* vcache, int ldkv, int Tmax, float* o, int ldo, int B,
                        int H, int Hkv, int dh, int nkeys, float scale);

/* fp32 cache extension (HF's forward(input_ids [B,S], past_key_values) on an fp32 model; shared-prefix candidate scoring): S new query rows
 * per row.  qkv [B*S, ld] roped, row b*S + s: q at column 0, the new K at H*dh, the new V at (H+Hkv)*dh.  Query s of row b attends slots
 * [0, t_past) of cache row cache_row[b] (NULL = b; token-major caches [rows][Tmax][Hkv*dh], row stride ldkv floats) and then the new keys
 * 0..s of its own row, read from qkv -- never from the cache, so rows may share a prefix row, and slots >= t_past are not read.  keep
 * (may be NULL) [B, ldkeep >= t_past + S] bytes: 0 = the key is masked, old and new alike.  Exact fp32 softmax, keys in ascending slot
 * order; o [B*S, ldo].  A query row without any kept key gets the family's value (pcy_f32_attention): the plain average of V over ALL
 * t_past + S keys of its row.  S == 1 without keep / cache_row: bit-equal to pcy_f32_attn_decode on the same cache with the new K / V at
 * slot t_past.  t_past == 0 is a causal prefill of the new tokens.  dh + t_past + S floats of LDS: larger sizes are refused (code 1). */
int pcy_f32_attn_extend(pcy_ctx*, const float* qkv, int ld, const float* kcache, const float* vcache, int ldkv, int Tmax,
                        const int32_t* cache_row, const uint8_t* keep, int ldkeep, float* o, int ldo, int B, int S, int t_past, int H, int Hkv,
                        int dh, float scale);

/* fp32 lm_head x cross-entropy without the [M, V] logits: nll[m] = lse[m] - l[m][targets[m]], lse = max + log sum exp(l - max), where
 * l[m][n] is the fp32 value pcy_f32_linear(x, W) stores from its matrix-core kernel (same main loop: label_logit_out and row_max_out are
 * bit-equal to the corresponding entries of that product).  x [M, d] final-normed, ldx floats between rows; W [V, d] in natural row order;
 * rows 16-byte aligned and d % 16 == 0 (the conditions of pcy_f32_linear's matrix-core path; anything else is code 1, never a slow
 * path).  targets [M] in [0, V): a target outside gives NaN in that row.  lse_out / row_max_out / label_logit_out may be NULL.  M == 0
 * returns 0 without a launch.  No atomics; the column partition and every merge order are functions of V alone: a row's bits depend
 * neither on M nor on the other rows, and two runs are bit-equal.  Workspace (the context's): rows are processed at most 1024 at a
 * time, pcy_f32_lm_head_xent_ws_bytes = min(M, 1024) * (n_col_blocks(V) * 8 + 4) bytes -- host arithmetic, callable without a device. */
int pcy_f32_lm_head_xent(pcy_ctx*, const float* x, int ldx, const float* W, int M, int V, int d, const int32_t* targets, float* nll_out,
                         float* lse_out, float* row_max_out, float* label_logit_out);
size_t pcy_f32_lm_head_xent_ws_bytes(int M, int V);

/* ---- fp32 generation on a streaming GEMV and a device-resident decode step ----
 * Opt-in, beside the operator-per-launch step that LlamaEngineF32.decode strings together from the entries above.
 *
 * The streaming GEMV.  y[b][n] = epi(sum_k x[b][k] * W[n][k]): W [N, K] fp32 in nn.Linear's natural layout (rows of K floats, 16-byte
 * aligned), x [B, ldx], y [B, ldy], resid [B, ldr] fp32, 1 <= B.  epi: 0 STORE y = v; 1 RESID y = v + resid (resid may alias y);
 * 4 SWIGLU y = silu(g) * u with g from W and u from W2 [N, K] (two separate matrices; x / (1 + exp(-x)) as pcy_f32_silu_mul).  W2 is read
 * for SWIGLU only.  Exact fp32 products and fp32 accumulation on the fp32-input matrix cores (a chain of fused multiply-adds per output).
 * Weight traffic: one pass over the matrix serves up to 32 rows of x (17..32 rows take ONE pass, two 16-row tiles against every weight
 * register); the launcher loops passes of 32 rows for larger B.
 * Order of a (row, output) sum: a function of K, the epilogue (SWIGLU cuts K over half as many waves) and the 16-row group of the OUTPUT
 * row (its workgroup walks the K range rotated by that group, so that the workgroups of a launch do not read the same window of their
 * rows -- rows of 4096 floats are a power-of-two stride -- at the same moment).  It depends neither on B, nor on the pass or tile the row
 * sits in, nor on what the other rows hold: row b of a B-row call has the bits of the one-row call on that row, NaN in another row does
 * not reach it, and equal calls give equal bits.  No atomics; the partial sums of a workgroup's waves are added in wave order.
 * Argument errors (code 1, nothing launched): a NULL W / x / y, W2 NULL with SWIGLU, resid NULL with RESID, an epi outside the three,
 * B < 1, N < 1, K < 4 or K % 4, ldx < K or ldx % 4, ldy < N, RESID with ldr < N, W / W2 / x not 16-byte aligned. */
int pcy_f32_gemv(pcy_ctx*, const float* W, const float* W2, const float* x, int ldx, const float* resid, int ldr, float* y, int ldy,
                 int N, int K, int B, int epi);
/* Decode attention of ONE new token per row that reads its position on the device.  qkv [B, ld]: the un-roped projections of the new
 * token (q heads | k heads | v heads; not written).  *pos (device scalar) = the cache length t = the rotary position of the new token for
 * EVERY row.  The launch ropes q and the new k at t (pcy_f32_rope's formula on cos_t / sin_t [>= Tmax, dh]), writes the roped K and V to
 * slot t of the token-major caches [B, Tmax, ldkv] and attends slots [0, t] without a mask, with pcy_f32_attn_decode's exact softmax:
 * scores (q . k) * scale in LDS, max, exp, sum, p / sum, o = sum p v in fp32.  One workgroup per (row, kv head): its H / Hkv query heads
 * (four at a time when there are more) share every K and V read; the waves of the workgroup split the keys, their partial o is added in
 * wave order.
 * Promised: a row's bits are a function of (*pos, the geometry) and the row's own qkv and cache contents; equal calls give equal bits;
 * slots above *pos never reach a result; only slot *pos of the caches is written; *pos < 0 or *pos >= Tmax writes nothing at all.
 * NOT promised: the bits of pcy_f32_rope + pcy_f32_attn_decode (another order of the sums).
 * Argument errors (code 1, nothing launched): a NULL pointer, B < 1, head_dim outside 16 / 64 / 128, Hkv < 1 or H % Hkv, ld / ldkv /
 * ldo shorter than their rows or not multiples of 4, qkv / caches not 16-byte aligned, and a capacity whose score rows exceed the LDS of
 * a CU: (min(H / Hkv, 4) * (Tmax + 9 * dh) + 2 * dh + 64) * 4 bytes > 159 KiB (the rule of pcy_f32_attn_decode, for the heads that share
 * a workgroup and sized by the capacity, since the host does not know *pos). */
int pcy_f32_attn_decode_pos(pcy_ctx*, const float* qkv, int ld, float* kcache, float* vcache, int ldkv, int Tmax, float* o, int ldo,
                            const int32_t* pos, const float* cos_t, const float* sin_t, int B, int H, int Hkv, int dh, float scale);
/* The fp32 decoder as the step reads it: every pointer is fp32 device memory in HF's layout; wqkv = [q; k; v] rows stacked, gate and up
 * stay separate matrices; rope_cos / rope_sin [max_pos, head_dim].  layers is a HOST array [n_layers]. */
typedef struct {
  const float *wqkv, *wo, *wg, *wu, *wd, *ln1, *ln2;
} pcy_f32_llama_layer;
typedef struct {
  int32_t vocab, d, n_layers, n_heads, n_kv_heads, head_dim, ffn, max_pos;
  float rms_eps;
  const float *embed, *final_norm, *lm_head, *rope_cos, *rope_sin;
  const pcy_f32_llama_layer* layers;
} pcy_f32_llama_desc;
/* token-major fp32 K (roped) / V caches [n_layers][B][Tmax][n_kv_heads * head_dim] (KVCacheF32) */
typedef struct {
  float *k, *v;
  int32_t B, Tmax;
} pcy_f32_kv_cache;
/* One decode step, pcy_llama_decode's contract in fp32: next_tok -> logits in state->logits ([B, vocab] fp32), K / V of the new token
 * appended at slot *pos of rows [0, B) of every layer; no pick, no advance; next_tok and *pos are read from device memory, no host read,
 * no synchronisation.  The state is a pcy_gen_state whose logits / logits_all hold fp32; keep must be NULL (the reference passes no mask
 * after the prefill).  Launch chain, all ordinary grids on the context's stream: token gather; per layer RMSNorm -> qkv GEMV ->
 * pcy_f32_attn_decode_pos -> o GEMV (+ residual) -> RMSNorm -> gate / up GEMV (SwiGLU) -> down GEMV (+ residual), seven launches; final
 * RMSNorm and the lm_head GEMV.  The workspace is the context's.  A row's logits and appended K / V depend on that row's inputs alone.
 * NOT promised: the bits of the operator-per-launch step.
 * Argument errors (code 1, nothing launched, nothing written): an incomplete descriptor / cache / state, keep != NULL, B outside
 * [1, cache rows], d / ffn / H * dh not multiples of 4, whatever pcy_f32_attn_decode_pos refuses for this geometry and capacity,
 * Tmax > max_pos. */
int pcy_f32_llama_decode(pcy_ctx*, const pcy_f32_llama_desc*, const pcy_f32_kv_cache*, const pcy_gen_state*, int B);
/* the same step, same bits, as ONE replayed hipGraph: a linear chain on one stream without parallel branches, captured on first use per
 * (descriptor and its weight pointers, cache, state, B) -- for host-driven loops (sampling, beam search) that write next_tok and *pos on
 * the device between steps */
int pcy_f32_llama_decode_graph(pcy_ctx*, const pcy_f32_llama_desc*, const pcy_f32_kv_cache*, const pcy_gen_state*, int B);
/* argmax of state->logits (fp32; lowest index on ties) -> next_tok / tokens_out[b][*step]; logprob[b] += fp32 log_softmax(logits)[token];
 * then ++*step and, when advance_pos != 0, ++*pos -- pcy_greedy_pick's rules.  Writes row *step of the optional fp32 record logits_all
 * ([max_steps, B, logits_all_ld or vocab]; may be pinned host memory) first.  -inf logits mean "never chosen"; NaN is outside the contract. */
int pcy_f32_greedy_pick(pcy_ctx*, const pcy_f32_llama_desc*, const pcy_f32_kv_cache*, const pcy_gen_state*, int B, int advance_pos);
/* n_steps x (pcy_f32_llama_decode + pcy_f32_greedy_pick with advance) with no host synchronisation; use_graph != 0 replays one captured
 * graph per step.  Eager and replayed runs give equal bits.  The caller keeps *step + n_steps <= max_steps and *pos + n_steps <= Tmax. */
int pcy_f32_llama_greedy(pcy_ctx*, const pcy_f32_llama_desc*, const pcy_f32_kv_cache*, const pcy_gen_state*, int B, int n_steps, int use_graph);
/* steps enqueued by the three entries above outside a graph replay (an eager step, or the capture of a graph) since the library was loaded */
unsigned long long pcy_debug_f32_stream_count(void);

/* ---- fp32 generation: beam search and sampling selection on the device ----
 * Opt-in (generate(decode_f32="device")), beside the host-side selection that the "ops" and "stream" modes keep.  Every entry checks its
 * arguments first and launches nothing when it refuses (code 1).  No floating-point atomics anywhere: equal calls give equal bits, and a
 * replayed chain gives the bits of the separate calls.
 *
 * One step of the diverse beam search on fp32 logits [B * beam, vocab]: pcy_beam_step's contract and state (pcy_beam_state above; step 0
 * extends beam 0 of a group only, top-g by rounds of arg-max with ties to the lowest flat index row * vocab + token, the penalty inside
 * the running score, double-buffered histories, src / anc parents, next_tok, EOS flags and the eos_id == 0 rule, the last workgroup
 * advances *step / *pos and raises *done, a launch with *done set changes nothing but src, which it sets to the identity so that the
 * reorder behind it moves nothing) with ONE difference: the candidate score is
 *   s(r, v) = ((x[r][v] - max_r) - lse_r) + cur[r] - penalty * #{earlier picks of this step == v},  lse_r = logf(sum expf(x - max_r)),
 * in fp32 throughout -- nothing is rounded to bf16 (the reference takes log_softmax in the model dtype, fp32 here).  The row statistics
 * come from 16 slices per row, combined in slice order; an all -inf slice or row gives (max = -inf, sum = 0), never a NaN.
 * beam <= 32, vocab <= 163840. */
int pcy_f32_beam_step(pcy_ctx*, const float* logits, int vocab, int B, int beam, int group_size, float diversity_penalty,
                      const pcy_beam_state* state);
/* K / V rows of a beam search on the token-major fp32 caches: row b of rows [0, B) takes slots [t0, t) of row src_rows[b] (device int32
 * [B]; any row of the cache), every layer, K and V, in place.  Correct for any map (cycles, one source for many rows): two launches, a
 * gather into the context's workspace and the write back; rows that keep their place are skipped; slots outside [t0, t), rows >= B and the
 * rows of a source outside the cache are not touched.  The scratch is sized for the suffix capacity Tmax - t0, not for t.  t <= t0: nothing. */
int pcy_f32_kv_reorder_range(pcy_ctx*, const pcy_f32_llama_desc*, const pcy_f32_kv_cache* kv, const int32_t* src_rows, int B, int t0, int t);
/* out of place: row r of dst_kv, r in [0, B), takes slots [0, t) of row src_rows[r] of src_kv (another cache of the same model; its own
 * row count and capacity): replicates a B-row prefill into B * beam rows with the map r / beam.  Nothing else of dst_kv is written. */
int pcy_f32_kv_copy_rows(pcy_ctx*, const pcy_f32_llama_desc*, const pcy_f32_kv_cache* dst_kv, const pcy_f32_kv_cache* src_kv, const int32_t* src_rows,
                         int B, int t);
/* n_steps iterations (steps >= 1) of an fp32 beam search for the B * beam rows: pcy_f32_llama_decode -> logits_rec[*step][row][vocab] = the
 * step's logits (NULL: no record) -> pcy_f32_beam_step -> the reorder of slots [kv_t0, *pos), *pos read on the device behind the beam step.
 * Each iteration is ONE replayed linear launch chain (no parallel branches), captured on first use per (descriptor and its weights, cache,
 * both states, every argument).  gen_state->pos / next_tok must be the beam state's arrays.  The kernels and the bits of
 * pcy_f32_llama_decode_graph + a copy + pcy_f32_beam_step + pcy_f32_kv_reorder_range(t0 = kv_t0, t = *pos).  The caller keeps
 * *step + n_steps <= max_len and *pos + n_steps <= Tmax.  Refuses what those entries refuse, and kv_t0 outside [0, Tmax]. */
int pcy_f32_llama_beam_steps(pcy_ctx*, const pcy_f32_llama_desc*, const pcy_f32_kv_cache* kv, const pcy_gen_state*, int B, int beam, int group_size,
                             float diversity_penalty, const pcy_beam_state* state, float* logits_rec, int n_steps, int kv_t0);
/* Sampling / nucleus selection (`_generate_sampling` without greedy, model_unified.py:896-906) on state->logits [B, vocab] fp32:
 *   probs = softmax(logits / temperature) in fp32 (the correctly rounded quotient, then exp(. - max) / sum);
 *   nucleus_prob in (0, 1): probs = softmax(logits) (no temperature) times the mask of the tokens whose ascending cumulative probability
 *   has reached 1 - nucleus_prob -- equal probabilities in token order (a stable sort: the lower index counts as the smaller), the kept
 *   mass not renormalised, everything kept when nothing reaches the threshold; nucleus_prob <= 0: no mask;
 *   token = first index in vocabulary order whose cumulative kept probability exceeds uniforms[*step * B + b] * total (the CALLER's
 *   variates in [0, 1), device fp32 [max_steps * B]; the last kept token when a variate >= 1 pushes the draw past the end);
 *   logprob[b] += fp32 log_softmax(unscaled logits)[token]; next_tok / tokens_out[b][*step]; row *step of the optional fp32 record
 *   logits_all first; then ++*step and, when advance_pos != 0, ++*pos.  probs_out: optional [B, vocab] fp32, the masked vector.
 * The nucleus threshold is found by a radix select over the bit patterns of the probabilities (12 + 12 + 8 bits; non-negative floats order
 * like their patterns); bucket masses, the kept total and the CDF are sums of trunc(p * 2^44) in 64-bit integers, so the token is a
 * deterministic function of (logits, variate): a mass differs from the exact sum of the fp32 probabilities by less than vocab * 2^-44
 * (a threshold that the row's mass misses by no more than that counts as reached by the largest token).  The fp32 probabilities of a row
 * sum to 1 only within fp32 rounding, about 2^-22: a nucleus_prob below that is accepted but not resolved -- whether 1 - nucleus_prob is
 * reached (the top token alone is kept) or not (everything is kept) then depends on that rounding.
 * -inf logits mean "never chosen" (probability exactly 0); a row must hold a finite logit; NaN is outside the contract.  *step outside
 * [0, max_steps) selects nothing.  temperature > 0, nucleus_prob < 1, vocab <= 163840. */
int pcy_f32_sample_pick(pcy_ctx*, const pcy_f32_llama_desc*, const pcy_f32_kv_cache*, const pcy_gen_state*, int B, int advance_pos, float temperature,
                        float nucleus_prob, const float* uniforms, float* probs_out);
/* n_steps x (pcy_f32_llama_decode + pcy_f32_sample_pick with advance) with no host synchronisation; use_graph != 0 replays one captured
 * chain per step.  Eager and replayed runs give equal bits.  The caller keeps *step + n_steps <= max_steps and *pos + n_steps <= Tmax. */
int pcy_f32_llama_sample(pcy_ctx*, const pcy_f32_llama_desc*, const pcy_f32_kv_cache*, const pcy_gen_state*, int B, int n_steps, float temperature,
                         float nucleus_prob, const float* uniforms, int use_graph);
/* steps enqueued by the entries above since the library was loaded (eager, captured or replayed) -- 0: beam steps (pcy_f32_beam_step,
 * pcy_f32_llama_beam_steps), 1: sampling steps (pcy_f32_sample_pick, pcy_f32_llama_sample); anything else reads 0 */
unsigned long long pcy_debug_f32_select_count(int which);

#ifdef __cplusplus
}
#endif
#endif /* PCY_H */
