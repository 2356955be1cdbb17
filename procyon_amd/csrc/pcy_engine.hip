// Host side of libpcy.so: context, workspace, layer loops, hipGraph capture, and the extern "C" ABI
// declared in include/pcy.h.  No torch types; everything is raw device pointers on one HIP stream.
#include <stdio.h>
#include <stdlib.h>
#include <stdarg.h>
#include <string.h>
#include <dlfcn.h>
#include <vector>

#include "../../include/pcy.h"
#include "pcy_internal.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(2, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// A cache with a shared prefix (pcy.h, pcy_kv_cache): k / v hold the suffix slots only and the LOGICAL capacity -- what *pos, the keep mask
// and the score rows count in -- is prefix_T + Tmax.  A plain cache has all-zero prefix fields: kv_cap == Tmax.
inline bool kv_shared(const pcy_kv_cache* kv) { return kv->prefix_k != nullptr || kv->prefix_v != nullptr || kv->prefix_T != 0; }
inline int kv_cap(const pcy_kv_cache* kv) { return kv->Tmax + (kv_shared(kv) ? kv->prefix_T : 0); }
// calls of pcy_llama_extend_grouped (pcy_debug_extend_grouped_count).  A word of its own, not a kind of pcy_debug_dispatch_count: the kinds
// [0, PCY_DISPATCH_N) and the ABI number are pinned by the suite, and a new entry point is an addition that old callers never see.
unsigned long long g_pcy_extend_grouped = 0;
// calls of pcy_look_draft / pcy_look_verify (pcy_debug_look_count): words of their own for the same reason
unsigned long long g_pcy_look[2] = {0, 0};
// steps enqueued by pcy_llama_decode_gemm (pcy_debug_decode_gemm_count): a word of its own for the same reason
unsigned long long g_pcy_decode_gemm = 0;
// ... of which by pcy_llama_decode_gemm_mq (pcy_debug_attn_mq_count)
unsigned long long g_pcy_attn_mq = 0;
// steps enqueued with the split-key attention (pcy_llama_decode_split / _beam_steps_split / _decode_gemm_split; pcy_debug_attn_split_count)
unsigned long long g_pcy_attn_split = 0;
// steps enqueued by pcy_llama_decode_w8 / pcy_llama_greedy_w8 outside a graph replay (pcy_debug_decode_w8_count): a word of its own as well
unsigned long long g_pcy_decode_w8 = 0;
// calls of pcy_llama_decode_window (pcy_debug_decode_window_count): a word of its own as well
unsigned long long g_pcy_decode_window = 0;
// steps enqueued by the fp32 stream step (pcy_f32_llama_decode / _decode_graph / _greedy) outside a graph replay (pcy_debug_f32_stream_count)
unsigned long long g_pcy_f32_stream = 0;
// steps enqueued by the fp32 selection entries (pcy_debug_f32_select_count) -- 0: beam steps, 1: sampling steps; eager, captured or replayed
unsigned long long g_pcy_f32_select[2] = {0, 0};

}  // namespace

// for the other translation units of the library (pcy_f32.hip): the thread-local error text behind pcy_last_error
void pcy_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// EVERYTHING a captured decode step (or beam-search step) was derived from, each value in a field of its own: every pointer of the state /
// cache / model the enqueue functions read AND the geometry (an allocator may hand a new state or a cache of another capacity the
// addresses of the previous one while e.g. the `keep` mask or the token buffer differ -- a stale graph would then run with dangling
// arguments), the context's buffers that are baked into the launches, and the switch snapshot the launches were chosen under.  Zero-filled
// before it is filled in (key_base) and compared with memcmp: no packing, no hashing.
// What a captured step is made of (the values are those of earlier logs: they stay)
enum GraphKind {
  KIND_GREEDY = 0,       // decode + greedy pick (pcy_llama_greedy)
  KIND_DECODE = 1,       // decode only (pcy_llama_decode_graph)
  KIND_BEAM = 2,         // a beam-search step (pcy_llama_beam_steps / _split)
  KIND_GREEDY_W8 = 3,    // decode on e4m3 weights + greedy pick (pcy_llama_greedy_w8)
  KIND_F32_DECODE = 4,   // the fp32 stream step alone (model = the pcy_f32_llama_desc, here and below)
  KIND_F32_GREEDY = 5,   // ... with its greedy pick
  KIND_F32_BEAM = 6,     // an fp32 beam-search step (pcy_f32_llama_beam_steps)
  KIND_F32_SAMPLE = 7,   // the fp32 step with its sampling pick
};
struct DecodeGraphKey {
  int kind;                           // a GraphKind
  int B;
  PcySwitches sw;
  const void *model, *layers, *embed, *kv_k, *kv_v, *pos, *step, *next_tok, *logits, *keep;
  int Tmax, kv_B;
  const void *kv_prefix_k, *kv_prefix_v;           // shared-prefix cache: a captured step is never replayed on another prefix
  int kv_prefix_T, kv_prefix_B, kv_rows_per_prefix;
  const void *ws, *mc_tags, *mb_flags, *nb_tags, *dev_layers;
  uint64_t layers_fp;
  const void *tokens_out, *logprob, *logits_all;   // key_record: what a pick behind the step writes
  int logits_all_ld, max_steps;
  pcy_beam_state beam_state;                       // key_beam: every array of the beam state is baked into the chain
  const void *logits_rec, *beam_ws;
  int beam, group_size, kv_t0;
  uint32_t penalty_bits;
  const void* w8;                                  // KIND_GREEDY_W8: the host array of e4m3 layers and a fingerprint of the device pointers it holds
  uint64_t w8_fp;
  int attn_split;                                  // 1: every layer's attention is the split-key one (pcy_attn_split.hip); never shares a graph with 0
  const void* uniforms;                            // KIND_F32_SAMPLE: the variates and the two parameters of the sampling pick
  uint32_t temperature_bits, nucleus_bits;
  const void *stop_finished, *stop_done, *stop_n_steps_run;   // key_base: the EOS stop of the state (all zero: none); a chain with a stop and
  int stop_eos_id;                                            // one without never share a graph
};

struct pcy_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t cap_stream = nullptr;  // capture needs a non-legacy stream; replays go to `stream`
  char* ws = nullptr;
  size_t ws_bytes = 0;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // captured decode step
  hipGraphExec_t graph = nullptr;
  DecodeGraphKey graph_key = {};      // what `graph` was captured for (meaningful while graph != nullptr)
  int n_cu = 0;
  // sticky error word: a cross-workgroup hand-over inside a launch hit its watchdog.  PINNED HOST memory (device-visible): the
  // kernels store it with system scope, every ABI entry looks at it without touching the stream (take_sticky_error below)
  unsigned* xwg_err = nullptr;
  // fused attention + o projection launches of the layered decode step: [0] = step epoch, [64 + 64*l ...] = flags of layer l
  unsigned* ao_sync = nullptr;
  // tagged hand-over vectors of the MLP chain launches: [layer][ffn + d] words, owned by one model geometry at a time
  uint32_t* mc_tags = nullptr;
  const void* mc_tags_model = nullptr;
  size_t mc_tags_words = 0;
  PcySwitches mc_tags_sw = {};        // the switch snapshot the slots were last zeroed under
  uint64_t layers_fp = 0;              // fingerprint of the weight pointers dev_layers was built from
  PcyLayerWeightsDev* dev_layers = nullptr;   // device copy of the layers' weight pointers (decode_step_kernel)
  // small-batch decode step (pcy_decode_nb.hip): hand-over slots and tag counter PER BATCH SIZE (a slot is rewritten in every step of its
  // own batch size and its counter only advances with those steps, so a word with the current tag can only come from the current step)
  uint32_t* nb_tags[9] = {};
  unsigned* nb_sync = nullptr;        // [16] tag counters, index = batch size
  // mid-batch decode step (pcy_decode_mb.hip): arrival flags [(layers + 1)][pcy_decode_mb_flag_words()] (a flag holds the epoch of the step that
  // raised it) and the epoch word, advanced once per step and never reset
  unsigned* mb_flags = nullptr;
  size_t mb_flags_words = 0;
  unsigned* mb_sync = nullptr;
  uint32_t* op_tags = nullptr;        // tagged `act` vector of pcy_decode_mlp ([ffn] words, its own counter)
  size_t op_tags_words = 0;
  unsigned* smp_hist = nullptr;       // [rows][65536] histogram scratch of the nucleus step (kept all-zero between calls)
  int smp_hist_rows = 0;
  bf16_t* smp_pbits = nullptr;        // [rows][vocab] bits of the probabilities of the sampling step
  size_t smp_pbits_elems = 0;
  char* beam_ws = nullptr;            // scratch of pcy_beam_step (its own allocation: never aliases the decode workspace)
  size_t beam_ws_bytes = 0;

  // Replayed launch chains of the short-sequence encoder (pcy_esm_encode of ONE protein = 230 launches of 5-35 us: on a busy host the
  // launch rate, not the GPU, sets the time -- measured 6.1 to 11 ms per call across gpurun boxes for 4.8 ms of kernels).  A slot is keyed
  // on every pointer and size that is baked into the launches; a key is captured the SECOND time it is seen (a stream of proteins of
  // ever-changing length never pays for captures it would not reuse).
  struct GraphSlot { uint64_t key[16]; hipGraphExec_t exec; unsigned long long stamp; };
  static constexpr int N_GSLOTS = 8;
  GraphSlot gslots[N_GSLOTS] = {};
  unsigned long long gstamp = 0;
  void drop_gslots() {
    for (auto& g : gslots) {
      if (g.exec) hipGraphExecDestroy(g.exec);
      g = GraphSlot{};
    }
  }

  int reserve(size_t bytes) {
    // PCY_DEBUG_POISON_WS=1 (tests): fill the workspace with NaN patterns before every use -- a kernel that reads a workspace
    // location before writing it then fails deterministically instead of depending on what the allocator handed out
    static const bool poison = [] { const char* e = getenv("PCY_DEBUG_POISON_WS"); return e && atoi(e) != 0; }();
    if (poison && ws && bytes <= ws_bytes) HIP_TRY(hipMemsetAsync(ws, 0xFF, ws_bytes, stream));
    if (bytes <= ws_bytes) return 0;
    if (ws) {
      HIP_TRY(hipStreamSynchronize(stream));
      HIP_TRY(hipFree(ws));
      ws = nullptr; ws_bytes = 0;
    }
    drop_graph();
    drop_gslots();
    bytes = align_up(bytes + (bytes >> 3), 1 << 20);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&ws), bytes));
    ws_bytes = bytes;
    if (poison) HIP_TRY(hipMemsetAsync(ws, 0xFF, ws_bytes, stream));
    return 0;
  }
  void drop_graph() {
    if (graph) { hipGraphExecDestroy(graph); graph = nullptr; }
  }
};

namespace {

struct Carver {
  char* p; size_t off = 0;   // base == nullptr: a sizing run, `off` is all that counts
  explicit Carver(char* base) : p(base) {}
  template <typename T> T* take(size_t n) {
    T* r = p ? reinterpret_cast<T*>(p + off) : nullptr;
    off = align_up(off + n * sizeof(T), 256);
    return r;
  }
};

// A watchdog of an in-launch wait has fired since the last look (results of that launch and of everything that consumed them are
// invalid): report it ONCE, from whichever ABI call comes next -- no stream synchronisation, the word lives in host memory.
int take_sticky_error(pcy_ctx* c) {
  if (!c->xwg_err) return 0;
  const unsigned code = *reinterpret_cast<volatile unsigned*>(c->xwg_err);
  if (!code) return 0;
  *reinterpret_cast<volatile unsigned*>(c->xwg_err) = 0;
  return fail(4, "decode kernel: a cross-workgroup dependency wait timed out (code %u): its workgroups were not all resident -- is "
                 "another kernel running on this device? -- results since the last successful pcy_ctx_sync are invalid", code);
}
#define PCY_STICKY(c)                                 \
  do {                                                \
    if (int r_ = take_sticky_error(c)) return r_;     \
  } while (0)

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(3, "kernel launch failed in %s: %s", what, hipGetErrorString(e));
  return 0;
}

// ---- the geometry rules of the attention and step entries, each in ONE place; `what` names the entry that was called ----
// the head size (dh32: 32 is served too), and with it the query heads per K/V head
int check_head_dim(const char* what, int dh, bool dh32) {
  return dh == 64 || dh == 128 || (dh32 && dh == 32) ? 0 : fail(1, "%s: head_dim %d unsupported (%s64/128)", what, dh, dh32 ? "32/" : "");
}
int check_heads(const char* what, int H, int Hkv, int dh, bool dh32) {
  if (int r = check_head_dim(what, dh, dh32)) return r;
  return Hkv < 1 || H % Hkv || !(H / Hkv == 1 || H / Hkv == 2 || H / Hkv == 4 || H / Hkv == 8) ? fail(1, "%s: H/Hkv must be 1, 2, 4 or 8", what) : 0;
}
// d, ffn, H*dh and the K/V columns (qkv_row: the whole qkv row) are multiples of `multiple`
int check_widths(const char* what, const pcy_llama_desc* m, int multiple, bool qkv_row) {
  const int HD = m->n_heads * m->head_dim, last = (qkv_row ? m->n_heads + 2 * m->n_kv_heads : m->n_kv_heads) * m->head_dim;
  if (m->d % multiple == 0 && m->ffn % multiple == 0 && HD % multiple == 0 && last % multiple == 0) return 0;
  return fail(1, "%s: d, ffn, H*dh, %s must be multiples of %d", what, qkv_row ? "(H+2Hkv)*dh" : "Hkv*dh", multiple);
}

// GEMM for any M: MFMA tiles when M is large enough to fill them, the streaming GEMV otherwise
// next_w / next_xn / fused (optional): RMSNorm(C) * next_w -> next_xn inside the projection's finish launch where that exists
// (*fused = 1), see PcyGemmArgs
void linear(hipStream_t s, const bf16_t* A, int lda, const bf16_t* W, const bf16_t* bias, const bf16_t* resid, int ldr,
            bf16_t* C, int ldc, int M, int N, int K, int epi, float* splitk_ws = nullptr, size_t splitk_ws_bytes = 0,
            const bf16_t* next_w = nullptr, bf16_t* next_xn = nullptr, int* fused = nullptr, float rms_eps = 0.f, int rms_cast = 0, int splitk_fill = 0) {
  if (M <= 8 && epi != EPI_SWIGLU && (resid == nullptr || ldr == ldc)) {
    PcyGemvArgs g{};
    g.W = W; g.x = A; g.y = C; g.bias = bias; g.resid = resid; g.rms_w = nullptr;
    g.N = N; g.K = K; g.B = M; g.ldx = lda; g.ldy = ldc; g.epi = epi;
    pcy_launch_gemv(s, g);
    return;
  }
  PcyGemmArgs a{};
  a.A = A; a.W = W; a.C = C; a.bias = bias; a.resid = resid;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.ldr = ldr; a.epi = epi;
  a.splitk_ws = splitk_ws; a.splitk_ws_bytes = splitk_ws_bytes;
  a.next_rms_w = next_w; a.next_xn = next_xn; a.fused_next = fused; a.rms_eps = rms_eps; a.rms_cast = rms_cast; a.splitk_fill = splitk_fill;
  pcy_launch_gemm(s, a);
}

// ------------------------------------------------------------------ decode step (enqueue only)
// The switches a decode step depends on arrive as ONE snapshot (PcySwitches, pcy_switch.h), taken by the ABI entry; nothing below reads the
// environment.  What each PCY_DISABLE name selects here (every twin has the same bits unless noted; tests compare them in one process):
//   attn_o           the decode attention and the o projection as two launches instead of one (batch 1, head_dim 128, d = 4096: 3.35 -> 3.28 ms/token fused)
//   decode_layer     the batch-1 step launch by launch (qkv GEMV, attention + o, gate/up, down) instead of one decode_layer_kernel per layer
//   decode_step      one launch per decoder layer instead of one for all layers (decode_step_kernel)
//   attn_qkv_finish  the qkv K-split finish as its own launch instead of inside the attention's
//   decode_nb        batches of 2..8 rows on the pre-round-5 path (streaming GEMVs below 4 rows, MFMA GEMVs from 4 on: ANOTHER arithmetic) instead
//                    of the small-batch step (pcy_decode_nb.hip);  decode_nb_step: its launch-per-stage twin (gemv_stream_kernel + attn_dec_kernel
//                    with the same column slices) instead of the one launch
//   decode_mb_step   batches of 9..32 rows launch by launch (seven per layer) instead of the mid-batch step (pcy_decode_mb.hip: the same work items
//                    as phases of ONE launch)
// PCY_AO_XMIN (PcySwitches::ao_xmin): the key split's exchange costs more on the small-batch step than the K reads it saves until much longer
// caches (t ~ 800: 2 / 4 rows 2.935 / 3.385 ms per step with the split, 2.868 / 3.287 without; t ~ 1540: 3.158 / 3.653 with, 3.180 / 3.632 without).
//
// The mid-batch step is OFF by default (round 6): bit-identical to the launches, and -- once the launches' GEMVs walk their K ranges in rotated
// order (pcy_gemv_kshift) -- no faster: 3.98 / 4.17 ms per step at 10 / 16 rows against 3.88 / 4.02 launch by launch, 4.8 / 5.1 against 4.1 / 4.3
// at 20 / 32 rows (two batch tiles double the activation bytes every CU fetches per weight byte).  Its streaming phases run at the HBM rate
// (G 6.3 TB/s, D 6.1); what it loses is the Q / O phases (16 / 8 tiles per wave against a ring of 7: two memory round trips whatever the
// prefetch) and the flag hops.  PCY_MB_MAX=<rows> (9..32) runs it up to that batch size: tests, tools/bench_decode_mb.py.
unsigned long long* g_mc_trace = nullptr;
constexpr int AO_MAX_LAYERS = 128, AO_FLAGS = 64;
// geometry of the small-batch step: Llama-3-8B, 256 CUs
// (7 and 8 rows: since the batched launches walk their K ranges in rotated order, ask for their finish loads at once and cut the attention
// into 64-column workgroups from 4 rows on, they take 3.69 / 3.70 ms per step against the fused step's 3.81 / 3.97 -- the fused step stops
// at 6 rows (3.65 against 3.69); PCY_NB_MAX=7 / 8 runs it there all the same: tests, tools)
bool decode_nb_covers(const pcy_ctx* c, const pcy_llama_desc* m, int B, const PcySwitches& sw) {
  return B >= 2 && B <= sw.nb_max && m->d == 4096 && m->ffn == 14336 && m->n_heads == 32 && m->n_kv_heads == 8 && m->head_dim == 128 &&
         c->n_cu >= 256 && m->n_layers <= AO_MAX_LAYERS / 2;   // (score-exchange flags: 2 x AO_FLAGS words per layer)
}
// geometry of the mid-batch step (9..32 rows): the same model and chip
bool decode_mb_covers(const pcy_ctx* c, const pcy_llama_desc* m, int B, const PcySwitches& sw) {
  return B >= 9 && B <= 32 && B <= sw.mb_max && m->d == 4096 && m->ffn == 14336 && m->n_heads == 32 && m->n_kv_heads == 8 && m->head_dim == 128 && c->n_cu >= 256;
}
// tagged vectors of one layer: act [ffn], qkv [(H + 2 Hkv) dh], attention output [H dh], x after o [d]
size_t tag_words_per_layer(const pcy_llama_desc* m) {
  return (size_t)m->ffn + (size_t)m->d + (size_t)(m->n_heads + 2 * m->n_kv_heads) * m->head_dim + (size_t)m->n_heads * m->head_dim;
}

// device words of the in-launch hand-overs; must run outside stream capture
int ensure_sync_words(pcy_ctx* c) {
  if (!c->n_cu) {
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device));
    c->n_cu = prop.multiProcessorCount;
  }
  if (!c->xwg_err) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->xwg_err), 64, hipHostMallocMapped | hipHostMallocCoherent));
    memset(c->xwg_err, 0, 64);
  }
  if (!c->ao_sync) {
    // [0] step epoch, [1] tag counter of the decode step's fused launches, [2] tag counter of pcy_decode_mlp, attention->o flags,
    // score-exchange flags
    const size_t bytes = (size_t)(64 + 2 * AO_MAX_LAYERS * AO_FLAGS) * sizeof(unsigned);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->ao_sync), bytes));
    HIP_TRY(hipMemset(c->ao_sync, 0, bytes));
  }
  return 0;
}
// FNV-1a over pointers, in the order they are given: the fingerprint of a set of weights that a captured step bakes in
uint64_t fnv1a(uint64_t h, std::initializer_list<const void*> ptrs) {
  for (const void* p : ptrs) h = (h ^ (uint64_t)(uintptr_t)p) * 1099511628211ull;
  return h;
}
constexpr uint64_t FNV_BASIS = 1469598103934665603ull;
uint64_t layers_fingerprint(const pcy_llama_desc* m) {   // every weight pointer the fused decode launches read
  uint64_t h = fnv1a(FNV_BASIS, {m->layers});
  for (int l = 0; l < m->n_layers; ++l) {
    const pcy_llama_layer& L = m->layers[l];
    h = fnv1a(h, {L.ln1, L.wqkv, L.wo, L.ln2, L.wgu, L.wdown});
  }
  return h;
}
int ensure_decode_state(pcy_ctx* c, const pcy_llama_desc* m, int B, const PcySwitches& sw) {
  if (int r = ensure_sync_words(c)) return r;
  // A tagged word counts as delivered when its tag equals the chain epoch, so the slots must never hold anything but words of
  // earlier chain launches OF THE SAME LAYOUT: another model -> zeroed slots and a restarted epoch (next tag 1).
  // (a change of the switch snapshot as well: a slot the new launch mix reads may not have been rewritten for a while)
  // "Another model" is decided on the weight POINTERS, not on the descriptor's address: a new engine of the same geometry may
  // get the address of a freed descriptor, and a descriptor may be mutated in place -- either would leave dev_layers stale.
  const size_t words = (size_t)m->n_layers * (tag_words_per_layer(m) + 32 * 256);   // + the residual stream between the layers, one line per workgroup
  const uint64_t fp = layers_fingerprint(m);
  if (c->mc_tags_model != m || c->mc_tags_words != words || c->mc_tags_sw != sw || c->layers_fp != fp) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->drop_graph();   // a captured step holds mc_tags / dev_layers as kernel arguments
    if (c->mc_tags) HIP_TRY(hipFree(c->mc_tags));
    c->mc_tags = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->mc_tags), words * 4));
    HIP_TRY(hipMemset(c->mc_tags, 0, words * 4));
    HIP_TRY(hipMemset(c->ao_sync + 1, 0, 4));
    for (auto& t : c->nb_tags) { if (t) HIP_TRY(hipFree(t)); t = nullptr; }
    if (c->dev_layers) HIP_TRY(hipFree(c->dev_layers));
    c->dev_layers = nullptr;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->dev_layers), (size_t)m->n_layers * sizeof(PcyLayerWeightsDev)));
    std::vector<PcyLayerWeightsDev> lw(m->n_layers);
    for (int l = 0; l < m->n_layers; ++l) {
      const pcy_llama_layer& L = m->layers[l];
      lw[l] = {(const bf16_t*)L.ln1, (const bf16_t*)L.wqkv, (const bf16_t*)L.wo, (const bf16_t*)L.ln2, (const bf16_t*)L.wgu, (const bf16_t*)L.wdown};
    }
    HIP_TRY(hipMemcpy(c->dev_layers, lw.data(), lw.size() * sizeof(PcyLayerWeightsDev), hipMemcpyHostToDevice));
    c->mc_tags_model = m; c->mc_tags_words = words; c->mc_tags_sw = sw; c->layers_fp = fp;
  }
  if (!sw.off(PCY_SW_decode_nb) && decode_nb_covers(c, m, B, sw) && !c->nb_tags[B]) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (!c->nb_sync) {
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->nb_sync), 16 * sizeof(unsigned)));
      HIP_TRY(hipMemset(c->nb_sync, 0, 16 * sizeof(unsigned)));
    }
    const size_t nbw = (size_t)m->n_layers * (pcy_decode_nb_tag_words(B) + pcy_decode_nb_line_words(B));
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->nb_tags[B]), nbw * 4));
    HIP_TRY(hipMemset(c->nb_tags[B], 0, nbw * 4));
    HIP_TRY(hipMemset(c->nb_sync + B, 0, 4));   // zeroed slots, next tag 1
  }
  if (decode_mb_covers(c, m, B, sw)) {
    const size_t fw = (size_t)(m->n_layers + 1) * pcy_decode_mb_flag_words();
    if (!c->mb_sync) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->mb_sync), 64));
      HIP_TRY(hipMemset(c->mb_sync, 0, 64));
    }
    if (c->mb_flags_words < fw) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      c->drop_graph();
      if (c->mb_flags) HIP_TRY(hipFree(c->mb_flags));
      c->mb_flags = nullptr; c->mb_flags_words = 0;
      HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->mb_flags), fw * 4));
      HIP_TRY(hipMemset(c->mb_flags, 0, fw * 4));   // (the epoch word keeps counting: a zeroed flag never equals a later epoch)
      c->mb_flags_words = fw;
    }
  }
  return 0;
}

size_t decode_ws_bytes(const pcy_llama_desc* m, int B, int Tmax) {
  const size_t qkvw = (size_t)(m->n_heads + 2 * m->n_kv_heads) * m->head_dim;
  return align_up((size_t)B * m->d * 2, 256) + align_up(B * qkvw * 2, 256) +
         align_up((size_t)B * m->n_heads * m->head_dim * 2, 256) + align_up((size_t)B * m->ffn * 2, 256) +
         align_up((size_t)B * m->n_heads * (Tmax + 1) * 4, 256) + align_up((size_t)B * 64 * 16, 256) +
         align_up((size_t)B * m->d * 2, 256) + (B >= pcy_mfma_min_batch() ? align_up((size_t)8 * B * qkvw * 4, 256) : 0) + 4096;
}

// The carve of the decode workspace (decode_ws_bytes), in ONE place: the step's launches and the pick / sampling launches behind it agree on it.
struct DecodeWs {
  bf16_t *x, *qkv, *ao, *act, *xn;   // (xn: normalised x for the batched (MFMA) GEMV path)
  float* scores;
  void* partials;                    // row partials of the greedy pick / the sampling step
  float* sk_ws; size_t sk_bytes;     // K-split partial sums of the batched GEMVs
};
DecodeWs carve_decode_ws(char* base, const pcy_llama_desc* m, int B, int Tmax) {
  const size_t qkvw = (size_t)(m->n_heads + 2 * m->n_kv_heads) * m->head_dim;
  Carver cv(base);
  DecodeWs w{};
  w.x = cv.take<bf16_t>((size_t)B * m->d);
  w.qkv = cv.take<bf16_t>((size_t)B * qkvw);
  w.ao = cv.take<bf16_t>((size_t)B * m->n_heads * m->head_dim);
  w.act = cv.take<bf16_t>((size_t)B * m->ffn);
  w.scores = cv.take<float>((size_t)B * m->n_heads * (Tmax + 1));
  w.partials = cv.take<char>((size_t)B * 64 * 16);
  w.xn = cv.take<bf16_t>((size_t)B * m->d);
  w.sk_bytes = B >= pcy_mfma_min_batch() ? (size_t)8 * B * qkvw * 4 : 0;
  w.sk_ws = w.sk_bytes ? cv.take<float>(w.sk_bytes / 4) : nullptr;
  return w;
}
// What the launches of one decode step share: the workspace and the call's arguments
struct DecodeCx : DecodeWs {
  pcy_ctx* c; const pcy_llama_desc* m; const pcy_kv_cache* kv; const pcy_gen_state* st; int B;
  int qkvw; size_t layer_stride;     // columns of the qkv projection; elements between the K (V) caches of consecutive layers
  size_t prefix_layer_stride;        // ... and between the layers of the shared prefix arrays (0: a plain cache)
  const pcy_llama_layer_fp8* w8;     // the e4m3 layers of the step that streams them (nullptr for every other step)
};
DecodeCx decode_cx(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, const pcy_llama_layer_fp8* w8 = nullptr) {
  return DecodeCx{carve_decode_ws(c->ws, m, B, kv_cap(kv)), c, m, kv, st, B, (m->n_heads + 2 * m->n_kv_heads) * m->head_dim,
                  (size_t)kv->B * m->n_kv_heads * kv->Tmax * m->head_dim,
                  kv_shared(kv) ? (size_t)kv->prefix_B * m->n_kv_heads * kv->prefix_T * m->head_dim : 0, w8};
}

// Which launches serve a step: decided once, from the context's state, the geometry, the batch size and the switch snapshot.  `path` is the
// FIRST path attempted; a launcher that declines at launch time (geometry, residency) hands the step on: the one-launch batch-1 step ->
// layer launches -> the loop; the small-batch step -> the loop on forced streaming kernels (its twin); the mid-batch step -> the MFMA loop.
enum DecodePath { DEC_STEP_GQA, DEC_STEP_MHA, DEC_LAYERS, DEC_STEP_NB, DEC_STEP_MB, DEC_LOOP_STREAM, DEC_LOOP_MFMA };
struct DecodePlan {
  DecodePath path;
  bool nb_on;               // 2..8 rows on the small-batch arithmetic (the one launch or its launch-per-stage twin; lm_head as before)
  bool batched;             // the loop's projections on the skinny-MFMA GEMVs, 32 rows per pass over the weights, fed from xn
  bool batched_head;        // ... and lm_head (F = 11008, Llama-2-7B / ProCyon-Split: 86 x 128)
  bool attn_o;              // loop, one row: attention and o projection in one launch (Wo rows wait in registers while the attention runs)
  bool defer_qkv_finish;    // loop, batched: the attention adds up the K-split partial sums of ITS rows instead of a finish launch (up to 32
                            // rows: above, the GEMV runs in 32-row passes that share the workspace -- the finish is a launch per pass, same bits)
  int krot;                 // one row: the projections over d walk their k-iterations rotated (PcyGemvArgs::krot) -- in the streaming launches, in
                            // the launches that fuse them (attn_o, mlp_chain) and in the one-launch steps alike: one set of bits
  int force_ds;             // output columns per workgroup of the loop's stand-alone attention: those of the fused step it is the twin of
  int xmin;                 // cached keys from which the fused launches split the keys across their slice workgroups
  unsigned* epoch_word;     // sync words this step advances (the embed launch, or one-thread launches for layers_only): the step epoch ...
  unsigned* tag_word;       // ... and the tag counter of the hand-over slots it uses
};
DecodePlan plan_decode(const pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, int B, const PcySwitches& sw) {
  DecodePlan p{};
  p.batched_head = B >= pcy_mfma_min_batch() && m->d % 128 == 0 && m->ffn % 128 == 0;
  // a cache with a shared prefix is read by the stand-alone attention launches of the batched loop only: never by a one-launch step
  // (check_decode_cache turns every other outcome into an argument error)
  const bool shared = kv_shared(kv);
  p.nb_on = !shared && !sw.off(PCY_SW_decode_nb) && decode_nb_covers(c, m, B, sw) && c->nb_tags[B] && c->nb_sync && c->dev_layers && c->ao_sync && c->xwg_err &&
            pcy_decode_nb_launchable(c->device, B, kv_cap(kv), c->n_cu, sw.nb_ub);
  p.batched = p.batched_head && !p.nb_on;
  const bool nb_step = p.nb_on && !sw.off(PCY_SW_decode_nb_step);
  const bool mb_step = !shared && p.batched && !sw.off(PCY_SW_decode_mb_step) && decode_mb_covers(c, m, B, sw) && pcy_decode_mb_fits(B, kv->Tmax) && c->mb_flags && c->mb_sync &&
                       c->dev_layers && c->xwg_err && (size_t)(m->n_layers + 1) * pcy_decode_mb_flag_words() <= c->mb_flags_words;
  p.attn_o = !sw.off(PCY_SW_attn_o) && B == 1 && c->ao_sync && c->xwg_err && m->n_layers <= AO_MAX_LAYERS;
  const bool try_layer = !sw.off(PCY_SW_decode_layer) && p.attn_o && c->mc_tags;
  // (multi-head geometry, one row: the column split of the fused step's attention workgroups, whatever the launch mix -- one set of bits)
  const bool mha1 = B == 1 && pcy_decode_mha_covers(m->d, m->n_heads, m->n_kv_heads, m->head_dim, m->ffn, c->n_cu);
  p.path = nb_step ? DEC_STEP_NB : mb_step ? DEC_STEP_MB
         : try_layer && !sw.off(PCY_SW_decode_step) && c->dev_layers ? (mha1 ? DEC_STEP_MHA : DEC_STEP_GQA)
         : try_layer ? DEC_LAYERS : p.batched ? DEC_LOOP_MFMA : DEC_LOOP_STREAM;
  p.defer_qkv_finish = p.batched && B <= 32 && !p.attn_o && !sw.off(PCY_SW_attn_qkv_finish);
  p.krot = B == 1 ? 1 : 0;
  p.force_ds = mha1 ? pcy_decode_mha_ds() : p.nb_on ? pcy_decode_nb_ds(B) : 0;
  p.xmin = sw.ao_xmin(B);
  p.epoch_word = (p.attn_o || nb_step) ? c->ao_sync : mb_step ? c->mb_sync : nullptr;
  p.tag_word = try_layer ? c->ao_sync + 1 : nb_step ? c->nb_sync + B : nullptr;
  return p;
}
// A cache with a shared prefix must be well formed and hold a prefix row for each of the call's B rows (decode and extension entries alike)
int check_shared_cache(const pcy_kv_cache* kv, int B, const char* what) {
  if (!kv_shared(kv)) return 0;
  if (!kv->prefix_k || !kv->prefix_v || kv->prefix_T <= 0 || kv->prefix_B <= 0 || kv->rows_per_prefix <= 0 || kv->Tmax <= 0)
    return fail(1, "%s: shared-prefix cache needs prefix_k, prefix_v, prefix_T, prefix_B, rows_per_prefix and a suffix capacity > 0", what);
  if (B < 1 || (B - 1) / kv->rows_per_prefix >= kv->prefix_B)
    return fail(1, "%s: %d rows of %d per prefix need more than the %d prefix rows of the cache", what, B, kv->rows_per_prefix, kv->prefix_B);
  return 0;
}
// ... and must take the batched loop: anything else is the caller's error, not a fallback.
int check_decode_cache(const pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, int B, const PcySwitches& sw, const char* what) {
  if (!kv_shared(kv)) return 0;
  if (int r = check_shared_cache(kv, B, what)) return r;
  if (plan_decode(c, m, kv, B, sw).path == DEC_LOOP_MFMA) return 0;
  if (B < pcy_mfma_min_batch())
    return fail(1, "%s: a shared-prefix cache is served by the batched decode loop only (>= %d rows), not %d row%s", what, pcy_mfma_min_batch(), B, B == 1 ? "" : "s");
  return fail(1, "%s: a shared-prefix cache is served by the batched decode loop only, which does not cover this geometry (d %% 128, ffn %% 128)", what);
}

// measurement aid (PCY_MC_TRACE, tools/bench_decode*.py): in-kernel time stamps, [layer][workgroup][16] behind a first half of the same size
unsigned long long* mc_trace(const PcySwitches& sw, int l = 0) {
  if (!sw.mc_trace) return nullptr;
  if (!g_mc_trace) { hipMalloc(&g_mc_trace, 2 * 128 * 256 * 16 * 8); hipMemset(g_mc_trace, 0, 2 * 128 * 256 * 16 * 8); }
  return g_mc_trace + (size_t)(128 + l) * 256 * 16;
}

// The argument structs of the decode launches, each built in ONE place.  l = decoder layer, or -1 for a launch that runs all layers (the
// kernel then applies the per-layer strides and takes the per-layer weights from PcyDecodeStepArgs::layers).
PcyDecAttnArgs attn_args(const DecodeCx& cx, const DecodePlan& p, int l) {
  const pcy_llama_desc* m = cx.m;
  PcyDecAttnArgs t{};
  t.qkv = cx.qkv; t.ld = cx.qkvw; t.kcache = (bf16_t*)cx.kv->k + (l > 0 ? l : 0) * cx.layer_stride; t.vcache = (bf16_t*)cx.kv->v + (l > 0 ? l : 0) * cx.layer_stride;
  t.o = cx.ao; t.ldo = m->n_heads * m->head_dim; t.pos_dev = cx.st->pos; t.cos_t = (const bf16_t*)m->rope_cos; t.sin_t = (const bf16_t*)m->rope_sin;
  t.keep = cx.st->keep; t.ld_keep = kv_cap(cx.kv); t.scratch = cx.scores; t.B = cx.B; t.H = m->n_heads; t.Hkv = m->n_kv_heads; t.dh = m->head_dim; t.Tmax = kv_cap(cx.kv);
  if (kv_shared(cx.kv)) {   // (per-layer strides of BOTH arrays: the suffix above, the prefix here)
    t.prefix_k = (const bf16_t*)cx.kv->prefix_k + (l > 0 ? l : 0) * cx.prefix_layer_stride;
    t.prefix_v = (const bf16_t*)cx.kv->prefix_v + (l > 0 ? l : 0) * cx.prefix_layer_stride;
    t.Tp = cx.kv->prefix_T; t.rows_per_prefix = cx.kv->rows_per_prefix;
  }
  t.scale = 1.0f / sqrtf((float)m->head_dim);
  t.xmin = p.xmin;
  if (l < 0) t.xflags = cx.c->ao_sync + 64 + AO_MAX_LAYERS * AO_FLAGS;   // (per-layer launches get their flags as a launcher argument)
  else t.force_ds = p.force_ds;
  return t;
}
// L / tags: the weights and the hand-over slots of the one layer the launch runs (nullptr for all layers in one launch)
PcyAttnBlockArgs block_args(const DecodeCx& cx, const unsigned* epoch, unsigned long long* trace, const pcy_llama_layer* L = nullptr, uint32_t* tags = nullptr) {
  const pcy_llama_desc* m = cx.m;
  PcyAttnBlockArgs bp{};
  bp.x = cx.x; bp.d = m->d; bp.Nq = cx.qkvw; bp.rms_eps = m->rms_eps; bp.rms_cast = m->rms_cast; bp.epoch = epoch; bp.err = cx.c->xwg_err; bp.trace = trace;
  if (L) {
    bp.ln1 = (const bf16_t*)L->ln1; bp.wqkv = (const bf16_t*)L->wqkv; bp.wo = (const bf16_t*)L->wo;
    bp.qkv_tag = tags + m->ffn; bp.ao_tag = bp.qkv_tag + cx.qkvw; bp.xo_tag = bp.ao_tag + m->n_heads * m->head_dim;
  }
  return bp;
}
PcyMlpChainArgs mlp_args(const DecodeCx& cx, const unsigned* epoch, const pcy_llama_layer* L = nullptr, uint32_t* tags = nullptr) {
  const pcy_llama_desc* m = cx.m;
  PcyMlpChainArgs mc{};
  mc.x = cx.x; mc.x_out = cx.x; mc.d = m->d; mc.F = m->ffn; mc.rms_eps = m->rms_eps; mc.rms_cast = m->rms_cast; mc.epoch = epoch; mc.err = cx.c->xwg_err;
  if (L) { mc.ln2 = (const bf16_t*)L->ln2; mc.wgu = (const bf16_t*)L->wgu; mc.wdown = (const bf16_t*)L->wdown; mc.act_tag = tags; }
  return mc;
}
// tags: [n_layers][tag_stride] hand-over slots, then [n_layers][line_stride] words of the residual stream between the layers
PcyDecodeStepArgs step_args(const DecodeCx& cx, uint32_t* tags, size_t tag_stride, size_t xflags_stride, size_t line_stride) {
  PcyDecodeStepArgs sa{};
  sa.layers = cx.c->dev_layers; sa.n_layers = cx.m->n_layers; sa.kv_layer_stride = cx.layer_stride;
  sa.tags = tags; sa.tag_stride = tag_stride; sa.xflags_stride = xflags_stride;
  sa.x_lines = tags + (size_t)cx.m->n_layers * tag_stride; sa.x_lines_stride = line_stride;
  return sa;
}
// WHAT the four projections of decoder layer l are, in ONE place: out[B][N] = epi(in[B][K] . W^T).  STORE / SWIGLU read the residual stream
// through RMSNorm * ln; RESID adds onto the residual stream, and next_ln is the norm in front of the projection that reads it next (behind
// the last layer's down projection: the final norm).  HOW a shape becomes a launch is the back-end's business (launch_proj).
enum ProjSlot { PROJ_QKV, PROJ_O, PROJ_GATE_UP, PROJ_DOWN };
struct ProjShape {
  ProjSlot slot; int l;          // which matrix of which layer (the e4m3 back-end takes its copy and scales by these)
  const void *W, *ln, *next_ln;  // ... its bf16 weights; the norms (above)
  const bf16_t* in; int K;
  bf16_t* out; int N;            // (SWIGLU: N features out of 2 N interleaved weight rows)
  int epi; bool splitk;          // splitk: may split K over the step's partial-sum workspace
};
ProjShape proj_shape(const DecodeCx& cx, int l, ProjSlot slot) {
  const pcy_llama_desc* m = cx.m;
  const pcy_llama_layer& L = m->layers[l];
  switch (slot) {
    case PROJ_QKV:     return {slot, l, L.wqkv, L.ln1, nullptr, cx.x, m->d, cx.qkv, cx.qkvw, EPI_STORE, true};
    case PROJ_O:       return {slot, l, L.wo, nullptr, L.ln2, cx.ao, m->n_heads * m->head_dim, cx.x, m->d, EPI_RESID, true};
    case PROJ_GATE_UP: return {slot, l, L.wgu, L.ln2, nullptr, cx.x, m->d, cx.act, m->ffn, EPI_SWIGLU, false};
    default:           return {slot, l, L.wdown, nullptr, l + 1 < m->n_layers ? m->layers[l + 1].ln1 : m->final_norm, cx.act, m->ffn, cx.x, m->d, EPI_RESID, true};
  }
}
// The three back-ends.  GEMV (the decode loop, the window pass): pcy_launch_gemv -- the norm fused into the streaming launch, or (p.batched)
// xn, which the loop has filled; RESID, batched up to 32 rows, leaves RMSNorm(x) * next_ln in xn from its K-split finish (*xn_ready = 1 where
// that happened).  GEMM (more than 32 rows): `linear` over all B rows, fed from xn, the next norm fused into the K-split finish.  W8: the
// e4m3 streaming GEMV, the norm always fused.
enum ProjBackend { BACKEND_GEMV, BACKEND_GEMM, BACKEND_W8 };
PcyGemvArgs proj_args(const DecodeCx& cx, const DecodePlan& p, const ProjShape& sh, int* xn_ready) {
  PcyGemvArgs g{};
  g.W = (const bf16_t*)sh.W; g.x = sh.in; g.y = sh.out; g.N = sh.N; g.K = sh.K; g.B = cx.B; g.ldx = sh.K; g.ldy = sh.N; g.epi = sh.epi;
  g.force_stream = p.nb_on; g.krot = sh.slot == PROJ_DOWN ? 0 : p.krot;   // (the rotated K order: the projections over d)
  if (sh.splitk) { g.splitk_ws = cx.sk_ws; g.splitk_ws_bytes = cx.sk_bytes; }
  if (sh.epi == EPI_RESID) {
    g.resid = sh.out;
    if (p.batched && cx.B <= 32) { g.next_rms_w = (const bf16_t*)sh.next_ln; g.next_xn = cx.xn; g.fused_next = xn_ready; g.rms_eps = cx.m->rms_eps; g.rms_cast = cx.m->rms_cast; }
  } else {
    g.rms_eps = cx.m->rms_eps; g.rms_cast = cx.m->rms_cast;
    if (p.batched) g.x = cx.xn; else g.rms_w = (const bf16_t*)sh.ln;
  }
  return g;
}
PcyGemvW8Args w8_args(const DecodeCx& cx, const ProjShape& sh) {
  const pcy_llama_layer_fp8& Q = cx.w8[sh.l];
  const void* const W[4] = {Q.wqkv, Q.wo, Q.wgu, Q.wdown}; const float* const scale[4] = {Q.sqkv, Q.so, Q.sgu, Q.sdown};   // (by ProjSlot)
  PcyGemvW8Args g{};
  g.W = (const uint8_t*)W[sh.slot]; g.scale = scale[sh.slot]; g.x = sh.in; g.y = sh.out; g.N = sh.N; g.K = sh.K; g.B = cx.B; g.ldx = sh.K; g.ldy = sh.N; g.epi = sh.epi;
  if (sh.epi == EPI_RESID) g.resid = sh.out;
  else { g.rms_w = (const bf16_t*)sh.ln; g.rms_eps = cx.m->rms_eps; g.rms_cast = cx.m->rms_cast; }
  return g;
}
// defer_splits (GEMV, the loop's qkv): the attention adds up the K-split partial sums, *defer_splits of them, instead of a finish launch
void launch_proj(const DecodeCx& cx, const DecodePlan& p, ProjBackend backend, const ProjShape& sh, int* xn_ready, int* defer_splits = nullptr) {
  hipStream_t s = cx.c->stream;
  switch (backend) {
    case BACKEND_GEMV: {
      PcyGemvArgs g = proj_args(cx, p, sh, xn_ready);
      g.defer_finish = defer_splits;
      // (the four-way K split of the small-batch step's down projection)
      if (!(sh.slot == PROJ_DOWN && p.nb_on && pcy_launch_gemv_kwin4(s, g))) pcy_launch_gemv(s, g);
      return;
    }
    case BACKEND_GEMM: {
      float* sk = sh.splitk ? cx.sk_ws : nullptr;
      if (sh.epi == EPI_RESID)   // (1: K splits that fill the chip at one or two row tiles)
        linear(s, sh.in, sh.K, (const bf16_t*)sh.W, nullptr, sh.out, sh.N, sh.out, sh.N, cx.B, sh.N, sh.K, sh.epi, sk, sk ? cx.sk_bytes : 0,
               (const bf16_t*)sh.next_ln, cx.xn, xn_ready, cx.m->rms_eps, cx.m->rms_cast, 1);
      else
        linear(s, cx.xn, sh.K, (const bf16_t*)sh.W, nullptr, nullptr, 0, sh.out, sh.N, cx.B, sh.epi == EPI_SWIGLU ? 2 * sh.N : sh.N, sh.K, sh.epi, sk, sk ? cx.sk_bytes : 0);
      return;
    }
    case BACKEND_W8:
      pcy_launch_gemv_w8(s, w8_args(cx, sh));
      return;
  }
}

// One call of an attention that has a workspace of its own -- split-key (pcy_attn_split.hip, DESIGN.md 4.3f: partial sums and statistics),
// many-queries (pcy_attn_mq.hip, 4.3d: score rows and partial sums), both on a complete shared-prefix cache, and window (pcy_attn_win.hip,
// 4.9a: roped queries, chunk statistics and partial sums; B = the W tokens of ONE row of a plain cache, no keep mask) -- on layer `layer`:
// what the operator entries and the steps that use them pass alike.  ws: attn_ws_bytes.
enum AttnKind { ATTN_DECODE, ATTN_SPLIT, ATTN_MQ, ATTN_WINDOW };   // (ATTN_DECODE: the decode attention, on the step's carve -- the loop's own)
struct AttnCall {
  const bf16_t* qkv; int ld; const pcy_kv_cache* kv; int layer; bf16_t* o; int ldo; const int32_t* pos; const bf16_t *cos_t, *sin_t; const uint8_t* keep;
  int B, H, Hkv, dh; char* ws;
};
size_t attn_ws_bytes(AttnKind kind, const pcy_kv_cache* kv, int B, int H, int Hkv, int dh) {
  switch (kind) {
    case ATTN_WINDOW: { const PcyWinPlan p = pcy_attn_win_plan(B, H, Hkv, dh, kv->Tmax); return align_up(p.qr_bytes, 256) + align_up(p.stats_bytes, 256) + align_up(p.part_bytes, 256) + 256; }
    case ATTN_MQ:     { const PcyMqPlan p = pcy_attn_mq_plan(B, kv->rows_per_prefix, H, Hkv, dh, kv->prefix_T); return align_up(p.sc_bytes, 256) + align_up(p.part_bytes, 256) + 256; }
    case ATTN_SPLIT:  { const PcySplitPlan p = pcy_attn_split_plan(B, kv->rows_per_prefix, H, Hkv, dh, kv->prefix_T); return align_up(p.part_bytes, 256) + align_up(p.stat_bytes, 256) + 256; }
    default:          return 0;   // (ATTN_DECODE: nothing beyond the step's carve)
  }
}
// The workspace of a step on B rows of a cache: [decode carve][K/V reorder scratch of a beam search][buffers of the split-key attention].
// The scratch copy of the two-launch reorder (enqueue_kv_reorder; pcy_kv_reorder_range, the beam chains) is sized for the cache's capacity,
// not for the slots in use: a workspace that grew step by step would be re-allocated, and the captured step dropped, several times per search.
size_t step_ws_bytes(const pcy_llama_desc* m, const pcy_kv_cache* kv, int B) { return decode_ws_bytes(m, B, kv_cap(kv)); }
size_t reorder_scratch_bytes(const pcy_llama_desc* m, const pcy_kv_cache* kv, int B) {
  return align_up((size_t)2 * m->n_layers * B * m->n_kv_heads * kv->Tmax * m->head_dim * 2, 256) + 4096;
}
bf16_t* reorder_scratch(const pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, int B) {
  return reinterpret_cast<bf16_t*>(c->ws + align_up(step_ws_bytes(m, kv, B), 256));
}
size_t reorder_ws_bytes(const pcy_llama_desc* m, const pcy_kv_cache* kv, int B) {   // the carve and the scratch
  return align_up(step_ws_bytes(m, kv, B), 256) + reorder_scratch_bytes(m, kv, B);
}
// Where a STEP keeps the split-key buffers: behind BOTH, so that the eager step, the replayed chain and the GEMM step agree on one offset and a
// reorder between two steps never meets them.
size_t split_ws_offset(const pcy_llama_desc* m, const pcy_kv_cache* kv, int B) { return reorder_ws_bytes(m, kv, B); }
size_t split_step_ws_bytes(const pcy_llama_desc* m, const pcy_kv_cache* kv, int B) {
  return split_ws_offset(m, kv, B) + attn_ws_bytes(ATTN_SPLIT, kv, B, m->n_heads, m->n_kv_heads, m->head_dim);
}
// the views of a layer of a complete shared-prefix cache, which the two attentions over it name alike
template <typename Args>
Args prefix_attn_args(const AttnCall& c) {
  const pcy_kv_cache* kv = c.kv;
  const size_t layer_stride = (size_t)kv->B * c.Hkv * kv->Tmax * c.dh, prefix_layer_stride = (size_t)kv->prefix_B * c.Hkv * kv->prefix_T * c.dh;
  Args a{};
  a.qkv = c.qkv; a.ld = c.ld; a.k_own = (bf16_t*)kv->k + c.layer * layer_stride; a.v_own = (bf16_t*)kv->v + c.layer * layer_stride;
  a.k_pre = (const bf16_t*)kv->prefix_k + c.layer * prefix_layer_stride; a.v_pre = (const bf16_t*)kv->prefix_v + c.layer * prefix_layer_stride;
  a.Town = kv->Tmax; a.Tp = kv->prefix_T; a.rows_per_prefix = kv->rows_per_prefix; a.o = c.o; a.ldo = c.ldo; a.pos_dev = c.pos; a.cos_t = c.cos_t; a.sin_t = c.sin_t;
  a.keep = c.keep; a.ld_keep = kv_cap(kv); a.B = c.B; a.H = c.H; a.Hkv = c.Hkv; a.dh = c.dh; a.scale = 1.0f / sqrtf((float)c.dh);
  return a;
}
bool launch_attn(hipStream_t s, AttnKind kind, const AttnCall& c) {   // false = shape not covered, nothing launched
  const pcy_kv_cache* kv = c.kv;
  Carver cv(c.ws);
  switch (kind) {
    case ATTN_SPLIT: {
      const PcySplitPlan p = pcy_attn_split_plan(c.B, kv->rows_per_prefix, c.H, c.Hkv, c.dh, kv->prefix_T);
      PcySplitAttnArgs a = prefix_attn_args<PcySplitAttnArgs>(c);
      a.part = cv.take<float>(p.part_bytes / sizeof(float)); a.stat = cv.take<float2>(p.stat_bytes / sizeof(float2));
      a.ntiles = p.ntiles; a.nchunk = p.nchunk; a.cblocks = p.cblocks;
      return pcy_launch_attn_split(s, a);
    }
    case ATTN_MQ: {
      const PcyMqPlan p = pcy_attn_mq_plan(c.B, kv->rows_per_prefix, c.H, c.Hkv, c.dh, kv->prefix_T);
      PcyMqAttnArgs a = prefix_attn_args<PcyMqAttnArgs>(c);
      a.sc = cv.take<bf16_t>(p.sc_bytes / sizeof(bf16_t)); a.part = cv.take<float>(p.part_bytes / sizeof(float));
      a.ntiles = p.ntiles; a.nchunk = p.nchunk; a.cblocks = p.cblocks; a.lds = p.lds;
      return pcy_launch_attn_mq(s, a);
    }
    case ATTN_WINDOW: {
      const PcyWinPlan p = pcy_attn_win_plan(c.B, c.H, c.Hkv, c.dh, kv->Tmax);
      const size_t layer_stride = (size_t)kv->B * c.Hkv * kv->Tmax * c.dh;
      PcyWinAttnArgs a{};
      a.qkv = c.qkv; a.ld = c.ld; a.kcache = (bf16_t*)kv->k + c.layer * layer_stride; a.vcache = (bf16_t*)kv->v + c.layer * layer_stride;
      a.o = c.o; a.ldo = c.ldo; a.pos_dev = c.pos; a.cos_t = c.cos_t; a.sin_t = c.sin_t; a.W = c.B; a.H = c.H; a.Hkv = c.Hkv; a.dh = c.dh; a.Tmax = kv->Tmax;
      a.scale = 1.0f / sqrtf((float)c.dh);
      a.qr = cv.take<bf16_t>(p.qr_bytes / sizeof(bf16_t)); a.stats = cv.take<float2>(p.stats_bytes / sizeof(float2)); a.part = cv.take<float>(p.part_bytes / sizeof(float));
      a.nchunk = p.nchunk;
      return pcy_launch_attn_window(s, a);
    }
    default: return false;
  }
}

// *xn_ready: xn = RMSNorm(x) * (the norm of the NEXT projection) already stands in xn, written by a K-split finish (or by a fused step)
void norm_if_needed(const DecodeCx& cx, bool feeds_xn, const void* ln, int* xn_ready) {
  if (feeds_xn && !*xn_ready) pcy_launch_rmsnorm(cx.c->stream, cx.x, (const bf16_t*)ln, cx.xn, cx.B, cx.m->d, cx.m->rms_eps, cx.m->rms_cast);
  *xn_ready = 0;
}
// THE layer loop of every launch-per-stage bf16 step, layers [l0, n_layers): norm if needed -> qkv -> attention -> o -> norm if needed ->
// gate / up -> down.  The caller picks the projection back-end (BACKEND_W8: on cx.w8) and the attention (attn_ws: the workspace of a kind
// other than ATTN_DECODE); the plan says what else happens -- attn_o (the decode attention and o in one launch where the launcher takes it),
// defer_qkv_finish, krot, nb_on, batched, force_ds: all off in a zeroed plan.  *xn_ready: as above, on entry and on return.
void enqueue_layers(const DecodeCx& cx, const DecodePlan& p, ProjBackend backend, AttnKind attn, char* attn_ws, int l0, int* xn_ready) {
  pcy_ctx* c = cx.c;
  const pcy_llama_desc* m = cx.m;
  const bool feeds_xn = backend == BACKEND_GEMM || (backend == BACKEND_GEMV && p.batched);   // the projections over x read xn, not a fused norm
  for (int l = l0; l < m->n_layers; ++l) {
    const ProjShape qkv = proj_shape(cx, l, PROJ_QKV), o = proj_shape(cx, l, PROJ_O), gu = proj_shape(cx, l, PROJ_GATE_UP), down = proj_shape(cx, l, PROJ_DOWN);
    norm_if_needed(cx, feeds_xn, qkv.ln, xn_ready);
    int qkv_splits = 0;
    launch_proj(cx, p, backend, qkv, nullptr, p.defer_qkv_finish ? &qkv_splits : nullptr);
    bool o_done = false;
    if (attn == ATTN_DECODE) {
      PcyDecAttnArgs t = attn_args(cx, p, l);
      if (qkv_splits > 1) { t.qkv_partials = cx.sk_ws; t.qkv_splits = qkv_splits; }
      o_done = p.attn_o && pcy_launch_attn_o(c->stream, t, proj_args(cx, p, o, xn_ready), c->n_cu, c->ao_sync, c->ao_sync + 64 + l * AO_FLAGS, AO_FLAGS, c->xwg_err,
                                                     c->ao_sync + 64 + (AO_MAX_LAYERS + l) * AO_FLAGS);   // (the last: key-split flags of this layer's launch)
      if (!o_done) { t.xmin = 0; pcy_launch_attn_decode(c->stream, t); }   // (no key split in the stand-alone attention)
    } else {
      launch_attn(c->stream, attn, AttnCall{cx.qkv, cx.qkvw, cx.kv, l, cx.ao, m->n_heads * m->head_dim, cx.st->pos, (const bf16_t*)m->rope_cos, (const bf16_t*)m->rope_sin, cx.st->keep,
                                            cx.B, m->n_heads, m->n_kv_heads, m->head_dim, attn_ws});
    }
    if (!o_done) launch_proj(cx, p, backend, o, xn_ready);
    norm_if_needed(cx, feeds_xn, gu.ln, xn_ready);
    launch_proj(cx, p, backend, gu, nullptr);
    launch_proj(cx, p, backend, down, xn_ready);
  }
}
// THE lm_head tail of the GEMV steps, on cx.B rows: the streaming GEMV with the final norm fused, or norm + MFMA GEMV from xn (p.batched_head).
// force_stream (and the small-batch arithmetic, p.nb_on): the fused norm on the streaming kernel whatever B -- rows in groups of <= 4, a
// row's bits do not depend on the batch (the e4m3 step; the fused norm selects that kernel anyway).
// (4 rows on the small-batch step: the streaming kernel -- one pass over the matrix for up to 4 rows -- instead of norm + MFMA GEMV: 3.178 ->
// 3.153 ms per step; 5 and 8 rows would take two passes: 3.51 -> 3.65, 4.00 -> 4.15)
void enqueue_lm_head(const DecodeCx& cx, const DecodePlan& p, void* logits_out, int xn_ready, bool force_stream = false) {
  const pcy_llama_desc* m = cx.m;
  PcyGemvArgs h{};
  h.W = (const bf16_t*)m->lm_head; h.x = cx.x; h.y = (bf16_t*)logits_out; h.rms_w = (const bf16_t*)m->final_norm; h.rms_eps = m->rms_eps;
  h.rms_cast = m->rms_cast; h.N = m->vocab; h.K = m->d; h.B = cx.B; h.ldx = m->d; h.ldy = m->vocab; h.epi = EPI_STORE;
  if (p.batched_head && !(p.nb_on && cx.B <= 4)) {
    norm_if_needed(cx, true, m->final_norm, &xn_ready);
    h.x = cx.xn; h.rms_w = nullptr;
  } else {
    h.force_stream = p.nb_on || force_stream;
  }
  pcy_launch_gemv(cx.c->stream, h);
}

// layers_only (measurement, pcy_llama_decode_layers): the decoder layers without the token embedding (the residual stream is whatever
// the workspace holds) and without lm_head; the hand-over counters are advanced by one-thread launches instead.
// split (the batched loop on a shared-prefix cache only -- the callers have checked both): every layer's attention is the split-key one, its
// buffers at split_ws_offset; it reads FINISHED qkv, so the projection runs its own K-split finish, and the o projection is a launch of its own.
void enqueue_decode(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, const PcySwitches& sw, bool layers_only = false,
                    bool split = false) {
  hipStream_t s = c->stream;
  const int d = m->d, dh = m->head_dim;
  const DecodeCx cx = decode_cx(c, m, kv, st, B);
  DecodePlan p = plan_decode(c, m, kv, B, sw);
  if (split) { p.defer_qkv_finish = false; p.attn_o = false; }
  if (layers_only) {
    if (p.epoch_word) pcy_launch_bump(s, p.epoch_word);
    if (p.tag_word) pcy_launch_bump(s, p.tag_word);
  } else {
    pcy_launch_embed_tokens_dev(s, (const bf16_t*)m->embed, st->next_tok, cx.x, B, d, p.epoch_word, p.tag_word);
  }
  const size_t tag_stride = tag_words_per_layer(m);
  bool step_done = false;
  const bool try_layer = p.path == DEC_STEP_GQA || p.path == DEC_STEP_MHA || p.path == DEC_LAYERS;   // one launch per decoder layer (behind a step that declines, too)
  int xn_ready = 0;   // batched path: xn = RMSNorm(x) of the NEXT projection already produced by a fused finish kernel
  if (p.path == DEC_STEP_NB) {   // 2..8 rows, all layers in one launch
    const PcyDecodeStepArgs sa = step_args(cx, c->nb_tags[B], pcy_decode_nb_tag_words(B), 2 * AO_FLAGS, pcy_decode_nb_line_words(B));   // up to 128 attention units per layer
    step_done = pcy_launch_decode_step_nb(s, c->device, attn_args(cx, p, -1), block_args(cx, p.tag_word, mc_trace(sw)), mlp_args(cx, p.tag_word), sa, c->n_cu,
                                          c->ao_sync, B, sw.nb_ub);
    if (step_done) ++g_pcy_dispatch[PCY_DISPATCH_DEC_STEP_NB];
  } else if (p.path == DEC_STEP_GQA || p.path == DEC_STEP_MHA) {   // one row, all layers in one launch
    const PcyDecodeStepArgs sa = step_args(cx, c->mc_tags, tag_stride, AO_FLAGS, 32 * 256);
    step_done = pcy_launch_decode_step(s, attn_args(cx, p, -1), block_args(cx, p.tag_word, mc_trace(sw)), mlp_args(cx, p.tag_word), sa, c->n_cu,
                                       c->ao_sync);   // (counts its own kind: grouped-query or multi-head)
  } else if (p.path == DEC_STEP_MB) {   // 9..32 rows: the batched path's work items as phases of one launch
    PcyMbArgs ma{};
    ma.layers = c->dev_layers; ma.n_layers = m->n_layers; ma.final_norm = (const bf16_t*)m->final_norm;
    ma.x = cx.x; ma.xn = cx.xn; ma.ao = cx.ao; ma.act = cx.act;
    ma.qkv_ws = cx.sk_ws; ma.sk_ws = cx.sk_ws + (size_t)2 * B * cx.qkvw;
    ma.kcache = (bf16_t*)kv->k; ma.vcache = (bf16_t*)kv->v; ma.kv_layer_stride = cx.layer_stride; ma.Bcache = kv->B;
    ma.pos_dev = st->pos; ma.cos_t = (const bf16_t*)m->rope_cos; ma.sin_t = (const bf16_t*)m->rope_sin; ma.keep = st->keep; ma.ld_keep = kv->Tmax;
    ma.B = B; ma.Tmax = kv->Tmax; ma.scale = 1.0f / sqrtf((float)dh); ma.rms_eps = m->rms_eps; ma.rms_cast = m->rms_cast;
    ma.flags = c->mb_flags; ma.epoch = c->mb_sync; ma.err = c->xwg_err; ma.abl = sw.mb_abl; ma.trace = mc_trace(sw);
    pcy_launch_rmsnorm(s, cx.x, (const bf16_t*)m->layers[0].ln1, cx.xn, B, d, m->rms_eps, m->rms_cast);
    if (pcy_launch_decode_step_mb(s, c->device, ma, c->n_cu)) { step_done = true; xn_ready = 1; ++g_pcy_dispatch[PCY_DISPATCH_DEC_STEP_MB]; }
  }
  int l = step_done ? m->n_layers : 0;
  for (; try_layer && l < m->n_layers; ++l) {   // the whole layer as one launch (a geometry it does not cover: the same for every layer)
    const pcy_llama_layer& L = m->layers[l];
    uint32_t* tags = c->mc_tags + (size_t)l * tag_stride;
    if (!pcy_launch_decode_layer(s, attn_args(cx, p, l), block_args(cx, p.tag_word, mc_trace(sw, l), &L, tags), mlp_args(cx, p.tag_word, &L, tags), c->n_cu,
                                 c->ao_sync, c->ao_sync + 64 + (AO_MAX_LAYERS + l) * AO_FLAGS))   // (the last: key-split flags of this layer's launch)
      break;
    if (l == 0) ++g_pcy_dispatch[PCY_DISPATCH_DEC_LAYER];   // (one count per step)
  }
  if (l == 0 && m->n_layers > 0) {
    ++g_pcy_dispatch[p.batched ? PCY_DISPATCH_DEC_LOOP_MFMA : PCY_DISPATCH_DEC_LOOP_STREAM];
    if (kv_shared(kv)) ++g_pcy_dispatch[PCY_DISPATCH_SHARED_PREFIX];
  }
  enqueue_layers(cx, p, BACKEND_GEMV, split ? ATTN_SPLIT : ATTN_DECODE, split ? c->ws + split_ws_offset(m, kv, B) : nullptr, l, &xn_ready);
  if (layers_only) return;
  if (split) ++g_pcy_attn_split;
  enqueue_lm_head(cx, p, st->logits, xn_ready);
}

// Record of the per-step logits (the reference returns it on the CPU, model_unified.py:892,917-921).  `all` may be PINNED
// HOST memory: the rows then cross PCIe while the next decode step runs, instead of as one 65 MB (batch 1, 256 tokens) to
// 4.2 GB (batch 32, 512 tokens) device-to-host copy after the loop -- batch-32 generation 8.3 -> see DESIGN.md ms per token end to end.
// Row (step, b) starts at all + (step*B + b)*ld; with ld % 8 == 0 every row is 16-byte aligned and is written with 16-byte
// stores (the source rows have the odd stride V, so they are gathered with 2-byte loads from L2).
__global__ void store_logits_kernel(const bf16_t* __restrict__ logits, bf16_t* __restrict__ all, const int32_t* step_dev,
                                    int B, int V, int ld, const int32_t* __restrict__ done) {
  if (done && *done) return;   // EOS stop: a launch behind *done changes nothing (the word is written by the pick behind this launch only)
  const size_t step = (size_t)(*step_dev);
  const int chunks = (V + 7) / 8;
  const bool vec = (ld % 8 == 0) && ((reinterpret_cast<uintptr_t>(all) & 15) == 0);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < (size_t)B * chunks; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / chunks), c = (int)(i % chunks);
    const bf16_t* src = logits + (size_t)b * V + c * 8;
    bf16_t* dst = all + (step * B + b) * ld + c * 8;
    if (vec && c * 8 + 8 <= V) {
      const uint32_t w0 = src[0] | ((uint32_t)src[1] << 16), w1 = src[2] | ((uint32_t)src[3] << 16);
      const uint32_t w2 = src[4] | ((uint32_t)src[5] << 16), w3 = src[6] | ((uint32_t)src[7] << 16);
      *reinterpret_cast<uint4*>(dst) = make_uint4(w0, w1, w2, w3);
    } else {
      for (int e = 0; e < 8 && c * 8 + e < V; ++e) dst[e] = src[e];
    }
  }
}
// the step's logits -> row (step, b) of `all` (nullptr: no record; ld <= 0: rows of V)
// (done: the word of an EOS stop, nullptr without one)
void enqueue_store_logits(hipStream_t s, const void* logits, void* all, int ld, const int32_t* step_dev, int B, int V, const int32_t* done = nullptr) {
  if (all) hipLaunchKernelGGL(store_logits_kernel, dim3(B >= 8 ? 256 : 64), dim3(256), 0, s, (const bf16_t*)logits, (bf16_t*)all, step_dev, B, V, ld > 0 ? ld : V, done);
}
// the EOS stop of a state as the pick launchers take it (pcy.h; without `finished` the other three fields are not read: all zero)
PcyStop stop_of(const pcy_gen_state* st) {
  return st->finished ? PcyStop{st->finished, st->done, st->n_steps_run, st->eos_id} : PcyStop{};
}
// ... and what every entry with a pick refuses about it, before anything is launched
int check_stop(const pcy_gen_state* st, int vocab, const char* what) {
  if (!st || !st->finished) return 0;
  if (!st->done) return fail(1, "%s: an EOS stop (finished != NULL) needs the done word", what);
  if (st->eos_id < 0 || st->eos_id >= vocab) return fail(1, "%s: eos_id %d outside [0, vocab %d)", what, st->eos_id, vocab);
  return 0;
}
void enqueue_pick(pcy_ctx* c, const pcy_llama_desc* m, const pcy_gen_state* st, int B, int advance_pos, int Tmax) {
  const PcyStop stop = stop_of(st);
  enqueue_store_logits(c->stream, st->logits, st->logits_all, st->logits_all_ld, st->step, B, m->vocab, stop.done);
  pcy_launch_greedy_pick(c->stream, (const bf16_t*)st->logits, B, m->vocab, st->next_tok, st->tokens_out, st->max_steps,
                         st->logprob, st->pos, st->step, advance_pos, carve_decode_ws(c->ws, m, B, Tmax).partials, stop);
}

// sampling / nucleus selection on state->logits (the non-greedy branch of `_generate_sampling`, model_unified.py:896-906)
void enqueue_sample(pcy_ctx* c, const pcy_llama_desc* m, const pcy_gen_state* st, int B, int advance_pos, int Tmax, float temperature,
                    float nucleus_p, const float* uniforms, bf16_t* probs_out) {
  hipStream_t s = c->stream;
  // the nucleus branch of the reference is softmax(logits) * mask -- the temperature is not applied there (model_unified.py:899-901)
  if (nucleus_p > 0.f) temperature = 1.0f;
  const PcyStop stop = stop_of(st);
  enqueue_store_logits(s, st->logits, st->logits_all, st->logits_all_ld, st->step, B, m->vocab, stop.done);
  void* partials = carve_decode_ws(c->ws, m, B, Tmax).partials;
  pcy_launch_sample_step(s, (const bf16_t*)st->logits, B, m->vocab, temperature, nucleus_p, uniforms, c->smp_hist, probs_out, st->next_tok,
                         st->tokens_out, st->max_steps, st->logprob, st->pos, st->step, advance_pos, partials, c->smp_pbits, stop);
}
int ensure_sample_state(pcy_ctx* c, int B, int V) {
  if ((size_t)B * V > c->smp_pbits_elems) {
    if (c->smp_pbits) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->smp_pbits)); c->smp_pbits = nullptr; c->smp_pbits_elems = 0; }
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->smp_pbits), (size_t)B * V * 2));
    c->smp_pbits_elems = (size_t)B * V;
  }
  if (B <= c->smp_hist_rows) return 0;
  if (c->smp_hist) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->smp_hist)); c->smp_hist = nullptr; }
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->smp_hist), (size_t)B * 65536 * sizeof(unsigned)));
  HIP_TRY(hipMemset(c->smp_hist, 0, (size_t)B * 65536 * sizeof(unsigned)));
  c->smp_hist_rows = B;
  return 0;
}

// Beam-search cache reorder, cache[:, b] = cache[:, rows[b]] over slots [0, t), for EVERY layer and for K and V in two
// launches (gather into a scratch copy, copy back): grid (B, Hkv, 2L).  Rows that keep their place (rows[b] == b: most rows
// once the beams of a group have settled) are skipped in both passes.  The per-layer version took 4 launches per layer
// (128 launches, ~1 ms of a 8.8 ms beam step at beam 10).
// The same reorder in ONE pass and in place for up to 32 rows: a thread owns one 16-byte piece of every row of a (layer, K | V, head) slab --
// it loads the piece of ALL rows (through LDS: the source row of a destination is only known at run time), then stores row b's piece from
// row rows[b]'s.  The rows that are somebody's source are read once and the moved rows written once (the two-launch form reads and writes
// the moved rows twice and needs a scratch copy); nothing is touched when no row moves.  Vanilla beam search (beam_group_size = beam_size, the reference's default)
// re-ranks most rows at every step: 3.87 -> see DESIGN.md ms per beam-5 step at a 570-token cache.
template <int MAXB>
__global__ __launch_bounds__(128) void kv_permute_kernel(bf16_t* __restrict__ kbase, bf16_t* __restrict__ vbase, const int32_t* __restrict__ rows, int B,
                                                         int Bcache, int Hkv, int Tmax, int t, int dh, const int32_t* __restrict__ t_dev, int t0, int t_off) {
  __shared__ uint4 stage[MAXB * 128];
  const int h = blockIdx.x, lw = blockIdx.y, l = lw >> 1;
  unsigned need = 0;                                       // rows some OTHER row takes its contents from (uniform)
  bool moves = false;
  for (int b = 0; b < B; ++b) {
    const int sb = rows[b];
    if (sb != b) { moves = true; if (sb >= 0 && sb < B) need |= 1u << sb; }
  }
  if (!moves) return;                                      // no row moves
  // (t_off: the slots of a shared-prefix cache's suffix panels start at logical slot t_off = prefix_T; 0 for a plain cache)
  if (t_dev) { t = *t_dev - t_off; t = t < Tmax ? t : Tmax; t = t > 0 ? t : 0; }
  bf16_t* cache = ((lw & 1) ? vbase : kbase) + (size_t)l * Bcache * Hkv * Tmax * dh + (size_t)h * Tmax * dh;
  const size_t rstride = (size_t)Hkv * Tmax * dh;          // elements between two rows of the slab
  const size_t n8 = (size_t)t * dh / 8;
  // slots [t0, t) only: the caller knows that the rows hold the same contents below t0 (beam search: the beams of a prompt share its prefix)
  for (size_t i = (size_t)t0 * dh / 8 + (size_t)blockIdx.z * 128 + threadIdx.x; i < n8; i += (size_t)gridDim.z * 128) {
#pragma unroll 4
    for (int b = 0; b < B; ++b)
      if ((need >> b) & 1u) stage[b * 128 + threadIdx.x] = *reinterpret_cast<const uint4*>(cache + (size_t)b * rstride + i * 8);
#pragma unroll 4
    for (int b = 0; b < B; ++b) {
      const int sb = rows[b];
      if (sb == b) continue;
      // (a source beyond the permuted rows -- pcy_kv_reorder accepts any cache row -- is not staged, and is nobody's destination: straight from memory)
      const uint4 v = (sb >= 0 && sb < B) ? stage[sb * 128 + threadIdx.x] : *reinterpret_cast<const uint4*>(cache + (size_t)sb * rstride + i * 8);
      *reinterpret_cast<uint4*>(cache + (size_t)b * rstride + i * 8) = v;
    }
  }
}
// t_dev != nullptr (the replayed beam step): the number of slots is read from the device (the position counter the beam step has just
// advanced) and the scratch rows are Tmax slots apart -- nothing in the launch depends on the step.
__global__ void kv_gather_kernel(bf16_t* __restrict__ kbase, bf16_t* __restrict__ vbase, bf16_t* __restrict__ tmp,
                                 const int32_t* __restrict__ rows, int B, int Bcache, int Hkv, int Tmax, int t, int dh, int to_tmp,
                                 const int32_t* __restrict__ t_dev, int t0, int t_off) {
  const int b = blockIdx.x, h = blockIdx.y, lw = blockIdx.z, l = lw >> 1;
  const int src_b = rows[b];
  if (src_b == b) return;
  int ts = t;                 // slots between two scratch rows
  if (t_dev) { t = *t_dev - t_off; t = t < Tmax ? t : Tmax; t = t > 0 ? t : 0; ts = Tmax; }   // (t_off: see kv_permute_kernel)
  bf16_t* cache = ((lw & 1) ? vbase : kbase) + (size_t)l * Bcache * Hkv * Tmax * dh;
  bf16_t* scratch = tmp + (size_t)lw * B * Hkv * ts * dh;
  const size_t n8 = (size_t)t * dh / 8;
  const uint4* sp; uint4* dp;
  if (to_tmp) {
    sp = reinterpret_cast<const uint4*>(cache + ((size_t)src_b * Hkv + h) * Tmax * dh);
    dp = reinterpret_cast<uint4*>(scratch + ((size_t)b * Hkv + h) * ts * dh);
  } else {
    sp = reinterpret_cast<const uint4*>(scratch + ((size_t)b * Hkv + h) * ts * dh);
    dp = reinterpret_cast<uint4*>(cache + ((size_t)b * Hkv + h) * Tmax * dh);
  }
  for (size_t i = (size_t)t0 * dh / 8 + threadIdx.x; i < n8; i += blockDim.x) dp[i] = sp[i];
}
// The reorder of rows [0, B) over slots [t0, t) -- or [t0, *t_dev - t_off) -- of every layer: the one-pass form for <= 32 rows, else
// (PCY_DISABLE=kv_permute too; same result) the two launches through the scratch copy `tmp` (reorder_scratch)
void enqueue_kv_reorder(hipStream_t s, const pcy_llama_desc* m, const pcy_kv_cache* kv, const int32_t* rows, int B, int t, const int32_t* t_dev, int t0,
                        int t_off, bf16_t* tmp) {
  const int Hkv = m->n_kv_heads, dh = m->head_dim, L = m->n_layers;
  bf16_t *k = (bf16_t*)kv->k, *v = (bf16_t*)kv->v;
  if (B <= 32 && !pcy_off("kv_permute")) {
    const dim3 grid(Hkv, 2 * L, 4);
    if (B <= 8) hipLaunchKernelGGL(kv_permute_kernel<8>, grid, dim3(128), 0, s, k, v, rows, B, kv->B, Hkv, kv->Tmax, t, dh, t_dev, t0, t_off);
    else hipLaunchKernelGGL(kv_permute_kernel<32>, grid, dim3(128), 0, s, k, v, rows, B, kv->B, Hkv, kv->Tmax, t, dh, t_dev, t0, t_off);
    return;
  }
  for (int to_tmp = 1; to_tmp >= 0; --to_tmp)   // gather into the scratch copy, copy back
    hipLaunchKernelGGL(kv_gather_kernel, dim3(B, Hkv, 2 * L), dim3(256), 0, s, k, v, tmp, rows, B, kv->B, Hkv, kv->Tmax, t, dh, to_tmp, t_dev, t0, t_off);
}

}  // namespace

// Operand contract of pcy_gemm / pcy_gemm_fp8 (include/pcy.h), checked before any launch.  row_align = elements per 16 bytes of A and W (8 bf16,
// 16 e4m3): every kernel stages their rows as 16-byte LDS-DMA pieces.  C / resid / bias go through epilogues that test strides and bases
// themselves and fall back to single elements -- except the SwiGLU epilogue of the natural row order, which always stores 8 bytes.
static int check_gemm_operands(const char* who, const void* A, int lda, int row_align, const void* W, const void* bias, const void* resid, int ldr,
                        void* C, int ldc, int M, int N, int K, int epi, int epi_max) {
  if (epi < EPI_STORE || epi > epi_max) return fail(1, "%s: epilogue %d unknown", who, epi);
  if (M < 0 || N < 0) return fail(1, "%s: M=%d N=%d", who, M, N);
  if (M == 0 || N == 0) return 0;
  if (!A || !W || !C) return fail(1, "%s: A, W and C are required", who);
  if (lda < K || lda % row_align != 0 || ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W)) & 15))
    return fail(1, "%s: rows of A and W must be 16-byte aligned (lda=%d a multiple of %d), lda >= K=%d", who, lda, row_align, K);
  const int Nout = epi == EPI_SWIGLU ? N / 2 : N;
  if (ldc < Nout || (epi == EPI_RESID && ldr < N)) return fail(1, "%s: ldc=%d / ldr=%d must cover the %d output columns", who, ldc, ldr, Nout);
  if ((reinterpret_cast<uintptr_t>(C) | reinterpret_cast<uintptr_t>(resid) | reinterpret_cast<uintptr_t>(bias)) & 1)
    return fail(1, "%s: C, resid and bias hold bf16 elements (2-byte aligned)", who);
  if (epi == EPI_RESID && resid == C && ldr != ldc) return fail(1, "%s: an in-place residual needs ldr == ldc (%d, %d)", who, ldr, ldc);
  if (epi == EPI_SWIGLU && (ldc % 4 != 0 || (reinterpret_cast<uintptr_t>(C) & 7)))
    return fail(1, "%s: SwiGLU needs ldc %% 4 == 0 (ldc=%d) and an 8-byte aligned C", who, ldc);
  return 0;
}

// ====================================================================================== C ABI
hipStream_t pcy_ctx_stream(pcy_ctx* c) { return c->stream; }
void* pcy_ctx_reserve(pcy_ctx* c, size_t bytes) { return c->reserve(bytes) == 0 ? c->ws : nullptr; }
extern "C" {
int pcy_abi_version(void) { return PCY_ABI_VERSION; }
unsigned long long pcy_debug_dispatch_count(int kind) { return (kind >= 0 && kind < PCY_DISPATCH_N) ? g_pcy_dispatch[kind] : 0; }
unsigned long long pcy_debug_attn_route_count(int which) { return (which >= 0 && which < PCY_ATTN_ROUTE_N) ? g_pcy_attn_route[which] : 0; }
unsigned long long pcy_debug_gemv_route_count(int which) { return (which >= 0 && which < PCY_GEMV_ROUTE_N) ? g_pcy_gemv_route[which] : 0; }
const char* pcy_last_error(void) { return g_err; }

int pcy_ctx_create(int device_id, void* stream, pcy_ctx** out) {
  if (!out) return fail(1, "pcy_ctx_create: out is NULL");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device_id < 0 || device_id >= n) return fail(1, "pcy_ctx_create: device %d of %d", device_id, n);
  HIP_TRY(hipSetDevice(device_id));
  pcy_ctx* c = new pcy_ctx();
  c->device = device_id;
  c->stream = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  HIP_TRY(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
  *out = c;
  return 0;
}
void pcy_ctx_destroy(pcy_ctx* c) {
  if (!c) return;
  hipStreamSynchronize(c->stream);
  c->drop_graph();
  c->drop_gslots();
  if (c->ws) hipFree(c->ws);
  if (c->xwg_err) hipHostFree(c->xwg_err);
  if (c->ao_sync) hipFree(c->ao_sync);
  if (c->mc_tags) hipFree(c->mc_tags);
  if (c->dev_layers) hipFree(c->dev_layers);
  for (auto& t : c->nb_tags) if (t) hipFree(t);
  if (c->nb_sync) hipFree(c->nb_sync);
  if (c->mb_flags) hipFree(c->mb_flags);
  if (c->mb_sync) hipFree(c->mb_sync);
  if (c->op_tags) hipFree(c->op_tags);
  if (c->beam_ws) hipFree(c->beam_ws);
  if (c->smp_hist) hipFree(c->smp_hist);
  if (c->smp_pbits) hipFree(c->smp_pbits);
  if (c->ev0) hipEventDestroy(c->ev0);
  if (c->ev1) hipEventDestroy(c->ev1);
  if (c->cap_stream) hipStreamDestroy(c->cap_stream);
  delete c;
}
int pcy_ctx_sync(pcy_ctx* c) {
  HIP_TRY(hipStreamSynchronize(c->stream));
  return take_sticky_error(c);
}
int pcy_timer_start(pcy_ctx* c) { HIP_TRY(hipEventRecord(c->ev0, c->stream)); return 0; }
int pcy_timer_stop(pcy_ctx* c, float* ms) {
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
  return 0;
}

int pcy_gemm(pcy_ctx* c, const void* A, int lda, const void* W, const void* bias, const void* resid, int ldr, void* C,
             int ldc, int M, int N, int K, int epi) {
  if (K <= 0 || K % 64 != 0) return fail(1, "pcy_gemm: K=%d must be a positive multiple of 64", K);
  if (epi == EPI_SWIGLU && N % 32 != 0) return fail(1, "pcy_gemm: SwiGLU needs N %% 32 == 0");
  if (epi == EPI_RESID && !resid) return fail(1, "pcy_gemm: EPI_RESID without residual");
  if (int r = check_gemm_operands("pcy_gemm", A, lda, 8, W, bias, resid, ldr, C, ldc, M, N, K, epi, EPI_SWIGLU)) return r;
  PcyGemmArgs a{};
  a.A = (const bf16_t*)A; a.W = (const bf16_t*)W; a.C = (bf16_t*)C; a.bias = (const bf16_t*)bias; a.resid = (const bf16_t*)resid;
  a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldc = ldc; a.ldr = ldr; a.epi = epi;
  pcy_launch_gemm(c->stream, a);
  return check_launch("pcy_gemm");
}

size_t pcy_lm_head_xent_ws_bytes(int M, int V) { return M > 0 && V > 0 ? pcy_xent_ws_bytes(M, V) : 0; }

int pcy_lm_head_xent(pcy_ctx* c, const void* x, int ldx, const void* W, int M, int V, int d, const int32_t* targets, float* nll_out,
                     float* lse_out, float* row_max_out, float* label_logit_out) {
  if (M < 0 || V <= 0 || d <= 0 || d % 64 != 0) return fail(1, "pcy_lm_head_xent: M=%d V=%d d=%d (d must be a multiple of 64)", M, V, d);
  if (M == 0) return 0;
  if (!x || !W || !targets || !nll_out) return fail(1, "pcy_lm_head_xent: x, W, targets and nll_out are required");
  if (ldx < d || ldx % 8 != 0 || (reinterpret_cast<uintptr_t>(x) & 15) || (reinterpret_cast<uintptr_t>(W) & 15))
    return fail(1, "pcy_lm_head_xent: rows of x and W must be 16-byte aligned (ldx=%d)", ldx);
  if (int r = c->reserve(pcy_xent_ws_bytes(M, V) + 256)) return r;
  PcyXentArgs a{};
  a.x = (const bf16_t*)x; a.ldx = ldx; a.W = (const bf16_t*)W; a.targets = targets; a.M = M; a.V = V; a.d = d;
  a.nll = nll_out; a.lse = lse_out; a.row_max = row_max_out; a.label_logit = label_logit_out; a.ws = c->ws;
  pcy_launch_lm_head_xent(c->stream, a);
  return check_launch("pcy_lm_head_xent");
}

int pcy_gemv(pcy_ctx* c, const void* W, const void* x, int ldx, const void* bias, const void* resid, void* y, int ldy,
             const void* rms_w, float rms_eps, int rms_cast, int N, int K, int B, int epi) {
  if (K <= 0 || K % 8 != 0 || ldx % 8 != 0) return fail(1, "pcy_gemv: K=%d and ldx=%d must be multiples of 8, K > 0", K, ldx);
  if (epi < EPI_STORE || epi > EPI_SWIGLU) return fail(1, "pcy_gemv: epilogue %d unknown", epi);
  if (N < 0 || B < 0) return fail(1, "pcy_gemv: N=%d B=%d", N, B);
  if (N == 0 || B == 0) return 0;
  if (!W || !x || !y) return fail(1, "pcy_gemv: W, x and y are required");
  // every kernel reads W and x (and rms_w) as 16-byte pieces of a row, straight or through LDS-DMA
  if (ldx < K || ((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(rms_w)) & 15))
    return fail(1, "pcy_gemv: rows of W, x and rms_w must be 16-byte aligned, ldx=%d >= K=%d", ldx, K);
  if (ldy < N || ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(resid) | reinterpret_cast<uintptr_t>(bias)) & 1))
    return fail(1, "pcy_gemv: ldy=%d must cover N=%d; y, resid and bias hold bf16 elements (2-byte aligned)", ldy, N);
  if (epi == EPI_RESID && !resid) return fail(1, "pcy_gemv: EPI_RESID without residual");
  // the MFMA kernels store four SwiGLU outputs as one 8-byte piece, with no element-wise form
  if (epi == EPI_SWIGLU && (N % 16 != 0 || ldy % 4 != 0 || (reinterpret_cast<uintptr_t>(y) & 7)))
    return fail(1, "pcy_gemv: SwiGLU needs N %% 16 == 0 (N=%d), ldy %% 4 == 0 (ldy=%d) and an 8-byte aligned y", N, ldy);
  if (rms_w && !(epi == EPI_STORE || epi == EPI_SWIGLU)) return fail(1, "pcy_gemv: fused RMSNorm only with STORE/SWIGLU");
  if (rms_w && (size_t)K * 2 * (B < 4 ? B : 4) > 65536) return fail(1, "pcy_gemv: fused RMSNorm needs x to fit LDS");
  PcyGemvArgs g{};
  g.W = (const bf16_t*)W; g.x = (const bf16_t*)x; g.y = (bf16_t*)y; g.bias = (const bf16_t*)bias; g.resid = (const bf16_t*)resid;
  g.rms_w = (const bf16_t*)rms_w; g.rms_eps = rms_eps; g.rms_cast = rms_cast; g.N = N; g.K = K; g.B = B; g.ldx = ldx; g.ldy = ldy; g.epi = epi;
  pcy_launch_gemv(c->stream, g);
  return check_launch("pcy_gemv");
}

int pcy_decode_mlp(pcy_ctx* c, void* x, const void* ln2, const void* wgu, const void* wdown, int d, int ffn, float rms_eps, int rms_cast) {
  PCY_STICKY(c);
  if (d % 8 || ffn % 8 || (size_t)d * 2 > 65536) return fail(1, "pcy_decode_mlp: d=%d ffn=%d not covered", d, ffn);
  if (int r = ensure_sync_words(c)) return r;
  const size_t words = (size_t)ffn;
  if (c->op_tags_words != words) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->op_tags) HIP_TRY(hipFree(c->op_tags));
    c->op_tags = nullptr; c->op_tags_words = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->op_tags), words * 4));
    HIP_TRY(hipMemset(c->op_tags, 0, words * 4));
    HIP_TRY(hipMemset(c->ao_sync + 2, 0, 4));
    c->op_tags_words = words;
  }
  if (!pcy_off("mlp_chain")) {   // (the two GEMV launches instead of mlp_chain_kernel: read on every call, tests compare -- bit-identical)
    PcyMlpChainArgs mc{};
    mc.x = (const bf16_t*)x; mc.x_out = (bf16_t*)x; mc.ln2 = (const bf16_t*)ln2; mc.wgu = (const bf16_t*)wgu; mc.wdown = (const bf16_t*)wdown;
    mc.d = d; mc.F = ffn; mc.rms_eps = rms_eps; mc.rms_cast = rms_cast;
    mc.act_tag = c->op_tags; mc.epoch = c->ao_sync + 2; mc.err = c->xwg_err;
    pcy_launch_bump(c->stream, c->ao_sync + 2);   // a fresh tag for every use of the slot
    if (pcy_launch_mlp_chain(c->stream, mc, c->n_cu)) return check_launch("pcy_decode_mlp");
  }
  if (int r = c->reserve((size_t)ffn * 2 + 256)) return r;
  PcyGemvArgs u{};
  u.W = (const bf16_t*)wgu; u.x = (const bf16_t*)x; u.y = (bf16_t*)c->ws; u.rms_w = (const bf16_t*)ln2; u.rms_eps = rms_eps; u.rms_cast = rms_cast;
  u.N = ffn; u.K = d; u.B = 1; u.ldx = d; u.ldy = ffn; u.epi = EPI_SWIGLU; u.krot = 1;   // (as mlp_chain_kernel walks it)
  pcy_launch_gemv(c->stream, u);
  PcyGemvArgs w{};
  w.W = (const bf16_t*)wdown; w.x = (const bf16_t*)c->ws; w.y = (bf16_t*)x; w.resid = (const bf16_t*)x; w.N = d; w.K = ffn; w.B = 1; w.ldx = ffn; w.ldy = d;
  w.epi = EPI_RESID;
  pcy_launch_gemv(c->stream, w);
  return check_launch("pcy_decode_mlp");
}

int pcy_rmsnorm(pcy_ctx* c, const void* x, const void* w, void* y, int rows, int d, float eps, int cast) {
  if (d % 8) return fail(1, "pcy_rmsnorm: d %% 8 != 0");
  pcy_launch_rmsnorm(c->stream, (const bf16_t*)x, (const bf16_t*)w, (bf16_t*)y, rows, d, eps, cast);
  return check_launch("pcy_rmsnorm");
}
int pcy_layernorm(pcy_ctx* c, const void* x, const void* w, const void* b, void* y, int rows, int d, float eps) {
  if (d % 8) return fail(1, "pcy_layernorm: d %% 8 != 0");
  pcy_launch_layernorm(c->stream, (const bf16_t*)x, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y, rows, d, eps);
  return check_launch("pcy_layernorm");
}
int pcy_embed_splice(pcy_ctx* c, const void* table, const int32_t* ids, const void* soft, const int32_t* soft_map, void* out,
                     int rows, int d) {
  if (d % 8) return fail(1, "pcy_embed_splice: d %% 8 != 0");
  pcy_launch_embed_gather(c->stream, (const bf16_t*)table, ids, (const bf16_t*)soft, soft_map, (bf16_t*)out, rows, d);
  return check_launch("pcy_embed_splice");
}
int pcy_pool(pcy_ctx* c, const void* hidden, int d, const int32_t* seg, const int32_t* rng, int nprot, int mode, void* out) {
  if (mode < 0 || mode > 2) return fail(1, "pcy_pool: mode %d", mode);
  if (d % 8) return fail(1, "pcy_pool: d=%d must be a multiple of 8", d);
  if (int r = c->reserve(pcy_pool_ws_bytes(nprot, d) + 256)) return r;
  pcy_launch_pool(c->stream, (const bf16_t*)hidden, d, seg, rng, nprot, mode, (bf16_t*)out, c->ws);
  return check_launch("pcy_pool");
}

int pcy_rope(pcy_ctx* c, void* buf, int ld, int col0, int nh, int dh, const int32_t* pos, const void* cos_t, const void* sin_t,
             int ntok, int mode, float prescale) {
  // rope_row moves 8 elements of each half head per 16-byte access: a head_dim that is no multiple of 16 would leave the tail of
  // each half unrotated, a row stride or a first column off the 8-element grid would misalign every access
  if (dh <= 0 || dh % 16) return fail(1, "pcy_rope: head_dim %d must be a positive multiple of 16", dh);
  if (ld % 8 || col0 % 8) return fail(1, "pcy_rope: ld=%d and col0=%d must be multiples of 8", ld, col0);
  if (nh < 0 || col0 < 0 || (long long)col0 + (long long)nh * dh > ld)
    return fail(1, "pcy_rope: heads [%d, %d + %d*%d) do not fit a row of ld=%d", col0, col0, nh, dh, ld);
  pcy_launch_rope(c->stream, (bf16_t*)buf, ld, col0, nh, dh, pos, (const bf16_t*)cos_t, (const bf16_t*)sin_t, ntok, mode, prescale);
  return check_launch("pcy_rope");
}

int pcy_attention(pcy_ctx* c, const void* q, int ldq, int qcol0, const void* k, int ldk, int kcol0, const void* v, int ldv,
                  int vcol0, void* o, int ldo, const int32_t* cu, const int32_t* vt_cu, const uint8_t* keep, int nseq,
                  int max_len, int vt_total, int H, int Hkv, int dh, int causal, float scale) {
  if (int r = check_head_dim("pcy_attention", dh, true)) return r;
  if ((Hkv * dh) % 64 || H % Hkv) return fail(1, "pcy_attention: Hkv*dh must be a multiple of 64 and Hkv | H");
  // the single-pass kernel wants every sequence's Vt slice zero-padded to a multiple of 64 keys: it lays Vt out itself (offsets
  // computed on the device from cu), whatever vt_cu / vt_total the caller passed
  const bool fast = pcy_attn_fast_eligible(dh, causal, keep != nullptr, scale, H, Hkv, ldq, qcol0, ldk, kcol0, ldo);
  int32_t* vt_cu64 = nullptr;
  if (fast) {
    int ntok_ub = 0;   // upper bound of the token count: nseq * max_len
    ntok_ub = nseq * max_len;
    vt_total = (int)align_up((size_t)ntok_ub + 64 * (size_t)nseq, 8);
  }
  if (int r = c->reserve(align_up((size_t)Hkv * dh * vt_total * 2, 256) + align_up((size_t)(nseq + 1) * 4, 256) + 4096)) return r;
  bf16_t* vt = reinterpret_cast<bf16_t*>(c->ws);
  // the single-pass kernel reads V token-major where it is (PCY_DISABLE=fa_vrow: from a transposed copy, as the other kernels do)
  const bool vrow = fast && pcy_attn_fast_vrow(ldv, vcol0);
  if (fast && !vrow) {
    vt_cu64 = reinterpret_cast<int32_t*>(c->ws + align_up((size_t)Hkv * dh * vt_total * 2, 256));
    pcy_launch_vt_offsets(c->stream, cu, nseq, 64, vt_cu64);
    vt_cu = vt_cu64;
  }
  if (!vrow) pcy_launch_transpose_v(c->stream, (const bf16_t*)v, ldv, vcol0, Hkv, dh, cu, vt_cu, nseq, max_len, vt, vt_total);
  PcyAttnArgs t{};
  if (vrow) { t.v = (const bf16_t*)v; t.ldv = ldv; t.vcol0 = vcol0; }
  t.q = (const bf16_t*)q; t.ldq = ldq; t.qcol0 = qcol0; t.k = (const bf16_t*)k; t.ldk = ldk; t.kcol0 = kcol0; t.vt = vt;
  t.vt_total = vt_total; t.o = (bf16_t*)o; t.ldo = ldo; t.cu = cu; t.vt_cu = vt_cu; t.keep = keep; t.nseq = nseq; t.max_len = max_len;
  t.H = H; t.Hkv = Hkv; t.dh = dh; t.causal = causal; t.scale = scale; t.vt_pad64 = fast ? 1 : 0;
  pcy_launch_attn(c->stream, t);
  return check_launch("pcy_attention");
}

int pcy_attn_decode(pcy_ctx* c, void* qkv, int ld, void* kcache, void* vcache, void* o, int ldo, const int32_t* pos,
                    const void* cos_t, const void* sin_t, const uint8_t* keep, int B, int H, int Hkv, int dh, int Tmax) {
  if (int r = check_heads("pcy_attn_decode", H, Hkv, dh, true)) return r;
  PcyDecAttnArgs t{};
  t.qkv = (bf16_t*)qkv; t.ld = ld; t.kcache = (bf16_t*)kcache; t.vcache = (bf16_t*)vcache; t.o = (bf16_t*)o; t.ldo = ldo;
  t.pos_dev = pos; t.cos_t = (const bf16_t*)cos_t; t.sin_t = (const bf16_t*)sin_t; t.keep = keep; t.ld_keep = Tmax;
  t.scratch = nullptr; t.B = B; t.H = H; t.Hkv = Hkv; t.dh = dh; t.Tmax = Tmax; t.scale = 1.0f / sqrtf((float)dh);
  pcy_launch_attn_decode(c->stream, t);
  return check_launch("pcy_attn_decode");
}

int pcy_quant_rows_fp8(pcy_ctx* c, const void* x, int ldx, int rows, int K, void* q_out, float* scale_out) {
  if (rows < 0 || K <= 0 || K % 8 || ldx % 8) return fail(1, "pcy_quant_rows_fp8: K=%d ldx=%d must be multiples of 8", K, ldx);
  pcy_launch_quant_rows_fp8(c->stream, (const bf16_t*)x, ldx, rows, K, (unsigned char*)q_out, scale_out);
  return check_launch("pcy_quant_rows_fp8");
}
int pcy_gemm_fp8(pcy_ctx* c, const void* A8, const float* sa, const void* W8, const float* sw, const void* resid, int ldr,
                 void* C, int ldc, int M, int N, int K, int epi) {
  if (K <= 0 || K % 128) return fail(1, "pcy_gemm_fp8: K=%d must be a multiple of 128", K);
  if (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU) return fail(1, "pcy_gemm_fp8: epilogue %d unsupported", epi);
  if (epi == EPI_SWIGLU && N % 32) return fail(1, "pcy_gemm_fp8: SwiGLU needs N %% 32 == 0");
  if (epi == EPI_RESID && !resid) return fail(1, "pcy_gemm_fp8: EPI_RESID without residual");
  if (int r = check_gemm_operands("pcy_gemm_fp8", A8, K, 16, W8, nullptr, resid, ldr, C, ldc, M, N, K, epi, EPI_SWIGLU)) return r;
  if (M > 0 && N > 0 && (!sa || !sw || ((reinterpret_cast<uintptr_t>(sa) | reinterpret_cast<uintptr_t>(sw)) & 3)))
    return fail(1, "pcy_gemm_fp8: sa and sw are required, 4-byte aligned");
  PcyGemmArgs a{};
  a.A = (const bf16_t*)A8; a.W = (const bf16_t*)W8; a.C = (bf16_t*)C; a.resid = (const bf16_t*)resid;
  a.M = M; a.N = N; a.K = K; a.lda = K; a.ldc = ldc; a.ldr = ldr; a.epi = epi; a.fp8 = 1; a.sa = sa; a.sw = sw;
  pcy_launch_gemm(c->stream, a);
  return check_launch("pcy_gemm_fp8");
}
// ---- RCCL all-gather of the sharded retrieval path (the reference's gather: training/trainIT.py:1594-1610)
// RCCL is resolved at first use with dlopen -- in a PyTorch process that is the copy torch has already loaded (torch/lib/librccl.so),
// so the engine and torch.distributed share one RCCL; libpcy.so itself carries no link-time dependency on it.
struct Id128 { char b[128]; };   // ncclUniqueId (passed by value)
namespace {
struct Rccl {
  void* h = nullptr;
  int (*get_unique_id)(void*) = nullptr;
  int (*comm_init_rank)(void**, int, Id128, int) = nullptr;
  int (*all_gather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
  int (*comm_destroy)(void*) = nullptr;
  const char* (*get_error_string)(int) = nullptr;
};
Rccl* rccl() {
  static Rccl r;
  static bool tried = false;
  if (!tried) {
    tried = true;
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      r.h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.h) break;
    }
    if (r.h) {
      r.get_unique_id = reinterpret_cast<decltype(r.get_unique_id)>(dlsym(r.h, "ncclGetUniqueId"));
      r.comm_init_rank = reinterpret_cast<decltype(r.comm_init_rank)>(dlsym(r.h, "ncclCommInitRank"));
      r.all_gather = reinterpret_cast<decltype(r.all_gather)>(dlsym(r.h, "ncclAllGather"));
      r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(r.h, "ncclCommDestroy"));
      r.get_error_string = reinterpret_cast<decltype(r.get_error_string)>(dlsym(r.h, "ncclGetErrorString"));
    }
  }
  return (r.h && r.get_unique_id && r.comm_init_rank && r.all_gather && r.comm_destroy) ? &r : nullptr;
}
int rccl_fail(const char* what, int rc) {
  Rccl* r = rccl();
  return fail(5, "%s failed: %s", what, (r && r->get_error_string) ? r->get_error_string(rc) : "RCCL error");
}
}  // namespace
int pcy_comm_unique_id(void* id128) {
  Rccl* r = rccl();
  if (!r) return fail(5, "pcy_comm_unique_id: librccl.so not found");
  if (int rc = r->get_unique_id(id128)) return rccl_fail("ncclGetUniqueId", rc);
  return 0;
}
int pcy_comm_init(pcy_ctx* c, int nranks, int rank, const void* id128, void** comm_out) {
  Rccl* r = rccl();
  if (!r) return fail(5, "pcy_comm_init: librccl.so not found");
  HIP_TRY(hipSetDevice(c->device));
  Id128 id;
  memcpy(id.b, id128, sizeof(id.b));
  if (int rc = r->comm_init_rank(comm_out, nranks, id, rank)) return rccl_fail("ncclCommInitRank", rc);
  return 0;
}
void pcy_comm_destroy(void* comm) {
  Rccl* r = rccl();
  if (r && comm) r->comm_destroy(comm);
}
int pcy_allgather(pcy_ctx* c, void* comm, const void* sendbuf, void* recvbuf, size_t bytes) {
  Rccl* r = rccl();
  if (!r) return fail(5, "pcy_allgather: librccl.so not found");
  if (int rc = r->all_gather(sendbuf, recvbuf, bytes, /* ncclUint8 */ 1, comm, c->stream)) return rccl_fail("ncclAllGather", rc);
  return 0;
}

int pcy_retrieval_topk(pcy_ctx* c, const void* query, int Q, const void* targets, int N, int D, int k, int32_t* idx_out, void* score_out) {
  PCY_STICKY(c);
  if (D % 64) return fail(1, "pcy_retrieval_topk: D=%d must be a multiple of 64", D);
  if (k < 1 || k > N) return fail(1, "pcy_retrieval_topk: k=%d must be in [1, N=%d]", k, N);
  const size_t qb = align_up((size_t)Q * D * 2, 256), tb = align_up((size_t)N * D * 2, 256), sb = align_up((size_t)Q * N * 2, 256);
  if (int r = c->reserve(qb + tb + sb + 4096)) return r;
  bf16_t* qn = reinterpret_cast<bf16_t*>(c->ws);
  bf16_t* tn = reinterpret_cast<bf16_t*>(c->ws + qb);
  bf16_t* sims = reinterpret_cast<bf16_t*>(c->ws + qb + tb);
  pcy_launch_l2norm_rows(c->stream, (const bf16_t*)query, qn, Q, D, 1e-12f);
  pcy_launch_l2norm_rows(c->stream, (const bf16_t*)targets, tn, N, D, 1e-12f);
  linear(c->stream, qn, D, tn, nullptr, nullptr, 0, sims, N, Q, N, D, EPI_STORE);
  pcy_launch_retrieval_rank(c->stream, sims, Q, N, k, idx_out, (bf16_t*)score_out);
  return check_launch("pcy_retrieval_topk");
}
int pcy_retrieval_scores(pcy_ctx* c, const void* query, int Q, const void* targets, int N, int D, void* sims_out) {
  PCY_STICKY(c);
  if (D % 64) return fail(1, "pcy_retrieval_scores: D=%d must be a multiple of 64", D);
  const size_t qb = align_up((size_t)Q * D * 2, 256), tb = align_up((size_t)N * D * 2, 256);
  if (int r = c->reserve(qb + tb + 4096)) return r;
  bf16_t* qn = reinterpret_cast<bf16_t*>(c->ws);
  bf16_t* tn = reinterpret_cast<bf16_t*>(c->ws + qb);
  pcy_launch_l2norm_rows(c->stream, (const bf16_t*)query, qn, Q, D, 1e-12f);
  pcy_launch_l2norm_rows(c->stream, (const bf16_t*)targets, tn, N, D, 1e-12f);
  linear(c->stream, qn, D, tn, nullptr, nullptr, 0, (bf16_t*)sims_out, N, Q, N, D, EPI_STORE);
  return check_launch("pcy_retrieval_scores");
}

int pcy_retrieval_scores_f32(pcy_ctx* c, const float* query, int Q, const void* targets, int targets_bf16, int N, int D, float* sims_out) {
  PCY_STICKY(c);
  if (D % 4 || D <= 0) return fail(1, "pcy_retrieval_scores_f32: D=%d must be a positive multiple of 4", D);
  if (pcy_retrieval_dot_smem(D) > 159 * 1024) return fail(1, "pcy_retrieval_scores_f32: D=%d does not fit the query tile in LDS", D);
  pcy_launch_retrieval_dot_f32(c->stream, query, Q, targets, targets_bf16, N, D, 1e-12f, sims_out);
  return check_launch("pcy_retrieval_scores_f32");
}
int pcy_retrieval_topk_f32(pcy_ctx* c, const float* query, int Q, const void* targets, int targets_bf16, int N, int D, int k, int32_t* idx_out,
                           float* score_out) {
  PCY_STICKY(c);
  if (D % 4 || D <= 0) return fail(1, "pcy_retrieval_topk_f32: D=%d must be a positive multiple of 4", D);
  if (pcy_retrieval_dot_smem(D) > 159 * 1024) return fail(1, "pcy_retrieval_topk_f32: D=%d does not fit the query tile in LDS", D);
  if (k < 1 || k > N) return fail(1, "pcy_retrieval_topk_f32: k=%d must be in [1, N=%d]", k, N);
  if (int r = c->reserve(align_up((size_t)Q * N * 4, 256) + 4096)) return r;
  float* sims = reinterpret_cast<float*>(c->ws);
  pcy_launch_retrieval_dot_f32(c->stream, query, Q, targets, targets_bf16, N, D, 1e-12f, sims);
  pcy_launch_retrieval_rank_f32(c->stream, sims, Q, N, k, idx_out, score_out);
  return check_launch("pcy_retrieval_topk_f32");
}

int pcy_qa_probs(pcy_ctx* c, const void* logits, int is_f32, int rows, int V, int yes_id, int no_id, void* probs_out, float* yes_no_out,
                 int32_t* argmax_out) {
  PCY_STICKY(c);
  if (!logits || rows < 0 || V <= 0) return fail(1, "pcy_qa_probs: logits NULL or bad shape (rows %d, V %d)", rows, V);
  if (yes_no_out && (yes_id < 0 || yes_id >= V || no_id < 0 || no_id >= V)) return fail(1, "pcy_qa_probs: yes / no token outside the vocabulary");
  pcy_launch_qa_probs(c->stream, logits, is_f32, rows, V, yes_id, no_id, probs_out, yes_no_out, argmax_out);
  return check_launch("pcy_qa_probs");
}

int pcy_mlp_forward(pcy_ctx* c, const pcy_mlp_desc* m, const void* x, int M, void* out) {
  PCY_STICKY(c);
  if (m->n_layers < 1 || m->n_layers > 8) return fail(1, "pcy_mlp_forward: n_layers %d", m->n_layers);
  int maxw = 0;
  for (int i = 0; i <= m->n_layers; ++i) {
    if (m->dims[i] % 8) return fail(1, "pcy_mlp_forward: dims must be multiples of 8");
    if (i > 0 && i < m->n_layers && m->dims[i] > maxw) maxw = m->dims[i];
  }
  if (int r = c->reserve(2 * align_up((size_t)M * (maxw + 8) * 2, 256) + 4096)) return r;
  Carver cv(c->ws);
  bf16_t* t[2] = {cv.take<bf16_t>((size_t)M * (maxw + 8)), cv.take<bf16_t>((size_t)M * (maxw + 8))};
  const bf16_t* cur = (const bf16_t*)x;
  for (int i = 0; i < m->n_layers; ++i) {
    const bool last = i == m->n_layers - 1;
    bf16_t* dst = last ? (bf16_t*)out : t[i & 1];
    const int K = m->dims[i], N = m->dims[i + 1];
    if (M > 8 && K % 64 != 0) return fail(1, "pcy_mlp_forward: K=%d must be a multiple of 64 for M>8", K);
    linear(c->stream, cur, K, (const bf16_t*)m->w[i], (const bf16_t*)m->b[i], nullptr, 0, dst, N, M, N, K,
           last ? EPI_STORE : EPI_GELU_ERF);
    cur = dst;
  }
  return check_launch("pcy_mlp_forward");
}

static int esm_encode_enqueue(pcy_ctx* c, const pcy_esm_desc* m, const int32_t* tokens, const int32_t* pos, const int32_t* cu,
                              const int32_t* vt_cu, int ntok, int nseq, int max_len, int vt_total, int mask_pads, void* hidden_out);
// FNV-1a over EVERY model pointer and constant a captured pcy_esm_encode chain bakes in (the CONTENTS of the host layer array, not its address:
// a freed engine's descriptor array and device blocks can come back at the same addresses with other weights behind them)
static uint64_t esm_weights_fingerprint(const pcy_esm_desc* m) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
  mix((uint64_t)(uintptr_t)m->layers); mix((uint64_t)(uintptr_t)m->final_ln_w); mix((uint64_t)(uintptr_t)m->final_ln_b);
  mix((uint64_t)(uintptr_t)m->rope_cos); mix((uint64_t)(uintptr_t)m->rope_sin);
  uint32_t eps; memcpy(&eps, &m->ln_eps, 4); mix(eps); mix((uint64_t)(uint32_t)m->vocab);
  for (int l = 0; l < m->n_layers; ++l) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(&m->layers[l]);
    for (size_t i = 0; i < sizeof(pcy_esm_layer); ++i) mix(p[i]);
  }
  return h;
}
// tokens at or below which pcy_esm_encode replays a captured launch chain (PCY_DISABLE=esm_graph: always launch by launch; read per call)
static int esm_graph_max_tokens() {
  return pcy_off("esm_graph") ? 0 : 40000;   // (round 5: bulk batches too -- see EsmEngine.GRAPH_MAX_TOKENS)
}
int pcy_esm_encode(pcy_ctx* c, const pcy_esm_desc* m, const int32_t* tokens, const int32_t* pos, const int32_t* cu,
                   const int32_t* vt_cu, int ntok, int nseq, int max_len, int vt_total, int mask_pads, void* hidden_out) {
  PCY_STICKY(c);
  if (ntok <= 0 || ntok > esm_graph_max_tokens() || !c->cap_stream)
    return esm_encode_enqueue(c, m, tokens, pos, cu, vt_cu, ntok, nseq, max_len, vt_total, mask_pads, hidden_out);
  // everything a launch of the chain bakes in: argument pointers, sizes, the model's arrays, the workspace base, and the run-time
  // switches that select kernels (read per launch from the environment: a changed switch is another key)
  auto envh = [](const char* n) { const char* e = getenv(n); uint64_t h = 1469598103934665603ull; for (; e && *e; ++e) h = (h ^ (unsigned char)*e) * 1099511628211ull; return h; };
  uint64_t key[16] = {(uint64_t)(uintptr_t)tokens, (uint64_t)(uintptr_t)pos, (uint64_t)(uintptr_t)cu, (uint64_t)(uintptr_t)vt_cu,
                      (uint64_t)(uintptr_t)hidden_out, esm_weights_fingerprint(m), (uint64_t)(uintptr_t)m->embed,
                      ((uint64_t)(uint32_t)ntok << 32) | (uint32_t)nseq, ((uint64_t)(uint32_t)max_len << 32) | (uint32_t)vt_total,
                      ((uint64_t)(uint32_t)m->d << 32) | (uint32_t)m->ffn, ((uint64_t)(uint32_t)m->n_layers << 32) | (uint32_t)m->n_heads,
                      (uint64_t)mask_pads | ((uint64_t)m->rope_mode << 8), 0 /* workspace base, below */,
                      envh("PCY_ESM_ATTN") ^ (envh("PCY_DISABLE") << 1), envh("PCY_GEMM_MID") ^ (envh("PCY_GEMM_PERM") << 1),
                      envh("PCY_DEBUG_POISON_WS")};
  // the workspace is sized (and possibly re-allocated: every slot is dropped then) before the key is final
  {
    const int d = m->d, F = m->ffn;
    const size_t vtt = align_up((size_t)ntok + 64 * (size_t)nseq, 8) > (size_t)vt_total ? align_up((size_t)ntok + 64 * (size_t)nseq, 8) : (size_t)vt_total;
    const size_t need = align_up((size_t)ntok * d * 2, 256) * 3 + align_up((size_t)ntok * 3 * d * 2, 256) + align_up((size_t)ntok * F * 2, 256) +
                        align_up((size_t)d * vtt * 2, 256) + align_up((size_t)(nseq + 1) * 4, 256) + 4096;
    if (int r = c->reserve(need)) return r;
  }
  key[12] = (uint64_t)(uintptr_t)c->ws;
  pcy_ctx::GraphSlot* slot = nullptr;
  for (auto& g : c->gslots)
    if (g.stamp && memcmp(g.key, key, sizeof(key)) == 0) { slot = &g; break; }
  if (slot && slot->exec) {
    slot->stamp = ++c->gstamp;
    ++g_pcy_dispatch[PCY_DISPATCH_ESM_GRAPH];
    HIP_TRY(hipGraphLaunch(slot->exec, c->stream));
    return 0;
  }
  if (!slot) {   // first sight of this key: remember it (evicting the least recently used slot), run launch by launch
    slot = &c->gslots[0];
    for (auto& g : c->gslots)
      if (g.stamp < slot->stamp) slot = &g;
    if (slot->exec) hipGraphExecDestroy(slot->exec);
    *slot = pcy_ctx::GraphSlot{};
    memcpy(slot->key, key, sizeof(key));
    slot->stamp = ++c->gstamp;
    return esm_encode_enqueue(c, m, tokens, pos, cu, vt_cu, ntok, nseq, max_len, vt_total, mask_pads, hidden_out);
  }
  // second sight: capture (on the capture stream -- the caller's may be the legacy stream), then replay on the caller's stream
  pcy_gemm_prepare(c->stream);   // one-time device tables must not be built inside the capture
  hipGraph_t g = nullptr;
  hipStream_t user = c->stream;
  c->stream = c->cap_stream;
  hipError_t e0 = hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal);
  int rc = 0;
  if (e0 == hipSuccess) {
    rc = esm_encode_enqueue(c, m, tokens, pos, cu, vt_cu, ntok, nseq, max_len, vt_total, mask_pads, hidden_out);
    e0 = hipStreamEndCapture(c->cap_stream, &g);
  }
  c->stream = user;
  if (e0 != hipSuccess || rc != 0 || !g) {   // could not capture: forget the key, run launch by launch
    (void)hipGetLastError();
    if (g) hipGraphDestroy(g);
    *slot = pcy_ctx::GraphSlot{};
    return esm_encode_enqueue(c, m, tokens, pos, cu, vt_cu, ntok, nseq, max_len, vt_total, mask_pads, hidden_out);
  }
  e0 = hipGraphInstantiate(&slot->exec, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (e0 != hipSuccess) {
    (void)hipGetLastError();
    *slot = pcy_ctx::GraphSlot{};
    return esm_encode_enqueue(c, m, tokens, pos, cu, vt_cu, ntok, nseq, max_len, vt_total, mask_pads, hidden_out);
  }
  slot->stamp = ++c->gstamp;
  ++g_pcy_dispatch[PCY_DISPATCH_ESM_GRAPH];
  HIP_TRY(hipGraphLaunch(slot->exec, c->stream));
  return 0;
}
static int esm_encode_enqueue(pcy_ctx* c, const pcy_esm_desc* m, const int32_t* tokens, const int32_t* pos, const int32_t* cu,
                              const int32_t* vt_cu, int ntok, int nseq, int max_len, int vt_total, int mask_pads, void* hidden_out) {
  const int d = m->d, H = m->n_heads, F = m->ffn;
  if (d % H) return fail(1, "pcy_esm_encode: d %% heads");
  const int dh = d / H;
  if (int r = check_head_dim("pcy_esm_encode", dh, true)) return r;
  if (d % 64 || F % 64) return fail(1, "pcy_esm_encode: d and ffn must be multiples of 64");
  if (ntok <= 0) return 0;
  // single-pass attention (default at head_dim 64): Vt slices zero-padded to 64 keys, laid out by the engine itself
  const bool fast = pcy_attn_fast_eligible(dh, 0, false, 1.0f, H, H, 3 * d, 0, 3 * d, d, d);
  if (fast) vt_total = (int)align_up((size_t)ntok + 64 * (size_t)nseq, 8);
  const size_t need = align_up((size_t)ntok * d * 2, 256) * 3 + align_up((size_t)ntok * 3 * d * 2, 256) +
                      align_up((size_t)ntok * F * 2, 256) + align_up((size_t)d * vt_total * 2, 256) + align_up((size_t)(nseq + 1) * 4, 256) + 4096;
  if (int r = c->reserve(need)) return r;
  Carver cv(c->ws);
  bf16_t* x = cv.take<bf16_t>((size_t)ntok * d);
  bf16_t* xn = cv.take<bf16_t>((size_t)ntok * d);
  bf16_t* ao = cv.take<bf16_t>((size_t)ntok * d);
  bf16_t* qkv = cv.take<bf16_t>((size_t)ntok * 3 * d);
  bf16_t* act = cv.take<bf16_t>((size_t)ntok * F);
  bf16_t* vt = cv.take<bf16_t>((size_t)d * vt_total);
  int32_t* vt_cu64 = cv.take<int32_t>((size_t)nseq + 1);
  const bool vrow = fast && pcy_attn_fast_vrow(3 * d, 2 * d);   // the single-pass kernel reads V out of qkv: no transposed copy
  if (fast && !vrow) {
    pcy_launch_vt_offsets(c->stream, cu, nseq, 64, vt_cu64);
    vt_cu = vt_cu64;
  }
  hipStream_t s = c->stream;
  pcy_launch_esm_embed(s, (const bf16_t*)m->embed, tokens, cu, nseq, max_len, x, d, mask_pads);
  const float qscale = 1.0f / sqrtf((float)dh);
  for (int l = 0; l < m->n_layers; ++l) {
    const pcy_esm_layer& L = m->layers[l];
    pcy_launch_layernorm(s, x, (const bf16_t*)L.ln1_w, (const bf16_t*)L.ln1_b, xn, ntok, d, m->ln_eps);
    if (dh == 64 && ntok > 8 && d % 64 == 0) {
      // rotary (q pre-scaled) fused into the projection's epilogue: saves a read+write pass over q and k
      PcyGemmArgs g{};
      g.A = xn; g.W = (const bf16_t*)L.wqkv; g.C = qkv; g.bias = (const bf16_t*)L.bqkv;
      g.M = ntok; g.N = 3 * d; g.K = d; g.lda = d; g.ldc = 3 * d; g.epi = EPI_STORE;
      g.rope_pos = pos; g.rope_cos = (const bf16_t*)m->rope_cos; g.rope_sin = (const bf16_t*)m->rope_sin;
      g.rope_ncols = 2 * d; g.rope_qcols = d; g.rope_mode = m->rope_mode; g.rope_scale = qscale;
      pcy_launch_gemm(s, g);
    } else {
      linear(s, xn, d, (const bf16_t*)L.wqkv, (const bf16_t*)L.bqkv, nullptr, 0, qkv, 3 * d, ntok, 3 * d, d, EPI_STORE);
      pcy_launch_rope(s, qkv, 3 * d, 0, H, dh, pos, (const bf16_t*)m->rope_cos, (const bf16_t*)m->rope_sin, ntok, m->rope_mode, qscale);
      pcy_launch_rope(s, qkv, 3 * d, d, H, dh, pos, (const bf16_t*)m->rope_cos, (const bf16_t*)m->rope_sin, ntok, m->rope_mode, 0.f);
    }
    if (!vrow) pcy_launch_transpose_v(s, qkv, 3 * d, 2 * d, H, dh, cu, vt_cu, nseq, max_len, vt, vt_total);
    PcyAttnArgs t{};
    if (vrow) { t.v = qkv; t.ldv = 3 * d; t.vcol0 = 2 * d; }
    t.q = qkv; t.ldq = 3 * d; t.qcol0 = 0; t.k = qkv; t.ldk = 3 * d; t.kcol0 = d; t.vt = vt; t.vt_total = vt_total;
    t.o = ao; t.ldo = d; t.cu = cu; t.vt_cu = vt_cu; t.keep = nullptr; t.nseq = nseq; t.max_len = max_len; t.H = H; t.Hkv = H;
    t.dh = dh; t.causal = 0; t.scale = 1.0f; t.vt_pad64 = fast ? 1 : 0;
    pcy_launch_attn(s, t);
    linear(s, ao, d, (const bf16_t*)L.wo, (const bf16_t*)L.bo, x, d, x, d, ntok, d, d, EPI_RESID);
    pcy_launch_layernorm(s, x, (const bf16_t*)L.ln2_w, (const bf16_t*)L.ln2_b, xn, ntok, d, m->ln_eps);
    linear(s, xn, d, (const bf16_t*)L.w1, (const bf16_t*)L.b1, nullptr, 0, act, F, ntok, F, d, EPI_GELU_ESM);
    linear(s, act, F, (const bf16_t*)L.w2, (const bf16_t*)L.b2, x, d, x, d, ntok, d, F, EPI_RESID);
  }
  pcy_launch_layernorm(s, x, (const bf16_t*)m->final_ln_w, (const bf16_t*)m->final_ln_b, (bf16_t*)hidden_out, ntok, d, m->ln_eps);
  return check_launch("pcy_esm_encode");
}

}  // extern "C"
namespace {
// The prefill family -- pcy_llama_prefill / _prefill_all / _score / _extend / _extend_packed -- is ONE request (PrefillReq) to ONE layer loop
// (llama_prefill_impl); every entry point fills the fields it has.  ScoreReq: token rows to score behind the layers (n == 0: none)
struct ScoreReq { const int32_t* rows; const int32_t* targets; int n; float* nll; };
// pcy_llama_extend: the T tokens of every row FOLLOW t_past tokens the cache already holds (on == false: a prefill from slot 0).  The layer loop
// is the prefill's; what differs is the rotary position (t_past + s, made on the device), where K / V go (logical slots t_past ..) and the
// attention (pcy_attn_ext.hip reads the keys from the cache: no transposed V workspace on this path).
// grp (pcy_llama_extend_grouped): the rows are groups with a prefix length each; t_past then counts the tokens in the rows' OWN panels (t_own)
struct ExtendReq { bool on; int t_past; bool packed; const pcy_prefix_groups* grp; };   // packed: the attention launch is pcy_launch_attn_extend_packed
struct PrefillReq {
  const void* embeds; const uint8_t* keep; int B, T;
  const int32_t *pos, *cu, *vt_cu;                                    // a prefill's (an extension makes its positions itself)
  const int32_t* logit_rows; int n_logit_rows; void* logits_out;
  const int32_t* sum_rows; int n_sum_rows; void* hidden_sum_out;      // ret_token_access='all'
  void *hidden_out, *hidden_all_out;                                  // final-normed [M][d]; [L+1][M][d] (pcy_llama_prefill_all)
  ScoreReq score; ExtendReq ext;
};
// the request of pcy_llama_extend / _packed / _grouped: what the three entries share, `ext` is what tells them apart
PrefillReq extend_req(const void* embeds, const uint8_t* keep, int B, int S, ExtendReq ext, const int32_t* logit_rows, int n_logit_rows, void* logits_out,
                      void* hidden_out, const int32_t* score_rows, const int32_t* targets, int n_score, float* nll_out) {
  PrefillReq r{};
  r.embeds = embeds; r.keep = keep; r.B = B; r.T = S; r.logit_rows = logit_rows; r.n_logit_rows = n_logit_rows; r.logits_out = logits_out;
  r.hidden_out = hidden_out; r.ext = ext;
  if (n_score > 0) r.score = ScoreReq{score_rows, targets, n_score, nll_out};
  return r;
}
// The carve of the prefill workspace, in ONE place; bytes = its end + slack, what a call reserves (sized by a carve of a null base).  vt_elems: the transposed V
struct PrefillWs {
  bf16_t *x, *xn, *qkv, *ao, *act, *vt, *lastx;
  float* sk_ws; size_t sk_bytes;      // split-K partials for the projections that under-fill the chip
  float* hsum; bf16_t* hsum_tmp;      // ret_token_access='all': fp32 sum of the L+1 hidden states
  unsigned char* a8; float* sa8;      // fp8 weight path: per-token e4m3 codes and scales of a projection's input
  bf16_t* score_x; char* score_ws; int32_t* pos_ext; size_t bytes;   // (pos_ext: rotary positions t_past + s of an extension's tokens)
};
PrefillWs carve_prefill_ws(char* base, const pcy_llama_desc* m, int M, size_t vt_elems, int n_logit_rows, int n_sum_rows, int n_score, bool fp8, bool ext) {
  const int d = m->d, H = m->n_heads, dh = m->head_dim, F = m->ffn, qkvw = (H + 2 * m->n_kv_heads) * dh;
  Carver cv(base);
  PrefillWs w{};
  w.x = cv.take<bf16_t>((size_t)M * d); w.xn = cv.take<bf16_t>((size_t)M * d);
  w.qkv = cv.take<bf16_t>((size_t)M * qkvw);
  w.ao = cv.take<bf16_t>((size_t)M * H * dh);
  w.act = cv.take<bf16_t>((size_t)M * F);
  w.vt = cv.take<bf16_t>(vt_elems);
  w.lastx = cv.take<bf16_t>((size_t)(n_logit_rows + 1) * d);
  w.sk_bytes = M <= 1024 ? (size_t)8 * M * qkvw * 4 : 0;
  w.sk_ws = w.sk_bytes ? cv.take<float>(w.sk_bytes / 4) : nullptr;
  w.hsum = cv.take<float>((size_t)(n_sum_rows + 1) * d);
  w.hsum_tmp = cv.take<bf16_t>((size_t)(n_sum_rows + 1) * d);
  if (fp8) { w.a8 = cv.take<unsigned char>((size_t)M * (F > H * dh ? F : H * dh)); w.sa8 = cv.take<float>((size_t)M); }
  if (n_score > 0) { w.score_x = cv.take<bf16_t>((size_t)n_score * d); w.score_ws = cv.take<char>(pcy_xent_ws_bytes(n_score, m->vocab)); }
  if (ext) w.pos_ext = cv.take<int32_t>((size_t)M);
  w.bytes = cv.off + 4096;
  return w;
}
// An extension of S tokens behind t_past: the rows exist, a shared prefix is well formed and is never written, the new slots fit
int check_extend_span(const pcy_kv_cache* kv, int B, int S, int t_past, const char* what) {
  if (B > kv->B) return fail(1, "%s: B=%d exceeds cache rows %d", what, B, kv->B);
  if (int r = check_shared_cache(kv, B, what)) return r;
  if (kv_shared(kv) && t_past < kv->prefix_T)
    return fail(1, "%s: t_past=%d lies inside the shared prefix of %d slots, which is never written", what, t_past, kv->prefix_T);
  if ((long)t_past + S > kv_cap(kv)) return fail(1, "%s: t_past=%d + S=%d exceed the cache capacity %d", what, t_past, S, kv_cap(kv));
  return 0;
}
// A grouped extension (include/pcy.h, pcy_prefix_groups), checked on the HOST arrays: the cache carries a prefix and no uniform rows_per_prefix,
// the groups cover the call's rows exactly, every prefix length is real, the new slots fit.  max_rows / max_len: the largest group / prefix length
int check_prefix_groups(const pcy_kv_cache* kv, const pcy_prefix_groups* gr, int B, int S, const char* what, int* max_rows, int* max_len) {
  if (!gr || !gr->rows || !gr->len || !gr->d_row0 || !gr->d_len || !gr->d_row_grp) return fail(1, "%s: group tables missing", what);
  if (gr->n_groups < 1 || gr->t_own < 0 || B < 1 || S < 1) return fail(1, "%s: n_groups=%d t_own=%d B=%d S=%d", what, gr->n_groups, gr->t_own, B, S);
  if (!kv || !kv->k || !kv->v) return fail(1, "%s: cache without k / v", what);
  if (!kv->prefix_k || !kv->prefix_v || kv->prefix_T <= 0 || kv->prefix_B <= 0 || kv->Tmax <= 0 || kv->rows_per_prefix != 0)
    return fail(1, "%s: a grouped extension needs a cache with prefix_k, prefix_v, prefix_T, prefix_B, a suffix capacity > 0 and rows_per_prefix == 0", what);
  if (gr->n_groups > kv->prefix_B) return fail(1, "%s: %d groups need more than the %d prefix rows of the cache", what, gr->n_groups, kv->prefix_B);
  long sum = 0;
  int mr = 0, ml = 0;
  for (int g = 0; g < gr->n_groups; ++g) {
    if (gr->rows[g] < 1) return fail(1, "%s: group %d has rows=%d (>= 1 expected)", what, g, gr->rows[g]);
    if (gr->len[g] < 1 || gr->len[g] > kv->prefix_T) return fail(1, "%s: group %d has len=%d outside [1, prefix_T=%d]", what, g, gr->len[g], kv->prefix_T);
    sum += gr->rows[g];
    mr = gr->rows[g] > mr ? gr->rows[g] : mr;
    ml = gr->len[g] > ml ? gr->len[g] : ml;
  }
  if (sum != B) return fail(1, "%s: the groups hold %ld rows, the call B=%d", what, sum, B);
  if (B > kv->B) return fail(1, "%s: B=%d exceeds cache rows %d", what, B, kv->B);
  if ((long)gr->t_own + S > kv->Tmax) return fail(1, "%s: t_own=%d + S=%d exceed the suffix capacity %d", what, gr->t_own, S, kv->Tmax);
  *max_rows = mr; *max_len = ml;
  return 0;
}
int check_prefill_req(const pcy_llama_desc* m, const pcy_kv_cache* kv, const PrefillReq& r, int* g_max_rows) {   // g_max_rows: of a grouped extension
  const int d = m->d, H = m->n_heads, Hkv = m->n_kv_heads, dh = m->head_dim, F = m->ffn, B = r.B, T = r.T;
  if (int e = check_head_dim("pcy_llama_prefill", dh, true)) return e;
  if (int e = check_widths("pcy_llama_prefill", m, 64, false)) return e;
  if (r.ext.on) {
    const int t_past = r.ext.t_past;
    if (int e = check_head_dim("pcy_llama_extend", dh, false)) return e;
    if (H % Hkv) return fail(1, "pcy_llama_extend: H=%d is no multiple of Hkv=%d", H, Hkv);
    if (m->layers_fp8) return fail(1, "pcy_llama_extend: fp8 projections are not supported on the extension path");
    if (B < 1 || T < 1 || t_past < 0) return fail(1, "pcy_llama_extend: B=%d S=%d t_past=%d", B, T, t_past);
    if (r.ext.grp) {
      int max_len = 0;
      if (int e = check_prefix_groups(kv, r.ext.grp, B, T, "pcy_llama_extend_grouped", g_max_rows, &max_len)) return e;
      if ((long)max_len + t_past + T > m->max_pos)
        return fail(1, "pcy_llama_extend_grouped: len=%d + t_own=%d + S=%d exceed rope table %d", max_len, t_past, T, m->max_pos);
    } else {
      if (!kv->k || !kv->v) return fail(1, "pcy_llama_extend: cache without k / v");
      if (int e = check_extend_span(kv, B, T, t_past, "pcy_llama_extend")) return e;
      if ((long)t_past + T > m->max_pos) return fail(1, "pcy_llama_extend: t_past=%d + S=%d exceed rope table %d", t_past, T, m->max_pos);
    }
  } else {
    if (kv_shared(kv)) return fail(1, "pcy_llama_prefill: a cache with a shared prefix cannot be prefilled (prefill the prefix cache itself)");
    if (B > kv->B || T > kv->Tmax) return fail(1, "pcy_llama_prefill: B=%d T=%d exceed cache (%d,%d)", B, T, kv->B, kv->Tmax);
    if (T > m->max_pos) return fail(1, "pcy_llama_prefill: T=%d exceeds rope table %d", T, m->max_pos);
  }
  if (r.score.n < 0 || (r.score.n > 0 && (!r.score.rows || !r.score.targets || !r.score.nll))) return fail(1, "pcy_llama_score: score_rows / targets / nll_out missing");
  if (r.n_sum_rows > 0 && (!r.sum_rows || !r.hidden_sum_out)) return fail(1, "pcy_llama_prefill: sum_rows / hidden_sum_out missing");
  if (m->layers_fp8 && (d % 128 || F % 128 || (H * dh) % 128)) return fail(1, "pcy_llama_prefill: the fp8 path needs d, ffn, H*dh %% 128 == 0");
  return 0;
}
// The extension attention stage of a layer (pcy_attn_extend, pcy_llama_extend): rope (q, k) in place at `pos`, K / V of token s to slot own_slot0 + s of
// the row's own panel (the panel pointer carries the offset, the row stride stays Tmax * dh), then the S queries of every row against the cache
void enqueue_extend_attention(hipStream_t s, bf16_t* qkv, int ld, const pcy_kv_cache* kv, int layer, bf16_t* o, int ldo, int t_past, const int32_t* pos,
                              const bf16_t* cos_t, const bf16_t* sin_t, const uint8_t* keep, int B, int S, int H, int Hkv, int dh, bool packed,
                              const pcy_prefix_groups* grp, int g_max_rows) {   // (g_max_rows: the largest group, from check_prefix_groups)
  const bool shared = kv_shared(kv);
  // first written slot inside the rows' own panels (grouped: t_past IS the count of own tokens, the same for every row)
  const int own_slot0 = grp ? t_past : shared ? t_past - kv->prefix_T : t_past;
  const size_t layer_stride = (size_t)kv->B * Hkv * kv->Tmax * dh;
  bf16_t *kl = (bf16_t*)kv->k + layer * layer_stride, *vl = (bf16_t*)kv->v + layer * layer_stride;
  pcy_launch_rope(s, qkv, ld, 0, H + Hkv, dh, pos, cos_t, sin_t, B * S, 0, 0.f);
  pcy_launch_kv_scatter(s, qkv, ld, H * dh, (H + Hkv) * dh, Hkv, dh, kl + (size_t)own_slot0 * dh, vl + (size_t)own_slot0 * dh, B, S, kv->Tmax);
  PcyExtAttnArgs e{};
  e.q = qkv; e.ldq = ld; e.k_own = kl; e.v_own = vl; e.Town = kv->Tmax; e.scale = 1.0f / sqrtf((float)dh);
  if (shared) {
    const size_t prefix_layer_stride = (size_t)kv->prefix_B * Hkv * kv->prefix_T * dh;
    e.k_pre = (const bf16_t*)kv->prefix_k + layer * prefix_layer_stride; e.v_pre = (const bf16_t*)kv->prefix_v + layer * prefix_layer_stride;
    e.Tp = kv->prefix_T; e.rows_per_prefix = kv->rows_per_prefix;
  }
  e.o = o; e.ldo = ldo; e.keep = keep; e.ld_keep = kv_cap(kv); e.B = B; e.S = S; e.H = H; e.Hkv = Hkv; e.dh = dh; e.t_past = t_past;
  if (grp) { e.g_row0 = grp->d_row0; e.g_len = grp->d_len; e.g_row_grp = grp->d_row_grp; e.n_groups = grp->n_groups; e.g_max_rows = g_max_rows; }
  if (packed) pcy_launch_attn_extend_packed(s, e);
  else pcy_launch_attn_extend(s, e);
}
// The prefill's own attention stage: rope, K / V into the cache from slot 0, the transposed V copy, causal attention over the rows' own tokens
void enqueue_prefill_attention(hipStream_t s, const pcy_llama_desc* m, const pcy_kv_cache* kv, const PrefillReq& r, const PrefillWs& w, int l, int vt_total) {
  const int H = m->n_heads, Hkv = m->n_kv_heads, dh = m->head_dim, qkvw = (H + 2 * Hkv) * dh, B = r.B, T = r.T;
  const size_t layer_stride = (size_t)kv->B * Hkv * kv->Tmax * dh;
  bf16_t *kl = (bf16_t*)kv->k + l * layer_stride, *vl = (bf16_t*)kv->v + l * layer_stride;
  const bf16_t *cos_t = (const bf16_t*)m->rope_cos, *sin_t = (const bf16_t*)m->rope_sin;
  if (pcy_off("prefill_post_qkv") ||   // (the three launches: the test compares both)
      !pcy_launch_prefill_post_qkv(s, w.qkv, qkvw, H, Hkv, dh, r.pos, cos_t, sin_t, kl, vl, B, T, kv->Tmax, r.cu, r.vt_cu, w.vt, vt_total)) {
    pcy_launch_rope(s, w.qkv, qkvw, 0, H + Hkv, dh, r.pos, cos_t, sin_t, B * T, 0, 0.f);
    pcy_launch_kv_scatter(s, w.qkv, qkvw, H * dh, (H + Hkv) * dh, Hkv, dh, kl, vl, B, T, kv->Tmax);
    pcy_launch_transpose_v(s, w.qkv, qkvw, (H + Hkv) * dh, Hkv, dh, r.cu, r.vt_cu, B, T, w.vt, vt_total);
  }
  PcyAttnArgs t{};
  t.q = w.qkv; t.ldq = qkvw; t.qcol0 = 0; t.k = w.qkv; t.ldk = qkvw; t.kcol0 = H * dh; t.vt = w.vt; t.vt_total = vt_total;
  t.o = w.ao; t.ldo = H * dh; t.cu = r.cu; t.vt_cu = r.vt_cu; t.keep = r.keep; t.nseq = B; t.max_len = T; t.H = H; t.Hkv = Hkv; t.dh = dh;
  t.causal = 1; t.scale = 1.0f / sqrtf((float)dh);
  pcy_launch_attn(s, t);
}
// ---- what follows the layers: x = the un-normed output of the last layer
void enqueue_logit_rows(hipStream_t s, const pcy_llama_desc* m, const PrefillReq& r, const bf16_t* x, bf16_t* lastx) {
  const int d = m->d, n = r.n_logit_rows;
  if (n <= 0 || !r.logits_out) return;
  pcy_launch_copy_rows(s, x, d, lastx, d, r.logit_rows, n, d);
  if (r.hidden_all_out && n > 64) {
    // pcy_llama_prefill_all with many rows (the reference's full [B,T,V] logits): final norm of those rows, then lm_head as an MFMA
    // GEMM -- the GEMV would stream the 1 GB matrix once per 32 rows.  ONLY on this entry point: the GEMM accumulates in another
    // order than the fused-norm GEMV, and a row's logits from pcy_llama_prefill must not depend on how many rows were asked for
    // (QA / pair scoring with 64 or 65 rows: same bits per row; tests/test_gpu_round4.py).
    pcy_launch_rmsnorm(s, lastx, (const bf16_t*)m->final_norm, lastx, n, d, m->rms_eps, m->rms_cast);
    linear(s, lastx, d, (const bf16_t*)m->lm_head, nullptr, nullptr, 0, (bf16_t*)r.logits_out, m->vocab, n, m->vocab, d, EPI_STORE);
    return;
  }
  // final norm of the selected rows, then lm_head on the MFMA GEMV (32 rows per pass over the matrix) for EVERY row count, one row
  // included: the same arithmetic per row whatever the number of rows asked for (the fused-norm streaming GEMV it replaces ran 4 rows
  // per pass: QA / pair scoring with more than 64 rows streamed the 1 GB matrix rows / 4 times -- advisor finding, round 4)
  PcyGemvArgs h{};
  h.W = (const bf16_t*)m->lm_head; h.x = lastx; h.y = (bf16_t*)r.logits_out; h.N = m->vocab; h.K = d; h.B = n; h.ldx = d; h.ldy = m->vocab; h.epi = EPI_STORE;
  if (d % 512 == 0) {
    pcy_launch_rmsnorm(s, lastx, (const bf16_t*)m->final_norm, lastx, n, d, m->rms_eps, m->rms_cast);
    h.force_mfma = 1;
  } else {   // (toy geometries: the streaming kernel with the norm fused)
    h.rms_w = (const bf16_t*)m->final_norm; h.rms_eps = m->rms_eps; h.rms_cast = m->rms_cast;
  }
  pcy_launch_gemv(s, h);
}
// the last of the L+1 hidden states of the sum rows (the final-normed one) onto the fp32 sums, then the one rounding
void enqueue_sum_rows(hipStream_t s, const pcy_llama_desc* m, const PrefillReq& r, const bf16_t* x, const PrefillWs& w) {
  const int d = m->d, n = r.n_sum_rows;
  if (n <= 0) return;
  pcy_launch_copy_rows(s, x, d, w.hsum_tmp, d, r.sum_rows, n, d);
  pcy_launch_rmsnorm(s, w.hsum_tmp, (const bf16_t*)m->final_norm, w.hsum_tmp, n, d, m->rms_eps, m->rms_cast);
  pcy_launch_acc_rows(s, w.hsum_tmp, d, nullptr, w.hsum, n, d, 0);
  pcy_launch_acc_finish(s, w.hsum, (bf16_t*)r.hidden_sum_out, (size_t)n * d);
}
// teacher-forced scoring: final norm of the scored rows, then lm_head x cross-entropy with the logits kept in registers
void enqueue_scored_rows(hipStream_t s, const pcy_llama_desc* m, const ScoreReq& sc, const bf16_t* x, const PrefillWs& w) {
  const int d = m->d;
  if (sc.n <= 0) return;
  pcy_launch_copy_rows(s, x, d, w.score_x, d, sc.rows, sc.n, d);
  pcy_launch_rmsnorm(s, w.score_x, (const bf16_t*)m->final_norm, w.score_x, sc.n, d, m->rms_eps, m->rms_cast);
  PcyXentArgs xa{};
  xa.x = w.score_x; xa.ldx = d; xa.W = (const bf16_t*)m->lm_head; xa.targets = sc.targets; xa.M = sc.n; xa.V = m->vocab; xa.d = d;
  xa.nll = sc.nll; xa.ws = w.score_ws;
  pcy_launch_lm_head_xent(s, xa);
}
int llama_prefill_impl(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const PrefillReq& r) {
  PCY_STICKY(c);
  int g_max_rows = 0;
  if (int e = check_prefill_req(m, kv, r, &g_max_rows)) return e;
  const int d = m->d, H = m->n_heads, Hkv = m->n_kv_heads, dh = m->head_dim, F = m->ffn, B = r.B, T = r.T;
  const int M = B * T, qkvw = (H + 2 * Hkv) * dh, Tp = (T + 31) / 32 * 32, n_sum_rows = r.n_sum_rows;
  const bool ext = r.ext.on;
  // Row stride of the transposed V ([Hkv*dh][vt_total]): a power-of-two stride (one 512-token prompt: 1 KB) sends the 128 rows of a
  // key block's V tile to the same few L2 channels; pad it to an odd multiple of 64 bytes
  int vt_total = ext ? 0 : B * Tp;   // (the extension attention reads V from the cache)
  if (!ext && (vt_total / 32) % 2 == 0) vt_total += 32;
  const size_t need = carve_prefill_ws(nullptr, m, M, (size_t)Hkv * dh * vt_total, r.n_logit_rows, n_sum_rows, r.score.n, m->layers_fp8 != nullptr, ext).bytes;
  if (int e = c->reserve(need)) return e;
  const PrefillWs w = carve_prefill_ws(c->ws, m, M, (size_t)Hkv * dh * vt_total, r.n_logit_rows, n_sum_rows, r.score.n, m->layers_fp8 != nullptr, ext);
  bf16_t *x = w.x, *xn = w.xn, *hall = (bf16_t*)r.hidden_all_out;
  hipStream_t s = c->stream;
  if (ext) {   // rotary positions t_past + s of the new tokens (every row: quirk Q2)
    if (r.ext.grp) pcy_launch_ext_pos_grouped(s, w.pos_ext, B, T, r.ext.t_past, r.ext.grp->d_len, r.ext.grp->d_row_grp);
    else pcy_launch_ext_pos(s, w.pos_ext, B, T, r.ext.t_past);
    ++g_pcy_dispatch[PCY_DISPATCH_EXTEND];
    if (r.ext.packed) ++g_pcy_dispatch[PCY_DISPATCH_EXTEND_PACKED];
    if (r.ext.grp) ++g_pcy_extend_grouped;
  }
  // fp8 weight path: every projection = per-token e4m3 quantisation of its bf16 input + the fp8 MFMA GEMM
  // ln != nullptr: A is the raw hidden state, RMSNorm(A) * ln is what gets quantised (one fused pass; PCY_DISABLE=fp8_fused_norm = two launches)
  auto linear8 = [&](const bf16_t* A, int K, const void* W8, const float* sw, const bf16_t* resid, bf16_t* Cout, int ldc, int N, int epi,
                     const bf16_t* ln = nullptr) {
    if (ln && !pcy_off("fp8_fused_norm") && pcy_launch_rmsnorm_quant_fp8(s, A, ln, M, K, m->rms_eps, m->rms_cast, w.a8, w.sa8)) {
    } else {
      if (ln) { pcy_launch_rmsnorm(s, A, ln, xn, M, K, m->rms_eps, m->rms_cast); A = xn; }
      pcy_launch_quant_rows_fp8(s, A, K, M, K, w.a8, w.sa8);
    }
    PcyGemmArgs g{};
    g.A = (const bf16_t*)w.a8; g.W = (const bf16_t*)W8; g.C = Cout; g.resid = resid; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldc = ldc;
    g.ldr = ldc; g.epi = epi; g.fp8 = 1; g.sa = w.sa8; g.sw = sw;
    pcy_launch_gemm(s, g);
  };
  HIP_TRY(hipMemcpyAsync(x, r.embeds, (size_t)M * d * 2, hipMemcpyDeviceToDevice, s));
  // hidden_all_out [L+1][M][d]: HF's `hidden_states` tuple -- the embeddings, the output of layers 0..L-2, and the FINAL-NORMED
  // output of layer L-1 (pmc_llama.py:575,584 always asks for it; only materialised here when the caller does)
  if (hall) HIP_TRY(hipMemcpyAsync(hall, r.embeds, (size_t)M * d * 2, hipMemcpyDeviceToDevice, s));
  pcy_launch_acc_rows(s, x, d, r.sum_rows, w.hsum, n_sum_rows, d, 1);
  int xn_ready = 0;   // xn = RMSNorm(x) of the next projection already written by a K-split finish launch
  for (int l = 0; l < m->n_layers; ++l) {
    const pcy_llama_layer& L = m->layers[l];
    const pcy_llama_layer_fp8* L8 = m->layers_fp8 ? &m->layers_fp8[l] : nullptr;
    const bool last = l + 1 == m->n_layers;
    if (L8) linear8(x, d, L8->wqkv, L8->sqkv, nullptr, w.qkv, qkvw, qkvw, EPI_STORE, (const bf16_t*)L.ln1);
    else {
      if (!xn_ready) pcy_launch_rmsnorm(s, x, (const bf16_t*)L.ln1, xn, M, d, m->rms_eps, m->rms_cast);
      xn_ready = 0;
      linear(s, xn, d, (const bf16_t*)L.wqkv, nullptr, nullptr, 0, w.qkv, qkvw, M, qkvw, d, EPI_STORE, w.sk_ws, w.sk_bytes);
    }
    if (ext) enqueue_extend_attention(s, w.qkv, qkvw, kv, l, w.ao, H * dh, r.ext.t_past, w.pos_ext, (const bf16_t*)m->rope_cos, (const bf16_t*)m->rope_sin,
                                      r.keep, B, T, H, Hkv, dh, r.ext.packed, r.ext.grp, g_max_rows);
    else enqueue_prefill_attention(s, m, kv, r, w, l, vt_total);
    if (L8) {
      linear8(w.ao, H * dh, L8->wo, L8->so, x, x, d, d, EPI_RESID);
      linear8(x, d, L8->wgu, L8->sgu, nullptr, w.act, F, 2 * F, EPI_SWIGLU, (const bf16_t*)L.ln2);
      linear8(w.act, F, L8->wdown, L8->sdown, x, x, d, d, EPI_RESID);
    } else {
      linear(s, w.ao, H * dh, (const bf16_t*)L.wo, nullptr, x, d, x, d, M, d, H * dh, EPI_RESID, w.sk_ws, w.sk_bytes,
             (const bf16_t*)L.ln2, xn, &xn_ready, m->rms_eps, m->rms_cast);   // (M <= 1024: the K-split finish also writes RMSNorm(x) * ln2)
      if (!xn_ready) pcy_launch_rmsnorm(s, x, (const bf16_t*)L.ln2, xn, M, d, m->rms_eps, m->rms_cast);
      xn_ready = 0;
      if (M <= 8) {
        PcyGemvArgs u{};
        u.W = (const bf16_t*)L.wgu; u.x = xn; u.y = w.act; u.N = F; u.K = d; u.B = M; u.ldx = d; u.ldy = F; u.epi = EPI_SWIGLU;
        pcy_launch_gemv(s, u);
      } else {
        linear(s, xn, d, (const bf16_t*)L.wgu, nullptr, nullptr, 0, w.act, F, M, 2 * F, d, EPI_SWIGLU);
      }
      if (!last)   // ... and the next layer's input norm
        linear(s, w.act, F, (const bf16_t*)L.wdown, nullptr, x, d, x, d, M, d, F, EPI_RESID, w.sk_ws, w.sk_bytes,
               (const bf16_t*)m->layers[l + 1].ln1, xn, &xn_ready, m->rms_eps, m->rms_cast);
      else linear(s, w.act, F, (const bf16_t*)L.wdown, nullptr, x, d, x, d, M, d, F, EPI_RESID, w.sk_ws, w.sk_bytes);
    }
    // hidden_states = (embeddings, output of layers 0..L-2, final-normed output of layer L-1)  [HF LlamaModel.forward]
    if (!last) {
      pcy_launch_acc_rows(s, x, d, r.sum_rows, w.hsum, n_sum_rows, d, 0);
      if (hall) HIP_TRY(hipMemcpyAsync(hall + (size_t)(l + 1) * M * d, x, (size_t)M * d * 2, hipMemcpyDeviceToDevice, s));
    }
  }
  if (hall) pcy_launch_rmsnorm(s, x, (const bf16_t*)m->final_norm, hall + (size_t)m->n_layers * M * d, M, d, m->rms_eps, m->rms_cast);
  if (r.hidden_out) pcy_launch_rmsnorm(s, x, (const bf16_t*)m->final_norm, (bf16_t*)r.hidden_out, M, d, m->rms_eps, m->rms_cast);
  enqueue_sum_rows(s, m, r, x, w);
  enqueue_logit_rows(s, m, r, x, w.lastx);
  enqueue_scored_rows(s, m, r.score, x, w);
  return check_launch(ext ? "pcy_llama_extend" : "pcy_llama_prefill");
}
// pcy_attn_extend / _packed (grp == nullptr) and pcy_attn_extend_grouped (t_past = the tokens in the rows' own panels)
int attn_extend_entry(pcy_ctx* c, void* qkv, int ld, const pcy_kv_cache* kv, const pcy_prefix_groups* grp, int layer, void* o, int ldo, int t_past,
                      const void* cos_t, const void* sin_t, const uint8_t* keep, int B, int S, int H, int Hkv, int dh, bool packed) {
  PCY_STICKY(c);
  const char* what = grp ? "pcy_attn_extend_grouped" : "pcy_attn_extend";
  if (int r = check_head_dim(what, dh, false)) return r;
  if (Hkv < 1 || H % Hkv) return fail(1, "%s: H=%d is no multiple of Hkv=%d", what, H, Hkv);
  if (layer < 0 || (!grp && (!kv || !kv->k || !kv->v || B < 1 || S < 1 || t_past < 0)))   // (a grouped call: check_prefix_groups has words of its own)
    return fail(1, "%s: B=%d S=%d t_past=%d layer=%d", what, B, S, t_past, layer);
  if (ld % 8 || ld < (H + 2 * Hkv) * dh) return fail(1, "%s: ld=%d (rows of qkv must be 16-byte aligned)", what, ld);
  int g_max_rows = 0, g_max_len = 0;
  if (int r = grp ? check_prefix_groups(kv, grp, B, S, what, &g_max_rows, &g_max_len) : check_extend_span(kv, B, S, t_past, what)) return r;
  if (int r = c->reserve(align_up((size_t)B * S * 4, 256) + 256)) return r;
  int32_t* pos = reinterpret_cast<int32_t*>(c->ws);
  if (grp) pcy_launch_ext_pos_grouped(c->stream, pos, B, S, t_past, grp->d_len, grp->d_row_grp);
  else pcy_launch_ext_pos(c->stream, pos, B, S, t_past);
  enqueue_extend_attention(c->stream, (bf16_t*)qkv, ld, kv, layer, (bf16_t*)o, ldo, t_past, pos, (const bf16_t*)cos_t, (const bf16_t*)sin_t, keep,
                           B, S, H, Hkv, dh, packed, grp, g_max_rows);
  return check_launch(what);
}

PcyBeamState beam_state_args(const pcy_beam_state* st) {
  PcyBeamState b{};
  b.out = st->out; b.max_len = st->max_len; b.cur = st->cur; b.cur_new = st->cur_new; b.next_tok = st->next_tok; b.src = st->src;
  b.anc = st->anc; b.has_eos = st->has_eos; b.blk_eos = st->blk_eos; b.ticket = st->ticket; b.pos = st->pos; b.step = st->step;
  b.done = st->done; b.eos_id = st->eos_id;
  return b;
}
// row-statistics partials of pcy_beam_step in an allocation of their own: never inside the decode workspace (a captured decode graph points
// into that one, and its tail belongs to the KV-reorder scratch)
int ensure_beam_ws(pcy_ctx* c, int B, int beam) {
  const size_t need = align_up(pcy_beam_ws_bytes(B, beam), 256);
  if (need <= c->beam_ws_bytes) return 0;
  if (c->beam_ws) { HIP_TRY(hipStreamSynchronize(c->stream)); HIP_TRY(hipFree(c->beam_ws)); c->beam_ws = nullptr; c->beam_ws_bytes = 0; }
  c->drop_graph();   // (a captured beam step holds it as a kernel argument)
  HIP_TRY(hipMalloc(reinterpret_cast<void**>(&c->beam_ws), need * 2));
  c->beam_ws_bytes = need * 2;
  return 0;
}

// The part of a graph key that EVERY kind shares, the bf16 steps and the fp32 ones (M / KV: their descriptor and cache; fp: the fingerprint
// of the weight pointers the step reads).  Call it when the workspace is final.  Filled in place behind a memset: the padding bytes take
// part in the comparison.
template <typename M, typename KV>
void key_base(DecodeGraphKey& k, GraphKind kind, int B, const M* m, const KV* kv, const pcy_gen_state* st, const pcy_ctx* c, uint64_t fp) {
  memset(&k, 0, sizeof(k));
  k.kind = kind; k.B = B;
  k.model = m; k.layers = m->layers; k.embed = m->embed; k.kv_k = kv->k; k.kv_v = kv->v; k.Tmax = kv->Tmax; k.kv_B = kv->B;
  k.pos = st->pos; k.step = st->step; k.next_tok = st->next_tok; k.logits = st->logits;
  k.ws = c->ws; k.layers_fp = fp;
  if (st->finished) { k.stop_finished = st->finished; k.stop_done = st->done; k.stop_n_steps_run = st->n_steps_run; k.stop_eos_id = st->eos_id; }
}
// ... and what enqueue_decode reads on top (call after ensure_decode_state: the context's buffers are final)
void decode_graph_key(DecodeGraphKey& k, const pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, GraphKind kind, const PcySwitches& sw) {
  key_base(k, kind, B, m, kv, st, c, c->layers_fp);
  k.sw = sw; k.keep = st->keep;
  if (kv_shared(kv)) { k.kv_prefix_k = kv->prefix_k; k.kv_prefix_v = kv->prefix_v; k.kv_prefix_T = kv->prefix_T; k.kv_prefix_B = kv->prefix_B; k.kv_rows_per_prefix = kv->rows_per_prefix; }
  k.mc_tags = c->mc_tags; k.mb_flags = c->mb_flags; k.nb_tags = B <= 8 ? c->nb_tags[B] : nullptr; k.dev_layers = c->dev_layers;
}
// a pick behind the step (greedy, sampling): where it records
void key_record(DecodeGraphKey& k, const pcy_gen_state* st) {
  k.tokens_out = st->tokens_out; k.logprob = st->logprob; k.logits_all = st->logits_all; k.logits_all_ld = st->logits_all_ld; k.max_steps = st->max_steps;
}
// a beam-search chain: the beam state by value, its record and scratch, its parameters
void key_beam(DecodeGraphKey& k, const pcy_beam_state* bs, const void* logits_rec, const void* beam_ws, int beam, int group_size, int kv_t0, float penalty) {
  memcpy(&k.beam_state, bs, sizeof(*bs)); k.logits_rec = logits_rec; k.beam_ws = beam_ws; k.beam = beam; k.group_size = group_size; k.kv_t0 = kv_t0;
  memcpy(&k.penalty_bits, &penalty, 4);
}
// THE step driver: `enqueue` puts the launches of ONE step on c->stream.  Eager: n_steps times, launch by launch.  use_graph: captured once per
// key, then replayed n_steps times.  Everything that allocates (workspace, beam scratch, sample state, sync words) happens before the call.
template <typename Enqueue>
int run_steps(pcy_ctx* c, int n_steps, bool use_graph, const char* what, const DecodeGraphKey& key, Enqueue&& enqueue) {
  if (!use_graph) {
    for (int i = 0; i < n_steps; ++i) enqueue();
    return check_launch(what);
  }
  if (!c->graph || memcmp(&key, &c->graph_key, sizeof(key)) != 0) {
    c->drop_graph();
    hipGraph_t g = nullptr;
    hipStream_t user = c->stream;
    c->stream = c->cap_stream;
    hipError_t e0 = hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal);
    if (e0 == hipSuccess) {
      enqueue();
      e0 = hipStreamEndCapture(c->cap_stream, &g);
    }
    c->stream = user;
    if (e0 != hipSuccess) return fail(2, "%s graph capture failed: %s", what, hipGetErrorString(e0));
    HIP_TRY(hipGraphInstantiate(&c->graph, g, nullptr, nullptr, 0));
    hipGraphDestroy(g);
    memcpy(&c->graph_key, &key, sizeof(key));
  }
  for (int i = 0; i < n_steps; ++i) HIP_TRY(hipGraphLaunch(c->graph, c->stream));
  return 0;
}

// ---- what the step entries refuse, each rule in ONE place; `what` names the entry that was called ----
// the descriptors a step dereferences, and the rows
int check_step_args(const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, const char* what) {
  if (!m || !kv || !st || !kv->k || !kv->v || !st->pos || !st->next_tok || !st->logits) return fail(1, "%s: model, cache or state incomplete", what);
  if (B < 1 || B > kv->B) return fail(1, "%s: B=%d outside [1, cache rows %d]", what, B, kv->B);
  return 0;
}
// a beam-search step, bf16 or fp32 logits
int check_beam_args(const char* what, int B, int beam, int group_size, int vocab) {
  if (B <= 0 || beam <= 0 || beam > 32 || group_size <= 0 || beam % group_size)
    return fail(1, "%s: B=%d, beam=%d (1..32) must be a multiple of group_size=%d", what, B, beam, group_size);
  if (vocab <= 0 || vocab > 163840) return fail(1, "%s: vocab %d unsupported (<= 163840)", what, vocab);
  return 0;
}
// a sampling pick (max_vocab: what its selection kernel covers); the comparisons refuse a NaN
int check_sample_args(const char* what, int vocab, int max_vocab, float temperature, float nucleus_prob, const float* uniforms) {
  if (!(temperature > 0.f)) return fail(1, "%s: temperature must be > 0 (the greedy pick is an entry of its own)", what);
  if (!(nucleus_prob < 1.f)) return fail(1, "%s: nucleus_prob must be < 1 (<= 0 switches the nucleus mask off)", what);
  if (!uniforms) return fail(1, "%s: no uniform variates", what);
  if (vocab < 1 || vocab > max_vocab) return fail(1, "%s: vocab %d unsupported (<= %d)", what, vocab, max_vocab);
  return 0;
}
// a complete shared-prefix cache with a uniform rows_per_prefix and a geometry the many-queries attention covers: anything else is the caller's error
int check_mq_cache(const pcy_kv_cache* kv, int B, int H, int Hkv, int dh, const char* what) {
  if (!kv_shared(kv)) return fail(1, "%s: the cache has no shared prefix (plain caches: the decode attention)", what);
  if (kv->rows_per_prefix == 0) return fail(1, "%s: a grouped cache (rows_per_prefix == 0) is read by the extension entries only", what);
  if (int r = check_shared_cache(kv, B, what)) return r;
  if (int r = check_heads(what, H, Hkv, dh, false)) return r;
  if (!pcy_attn_mq_covers(H, Hkv, dh, kv->Tmax)) return fail(1, "%s: the scores of %d suffix slots do not fit in LDS", what, kv->Tmax);
  return 0;
}
// THE prologue of the bf16 entries that enqueue the step (enqueue_decode), in this order -- plan_decode reads the context state that
// ensure_decode_state builds: the call's descriptors and rows, the workspace (ws_bytes: step_ws_bytes, reorder_ws_bytes or split_step_ws_bytes),
// ONE switch snapshot (*sw), the context state, what the cache asks of the step's plan.  No launch before it.
// split (the steps on the split-key attention) asks beyond that for a complete shared-prefix cache with a uniform rows_per_prefix >= 1 and a
// geometry the attention covers -- before the workspace, whose size is a function of them -- and for bf16 projections.
int decode_prologue(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, const char* what,
                    size_t (*ws_bytes)(const pcy_llama_desc*, const pcy_kv_cache*, int), PcySwitches* sw, bool split = false) {
  if (int r = check_step_args(m, kv, st, B, what)) return r;
  if (split)
    if (int r = check_mq_cache(kv, B, m->n_heads, m->n_kv_heads, m->head_dim, what)) return r;
  if (int r = c->reserve(ws_bytes(m, kv, B))) return r;
  *sw = pcy_read_switches();
  if (int r = ensure_decode_state(c, m, B, *sw)) return r;
  if (int r = check_decode_cache(c, m, kv, B, *sw, what)) return r;
  if (split && m->layers_fp8) return fail(1, "%s: fp8 projections are not supported on this step", what);
  return 0;
}
}  // namespace
extern "C" {
int pcy_llama_prefill(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const void* embeds, const uint8_t* keep,
                      const int32_t* pos, const int32_t* cu, const int32_t* vt_cu, int B, int T, const int32_t* logit_rows,
                      int n_logit_rows, void* logits_out, void* hidden_out, const int32_t* sum_rows, int n_sum_rows,
                      void* hidden_sum_out) {
  PrefillReq r{};
  r.embeds = embeds; r.keep = keep; r.pos = pos; r.cu = cu; r.vt_cu = vt_cu; r.B = B; r.T = T; r.logit_rows = logit_rows; r.n_logit_rows = n_logit_rows;
  r.logits_out = logits_out; r.hidden_out = hidden_out; r.sum_rows = sum_rows; r.n_sum_rows = n_sum_rows; r.hidden_sum_out = hidden_sum_out;
  return llama_prefill_impl(c, m, kv, r);
}
int pcy_llama_prefill_all(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const void* embeds, const uint8_t* keep,
                          const int32_t* pos, const int32_t* cu, const int32_t* vt_cu, int B, int T, const int32_t* logit_rows,
                          int n_logit_rows, void* logits_out, void* hidden_all_out) {
  if (!hidden_all_out) return fail(1, "pcy_llama_prefill_all: hidden_all_out is NULL");
  PrefillReq r{};
  r.embeds = embeds; r.keep = keep; r.pos = pos; r.cu = cu; r.vt_cu = vt_cu; r.B = B; r.T = T;
  r.logit_rows = logit_rows; r.n_logit_rows = n_logit_rows; r.logits_out = logits_out; r.hidden_all_out = hidden_all_out;
  return llama_prefill_impl(c, m, kv, r);
}
int pcy_llama_score(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const void* embeds, const uint8_t* keep, const int32_t* pos,
                    const int32_t* cu, const int32_t* vt_cu, int B, int T, const int32_t* score_rows, const int32_t* targets, int n_score,
                    float* nll_out, const int32_t* logit_rows, int n_logit_rows, void* logits_out) {
  PrefillReq r{};
  r.embeds = embeds; r.keep = keep; r.pos = pos; r.cu = cu; r.vt_cu = vt_cu; r.B = B; r.T = T; r.logit_rows = logit_rows; r.n_logit_rows = n_logit_rows;
  r.logits_out = logits_out; r.score = ScoreReq{score_rows, targets, n_score, nll_out};
  return llama_prefill_impl(c, m, kv, r);
}
int pcy_llama_extend(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const void* embeds, const uint8_t* keep, int B, int S, int t_past,
                     const int32_t* logit_rows, int n_logit_rows, void* logits_out, void* hidden_out, const int32_t* score_rows,
                     const int32_t* targets, int n_score, float* nll_out) {
  return llama_prefill_impl(c, m, kv, extend_req(embeds, keep, B, S, ExtendReq{true, t_past, false}, logit_rows, n_logit_rows, logits_out, hidden_out,
                                                 score_rows, targets, n_score, nll_out));
}
int pcy_llama_extend_packed(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const void* embeds, const uint8_t* keep, int B, int S,
                            int t_past, const int32_t* logit_rows, int n_logit_rows, void* logits_out, void* hidden_out,
                            const int32_t* score_rows, const int32_t* targets, int n_score, float* nll_out) {
  return llama_prefill_impl(c, m, kv, extend_req(embeds, keep, B, S, ExtendReq{true, t_past, true}, logit_rows, n_logit_rows, logits_out, hidden_out,
                                                 score_rows, targets, n_score, nll_out));
}
int pcy_llama_extend_grouped(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_prefix_groups* groups, const void* embeds,
                             const uint8_t* keep, int B, int S, int packed, const int32_t* logit_rows, int n_logit_rows, void* logits_out,
                             void* hidden_out, const int32_t* score_rows, const int32_t* targets, int n_score, float* nll_out) {
  if (!groups) return fail(1, "pcy_llama_extend_grouped: group tables missing");
  return llama_prefill_impl(c, m, kv, extend_req(embeds, keep, B, S, ExtendReq{true, groups->t_own, packed != 0, groups}, logit_rows, n_logit_rows,
                                                 logits_out, hidden_out, score_rows, targets, n_score, nll_out));
}
unsigned long long pcy_debug_extend_grouped_count(void) { return g_pcy_extend_grouped; }
int pcy_attn_extend_grouped(pcy_ctx* c, void* qkv, int ld, const pcy_kv_cache* kv, const pcy_prefix_groups* groups, int layer, void* o, int ldo,
                            const void* cos_t, const void* sin_t, const uint8_t* keep, int B, int S, int H, int Hkv, int dh, int packed) {
  if (!groups) return fail(1, "pcy_attn_extend_grouped: group tables missing");
  return attn_extend_entry(c, qkv, ld, kv, groups, layer, o, ldo, groups->t_own, cos_t, sin_t, keep, B, S, H, Hkv, dh, packed != 0);
}
size_t pcy_llama_extend_ws_bytes(const pcy_llama_desc* m, int B, int S, int n_logit_rows, int n_score) {
  if (!m || B < 1 || S < 1) return 0;
  return carve_prefill_ws(nullptr, m, B * S, 0, n_logit_rows > 0 ? n_logit_rows : 0, 0, n_score > 0 ? n_score : 0, false, true).bytes;   // (no transposed V, no fp8, no sum rows)
}
int pcy_attn_extend(pcy_ctx* c, void* qkv, int ld, const pcy_kv_cache* kv, int layer, void* o, int ldo, int t_past, const void* cos_t,
                    const void* sin_t, const uint8_t* keep, int B, int S, int H, int Hkv, int dh) {
  return attn_extend_entry(c, qkv, ld, kv, nullptr, layer, o, ldo, t_past, cos_t, sin_t, keep, B, S, H, Hkv, dh, false);
}
int pcy_attn_extend_packed(pcy_ctx* c, void* qkv, int ld, const pcy_kv_cache* kv, int layer, void* o, int ldo, int t_past, const void* cos_t,
                           const void* sin_t, const uint8_t* keep, int B, int S, int H, int Hkv, int dh) {
  return attn_extend_entry(c, qkv, ld, kv, nullptr, layer, o, ldo, t_past, cos_t, sin_t, keep, B, S, H, Hkv, dh, true);
}

int pcy_llama_decode(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B) {
  PCY_STICKY(c);
  PcySwitches sw;
  if (int r = decode_prologue(c, m, kv, st, B, "pcy_llama_decode", step_ws_bytes, &sw)) return r;
  enqueue_decode(c, m, kv, st, B, sw);
  return check_launch("pcy_llama_decode");
}

int pcy_llama_decode_layers(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, int reps) {
  PCY_STICKY(c);
  PcySwitches sw;
  if (int r = decode_prologue(c, m, kv, st, B, "pcy_llama_decode_layers", step_ws_bytes, &sw)) return r;
  return run_steps(c, reps, false, "pcy_llama_decode_layers", DecodeGraphKey{}, [&] { enqueue_decode(c, m, kv, st, B, sw, true); });
}

int pcy_greedy_pick(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, int advance_pos) {
  PCY_STICKY(c);
  if (int r = check_stop(st, m->vocab, "pcy_greedy_pick")) return r;
  if (int r = c->reserve(decode_ws_bytes(m, B, kv_cap(kv)))) return r;
  enqueue_pick(c, m, st, B, advance_pos, kv_cap(kv));
  return check_launch("pcy_greedy_pick");
}

// ---- greedy decoding with lookahead (kernels: pcy_lookahead.hip) ----
static int look_args(const char* what, const pcy_look_state* ls, const pcy_gen_state* st, PcyLookArgs* a) {
  if (!ls || !st) return fail(1, "%s: state missing", what);
  if (ls->W < 2 || ls->W > 32) return fail(1, "%s: W=%d outside [2, 32]", what, ls->W);
  if (ls->ngram_min < 1 || ls->ngram_max < ls->ngram_min || ls->ngram_max > 16)
    return fail(1, "%s: n-gram range [%d, %d] (1 <= min <= max <= 16)", what, ls->ngram_min, ls->ngram_max);
  if (ls->cap < 1 || !ls->hist || !ls->n_hist || !ls->window || !ls->counters || !ls->last) return fail(1, "%s: history / window / counters missing", what);
  if (!st->pos || !st->step || !st->next_tok || !st->tokens_out || !st->logprob || st->max_steps < 1) return fail(1, "%s: generation state incomplete", what);
  *a = PcyLookArgs{ls->hist, ls->n_hist, ls->window, ls->forced, ls->counters, ls->last, ls->cap, ls->W, ls->ngram_max, ls->ngram_min,
                   st->pos, st->step, st->next_tok, st->tokens_out, st->logprob, st->max_steps};
  return 0;
}
int pcy_look_draft(pcy_ctx* c, const pcy_llama_desc* m, const pcy_look_state* ls, const pcy_gen_state* st, void* embeds_out) {
  PCY_STICKY(c);
  PcyLookArgs a;
  if (int r = look_args("pcy_look_draft", ls, st, &a)) return r;
  if (!embeds_out) return fail(1, "pcy_look_draft: embeds_out is NULL");
  if (m->d % 8) return fail(1, "pcy_look_draft: d %% 8 != 0");
  pcy_launch_look_draft(c->stream, a, (const bf16_t*)m->embed, m->vocab, m->d, (bf16_t*)embeds_out);
  ++g_pcy_look[0];
  return check_launch("pcy_look_draft");
}
int pcy_look_verify(pcy_ctx* c, const pcy_llama_desc* m, const pcy_look_state* ls, const pcy_gen_state* st, const void* logits) {
  PCY_STICKY(c);
  PcyLookArgs a;
  if (int r = look_args("pcy_look_verify", ls, st, &a)) return r;
  if (!logits) return fail(1, "pcy_look_verify: logits is NULL");
  if (int r = check_stop(st, m->vocab, "pcy_look_verify")) return r;
  if (int r = c->reserve(pcy_look_verify_ws_bytes(a.W))) return r;
  pcy_launch_look_verify(c->stream, a, (const bf16_t*)logits, m->vocab, (bf16_t*)st->logits_all, st->logits_all_ld, c->ws, stop_of(st));
  ++g_pcy_look[1];
  return check_launch("pcy_look_verify");
}
unsigned long long pcy_debug_look_count(int which) { return (which == 0 || which == 1) ? g_pcy_look[which] : 0; }


int pcy_llama_greedy(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, int n_steps,
                     int use_graph) {
  PCY_STICKY(c);
  PcySwitches sw;
  if (m) if (int r = check_stop(st, m->vocab, "pcy_llama_greedy")) return r;
  if (int r = decode_prologue(c, m, kv, st, B, "pcy_llama_greedy", step_ws_bytes, &sw)) return r;
  DecodeGraphKey key;
  decode_graph_key(key, c, m, kv, st, B, KIND_GREEDY, sw);
  key_record(key, st);
  return run_steps(c, n_steps, use_graph != 0, "pcy_llama_greedy", key, [&] {
    enqueue_decode(c, m, kv, st, B, sw);
    enqueue_pick(c, m, st, B, 1, kv_cap(kv));
  });
}

int pcy_llama_decode_graph(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B) {
  PCY_STICKY(c);
  PcySwitches sw;
  if (int r = decode_prologue(c, m, kv, st, B, "pcy_llama_decode_graph", step_ws_bytes, &sw)) return r;
  DecodeGraphKey key;
  decode_graph_key(key, c, m, kv, st, B, KIND_DECODE, sw);
  key_record(key, st);   // (no pick here: as every earlier key of this kind)
  return run_steps(c, 1, true, "pcy_llama_decode_graph", key, [&] { enqueue_decode(c, m, kv, st, B, sw); });
}

// ---- the decode step for more than 32 rows: every projection is ONE GEMM over all B rows ----
// The default loop above cuts a projection into 32-row passes that each stream the whole matrix (pcy_launch_gemv); here the B rows are the M of
// `linear`, the prefill's and the extension's dispatcher: MFMA tiles, the K-split finish and the RMSNorm fused into it, SwiGLU / residual
// epilogues.  The attention is the loop's stand-alone launch (all rows, *pos and the keep mask from device memory, shared-prefix caches).
// The workspace is the decode carve: the pick / sampling launches behind the step find their partials where they expect them.

// mq: the attention launch of every layer is the many-queries one, its buffers behind the decode carve (pcy_llama_decode_gemm_mq)
// split: ... the split-key one, its buffers at split_ws_offset (pcy_llama_decode_gemm_split)
static void enqueue_decode_gemm(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, bool mq, bool split = false) {
  const DecodeCx cx = decode_cx(c, m, kv, st, B);
  char* attn_ws = c->ws + (split ? split_ws_offset(m, kv, B) : align_up(decode_ws_bytes(m, B, kv_cap(kv)), 256));
  const DecodePlan p{};   // (the stand-alone attention: no key split, its own column cut)
  pcy_launch_embed_tokens_dev(c->stream, (const bf16_t*)m->embed, st->next_tok, cx.x, B, m->d);
  int xn_ready = 0;
  enqueue_layers(cx, p, BACKEND_GEMM, split ? ATTN_SPLIT : mq ? ATTN_MQ : ATTN_DECODE, attn_ws, 0, &xn_ready);
  norm_if_needed(cx, true, m->final_norm, &xn_ready);
  linear(c->stream, cx.xn, m->d, (const bf16_t*)m->lm_head, nullptr, nullptr, 0, (bf16_t*)st->logits, m->vocab, B, m->vocab, m->d, EPI_STORE);
  ++g_pcy_decode_gemm;
  if (mq) ++g_pcy_attn_mq;
  if (split) ++g_pcy_attn_split;
}

static int decode_gemm_entry(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, bool mq, bool split = false) {
  PCY_STICKY(c);
  const char* what = split ? "pcy_llama_decode_gemm_split" : mq ? "pcy_llama_decode_gemm_mq" : "pcy_llama_decode_gemm";
  if (int r = check_step_args(m, kv, st, B, what)) return r;
  const int H = m->n_heads, Hkv = m->n_kv_heads, dh = m->head_dim;
  if (m->layers_fp8) return fail(1, "%s: fp8 projections are not supported on this step", what);
  if (kv_shared(kv) && kv->rows_per_prefix == 0) return fail(1, "%s: a grouped cache (rows_per_prefix == 0) is read by the extension entries only", what);
  if (int r = check_shared_cache(kv, B, what)) return r;
  if (int r = check_heads(what, H, Hkv, dh, true)) return r;
  if (int r = check_widths(what, m, 64, false)) return r;
  size_t need = decode_ws_bytes(m, B, kv_cap(kv));
  if (mq || split) {   // (one set of cache and geometry rules for the two attentions on a shared prefix)
    if (int r = check_mq_cache(kv, B, H, Hkv, dh, what)) return r;
    need = split ? split_step_ws_bytes(m, kv, B) : align_up(need, 256) + attn_ws_bytes(ATTN_MQ, kv, B, H, Hkv, dh);
  }
  if (int r = c->reserve(need)) return r;
  enqueue_decode_gemm(c, m, kv, st, B, mq, split);
  return check_launch(what);
}
int pcy_llama_decode_gemm_split(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B) {
  return decode_gemm_entry(c, m, kv, st, B, false, true);
}
unsigned long long pcy_debug_attn_split_count(void) { return g_pcy_attn_split; }
int pcy_attn_split_chunk_keys(int B, int rows_per_prefix, int H, int Hkv, int dh, int prefix_T) {
  if (B < 1 || rows_per_prefix < 1 || Hkv < 1 || H < Hkv || prefix_T < 1) return 0;
  return pcy_attn_split_plan(B, rows_per_prefix, H, Hkv, dh, prefix_T).cblocks * 32;
}
int pcy_llama_decode_gemm(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B) {
  return decode_gemm_entry(c, m, kv, st, B, false);
}
int pcy_llama_decode_gemm_mq(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B) {
  return decode_gemm_entry(c, m, kv, st, B, true);
}
unsigned long long pcy_debug_decode_gemm_count(void) { return g_pcy_decode_gemm; }
unsigned long long pcy_debug_attn_mq_count(void) { return g_pcy_attn_mq; }

// ---- the decode step that streams e4m3 weights: weight-only fp8 projections, 1..8 rows ----
// One launch per stage, the layer loop on its e4m3 back-end: the four projections of a layer are pcy_launch_gemv_w8 launches (RMSNorm fused
// into qkv and gate/up, residual epilogue on o and down), the attention is the loop's stand-alone launch, lm_head stays bf16 on the streaming
// GEMV with the final norm fused.  The workspace is the decode carve.
static uint64_t w8_fingerprint(const pcy_llama_desc* m, const pcy_llama_layer_fp8* w8) {   // as layers_fingerprint
  uint64_t h = fnv1a(FNV_BASIS, {m->final_norm, m->lm_head, m->rope_cos, m->rope_sin});
  for (int l = 0; l < m->n_layers; ++l) {
    const pcy_llama_layer_fp8& Q = w8[l];
    h = fnv1a(h, {Q.wqkv, Q.wo, Q.wgu, Q.wdown, Q.sqkv, Q.so, Q.sgu, Q.sdown});
  }
  return h;
}
static void enqueue_decode_w8(pcy_ctx* c, const pcy_llama_desc* m, const pcy_llama_layer_fp8* w8, const pcy_kv_cache* kv, const pcy_gen_state* st, int B) {
  const DecodeCx cx = decode_cx(c, m, kv, st, B, w8);
  DecodePlan p{};   // (the stand-alone attention: no key split)
  // Its column cut is the one a ONE-row step gets, whatever B: the launcher otherwise widens the cut with Hkv * B, and the order of a row's
  // sums with it -- a row's bits would depend on the batch it sits in (head_dim 128; the other head sizes have one cut).
  p.force_ds = m->n_kv_heads >= 128 ? 128 : m->n_kv_heads >= 32 ? 64 : 16;
  pcy_launch_embed_tokens_dev(c->stream, (const bf16_t*)m->embed, st->next_tok, cx.x, B, m->d);
  int xn_ready = 0;
  enqueue_layers(cx, p, BACKEND_W8, ATTN_DECODE, nullptr, 0, &xn_ready);
  enqueue_lm_head(cx, p, st->logits, xn_ready, true);
  ++g_pcy_decode_w8;
}
// everything pcy_llama_decode_w8 / pcy_llama_greedy_w8 refuse; reserves the workspace behind the checks
static int decode_w8_check(pcy_ctx* c, const pcy_llama_desc* m, const pcy_llama_layer_fp8* w8, const pcy_kv_cache* kv, const pcy_gen_state* st, int B,
                           const char* what) {
  if (!m || !kv || !st || !kv->k || !kv->v || !st->pos || !st->next_tok || !st->logits || !m->layers) return fail(1, "%s: model, cache or state incomplete", what);
  if (!w8) return fail(1, "%s: w8 is NULL (the e4m3 copies of the projections are passed explicitly)", what);
  for (int l = 0; l < m->n_layers; ++l) {
    const pcy_llama_layer_fp8& Q = w8[l];
    if (!Q.wqkv || !Q.wo || !Q.wgu || !Q.wdown || !Q.sqkv || !Q.so || !Q.sgu || !Q.sdown) return fail(1, "%s: w8 layer %d holds a NULL pointer", what, l);
    if (((uintptr_t)Q.wqkv | (uintptr_t)Q.wo | (uintptr_t)Q.wgu | (uintptr_t)Q.wdown) & 15) return fail(1, "%s: w8 layer %d: matrices must be 16-byte aligned", what, l);
  }
  const int d = m->d, H = m->n_heads, Hkv = m->n_kv_heads, dh = m->head_dim, F = m->ffn;
  const int bmax = kv->B < 8 ? kv->B : 8;
  if (B < 1 || B > bmax) return fail(1, "%s: B=%d outside [1, min(8, cache rows %d)]", what, B, kv->B);
  if (kv_shared(kv)) return fail(1, "%s: a shared-prefix or grouped cache is not served by this step (plain caches only)", what);
  if (int r = check_heads(what, H, Hkv, dh, true)) return r;
  if (int r = check_widths(what, m, 16, true)) return r;
  if ((size_t)d * 2 * 4 > 65536) return fail(1, "%s: d=%d: the fused final norm of lm_head needs 4 rows of x in 64 KiB of LDS", what, d);
  if (pcy_gemv_w8_rows_per_pass(d) < 1 || pcy_gemv_w8_rows_per_pass(F) < 1 || pcy_gemv_w8_rows_per_pass(H * dh) < 1)
    return fail(1, "%s: a row of x (d, ffn or H*dh elements) does not fit in LDS", what);
  return c->reserve(decode_ws_bytes(m, B, kv_cap(kv)));
}
int pcy_llama_decode_w8(pcy_ctx* c, const pcy_llama_desc* m, const pcy_llama_layer_fp8* w8, const pcy_kv_cache* kv, const pcy_gen_state* st, int B) {
  PCY_STICKY(c);
  if (int r = decode_w8_check(c, m, w8, kv, st, B, "pcy_llama_decode_w8")) return r;
  enqueue_decode_w8(c, m, w8, kv, st, B);
  return check_launch("pcy_llama_decode_w8");
}
int pcy_llama_greedy_w8(pcy_ctx* c, const pcy_llama_desc* m, const pcy_llama_layer_fp8* w8, const pcy_kv_cache* kv, const pcy_gen_state* st, int B,
                        int n_steps, int use_graph) {
  PCY_STICKY(c);
  if (m) if (int r = check_stop(st, m->vocab, "pcy_llama_greedy_w8")) return r;
  if (int r = decode_w8_check(c, m, w8, kv, st, B, "pcy_llama_greedy_w8")) return r;
  if (!st->step || !st->tokens_out || !st->logprob) return fail(1, "pcy_llama_greedy_w8: generation state incomplete");
  // (this step reads no switch and none of the fused steps' buffers: the base key, whose fingerprint holds ln1 / ln2 of every layer, the keep
  // mask, and the e4m3 pointers through a fingerprint of their own; a shared-prefix cache never gets here)
  DecodeGraphKey key;
  key_base(key, KIND_GREEDY_W8, B, m, kv, st, c, layers_fingerprint(m));
  key.keep = st->keep; key.w8 = w8; key.w8_fp = w8_fingerprint(m, w8);
  key_record(key, st);
  return run_steps(c, n_steps, use_graph != 0, "pcy_llama_greedy_w8", key, [&] {
    enqueue_decode_w8(c, m, w8, kv, st, B);
    enqueue_pick(c, m, st, B, 1, kv_cap(kv));
  });
}
unsigned long long pcy_debug_decode_w8_count(void) { return g_pcy_decode_w8; }

// ---- fp32 generation: the device-resident decode step on the streaming fp32 GEMV (kernels: pcy_f32_gemv.hip) ----
// One launch per stage, every kernel an ordinary grid: token gather; per layer RMSNorm -> qkv -> attention (rope + append + softmax at *pos)
// -> o (+ residual) -> RMSNorm -> gate / up (SwiGLU) -> down (+ residual); final RMSNorm; lm_head.  next_tok and *pos come from device memory,
// so the chain can be captured once and replayed.
struct F32StreamCx { float *x, *xn, *qkv, *ao, *act; };
static F32StreamCx f32_stream_carve(char* ws, const pcy_f32_llama_desc* m, int B) {
  Carver cv(ws);
  F32StreamCx cx;
  cx.x = cv.take<float>((size_t)B * m->d);
  cx.xn = cv.take<float>((size_t)B * m->d);
  cx.qkv = cv.take<float>((size_t)B * (m->n_heads + 2 * m->n_kv_heads) * m->head_dim);
  cx.ao = cv.take<float>((size_t)B * m->n_heads * m->head_dim);
  cx.act = cv.take<float>((size_t)B * m->ffn);
  return cx;
}
static size_t f32_stream_ws_bytes(const pcy_f32_llama_desc* m, int B) {
  const size_t f = (size_t)B * (2 * (size_t)m->d + (size_t)(2 * m->n_heads + 2 * m->n_kv_heads) * m->head_dim + (size_t)m->ffn) * sizeof(float);
  return f + 8 * 256;
}
static uint64_t f32_stream_fingerprint(const pcy_f32_llama_desc* m) {   // every weight pointer the step reads, as layers_fingerprint
  uint64_t h = fnv1a(FNV_BASIS, {m->embed, m->final_norm, m->lm_head, m->rope_cos, m->rope_sin});
  for (int l = 0; l < m->n_layers; ++l) {
    const pcy_f32_llama_layer& L = m->layers[l];
    h = fnv1a(h, {L.wqkv, L.wo, L.wg, L.wu, L.wd, L.ln1, L.ln2});
  }
  return h;
}
static PcyF32GemvArgs f32_gemv_args(const float* W, const float* W2, const float* x, int K, float* y, int N, int B, int epi) {
  PcyF32GemvArgs g{};
  g.W = W; g.W2 = W2; g.x = x; g.y = y; g.N = N; g.K = K; g.B = B; g.ldx = K; g.ldy = N; g.ldr = N; g.epi = epi;
  if (epi == EPI_RESID) g.resid = y;
  return g;
}
static void enqueue_decode_f32(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const pcy_gen_state* st, int B) {
  hipStream_t s = c->stream;
  const int d = m->d, H = m->n_heads, Hkv = m->n_kv_heads, dh = m->head_dim, F = m->ffn;
  const int qkvw = (H + 2 * Hkv) * dh, kw = Hkv * dh;
  const F32StreamCx cx = f32_stream_carve(c->ws, m, B);
  const size_t layer_stride = (size_t)kv->B * kv->Tmax * kw;
  const float scale = 1.0f / sqrtf((float)dh);
  pcy_launch_f32_embed_dev(s, m->embed, st->next_tok, cx.x, B, d);
  for (int l = 0; l < m->n_layers; ++l) {
    const pcy_f32_llama_layer& L = m->layers[l];
    pcy_launch_f32_rmsnorm(s, cx.x, L.ln1, cx.xn, B, d, m->rms_eps);
    pcy_launch_f32_gemv(s, f32_gemv_args(L.wqkv, nullptr, cx.xn, d, cx.qkv, qkvw, B, EPI_STORE));
    pcy_launch_f32_attn_decode_pos(s, cx.qkv, qkvw, kv->k + l * layer_stride, kv->v + l * layer_stride, kw, kv->Tmax, cx.ao, H * dh, st->pos, m->rope_cos,
                                   m->rope_sin, B, H, Hkv, dh, scale);
    pcy_launch_f32_gemv(s, f32_gemv_args(L.wo, nullptr, cx.ao, H * dh, cx.x, d, B, EPI_RESID));
    pcy_launch_f32_rmsnorm(s, cx.x, L.ln2, cx.xn, B, d, m->rms_eps);
    pcy_launch_f32_gemv(s, f32_gemv_args(L.wg, L.wu, cx.xn, d, cx.act, F, B, EPI_SWIGLU));
    pcy_launch_f32_gemv(s, f32_gemv_args(L.wd, nullptr, cx.act, F, cx.x, d, B, EPI_RESID));
  }
  pcy_launch_f32_rmsnorm(s, cx.x, m->final_norm, cx.xn, B, d, m->rms_eps);
  pcy_launch_f32_gemv(s, f32_gemv_args(m->lm_head, nullptr, cx.xn, d, (float*)st->logits, m->vocab, B, EPI_STORE));
  ++g_pcy_f32_stream;
}
static void enqueue_pick_f32(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_gen_state* st, int B, int advance_pos) {
  pcy_launch_f32_pick(c->stream, (const float*)st->logits, B, m->vocab, st->next_tok, st->tokens_out, st->max_steps, st->logprob, st->pos, st->step,
                      advance_pos, (float*)st->logits_all, st->logits_all_ld, stop_of(st));
}
// everything the fp32 step entries refuse; reserves the workspace behind the checks
static int f32_stream_check(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const pcy_gen_state* st, int B, bool pick, const char* what) {
  if (!m || !kv || !st || !kv->k || !kv->v || !st->pos || !st->next_tok || !st->logits || !m->layers || !m->embed || !m->final_norm || !m->lm_head ||
      !m->rope_cos || !m->rope_sin)
    return fail(1, "%s: model, cache or state incomplete", what);
  if (pick && (!st->step || !st->tokens_out || !st->logprob || st->max_steps < 1)) return fail(1, "%s: generation state incomplete", what);
  if (pick) if (int r = check_stop(st, m->vocab, what)) return r;
  if (st->keep) return fail(1, "%s: keep must be NULL (the fp32 step attends every slot, as the reference does after the prefill)", what);
  const int d = m->d, H = m->n_heads, Hkv = m->n_kv_heads, dh = m->head_dim, F = m->ffn;
  if (m->n_layers < 1 || m->vocab < 1 || d < 4 || F < 4) return fail(1, "%s: geometry incomplete", what);
  for (int l = 0; l < m->n_layers; ++l) {
    const pcy_f32_llama_layer& L = m->layers[l];
    if (!L.wqkv || !L.wo || !L.wg || !L.wu || !L.wd || !L.ln1 || !L.ln2) return fail(1, "%s: layer %d holds a NULL pointer", what, l);
    if (((uintptr_t)L.wqkv | (uintptr_t)L.wo | (uintptr_t)L.wg | (uintptr_t)L.wu | (uintptr_t)L.wd) & 15) return fail(1, "%s: layer %d: matrices must be 16-byte aligned", what, l);
  }
  if (((uintptr_t)m->lm_head | (uintptr_t)kv->k | (uintptr_t)kv->v) & 15) return fail(1, "%s: lm_head and the caches must be 16-byte aligned", what);
  if (B < 1 || B > kv->B || B > 65535) return fail(1, "%s: B=%d outside [1, cache rows %d]", what, B, kv->B);
  if (dh != 16 && dh != 64 && dh != 128) return fail(1, "%s: head_dim %d unsupported (16/64/128)", what, dh);
  if (Hkv < 1 || H < 1 || H % Hkv) return fail(1, "%s: Hkv | H required", what);
  if (d % 4 || F % 4 || (H * dh) % 4) return fail(1, "%s: d, ffn and H*dh must be multiples of 4", what);
  if (kv->Tmax < 1 || kv->Tmax > m->max_pos) return fail(1, "%s: cache capacity %d outside the rotary table (%d)", what, kv->Tmax, m->max_pos);
  if (pcy_f32_attn_pos_lds(H, Hkv, dh, kv->Tmax) > 160 * 1024 - 1024) return fail(1, "%s: %d slots exceed the LDS score buffer of the attention", what, kv->Tmax);
  return c->reserve(f32_stream_ws_bytes(m, B));
}
// the key of an fp32 step: the base, and where the pick behind it records (the greedy and the sampling pick)
static void f32_stream_key(DecodeGraphKey& key, const pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const pcy_gen_state* st, int B, GraphKind kind) {
  key_base(key, kind, B, m, kv, st, c, f32_stream_fingerprint(m));
  if (kind == KIND_F32_GREEDY || kind == KIND_F32_SAMPLE) key_record(key, st);
}
int pcy_f32_llama_decode(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const pcy_gen_state* st, int B) {
  PCY_STICKY(c);
  if (int r = f32_stream_check(c, m, kv, st, B, false, "pcy_f32_llama_decode")) return r;
  enqueue_decode_f32(c, m, kv, st, B);
  return check_launch("pcy_f32_llama_decode");
}
int pcy_f32_llama_decode_graph(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const pcy_gen_state* st, int B) {
  PCY_STICKY(c);
  if (int r = f32_stream_check(c, m, kv, st, B, false, "pcy_f32_llama_decode_graph")) return r;
  DecodeGraphKey key;
  f32_stream_key(key, c, m, kv, st, B, KIND_F32_DECODE);
  return run_steps(c, 1, true, "pcy_f32_llama_decode_graph", key, [&] { enqueue_decode_f32(c, m, kv, st, B); });
}
int pcy_f32_greedy_pick(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const pcy_gen_state* st, int B, int advance_pos) {
  PCY_STICKY(c);
  if (!m || !st || !st->logits || !st->pos || !st->step || !st->next_tok || !st->tokens_out || !st->logprob || st->max_steps < 1)
    return fail(1, "pcy_f32_greedy_pick: generation state incomplete");
  if (B < 1 || B > 65535 || m->vocab < 1 || (kv && B > kv->B)) return fail(1, "pcy_f32_greedy_pick: B=%d", B);
  if (int r = check_stop(st, m->vocab, "pcy_f32_greedy_pick")) return r;
  enqueue_pick_f32(c, m, st, B, advance_pos);
  return check_launch("pcy_f32_greedy_pick");
}
int pcy_f32_llama_greedy(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const pcy_gen_state* st, int B, int n_steps, int use_graph) {
  PCY_STICKY(c);
  if (int r = f32_stream_check(c, m, kv, st, B, true, "pcy_f32_llama_greedy")) return r;
  DecodeGraphKey key;
  f32_stream_key(key, c, m, kv, st, B, KIND_F32_GREEDY);
  return run_steps(c, n_steps, use_graph != 0, "pcy_f32_llama_greedy", key, [&] {
    enqueue_decode_f32(c, m, kv, st, B);
    enqueue_pick_f32(c, m, st, B, 1);
  });
}
unsigned long long pcy_debug_f32_stream_count(void) { return g_pcy_f32_stream; }

// ---- fp32 selection on the device (pcy_f32_select.hip): beam search and sampling of an fp32 generation without a host
// round trip.  Workspace of the context: [the stream step's carve for the rows][behind it, from a 256-byte boundary: the K / V reorder
// scratch of a beam search, or the partials and probability rows of a sampling step].  Everything is reserved before a capture.
static int f32_beam_check(const char* what, const void* logits_or_state, int vocab, int B, int beam, int group_size, const pcy_beam_state* bs) {
  if (!logits_or_state || !bs || !bs->out || !bs->cur || !bs->cur_new || !bs->next_tok || !bs->src || !bs->has_eos || !bs->blk_eos || !bs->ticket ||
      !bs->pos || !bs->step || !bs->done || bs->max_len < 1)
    return fail(1, "%s: logits or beam state incomplete", what);
  if (B > 65535) return fail(1, "%s: B=%d exceeds the 65535 prompts of a launch", what, B);
  return check_beam_args(what, B, beam, group_size, vocab);
}
int pcy_f32_beam_step(pcy_ctx* c, const float* logits, int vocab, int B, int beam, int group_size, float diversity_penalty, const pcy_beam_state* bs) {
  PCY_STICKY(c);
  if (int r = f32_beam_check("pcy_f32_beam_step", logits, vocab, B, beam, group_size, bs)) return r;
  if (int r = ensure_beam_ws(c, B, beam)) return r;
  pcy_launch_f32_beam_step(c->stream, logits, vocab, B, beam, group_size, diversity_penalty, beam_state_args(bs), c->beam_ws);
  ++g_pcy_f32_select[0];
  return check_launch("pcy_f32_beam_step");
}
static int f32_kv_check(const char* what, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv) {
  if (!m || !kv || !kv->k || !kv->v || m->n_layers < 1 || m->n_kv_heads < 1 || m->head_dim < 1 || kv->B < 1 || kv->Tmax < 1)
    return fail(1, "%s: model or cache incomplete", what);
  if ((m->n_kv_heads * m->head_dim) % 4 || (((uintptr_t)kv->k | (uintptr_t)kv->v) & 15))
    return fail(1, "%s: cache rows must be multiples of 4 floats and 16-byte aligned", what);
  return 0;
}
static size_t f32_select_ws_offset(const pcy_f32_llama_desc* m, int B) { return align_up(f32_stream_ws_bytes(m, B), 256); }
int pcy_f32_kv_reorder_range(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const int32_t* src_rows, int B, int t0, int t) {
  PCY_STICKY(c);
  if (int r = f32_kv_check("pcy_f32_kv_reorder_range", m, kv)) return r;
  if (!src_rows || B < 1 || B > kv->B || B > 65535) return fail(1, "pcy_f32_kv_reorder_range: B=%d outside [1, cache rows %d] or no row map", B, kv->B);
  if (t0 < 0 || t > kv->Tmax) return fail(1, "pcy_f32_kv_reorder_range: slots [%d, %d) outside the cache's %d", t0, t, kv->Tmax);
  if (t <= t0) return 0;
  const int kw = m->n_kv_heads * m->head_dim;
  const size_t off = f32_select_ws_offset(m, B);
  if (int r = c->reserve(off + pcy_f32_kv_reorder_tmp_bytes(m->n_layers, B, kv->Tmax, t0, kw))) return r;
  pcy_launch_f32_kv_reorder(c->stream, kv->k, kv->v, reinterpret_cast<float*>(c->ws + off), src_rows, m->n_layers, B, kv->B, kv->Tmax, kw, t0, t, nullptr);
  return check_launch("pcy_f32_kv_reorder_range");
}
int pcy_f32_kv_copy_rows(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* dst, const pcy_f32_kv_cache* src, const int32_t* src_rows,
                         int B, int t) {
  PCY_STICKY(c);
  if (int r = f32_kv_check("pcy_f32_kv_copy_rows", m, dst)) return r;
  if (int r = f32_kv_check("pcy_f32_kv_copy_rows", m, src)) return r;
  if (dst->k == src->k || dst->v == src->v || dst->k == src->v || dst->v == src->k) return fail(1, "pcy_f32_kv_copy_rows: out of place only (pcy_f32_kv_reorder_range moves rows inside a cache)");
  if (!src_rows || B < 1 || B > dst->B || B > 65535) return fail(1, "pcy_f32_kv_copy_rows: B=%d outside [1, destination rows %d] or no row map", B, dst->B);
  if (t < 0 || t > dst->Tmax || t > src->Tmax) return fail(1, "pcy_f32_kv_copy_rows: %d slots exceed a cache (%d, %d)", t, dst->Tmax, src->Tmax);
  if (t == 0) return 0;
  pcy_launch_f32_kv_copy_rows(c->stream, dst->k, dst->v, dst->B, dst->Tmax, src->k, src->v, src->B, src->Tmax, src_rows, m->n_layers, B,
                              m->n_kv_heads * m->head_dim, t);
  return check_launch("pcy_f32_kv_copy_rows");
}
// n_steps x (fp32 step -> record row (*step, b) -> beam step -> reorder of slots [kv_t0, *pos)): ONE replayed linear launch chain per step, the
// kernels and bits of pcy_f32_llama_decode_graph + a copy + pcy_f32_beam_step + pcy_f32_kv_reorder_range
int pcy_f32_llama_beam_steps(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const pcy_gen_state* st, int B, int beam, int group_size,
                             float diversity_penalty, const pcy_beam_state* bs, float* logits_rec, int n_steps, int kv_t0) {
  PCY_STICKY(c);
  const char* what = "pcy_f32_llama_beam_steps";
  if (!m) return fail(1, "%s: model missing", what);
  if (int r = f32_beam_check(what, st, m->vocab, B, beam, group_size, bs)) return r;
  const int BB = B * beam;
  if (int r = f32_stream_check(c, m, kv, st, BB, false, what)) return r;
  if (st->pos != bs->pos || st->next_tok != bs->next_tok) return fail(1, "%s: the decode state must read the beam state's position and tokens", what);
  if (kv_t0 < 0 || kv_t0 > kv->Tmax) return fail(1, "%s: kv_t0 = %d outside [0, %d]", what, kv_t0, kv->Tmax);
  if (n_steps <= 0) return 0;
  const int kw = m->n_kv_heads * m->head_dim;
  const size_t off = f32_select_ws_offset(m, BB);
  if (int r = c->reserve(off + pcy_f32_kv_reorder_tmp_bytes(m->n_layers, BB, kv->Tmax, kv_t0, kw))) return r;
  if (int r = ensure_beam_ws(c, B, beam)) return r;
  DecodeGraphKey key;
  f32_stream_key(key, c, m, kv, st, BB, KIND_F32_BEAM);
  key_beam(key, bs, logits_rec, c->beam_ws, beam, group_size, kv_t0, diversity_penalty);
  g_pcy_f32_select[0] += (unsigned long long)n_steps;
  return run_steps(c, n_steps, true, what, key, [&] {
    hipStream_t s = c->stream;
    enqueue_decode_f32(c, m, kv, st, BB);
    pcy_launch_f32_record(s, (const float*)st->logits, logits_rec, bs->step, BB, m->vocab, 0);
    pcy_launch_f32_beam_step(s, (const float*)st->logits, m->vocab, B, beam, group_size, diversity_penalty, beam_state_args(bs), c->beam_ws);
    if (kv_t0 < kv->Tmax)
      pcy_launch_f32_kv_reorder(s, kv->k, kv->v, reinterpret_cast<float*>(c->ws + off), bs->src, m->n_layers, BB, kv->B, kv->Tmax, kw, kv_t0, 0, bs->pos);
  });
}
// record row *step -> the selection -> ++*step (/ ++*pos); the nucleus branch of the reference does not apply the temperature (model_unified.py:899-901)
static void enqueue_sample_f32(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_gen_state* st, int B, int advance_pos, float temperature,
                               float nucleus_prob, const float* uniforms, float* probs_out) {
  hipStream_t s = c->stream;
  const PcyStop stop = stop_of(st);
  pcy_launch_f32_record(s, (const float*)st->logits, (float*)st->logits_all, st->step, B, m->vocab, st->logits_all_ld, stop.done);
  pcy_launch_f32_sample_step(s, (const float*)st->logits, B, m->vocab, nucleus_prob > 0.f ? 1.0f : temperature, nucleus_prob, uniforms, probs_out,
                             st->next_tok, st->tokens_out, st->max_steps, st->logprob, st->step, c->ws + f32_select_ws_offset(m, B), stop);
  pcy_launch_f32_advance(s, st->step, st->pos, advance_pos, stop, B);
}
int pcy_f32_sample_pick(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const pcy_gen_state* st, int B, int advance_pos,
                        float temperature, float nucleus_prob, const float* uniforms, float* probs_out) {
  PCY_STICKY(c);
  if (!m || !st || !st->logits || !st->pos || !st->step || !st->next_tok || !st->tokens_out || !st->logprob || st->max_steps < 1)
    return fail(1, "pcy_f32_sample_pick: generation state incomplete");
  if (B < 1 || B > 65535 || (kv && B > kv->B)) return fail(1, "pcy_f32_sample_pick: B=%d", B);
  if (int r = check_sample_args("pcy_f32_sample_pick", m->vocab, 163840, temperature, nucleus_prob, uniforms)) return r;
  if (int r = check_stop(st, m->vocab, "pcy_f32_sample_pick")) return r;
  if (int r = c->reserve(f32_select_ws_offset(m, B) + pcy_f32_sample_ws_bytes(B, m->vocab))) return r;
  enqueue_sample_f32(c, m, st, B, advance_pos, temperature, nucleus_prob, uniforms, probs_out);
  ++g_pcy_f32_select[1];
  return check_launch("pcy_f32_sample_pick");
}
int pcy_f32_llama_sample(pcy_ctx* c, const pcy_f32_llama_desc* m, const pcy_f32_kv_cache* kv, const pcy_gen_state* st, int B, int n_steps,
                         float temperature, float nucleus_prob, const float* uniforms, int use_graph) {
  PCY_STICKY(c);
  if (int r = f32_stream_check(c, m, kv, st, B, true, "pcy_f32_llama_sample")) return r;
  if (int r = check_sample_args("pcy_f32_llama_sample", m->vocab, 163840, temperature, nucleus_prob, uniforms)) return r;
  if (n_steps <= 0) return 0;
  if (int r = c->reserve(f32_select_ws_offset(m, B) + pcy_f32_sample_ws_bytes(B, m->vocab))) return r;
  g_pcy_f32_select[1] += (unsigned long long)n_steps;
  DecodeGraphKey key;
  f32_stream_key(key, c, m, kv, st, B, KIND_F32_SAMPLE);
  key.uniforms = uniforms;
  memcpy(&key.temperature_bits, &temperature, 4); memcpy(&key.nucleus_bits, &nucleus_prob, 4);
  return run_steps(c, n_steps, use_graph != 0, "pcy_f32_llama_sample", key, [&] {
    enqueue_decode_f32(c, m, kv, st, B);
    enqueue_sample_f32(c, m, st, B, 1, temperature, nucleus_prob, uniforms, nullptr);
  });
}
unsigned long long pcy_debug_f32_select_count(int which) { return (which == 0 || which == 1) ? g_pcy_f32_select[which] : 0; }

int pcy_gemv_w8(pcy_ctx* c, const void* W8, const float* scale, const void* x, int ldx, const void* resid, void* y, int ldy, const void* rms_w,
                float rms_eps, int rms_cast, int N, int K, int B, int epi) {
  PCY_STICKY(c);
  if (!W8 || !scale || !x || !y) return fail(1, "pcy_gemv_w8: W8, scale, x or y is NULL");
  if (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU) return fail(1, "pcy_gemv_w8: epi=%d (STORE, RESID or SWIGLU)", epi);
  if (B < 1 || B > 8) return fail(1, "pcy_gemv_w8: B=%d outside [1, 8]", B);
  if (N < 1 || K < 16 || K % 16) return fail(1, "pcy_gemv_w8: N=%d K=%d (N >= 1, K a positive multiple of 16)", N, K);
  if (ldx % 8 || ldx < K || ldy < N) return fail(1, "pcy_gemv_w8: ldx=%d ldy=%d (ldx %% 8 == 0, rows must hold K / N elements)", ldx, ldy);
  if (((uintptr_t)W8 | (uintptr_t)x) & 15) return fail(1, "pcy_gemv_w8: W8 and x must be 16-byte aligned");
  if (epi == EPI_SWIGLU && N % 16) return fail(1, "pcy_gemv_w8: SWIGLU needs N %% 16 == 0 features (16-row gate/up interleave), got %d", N);
  if (epi == EPI_RESID && (!resid || rms_w)) return fail(1, "pcy_gemv_w8: RESID needs resid and takes no fused RMSNorm");
  if (rms_w && ((uintptr_t)rms_w & 15)) return fail(1, "pcy_gemv_w8: rms_w must be 16-byte aligned");
  if (pcy_gemv_w8_rows_per_pass(K) < 1) return fail(1, "pcy_gemv_w8: K=%d: a row of x does not fit in LDS", K);
  PcyGemvW8Args g{};
  g.W = (const uint8_t*)W8; g.scale = scale; g.x = (const bf16_t*)x; g.y = (bf16_t*)y; g.resid = epi == EPI_RESID ? (const bf16_t*)resid : nullptr;
  g.rms_w = (const bf16_t*)rms_w; g.rms_eps = rms_eps; g.rms_cast = rms_cast; g.N = N; g.K = K; g.B = B; g.ldx = ldx; g.ldy = ldy; g.epi = epi;
  if (!pcy_launch_gemv_w8(c->stream, g)) return fail(1, "pcy_gemv_w8: the device refused the LDS size for K=%d", K);
  return check_launch("pcy_gemv_w8");
}

// ---- the lookahead pass on the decode loop: W consecutive tokens of ONE cache row ----
// what the operator refuses, for the operator entry and the step alike
static int check_win_call(const pcy_kv_cache* kv, int W, int H, int Hkv, int dh, const char* what) {
  if (kv_shared(kv)) return fail(1, "%s: a shared-prefix or grouped cache is not served by the window attention (plain caches only)", what);
  if (kv->B != 1) return fail(1, "%s: the cache holds %d rows (the window is W tokens of ONE row: kv->B == 1)", what, kv->B);
  if (W < 2 || W > 32) return fail(1, "%s: W=%d outside [2, 32]", what, W);
  if (int r = check_heads(what, H, Hkv, dh, false)) return r;   // (H >= 1 follows from Hkv >= 1 and the ratio)
  if (kv->Tmax < W) return fail(1, "%s: the cache holds %d slots, fewer than the %d of a window", what, kv->Tmax, W);
  if (((uintptr_t)kv->k | (uintptr_t)kv->v) & 15) return fail(1, "%s: the cache must be 16-byte aligned", what);
  return 0;
}
// The layer loop at B = W on the GEMV back-end, never a fused step, with the window attention in the place of the decode attention and the
// GEMV's own finish launch; the final norm + lm_head GEMV.
static void enqueue_decode_window(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int W, void* logits_out) {
  const DecodeCx cx = decode_cx(c, m, kv, st, W);
  DecodePlan p{};   // (the loop alone: no fused step, no deferred qkv finish, no rotated K order, no key split)
  p.batched_head = W >= pcy_mfma_min_batch() && m->d % 128 == 0 && m->ffn % 128 == 0;
  p.batched = p.batched_head;
  int xn_ready = 0;
  enqueue_layers(cx, p, BACKEND_GEMV, ATTN_WINDOW, c->ws + align_up(decode_ws_bytes(m, W, kv_cap(kv)), 256), 0, &xn_ready);
  enqueue_lm_head(cx, p, logits_out, xn_ready);
  ++g_pcy_decode_window;
}
int pcy_llama_decode_window(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, const void* embeds, int W,
                            void* logits_out) {
  PCY_STICKY(c);
  const char* what = "pcy_llama_decode_window";
  if (!m || !kv || !st || !kv->k || !kv->v || !st->pos || !m->layers || !embeds || !logits_out) return fail(1, "%s: model, cache, state, embeds or logits_out incomplete", what);
  if (st->keep) return fail(1, "%s: a keep mask is not supported (lookahead prompts are unpadded)", what);
  if (m->layers_fp8) return fail(1, "%s: fp8 projections are not supported on this step", what);
  const int d = m->d, H = m->n_heads, Hkv = m->n_kv_heads, dh = m->head_dim;
  if (int r = check_win_call(kv, W, H, Hkv, dh, what)) return r;
  if (int r = check_widths(what, m, 16, true)) return r;
  const size_t need = align_up(decode_ws_bytes(m, W, kv_cap(kv)), 256) + attn_ws_bytes(ATTN_WINDOW, kv, W, H, Hkv, dh);
  if (int r = c->reserve(need)) return r;
  HIP_TRY(hipMemcpyAsync(carve_decode_ws(c->ws, m, W, kv_cap(kv)).x, embeds, (size_t)W * d * 2, hipMemcpyDeviceToDevice, c->stream));
  enqueue_decode_window(c, m, kv, st, W, logits_out);
  return check_launch(what);
}
unsigned long long pcy_debug_decode_window_count(void) { return g_pcy_decode_window; }
int pcy_attn_window_chunk(void) { return pcy_attn_win_chunk(); }

// The operator entries of the attentions with a workspace of their own: what they share.  An entry states its kind -- the cache check, the
// workspace size and the launcher follow from it (check_win_call / check_mq_cache, attn_ws_bytes, launch_attn).
static int attn_op_entry(pcy_ctx* c, const char* what, AttnKind kind, AttnCall a) {
  PCY_STICKY(c);
  const pcy_kv_cache* kv = a.kv;
  if (!a.qkv || !kv || !kv->k || !kv->v || !a.o || !a.pos || !a.cos_t || !a.sin_t || a.layer < 0) return fail(1, "%s: qkv, cache, o, pos or rope tables missing (layer=%d)", what, a.layer);
  if (kind != ATTN_WINDOW && (a.B < 1 || a.B > kv->B)) return fail(1, "%s: B=%d outside [1, cache rows %d]", what, a.B, kv->B);   // (the window: W, below)
  if (int r = kind == ATTN_WINDOW ? check_win_call(kv, a.B, a.H, a.Hkv, a.dh, what) : check_mq_cache(kv, a.B, a.H, a.Hkv, a.dh, what)) return r;
  if (a.ld % 8 || a.ld < (a.H + 2 * a.Hkv) * a.dh || a.ldo % 8 || a.ldo < a.H * a.dh) return fail(1, "%s: ld=%d ldo=%d (rows must be 16-byte aligned and hold all heads)", what, a.ld, a.ldo);
  if (int r = c->reserve(attn_ws_bytes(kind, kv, a.B, a.H, a.Hkv, a.dh))) return r;
  a.ws = c->ws;
  if (!launch_attn(c->stream, kind, a)) return fail(1, "%s: shape not covered", what);
  return check_launch(what);
}
int pcy_attn_window(pcy_ctx* c, void* qkv, int ld, const pcy_kv_cache* kv, int layer, void* o, int ldo, const int32_t* pos, const void* cos_t,
                    const void* sin_t, int W, int H, int Hkv, int dh) {
  return attn_op_entry(c, "pcy_attn_window", ATTN_WINDOW, AttnCall{(const bf16_t*)qkv, ld, kv, layer, (bf16_t*)o, ldo, pos, (const bf16_t*)cos_t, (const bf16_t*)sin_t, nullptr, W, H, Hkv, dh, nullptr});
}
int pcy_attn_decode_shared(pcy_ctx* c, void* qkv, int ld, const pcy_kv_cache* kv, int layer, void* o, int ldo, const int32_t* pos, const void* cos_t,
                           const void* sin_t, const uint8_t* keep, int B, int H, int Hkv, int dh) {
  return attn_op_entry(c, "pcy_attn_decode_shared", ATTN_MQ, AttnCall{(const bf16_t*)qkv, ld, kv, layer, (bf16_t*)o, ldo, pos, (const bf16_t*)cos_t, (const bf16_t*)sin_t, keep, B, H, Hkv, dh, nullptr});
}
int pcy_attn_decode_split(pcy_ctx* c, void* qkv, int ld, const pcy_kv_cache* kv, int layer, void* o, int ldo, const int32_t* pos, const void* cos_t,
                          const void* sin_t, const uint8_t* keep, int B, int H, int Hkv, int dh) {
  return attn_op_entry(c, "pcy_attn_decode_split", ATTN_SPLIT, AttnCall{(const bf16_t*)qkv, ld, kv, layer, (bf16_t*)o, ldo, pos, (const bf16_t*)cos_t, (const bf16_t*)sin_t, keep, B, H, Hkv, dh, nullptr});
}

int pcy_llama_decode_split(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B) {
  PCY_STICKY(c);
  PcySwitches sw;
  if (int r = decode_prologue(c, m, kv, st, B, "pcy_llama_decode_split", split_step_ws_bytes, &sw, true)) return r;
  enqueue_decode(c, m, kv, st, B, sw, false, true);
  return check_launch("pcy_llama_decode_split");
}

int pcy_sample_pick(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, int advance_pos,
                    float temperature, float nucleus_prob, const float* uniforms, void* probs_out) {
  PCY_STICKY(c);
  if (int r = check_sample_args("pcy_sample_pick", m->vocab, pcy_sample_max_vocab(), temperature, nucleus_prob, uniforms)) return r;
  if (int r = check_stop(st, m->vocab, "pcy_sample_pick")) return r;
  if (int r = c->reserve(decode_ws_bytes(m, B, kv_cap(kv)))) return r;
  if (int r = ensure_sample_state(c, B, m->vocab)) return r;
  enqueue_sample(c, m, st, B, advance_pos, kv_cap(kv), temperature, nucleus_prob, uniforms, (bf16_t*)probs_out);
  return check_launch("pcy_sample_pick");
}

int pcy_llama_sample(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, int n_steps,
                     float temperature, float nucleus_prob, const float* uniforms) {
  PCY_STICKY(c);
  const char* what = "pcy_llama_sample";
  if (int r = check_step_args(m, kv, st, B, what)) return r;   // (ahead of the prologue: the sampling arguments are refused before anything is allocated)
  if (int r = check_sample_args(what, m->vocab, pcy_sample_max_vocab(), temperature, nucleus_prob, uniforms)) return r;
  if (int r = check_stop(st, m->vocab, what)) return r;
  PcySwitches sw;
  if (int r = decode_prologue(c, m, kv, st, B, what, step_ws_bytes, &sw)) return r;
  if (int r = ensure_sample_state(c, B, m->vocab)) return r;
  return run_steps(c, n_steps, false, what, DecodeGraphKey{}, [&] {
    enqueue_decode(c, m, kv, st, B, sw);
    enqueue_sample(c, m, st, B, 1, kv_cap(kv), temperature, nucleus_prob, uniforms, nullptr);
  });
}

int pcy_beam_step(pcy_ctx* c, const void* logits, int vocab, int B, int beam, int group_size, float diversity_penalty,
                  const pcy_beam_state* st) {
  PCY_STICKY(c);
  if (int r = check_beam_args("pcy_beam_step", B, beam, group_size, vocab)) return r;
  if (int r = ensure_beam_ws(c, B, beam)) return r;
  pcy_launch_beam_step(c->stream, (const bf16_t*)logits, vocab, B, beam, group_size, diversity_penalty, beam_state_args(st), c->beam_ws);
  return check_launch("pcy_beam_step");
}

int pcy_kv_reorder(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const int32_t* src_rows, int B, int t) {
  return pcy_kv_reorder_range(c, m, kv, src_rows, B, 0, t);
}
int pcy_kv_reorder_range(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const int32_t* src_rows, int B, int t0, int t) {
  PCY_STICKY(c);
  const int dh = m->head_dim;
  if (!kv_shared(kv) && (t <= 0 || t0 >= t)) return 0;
  if (t0 < 0) return fail(1, "pcy_kv_reorder_range: t0 < 0");
  if (kv_shared(kv)) {   // the rows own their suffix slots only: logical [max(t0, Tp), t) = suffix [max(t0, Tp) - Tp, t - Tp)
    if (!kv->prefix_k || !kv->prefix_v || kv->prefix_T <= 0) return fail(1, "pcy_kv_reorder: malformed shared-prefix cache");
    const int Tp = kv->prefix_T;
    t0 = (t0 > Tp ? t0 : Tp) - Tp;
    t -= Tp;
    if (t > kv->Tmax) return fail(1, "pcy_kv_reorder: %d suffix slots exceed the cache's %d", t, kv->Tmax);
  }
  if (t <= 0 || t0 >= t) return 0;
  if ((t * dh) % 8 || (t0 * dh) % 8) return fail(1, "pcy_kv_reorder: t * head_dim (and t0 * head_dim) must be multiples of 8");
  if (int r = c->reserve(reorder_ws_bytes(m, kv, B))) return r;
  enqueue_kv_reorder(c->stream, m, kv, src_rows, B, t, nullptr, t0, 0, reorder_scratch(c, m, kv, B));
  return check_launch("pcy_kv_reorder");
}

// Steps 1 .. of the diverse beam search as ONE replayed launch chain per step: decode step (the graph of pcy_llama_decode_graph's launches)
// -> record of the step's logits (row (step, b) of logits_rec, step read from the device) -> pcy_beam_step -> pcy_kv_reorder over the
// slots the position counter names.  Same kernels, same order, same bits as the four calls (PCY_DISABLE=beam_graph: the callers keep
// them); it removes the ~12 launch boundaries of a step (3.43 -> see DESIGN.md ms per step at beam 5).
// split: the decode step of the chain is pcy_llama_decode_split's (pcy_llama_beam_steps_split)
static int beam_steps_entry(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, int beam, int group_size,
                            float diversity_penalty, const pcy_beam_state* bs, void* logits_rec, int n_steps, int kv_t0, bool split) {
  PCY_STICKY(c);
  const char* what = split ? "pcy_llama_beam_steps_split" : "pcy_llama_beam_steps";
  if (!m || !kv || !st || !bs) return fail(1, "%s: model, cache or state incomplete", what);
  if (kv_t0 < 0 || (kv_t0 * m->head_dim) % 8) return fail(1, "%s: kv_t0 = %d (>= 0, kv_t0 * head_dim a multiple of 8)", what, kv_t0);
  if (int r = check_beam_args(what, B, beam, group_size, m->vocab)) return r;
  const int BB = B * beam;
  if (BB > kv->B) return fail(1, "%s: %d rows exceed cache rows %d", what, BB, kv->B);
  if (st->pos != bs->pos || st->next_tok != bs->next_tok) return fail(1, "%s: the decode state must read the beam state's position and tokens", what);
  if ((kv->Tmax * m->head_dim) % 8) return fail(1, "%s: Tmax * head_dim must be a multiple of 8", what);
  if (split)   // (ahead of the prologue: refused for any n_steps)
    if (int r = check_mq_cache(kv, BB, m->n_heads, m->n_kv_heads, m->head_dim, what)) return r;
  if (n_steps <= 0) return 0;
  // everything the chain allocates, before the capture: decode workspace + the reorder scratch behind it (+ behind that the partial sums and
  // statistics of the split-key attention), decode state, beam scratch
  PcySwitches sw;
  if (int r = decode_prologue(c, m, kv, st, BB, what, split ? split_step_ws_bytes : reorder_ws_bytes, &sw, split)) return r;
  if (int r = ensure_beam_ws(c, B, beam)) return r;
  // (a shared-prefix cache: the rows own their suffix slots only -- the reorder starts at the first of them, and counts them from prefix_T)
  const int t_off = kv_shared(kv) ? kv->prefix_T : 0;
  const int sfx_t0 = (kv_t0 > t_off ? kv_t0 : t_off) - t_off;
  DecodeGraphKey key;
  decode_graph_key(key, c, m, kv, st, BB, KIND_BEAM, sw);
  key_beam(key, bs, logits_rec, c->beam_ws, beam, group_size, kv_t0, diversity_penalty);
  key.attn_split = split ? 1 : 0;
  return run_steps(c, n_steps, true, what, key, [&] {
    hipStream_t s = c->stream;
    enqueue_decode(c, m, kv, st, BB, sw, false, split);
    enqueue_store_logits(s, st->logits, logits_rec, 0, bs->step, BB, m->vocab);
    pcy_launch_beam_step(s, (const bf16_t*)st->logits, m->vocab, B, beam, group_size, diversity_penalty, beam_state_args(bs), c->beam_ws);
    enqueue_kv_reorder(s, m, kv, bs->src, BB, 0, (const int32_t*)bs->pos, sfx_t0, t_off, reorder_scratch(c, m, kv, BB));
  });
}
int pcy_llama_beam_steps(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, int beam, int group_size,
                         float diversity_penalty, const pcy_beam_state* bs, void* logits_rec, int n_steps, int kv_t0) {
  return beam_steps_entry(c, m, kv, st, B, beam, group_size, diversity_penalty, bs, logits_rec, n_steps, kv_t0, false);
}
int pcy_llama_beam_steps_split(pcy_ctx* c, const pcy_llama_desc* m, const pcy_kv_cache* kv, const pcy_gen_state* st, int B, int beam, int group_size,
                               float diversity_penalty, const pcy_beam_state* bs, void* logits_rec, int n_steps, int kv_t0) {
  return beam_steps_entry(c, m, kv, st, B, beam, group_size, diversity_penalty, bs, logits_rec, n_steps, kv_t0, true);
}

}  // extern "C"

extern "C" int pcy_debug_mc_trace(unsigned long long* out, int n) {
  if (!g_mc_trace) return 0;
  hipDeviceSynchronize();
  hipMemcpy(out, g_mc_trace, (size_t)n * 8, hipMemcpyDeviceToHost);
  return n;
}
