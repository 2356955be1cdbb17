// fp32 arithmetic for the callers of the reference that never call `.bfloat16()`:
//   /root/reference/examples/paper_analyses/protpep_qa_scores.py:55-58 (the loop that defines BASELINE configs[4]),
//   /root/reference/scripts/qa_filter_captions.py:17-18, /root/reference/scripts/caption_bulk.py:72-73.
// Their model holds fp32 weights and every torch op runs in fp32; the bf16 engine cannot reproduce that to better than 1e-2.  This
// file is the fp32 operator family those paths need -- encoder, pooler, projectors, splice, decoder prefill (QA scoring and retrieval
// read one forward pass), the cached decode step of an fp32 generation (pcy_f32_attn_decode), the loss and the many-token cache
// extension -- written for correctness first:
//   * Linear on the f32-input matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation in ascending k == an fmaf
//     chain; 155 TFLOP/s peak, 1/16 of the bf16 rate), 128 x 128 x 16 tiles, register-staged double buffer;
//   * attention as one wave per (sequence, head, query row): exact softmax in fp32 (scores in LDS), GQA, causal / key-keep masks;
//     decode attention as one wave per (row, head) over every slot of a token-major fp32 K / V cache;
//   * LayerNorm / RMSNorm / rotary / embedding / ESM token-dropout embedding / pooling / SiLU-mul as plain fp32 kernels;
//   * teacher-forced scoring: lm_head x cross-entropy fused on the Linear's own main loop (pcy_f32_tile.h), so the [M, V] fp32 logits
//     never reach memory (pcy_f32_lm_head_xent), and the cache extension -- S new query rows per row against a filled fp32 cache plus
//     the new keys, one wave per (query, head, row) (pcy_f32_attn_extend): the multi-token cached forward and shared-prefix scoring.
// The Python side (procyon_amd/engine_f32.py) strings them together exactly as the oracle's fp32 evaluation does (oracle/esm_ref.py,
// oracle/llama_ref.py); tests hold every op and the stacks to <= 1e-4 of it.
#include "pcy_internal.h"
#include "pcy_f32_tile.h"
#include "../../include/pcy.h"

namespace {

constexpr int NT = F_NT;

// ------------------------------------------------------------------------------------------------ Linear
// C[M,N] = act(A[M,K] . W[N,K]^T + bias) (+ resid);  act 0 none, 1 gelu (x * 0.5 * (1 + erf(x / sqrt 2)): nn.GELU and the ESM gelu are
// the same function in fp32).  Operands are fed swapped (W rows as the MFMA A operand) so a lane ends up with 4 consecutive output
// features of one token: 16-byte stores.
__global__ __launch_bounds__(NT) void linear_f32_kernel(const float* __restrict__ A, int lda, const float* __restrict__ W,
                                                        const float* __restrict__ bias, const float* resid, int ldr, float* C, int ldc,
                                                        int M, int N, int K, int act) {
  __shared__ float As[F_TILE_LDS], Ws[F_TILE_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;                 // 2 x 2 waves of 64 tokens x 64 features
  const int tiles_n = (N + F_TN - 1) / F_TN;
  const int m0 = (blockIdx.x / tiles_n) * F_TM, n0 = (blockIdx.x % tiles_n) * F_TN;
  f32x4 acc[4][4];
  f32_tile_mainloop(A, lda, W, M, N, K, m0, n0, As, Ws, acc);   // (pcy_f32_tile.h: the one copy of the loop)
  const int fr = lane & 15, fq = lane >> 4;
  // lane holds D[feature n = fq*4 + r][token m = fr] of tile (i, j)
  const bool vec = (ldc % 4 == 0) && (N % 4 == 0) && (resid == nullptr || ldr % 4 == 0) && ((reinterpret_cast<uintptr_t>(C) & 15) == 0) &&
                   (resid == nullptr || (reinterpret_cast<uintptr_t>(resid) & 15) == 0);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m0 + wm * 64 + j * 16 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + wn * 64 + i * 16 + fq * 4;
      if (n >= N) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int nn = n + r < N ? n + r : N - 1;
        float y = acc[i][j][r] + (bias ? bias[nn] : 0.f);
        if (act == 1) y = y * 0.5f * (1.0f + erff(y / 1.4142135623730951f));
        v[r] = y;
      }
      if (vec && n + 3 < N) {
        if (resid) {
          const float4 rr = *reinterpret_cast<const float4*>(resid + (size_t)m * ldr + n);
          v[0] += rr.x; v[1] += rr.y; v[2] += rr.z; v[3] += rr.w;
        }
        *reinterpret_cast<float4*>(C + (size_t)m * ldc + n) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (n + r < N) C[(size_t)m * ldc + n + r] = v[r] + (resid ? resid[(size_t)m * ldr + n + r] : 0.f);
      }
    }
  }
}

// small-K / unaligned fallback: one thread per output, fmaf chain over k (K % 16 != 0 or rows not 16-byte aligned)
__global__ __launch_bounds__(NT) void linear_f32_naive_kernel(const float* __restrict__ A, int lda, const float* __restrict__ W,
                                                              const float* __restrict__ bias, const float* resid, int ldr, float* C, int ldc,
                                                              int M, int N, int K, int act) {
  const size_t idx = (size_t)blockIdx.x * NT + threadIdx.x;
  if (idx >= (size_t)M * N) return;
  const int m = (int)(idx / N), n = (int)(idx % N);
  float y = 0.f;
  for (int k = 0; k < K; ++k) y = fmaf(A[(size_t)m * lda + k], W[(size_t)n * K + k], y);
  y += bias ? bias[n] : 0.f;
  if (act == 1) y = y * 0.5f * (1.0f + erff(y / 1.4142135623730951f));
  if (resid) y += resid[(size_t)m * ldr + n];
  C[(size_t)m * ldc + n] = y;
}

// ------------------------------------------------------------------------------------------------ lm_head x cross-entropy
// nll[m] = logsumexp_n(l[m][n]) - l[m][targets[m]], l = the fp32 value linear_f32_kernel stores for x . W^T (same loop, same bits),
// without the [M, V] logits reaching memory -- pcy_xent.hip carried over to fp32:
//   * the vocabulary is cut into 128-column tiles and these into f32_xent_ncb(V) column blocks of f32_xent_cb(V) consecutive tiles (at
//     most F_XENT_MAXCB blocks: one 128-row tile still puts two workgroups on every CU); functions of V alone;
//   * a workgroup walks the tiles of ONE column block for ONE 128-row tile and carries (max, sum exp) per lane and token across them
//     (online rescale).  Columns >= V are masked (their W rows are clamped on load).  At the end: merge over the four fq lane groups (xor
//     16, 32), over the two waves along N through LDS, and ONE (max, sumexp) pair per (column block, row) goes to part[cb][m] as a plain
//     8-byte store.  The one lane that holds column targets[m] stores label[m];
//   * finish kernel: one wave per row; lane l merges blocks l, l + 64, ... in order, then a xor butterfly;
//   * no atomics, every merge symmetric and its order a function of V alone, one row-tile shape for every M: a row's bits depend neither
//     on M nor on the other rows;
//   * rows in chunks of F_XENT_MCHUNK: the workspace is min(M, 1024) x (n_col_blocks x 8 + 4) bytes.
constexpr int F_XENT_MAXCB = 512, F_XENT_MCHUNK = 1024;
inline int f32_xent_cb(int V) { return ((V + F_TN - 1) / F_TN + F_XENT_MAXCB - 1) / F_XENT_MAXCB; }
inline int f32_xent_ncb(int V) { const int cb = f32_xent_cb(V); return ((V + F_TN - 1) / F_TN + cb - 1) / cb; }

// (m, s) <- merge of (m, s) and (om, os): s counts exp(. - m).  Symmetric in its two arguments; an empty side is (-inf, 0).
__device__ __forceinline__ void f32_xent_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  const float a = (m == nm) ? s : s * expf(m - nm);
  const float b = (om == nm) ? os : os * expf(om - nm);
  m = nm;
  s = a + b;
}

__global__ __launch_bounds__(NT) void f32_xent_partial_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ W,
                                                              const int32_t* __restrict__ targets, int M, int V, int d, int cb, int stride,
                                                              float2* __restrict__ part, float* __restrict__ label) {
  __shared__ float As[F_TILE_LDS], Ws[F_TILE_LDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int tiles_m = (M + F_TM - 1) / F_TM;
  const int cblk = blockIdx.x / tiles_m, m0 = (blockIdx.x - cblk * tiles_m) * F_TM;   // the row tiles of a column block are neighbours
  const float NEG_INF = -__builtin_inff();
  int tg[4];
  float mx[4], sm[4], lab[4];
  unsigned found = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = m0 + wm * 64 + j * 16 + fr;
    tg[j] = targets[m < M ? m : M - 1];
    mx[j] = NEG_INF; sm[j] = 0.f; lab[j] = 0.f;
  }
  for (int ct = 0; ct < cb; ++ct) {
    const int n0 = (cblk * cb + ct) * F_TN;
    if (n0 >= V) break;   // (uniform: the last column block may hold fewer tiles)
    f32x4 acc[4][4];
    f32_tile_mainloop(x, ldx, W, M, V, d, m0, n0, As, Ws, acc);
    // lane holds l[token m0 + wm*64 + j*16 + fr][column nb + i*16 + r] in acc[i][j][r]
    const int nb = n0 + wn * 64 + fq * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[4][4];
      float tmax = NEG_INF;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = nb + i * 16 + r;
          const float l = acc[i][j][r] + 0.f;     // (linear_f32_kernel's value without a bias)
          if (n == tg[j]) { lab[j] = l; found |= 1u << j; }
          v[i][r] = n < V ? l : NEG_INF;
          tmax = fmaxf(tmax, v[i][r]);
        }
      const float nm = fmaxf(mx[j], tmax);
      float s = (mx[j] == nm) ? sm[j] : sm[j] * expf(mx[j] - nm);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += v[i][r] > NEG_INF ? expf(v[i][r] - nm) : 0.f;
      mx[j] = nm; sm[j] = s;
    }
  }
  // the four fq groups hold disjoint columns of the same tokens
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float om = __shfl_xor(mx[j], off), os = __shfl_xor(sm[j], off);
      f32_xent_merge(mx[j], sm[j], om, os);
    }
  }
  // the two waves along N: through LDS (the tile buffers are free behind the main loop's last barrier)
  float2* red = reinterpret_cast<float2*>(As);
  if (wn == 1 && fq == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) red[wm * 64 + j * 16 + fr] = make_float2(mx[j], sm[j]);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ml = wm * 64 + j * 16 + fr, m = m0 + ml;
    if (m >= M) continue;
    if (wn == 0 && fq == 0) {
      const float2 o = red[ml];
      f32_xent_merge(mx[j], sm[j], o.x, o.y);
      part[(size_t)cblk * stride + m] = make_float2(mx[j], sm[j]);
    }
    if (found & (1u << j)) label[m] = lab[j];
  }
}

// one wave per row
__global__ __launch_bounds__(NT) void f32_xent_finish_kernel(const float2* __restrict__ part, int ncb, int stride, int M,
                                                             const int32_t* __restrict__ targets, int V, const float* __restrict__ label,
                                                             float* nll, float* lse_out, float* max_out, float* label_out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float m = -__builtin_inff(), s = 0.f;
  for (int c = lane; c < ncb; c += 64) {
    const float2 p = part[(size_t)c * stride + row];
    f32_xent_merge(m, s, p.x, p.y);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float om = __shfl_xor(m, off), os = __shfl_xor(s, off);
    f32_xent_merge(m, s, om, os);
  }
  if (lane != 0) return;
  const int tgt = targets[row];
  // a target outside [0, V) has no column: NaN, never an unwritten workspace word
  const float lab = (tgt >= 0 && tgt < V) ? label[row] : __builtin_nanf("");
  const float lse = m + logf(s);
  nll[row] = lse - lab;
  if (lse_out) lse_out[row] = lse;
  if (max_out) max_out[row] = m;
  if (label_out) label_out[row] = lab;
}

// ------------------------------------------------------------------------------------------------ norms
// LayerNorm as torch's fp32 kernel: mean, then biased variance around it, (x - mean) * rstd * w + b.  One workgroup per row.
__global__ __launch_bounds__(NT) void layernorm_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                           float* __restrict__ y, int d, float eps) {
  __shared__ float red[NT / 64];
  const float* xr = x + (size_t)blockIdx.x * d;
  float s = 0.f;
  for (int k = threadIdx.x; k < d; k += NT) s += xr[k];
  const float mean = block_sum<NT>(s, red) / (float)d;
  float v = 0.f;
  for (int k = threadIdx.x; k < d; k += NT) { const float t = xr[k] - mean; v += t * t; }
  const float rstd = rsqrtf(block_sum<NT>(v, red) / (float)d + eps);
  float* yr = y + (size_t)blockIdx.x * d;
  for (int k = threadIdx.x; k < d; k += NT) yr[k] = (xr[k] - mean) * rstd * w[k] + b[k];
}
// RMSNorm (HF Llama, fp32 model: the cast orders coincide): w * (x * rsqrt(mean(x^2) + eps))
__global__ __launch_bounds__(NT) void rmsnorm_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int d, float eps) {
  __shared__ float red[NT / 64];
  const float* xr = x + (size_t)blockIdx.x * d;
  float s = 0.f;
  for (int k = threadIdx.x; k < d; k += NT) s += xr[k] * xr[k];
  const float r = rsqrtf(block_sum<NT>(s, red) / (float)d + eps);
  float* yr = y + (size_t)blockIdx.x * d;
  for (int k = threadIdx.x; k < d; k += NT) yr[k] = w[k] * (xr[k] * r);
}

// ------------------------------------------------------------------------------------------------ rotary, embeddings, SiLU-mul
// heads [col0, col0 + nh * dh) of row t: x <- (x * prescale?) * cos[pos] + rotate_half(x * prescale?) * sin[pos]   (tables fp32 [n_pos, dh])
__global__ __launch_bounds__(NT) void rope_f32_kernel(float* __restrict__ buf, int ld, int col0, int nh, int dh, const int32_t* __restrict__ pos,
                                                      const float* __restrict__ cos_t, const float* __restrict__ sin_t, float prescale) {
  const int t = blockIdx.x, p = pos[t], half = dh / 2;
  float* row = buf + (size_t)t * ld + col0;
  for (int i = threadIdx.x; i < nh * half; i += NT) {
    const int h = i / half, e = i % half;
    float x1 = row[h * dh + e], x2 = row[h * dh + e + half];
    if (prescale != 0.f) { x1 *= prescale; x2 *= prescale; }
    const float c1 = cos_t[(size_t)p * dh + e], s1 = sin_t[(size_t)p * dh + e];
    const float c2 = cos_t[(size_t)p * dh + e + half], s2 = sin_t[(size_t)p * dh + e + half];
    row[h * dh + e] = x1 * c1 + (-x2) * s1;
    row[h * dh + e + half] = x2 * c2 + x1 * s2;
  }
}
// out[r] = soft_map[r] >= 0 ? soft[soft_map[r]] : table[ids[r]]   (token embedding + soft-token splice in one gather)
__global__ __launch_bounds__(NT) void embed_f32_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids, const float* __restrict__ soft,
                                                       const int32_t* __restrict__ soft_map, float* __restrict__ out, int d) {
  const int r = blockIdx.x;
  const int sm = soft_map ? soft_map[r] : -1;
  const float* src = sm >= 0 ? soft + (size_t)sm * d : table + (size_t)ids[r] * d;
  for (int k = threadIdx.x; k < d; k += NT) out[(size_t)r * d + k] = src[k];
}
// HF EsmEmbeddings with token_dropout (oracle/esm_ref.py::embed): <mask> rows zero, x * 0.88 / (1 - observed mask ratio), pads zero
__global__ __launch_bounds__(NT) void esm_embed_f32_kernel(const float* __restrict__ table, const int32_t* __restrict__ toks, const int32_t* __restrict__ cu,
                                                           float* __restrict__ out, int d, int mask_pads) {
  __shared__ float red[NT / 64];
  const int q = blockIdx.x;
  const int t0 = cu[q], len = cu[q + 1] - t0;
  float nmask = 0.f, nkeep = 0.f;
  for (int j = threadIdx.x; j < len; j += NT) {
    const int t = toks[t0 + j];
    nmask += (t == 32) ? 1.f : 0.f;
    nkeep += (t != 1) ? 1.f : 0.f;
  }
  nmask = block_sum<NT>(nmask, red);
  nkeep = block_sum<NT>(nkeep, red);
  const float denom = 1.0f - nmask / (mask_pads ? nkeep : (float)len);
  for (int j = blockIdx.y; j < len; j += gridDim.y) {
    const int t = toks[t0 + j];
    const bool zero = (t == 32) || (mask_pads && t == 1);
    for (int k = threadIdx.x; k < d; k += NT)
      out[(size_t)(t0 + j) * d + k] = zero ? 0.f : table[(size_t)t * d + k] * (1.0f - 0.15f * 0.8f) / denom;
  }
}
// dst[r] += src[rows[r]]  (sum over the L+1 hidden states at the [PROT] rows: ret_token_access='all', model_unified.py:560-563)
__global__ __launch_bounds__(NT) void acc_rows_f32_kernel(const float* __restrict__ src, int lds_, const int32_t* __restrict__ rows, float* __restrict__ dst, int d) {
  const int r = blockIdx.x;
  const float* s = src + (size_t)rows[r] * lds_;
  for (int k = threadIdx.x; k < d; k += NT) dst[(size_t)r * d + k] += s[k];
}
__global__ __launch_bounds__(NT) void silu_mul_f32_kernel(const float* __restrict__ g, const float* __restrict__ u, float* __restrict__ o, size_t n) {
  for (size_t i = (size_t)blockIdx.x * NT + threadIdx.x; i < n; i += (size_t)gridDim.x * NT) {
    const float x = g[i];
    o[i] = (x / (1.0f + expf(-x))) * u[i];
  }
}
// ProteinPooler (/root/reference/procyon/model/esm.py:131-173) over token ranges, as pcy_pool: mode 0 mean, 1 mean of x[1:-1], 2 max.
// One workgroup per (protein, 256-feature slab); sequential over the tokens (fp32 sum in token order).
__global__ __launch_bounds__(NT) void pool_f32_kernel(const float* __restrict__ h, int d, const int32_t* __restrict__ seg, const int32_t* __restrict__ rng,
                                                      int mode, float* __restrict__ out) {
  const int p = blockIdx.x, c = blockIdx.y * NT + threadIdx.x;
  if (c >= d) return;
  const int r0 = seg[p], r1 = seg[p + 1];
  float acc = mode == 2 ? -INFINITY : 0.f;
  int cnt = 0;
  for (int r = r0; r < r1; ++r) {
    int st = rng[2 * r], ln = rng[2 * r + 1];
    if (mode == 1) {
      if (r == r0) { st += 1; ln -= 1; }
      if (r == r1 - 1) ln -= 1;
    }
    for (int j = 0; j < ln; ++j) {
      const float v = h[(size_t)(st + j) * d + c];
      if (mode == 2) acc = fmaxf(acc, v);
      else if (v == v) { acc += v; ++cnt; }
    }
  }
  out[(size_t)p * d + c] = mode == 2 ? acc : acc / (float)cnt;
}

// ------------------------------------------------------------------------------------------------ attention
// One wave per (query row i, head h, sequence q).  Packed rows: token t0 + j of sequence q.  keys j < (causal ? i + 1 : len), dropped
// where keep[t0 + j] == 0.  scores = (q . k) * scale in LDS, exact softmax, o = P . V.  A query row without any kept key (a pad query
// row) writes the reference's value: the plain average of V over ALL `len` keys of its sequence, causal or not, pads and later keys
// included -- the softmax of a row whose every entry is finfo.min (oracle/llama_ref.py::build_additive_mask).  The cached decode
// attends every slot without a mask, so the K / V that the next layers compute from these rows are read (LlamaEngineF32.decode).
__global__ __launch_bounds__(64) void attn_f32_kernel(const float* __restrict__ q, int ldq, int qcol0, const float* __restrict__ k, int ldk, int kcol0,
                                                      const float* __restrict__ v, int ldv, int vcol0, float* __restrict__ o, int ldo,
                                                      const int32_t* __restrict__ cu, const uint8_t* __restrict__ keep, int H, int Hkv, int dh,
                                                      int causal, float scale) {
  extern __shared__ float smem_f[];
  const int i = blockIdx.x, h = blockIdx.y, sq = blockIdx.z, lane = threadIdx.x;
  const int t0 = cu[sq], len = cu[sq + 1] - t0;
  if (i >= len) return;
  float* qs = smem_f;            // [dh]
  float* sc = smem_f + dh;       // [nkeys]
  const int hk = h / (H / Hkv);
  const float* qrow = q + (size_t)(t0 + i) * ldq + qcol0 + h * dh;
  for (int e = lane; e < dh; e += 64) qs[e] = qrow[e];
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const int nkeys = causal ? i + 1 : len;
  float mx = -INFINITY;
  for (int j = lane; j < nkeys; j += 64) {
    float s = -INFINITY;
    if (!keep || keep[t0 + j]) {
      const float* kr = k + (size_t)(t0 + j) * ldk + kcol0 + hk * dh;
      float a = 0.f;
      for (int e = 0; e < dh; e += 4) {
        const float4 kv = *reinterpret_cast<const float4*>(kr + e);
        a = fmaf(qs[e], kv.x, a); a = fmaf(qs[e + 1], kv.y, a); a = fmaf(qs[e + 2], kv.z, a); a = fmaf(qs[e + 3], kv.w, a);
      }
      s = a * scale;
    }
    sc[j] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float* orow = o + (size_t)(t0 + i) * ldo + h * dh;
  if (mx == -INFINITY) {
    const float u = 1.0f / (float)len;
    for (int e = lane; e < dh; e += 64) {
      float a = 0.f;
      const float* vc = v + (size_t)t0 * ldv + vcol0 + hk * dh + e;
      for (int j = 0; j < len; ++j) a = fmaf(u, vc[(size_t)j * ldv], a);
      orow[e] = a;
    }
    return;
  }
  float sum = 0.f;
  for (int j = lane; j < nkeys; j += 64) { const float p = expf(sc[j] - mx); sc[j] = p; sum += p; }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  for (int e = lane; e < dh; e += 64) {
    float a = 0.f;
    const float* vc = v + (size_t)t0 * ldv + vcol0 + hk * dh + e;
    for (int j = 0; j < nkeys; ++j) a = fmaf(sc[j] * inv, vc[(size_t)j * ldv], a);
    orow[e] = a;
  }
}

// Decode attention in fp32: one wave per (head h, row b); the new token's query against the first `nkeys` slots of the row's cache
// (token-major [B][Tmax][Hkv dh]; every slot is attended: the reference passes no mask after the prefill, model_unified.py:769, :887).
__global__ __launch_bounds__(64) void attn_dec_f32_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ kc, const float* __restrict__ vc,
                                                          int ldkv, int Tmax, float* __restrict__ o, int ldo, int H, int Hkv, int dh, int nkeys,
                                                          float scale) {
  extern __shared__ float smem_f[];
  const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  float* qs = smem_f;            // [dh]
  float* sc = smem_f + dh;       // [nkeys]
  const int hk = h / (H / Hkv);
  const float* qrow = q + (size_t)b * ldq + h * dh;
  for (int e = lane; e < dh; e += 64) qs[e] = qrow[e];
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const float* kb = kc + (size_t)b * Tmax * ldkv + hk * dh;
  const float* vb = vc + (size_t)b * Tmax * ldkv + hk * dh;
  float mx = -INFINITY;
  for (int j = lane; j < nkeys; j += 64) {
    const float* kr = kb + (size_t)j * ldkv;
    float a = 0.f;
    for (int e = 0; e < dh; e += 4) {
      const float4 kv = *reinterpret_cast<const float4*>(kr + e);
      a = fmaf(qs[e], kv.x, a); a = fmaf(qs[e + 1], kv.y, a); a = fmaf(qs[e + 2], kv.z, a); a = fmaf(qs[e + 3], kv.w, a);
    }
    const float s_ = a * scale;
    sc[j] = s_;
    mx = fmaxf(mx, s_);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < nkeys; j += 64) { const float p = expf(sc[j] - mx); sc[j] = p; sum += p; }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  float* orow = o + (size_t)b * ldo + h * dh;
  for (int e = lane; e < dh; e += 64) {
    float a = 0.f;
    for (int j = 0; j < nkeys; ++j) a = fmaf(sc[j] * inv, vb[(size_t)j * ldkv + e], a);
    orow[e] = a;
  }
}

// Cache extension in fp32: one wave per (new query s, head h, row b).  Keys in ascending slot order: slots [0, t_past) of cache row
// cache_row[b] (b when NULL), then the new keys 0..s of the row's own qkv rows (never the cache: a shared prefix row needs no per-row
// slots, and slots >= t_past are not read).  keep[b][j] == 0 masks key j, old and new alike.  A query without any kept key takes the
// family's value (attn_f32_kernel): the plain average of V over ALL t_past + S keys of its row.  With S == 1 and no mask the operations
// and their order are attn_dec_f32_kernel's on a cache that holds the new K / V at slot t_past.
__global__ __launch_bounds__(64) void attn_ext_f32_kernel(const float* __restrict__ qkv, int ld, const float* __restrict__ kc,
                                                          const float* __restrict__ vc, int ldkv, int Tmax, const int32_t* __restrict__ cache_row,
                                                          const uint8_t* __restrict__ keep, int ldkeep, float* __restrict__ o, int ldo, int S,
                                                          int t_past, int H, int Hkv, int dh, float scale) {
  extern __shared__ float smem_f[];
  const int s = blockIdx.x, h = blockIdx.y, b = blockIdx.z, lane = threadIdx.x;
  float* qs = smem_f;            // [dh]
  float* sc = smem_f + dh;       // [t_past + S]
  const int hk = h / (H / Hkv);
  const float* qrow = qkv + (size_t)(b * S + s) * ld + h * dh;
  for (int e = lane; e < dh; e += 64) qs[e] = qrow[e];
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const int cr = cache_row ? cache_row[b] : b;
  const float* kb = kc + (size_t)cr * Tmax * ldkv + hk * dh;
  const float* vb = vc + (size_t)cr * Tmax * ldkv + hk * dh;
  const float* kn = qkv + (size_t)b * S * ld + (H + hk) * dh;          // new K / V of the row: qkv rows b*S + 0 .. S-1
  const float* vn = qkv + (size_t)b * S * ld + (H + Hkv + hk) * dh;
  const uint8_t* kp = keep ? keep + (size_t)b * ldkeep : nullptr;
  const int nkeys = t_past + s + 1;
  float mx = -INFINITY;
  for (int j = lane; j < nkeys; j += 64) {
    float s_ = -INFINITY;
    if (!kp || kp[j]) {
      const float* kr = j < t_past ? kb + (size_t)j * ldkv : kn + (size_t)(j - t_past) * ld;
      float a = 0.f;
      for (int e = 0; e < dh; e += 4) {
        const float4 kv = *reinterpret_cast<const float4*>(kr + e);
        a = fmaf(qs[e], kv.x, a); a = fmaf(qs[e + 1], kv.y, a); a = fmaf(qs[e + 2], kv.z, a); a = fmaf(qs[e + 3], kv.w, a);
      }
      s_ = a * scale;
    }
    sc[j] = s_;
    mx = fmaxf(mx, s_);
  }
  mx = wave_max(mx);
  float* orow = o + (size_t)(b * S + s) * ldo + h * dh;
  if (mx == -INFINITY) {
    const float u = 1.0f / (float)(t_past + S);
    for (int e = lane; e < dh; e += 64) {
      float a = 0.f;
      for (int j = 0; j < t_past; ++j) a = fmaf(u, vb[(size_t)j * ldkv + e], a);
      for (int j = 0; j < S; ++j) a = fmaf(u, vn[(size_t)j * ld + e], a);
      orow[e] = a;
    }
    return;
  }
  float sum = 0.f;
  for (int j = lane; j < nkeys; j += 64) { const float p = expf(sc[j] - mx); sc[j] = p; sum += p; }
  sum = wave_sum(sum);
  const float inv = 1.0f / sum;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  for (int e = lane; e < dh; e += 64) {
    float a = 0.f;
    for (int j = 0; j < t_past; ++j) a = fmaf(sc[j] * inv, vb[(size_t)j * ldkv + e], a);
    for (int j = t_past; j < nkeys; ++j) a = fmaf(sc[j] * inv, vn[(size_t)(j - t_past) * ld + e], a);
    orow[e] = a;
  }
}

int launch_ok(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { pcy_set_error("kernel launch failed in %s: %s", what, hipGetErrorString(e)); return 3; }
  return 0;
}

}  // namespace

extern "C" {

int pcy_f32_linear(pcy_ctx* c, const float* A, int lda, const float* W, const float* bias, const float* resid, int ldr, float* C, int ldc,
                   int M, int N, int K, int act) {
  if (M <= 0 || N <= 0) return 0;
  if (act != 0 && act != 1) { pcy_set_error("pcy_f32_linear: act %d (0 none, 1 gelu)", act); return 1; }
  hipStream_t s = pcy_ctx_stream(c);
  const bool fast = K % F_BK == 0 && lda % 4 == 0 && ((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(W)) & 15) == 0;
  if (fast) {
    const int tiles = ((M + F_TM - 1) / F_TM) * ((N + F_TN - 1) / F_TN);
    hipLaunchKernelGGL(linear_f32_kernel, dim3(tiles), dim3(NT), 0, s, A, lda, W, bias, resid, ldr, C, ldc, M, N, K, act);
  } else {
    const size_t n = (size_t)M * N;
    hipLaunchKernelGGL(linear_f32_naive_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, s, A, lda, W, bias, resid, ldr, C, ldc, M, N, K, act);
  }
  return launch_ok("pcy_f32_linear");
}
int pcy_f32_layernorm(pcy_ctx* c, const float* x, const float* w, const float* b, float* y, int rows, int d, float eps) {
  if (rows > 0) hipLaunchKernelGGL(layernorm_f32_kernel, dim3(rows), dim3(NT), 0, pcy_ctx_stream(c), x, w, b, y, d, eps);
  return launch_ok("pcy_f32_layernorm");
}
int pcy_f32_rmsnorm(pcy_ctx* c, const float* x, const float* w, float* y, int rows, int d, float eps) {
  if (rows > 0) hipLaunchKernelGGL(rmsnorm_f32_kernel, dim3(rows), dim3(NT), 0, pcy_ctx_stream(c), x, w, y, d, eps);
  return launch_ok("pcy_f32_rmsnorm");
}
int pcy_f32_rope(pcy_ctx* c, float* buf, int ld, int col0, int nh, int dh, const int32_t* pos, const float* cos_t, const float* sin_t, int ntok,
                 float prescale) {
  if (dh % 2) { pcy_set_error("pcy_f32_rope: odd head_dim"); return 1; }
  if (ntok > 0) hipLaunchKernelGGL(rope_f32_kernel, dim3(ntok), dim3(NT), 0, pcy_ctx_stream(c), buf, ld, col0, nh, dh, pos, cos_t, sin_t, prescale);
  return launch_ok("pcy_f32_rope");
}
int pcy_f32_embed(pcy_ctx* c, const float* table, const int32_t* ids, const float* soft, const int32_t* soft_map, float* out, int rows, int d) {
  if (rows > 0) hipLaunchKernelGGL(embed_f32_kernel, dim3(rows), dim3(NT), 0, pcy_ctx_stream(c), table, ids, soft, soft_map, out, d);
  return launch_ok("pcy_f32_embed");
}
int pcy_f32_esm_embed(pcy_ctx* c, const float* table, const int32_t* tokens, const int32_t* cu, int nseq, int max_len, float* out, int d, int mask_pads) {
  if (nseq > 0) {
    int sl = max_len < 64 ? max_len : 64;
    if (sl < 1) sl = 1;
    hipLaunchKernelGGL(esm_embed_f32_kernel, dim3(nseq, sl), dim3(NT), 0, pcy_ctx_stream(c), table, tokens, cu, out, d, mask_pads);
  }
  return launch_ok("pcy_f32_esm_embed");
}
int pcy_f32_silu_mul(pcy_ctx* c, const float* gate, const float* up, float* out, size_t n) {
  if (n > 0) {
    const size_t nb = (n + NT - 1) / NT;
    hipLaunchKernelGGL(silu_mul_f32_kernel, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(NT), 0, pcy_ctx_stream(c), gate, up, out, n);
  }
  return launch_ok("pcy_f32_silu_mul");
}
int pcy_f32_acc_rows(pcy_ctx* c, const float* src, int ld, const int32_t* rows, float* dst, int nrows, int d) {
  if (nrows > 0) hipLaunchKernelGGL(acc_rows_f32_kernel, dim3(nrows), dim3(NT), 0, pcy_ctx_stream(c), src, ld, rows, dst, d);
  return launch_ok("pcy_f32_acc_rows");
}
int pcy_f32_pool(pcy_ctx* c, const float* hidden, int d, const int32_t* seg, const int32_t* rng, int nprot, int mode, float* out) {
  if (mode < 0 || mode > 2) { pcy_set_error("pcy_f32_pool: mode %d", mode); return 1; }
  if (nprot > 0) hipLaunchKernelGGL(pool_f32_kernel, dim3(nprot, (d + NT - 1) / NT), dim3(NT), 0, pcy_ctx_stream(c), hidden, d, seg, rng, mode, out);
  return launch_ok("pcy_f32_pool");
}
int pcy_f32_attention(pcy_ctx* c, const float* q, int ldq, int qcol0, const float* k, int ldk, int kcol0, const float* v, int ldv, int vcol0,
                      float* o, int ldo, const int32_t* cu, const uint8_t* keep, int nseq, int max_len, int H, int Hkv, int dh, int causal,
                      float scale) {
  if (dh % 4 || H % Hkv) { pcy_set_error("pcy_f32_attention: head_dim %% 4 and Hkv | H required"); return 1; }
  if ((ldk | kcol0) % 4) { pcy_set_error("pcy_f32_attention: K rows must be 16-byte aligned"); return 1; }
  const size_t smem = (size_t)(dh + max_len) * sizeof(float);
  if (smem > 160 * 1024 - 1024) { pcy_set_error("pcy_f32_attention: %d keys exceed the LDS score buffer", max_len); return 1; }
  if (nseq > 0 && max_len > 0) {
    static PcyLdsAttr lds_attn_f32_kernel;   // (configured once per device and size, refused sizes fail the call)
    if (!lds_attn_f32_kernel.ensure(&attn_f32_kernel, smem)) { pcy_set_error("pcy_f32_attention: the device refused %zu bytes of LDS", smem); return 1; }
    hipLaunchKernelGGL(attn_f32_kernel, dim3(max_len, H, nseq), dim3(64), smem, pcy_ctx_stream(c), q, ldq, qcol0, k, ldk, kcol0, v, ldv, vcol0, o, ldo,
                       cu, keep, H, Hkv, dh, causal, scale);
  }
  return launch_ok("pcy_f32_attention");
}

int pcy_f32_attn_decode(pcy_ctx* c, const float* q, int ldq, const float* kcache, const float* vcache, int ldkv, int Tmax, float* o, int ldo, int B,
                        int H, int Hkv, int dh, int nkeys, float scale) {
  if (dh % 4 || H % Hkv || ldkv % 4) { pcy_set_error("pcy_f32_attn_decode: head_dim %% 4, Hkv | H and 16-byte aligned cache rows required"); return 1; }
  if (nkeys < 1 || nkeys > Tmax) { pcy_set_error("pcy_f32_attn_decode: %d keys outside the cache (%d slots)", nkeys, Tmax); return 1; }
  const size_t smem = (size_t)(dh + nkeys) * sizeof(float);
  if (smem > 160 * 1024 - 1024) { pcy_set_error("pcy_f32_attn_decode: %d keys exceed the LDS score buffer", nkeys); return 1; }
  if (B > 0) {
    static PcyLdsAttr lds_attn_dec_f32_kernel;   // (configured once per device and size, refused sizes fail the call)
    if (!lds_attn_dec_f32_kernel.ensure(&attn_dec_f32_kernel, smem)) { pcy_set_error("pcy_f32_attn_decode: the device refused %zu bytes of LDS", smem); return 1; }
    hipLaunchKernelGGL(attn_dec_f32_kernel, dim3(H, B), dim3(64), smem, pcy_ctx_stream(c), q, ldq, kcache, vcache, ldkv, Tmax, o, ldo, H, Hkv, dh, nkeys, scale);
  }
  return launch_ok("pcy_f32_attn_decode");
}

int pcy_f32_attn_extend(pcy_ctx* c, const float* qkv, int ld, const float* kcache, const float* vcache, int ldkv, int Tmax, const int32_t* cache_row,
                        const uint8_t* keep, int ldkeep, float* o, int ldo, int B, int S, int t_past, int H, int Hkv, int dh, float scale) {
  if (dh < 4 || dh % 4 || Hkv < 1 || H % Hkv || ldkv % 4 || ld % 4) {
    pcy_set_error("pcy_f32_attn_extend: head_dim %% 4, Hkv | H and 16-byte aligned qkv / cache rows required"); return 1;
  }
  if (B < 0 || S < 0 || t_past < 0 || t_past > Tmax) { pcy_set_error("pcy_f32_attn_extend: B=%d S=%d t_past=%d (the cache has %d slots)", B, S, t_past, Tmax); return 1; }
  if (ld < (H + 2 * Hkv) * dh || ldo < H * dh || ldkv < Hkv * dh) { pcy_set_error("pcy_f32_attn_extend: row strides shorter than the rows"); return 1; }
  if (keep && ldkeep < t_past + S) { pcy_set_error("pcy_f32_attn_extend: keep rows of %d bytes for %d keys", ldkeep, t_past + S); return 1; }
  if (B > 65535 || H > 65535) { pcy_set_error("pcy_f32_attn_extend: B=%d H=%d exceed the launch grid", B, H); return 1; }
  const size_t smem = ((size_t)dh + (size_t)t_past + (size_t)S) * sizeof(float);
  if (smem > 160 * 1024 - 1024) { pcy_set_error("pcy_f32_attn_extend: %d keys exceed the LDS score buffer", t_past + S); return 1; }
  if (B > 0 && S > 0) {
    if (!qkv || !o || (t_past > 0 && (!kcache || !vcache))) { pcy_set_error("pcy_f32_attn_extend: qkv, o and (with t_past > 0) the caches are required"); return 1; }
    static PcyLdsAttr lds_attn_ext_f32_kernel;   // (configured once per device and size, refused sizes fail the call)
    if (!lds_attn_ext_f32_kernel.ensure(&attn_ext_f32_kernel, smem)) { pcy_set_error("pcy_f32_attn_extend: the device refused %zu bytes of LDS", smem); return 1; }
    hipLaunchKernelGGL(attn_ext_f32_kernel, dim3(S, H, B), dim3(64), smem, pcy_ctx_stream(c), qkv, ld, kcache, vcache, ldkv, Tmax, cache_row, keep,
                       ldkeep, o, ldo, S, t_past, H, Hkv, dh, scale);
  }
  return launch_ok("pcy_f32_attn_extend");
}

size_t pcy_f32_lm_head_xent_ws_bytes(int M, int V) {
  if (M <= 0 || V <= 0) return 0;
  return (size_t)(M < F_XENT_MCHUNK ? M : F_XENT_MCHUNK) * ((size_t)f32_xent_ncb(V) * 8 + 4);
}

int pcy_f32_lm_head_xent(pcy_ctx* c, const float* x, int ldx, const float* W, int M, int V, int d, const int32_t* targets, float* nll_out,
                         float* lse_out, float* row_max_out, float* label_logit_out) {
  if (M < 0 || V <= 0 || d <= 0 || d % F_BK != 0) { pcy_set_error("pcy_f32_lm_head_xent: M=%d V=%d d=%d (d must be a multiple of 16)", M, V, d); return 1; }
  if (M == 0) return 0;
  if (!x || !W || !targets || !nll_out) { pcy_set_error("pcy_f32_lm_head_xent: x, W, targets and nll_out are required"); return 1; }
  if (ldx < d || ldx % 4 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(W)) & 15)) {
    pcy_set_error("pcy_f32_lm_head_xent: rows of x and W must be 16-byte aligned (ldx=%d)", ldx); return 1;
  }
  char* ws = static_cast<char*>(pcy_ctx_reserve(c, pcy_f32_lm_head_xent_ws_bytes(M, V) + 256));
  if (!ws) return 2;
  hipStream_t s = pcy_ctx_stream(c);
  const int cb = f32_xent_cb(V), ncb = f32_xent_ncb(V);
  const int stride = M < F_XENT_MCHUNK ? M : F_XENT_MCHUNK;
  float2* part = reinterpret_cast<float2*>(ws);                                   // [ncb][stride] (max, sumexp)
  float* label = reinterpret_cast<float*>(ws + (size_t)stride * ncb * 8);          // [stride] logit of the target column
  for (int r0 = 0; r0 < M; r0 += F_XENT_MCHUNK) {
    const int mc = M - r0 < F_XENT_MCHUNK ? M - r0 : F_XENT_MCHUNK;
    const int tiles_m = (mc + F_TM - 1) / F_TM;
    hipLaunchKernelGGL(f32_xent_partial_kernel, dim3(tiles_m * ncb), dim3(NT), 0, s, x + (size_t)r0 * ldx, ldx, W, targets + r0, mc, V, d, cb, stride,
                       part, label);
    hipLaunchKernelGGL(f32_xent_finish_kernel, dim3((mc + 3) / 4), dim3(NT), 0, s, part, ncb, stride, mc, targets + r0, V, label, nll_out + r0,
                       lse_out ? lse_out + r0 : nullptr, row_max_out ? row_max_out + r0 : nullptr, label_logit_out ? label_logit_out + r0 : nullptr);
  }
  return launch_ok("pcy_f32_lm_head_xent");
}

}  // extern "C"
