// fp32 generation: the streaming GEMV and the launches of the device-resident fp32 decode step (contracts in
// include/pcy.h).  The operator-per-launch step of LlamaEngineF32.decode sends 1..32 decode rows through the 128 x 128-tile Linear of
// pcy_f32.hip: one row tile, N / 128 workgroups, no split over K -- 32 workgroups walk 7.3 MB of the down projection each.  Here:
//
//   gemv_f32_kernel     y[b][n] = epi(sum_k x[b][k] * W[n][k]) with the weights streamed ONCE for up to 32 rows of x
//     * a workgroup owns 16 output rows (twice 16 weight rows for SwiGLU: gate and up are separate matrices) and ALL of K; its 8 waves split
//       every G_CH-float window of K between them (G_U k-steps of 16 floats per wave and window), so N / 16 workgroups x 8 waves stream
//     * a lane loads 16 bytes of ITS weight row per k-step straight into the A operand of v_mfma_f32_16x16x4_f32 (non-temporal; G_U loads
//       = 8 KiB per wave in flight, the next window's loads issued before the current window is consumed); element j of the four loaded
//       floats feeds MFMA j of the k-step, so MFMA j sums k = j, 4 + j, 8 + j, 12 + j of the step: a fixed permutation of K
//     * x is small and L2-resident: the window of all 16 / 32 rows is staged through LDS (row stride G_CH + 4 floats: the 16-byte fragment
//       reads of the 16 rows fall on 64 different banks), rows >= B are zeros; the B operand of MFMA j is element j of one ds_read_b128
//     * exact fp32 products, fp32 accumulation: per (wave, 16-row tile of x) two accumulators (even / odd k-steps), added at the end; the
//       waves' partial sums go through LDS and are added in wave order; then the epilogue.  No atomics
//     * an output's sum never involves another row of x (a column of the MFMA's B operand), and neither the tile count nor B changes the
//       chain of a row: row b of a B-row call has the bits of the one-row call
//     * the windows of a workgroup are walked rotated by (its index % the window count): all workgroups otherwise read the same window of
//       their rows at the same moment, and rows of 4096 floats are a power-of-two stride (channel aliasing)
//     * 17..32 rows take ONE pass with two x tiles against every weight register (the MFMA rate covers it: 32 rows x 7.5 G weights are
//       0.48 TFLOP per step against 155 TFLOP/s); the launcher loops passes of 32 rows above that
//   attn_pos_f32_kernel  the decode attention that reads *pos on the device: rope + append + exact softmax over slots [0, *pos], one workgroup
//     per (row, kv head), the query heads of the kv head share every K / V read, the waves split the keys
//   embed / rmsnorm / pick / record kernels of the step: plain fp32
#include "pcy_internal.h"
#include "../../include/pcy.h"

namespace {

constexpr int G_NW = 8, G_NT = G_NW * 64;     // waves / threads of a GEMV workgroup
constexpr int G_U = 8;                        // k-steps (16 floats = one 16-byte load per lane) per wave and window
constexpr int G_ROWS = 16;                    // output rows per workgroup
constexpr size_t LDS_MAX = 160 * 1024;

typedef __attribute__((ext_vector_type(4))) float g_f32x4;
typedef const __attribute__((address_space(1))) g_f32x4* g_gptr;
__device__ __forceinline__ float4 ldg_nt_f32(const float* p) {
  const g_f32x4 v = __builtin_nontemporal_load((g_gptr)(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}

template <int NBT, int EPI>
__global__ __launch_bounds__(G_NT) void gemv_f32_kernel(PcyF32GemvArgs a) {
  constexpr int NMAT = EPI == EPI_SWIGLU ? 2 : 1;
  constexpr int KW = G_NW / NMAT;             // waves that split a window of K
  constexpr int CH = KW * G_U * 16;           // floats of K per window: 1024 (STORE / RESID), 512 (SWIGLU)
  constexpr int XLD = CH + 4;
  extern __shared__ __attribute__((aligned(16))) float g_smem[];   // xs [16 NBT][XLD]; behind the main loop: red [G_NW][NBT][16 tokens][16 features]
  float* xs = g_smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int kw = wave % KW, mat = wave / KW;
  const int n0 = blockIdx.x * G_ROWS;
  const int K = a.K;
  const int niter = (K + CH - 1) / CH;
  const int rot = blockIdx.x % niter;
  int nrow = n0 + fr;
  nrow = nrow < a.N ? nrow : a.N - 1;         // (rows past N: a duplicate of the last row, never stored)
  const float* wrow = (mat ? a.W2 : a.W) + (size_t)nrow * K;
  const int koff = kw * (G_U * 16) + fq * 4;  // the lane's first float inside a window

  auto window = [&](int it) { const int r = it + rot; return (r >= niter ? r - niter : r) * CH; };
  auto issue = [&](int it, float4 (&w)[G_U]) {
    const int kb = window(it) + koff;
#pragma unroll
    for (int u = 0; u < G_U; ++u) {
      const int k = kb + u * 16;
      w[u] = k < K ? ldg_nt_f32(wrow + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  f32x4 acc[2][NBT];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int t = 0; t < NBT; ++t) acc[p][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

  float4 wc[G_U], wn[G_U];
#pragma unroll
  for (int u = 0; u < G_U; ++u) wn[u] = make_float4(0.f, 0.f, 0.f, 0.f);
  issue(0, wc);
  for (int it = 0; it < niter; ++it) {
    const int kb = window(it);
    lds_barrier();                            // the previous window's fragments have been read
    // the window of x for every row of the pass -> LDS (a wave stages one row at a time: the row test is uniform)
#pragma unroll 4
    for (int idx = tid; idx < 16 * NBT * (CH / 4); idx += G_NT) {
      const int row = idx / (CH / 4), c4 = idx % (CH / 4);
      const int k = kb + c4 * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row < a.B && k < K) v = *reinterpret_cast<const float4*>(a.x + (size_t)row * a.ldx + k);
      *reinterpret_cast<float4*>(xs + row * XLD + c4 * 4) = v;
    }
    if (it + 1 < niter) issue(it + 1, wn);    // in flight while this window is consumed
    lds_barrier();
#pragma unroll
    for (int u = 0; u < G_U; ++u) {
#pragma unroll
      for (int t = 0; t < NBT; ++t) {
        const float4 xv = *reinterpret_cast<const float4*>(xs + (t * 16 + fr) * XLD + kw * (G_U * 16) + u * 16 + fq * 4);
        f32x4 c = acc[u & 1][t];
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].x, xv.x, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].y, xv.y, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].z, xv.z, c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[u].w, xv.w, c, 0, 0, 0);
        acc[u & 1][t] = c;
      }
    }
#pragma unroll
    for (int u = 0; u < G_U; ++u) wc[u] = wn[u];
  }
  // lane holds D[feature fq*4 + r][token fr] of tile t in acc[.][t][r]
  lds_barrier();
  float* red = g_smem;
#pragma unroll
  for (int t = 0; t < NBT; ++t) {
    const f32x4 s = acc[0][t] + acc[1][t];
    *reinterpret_cast<float4*>(red + ((wave * NBT + t) * 16 + fr) * 16 + fq * 4) = make_float4(s[0], s[1], s[2], s[3]);
  }
  lds_barrier();
  for (int o = tid; o < NBT * 256; o += G_NT) {
    const int t = o >> 8, tok = (o >> 4) & 15, f = o & 15;
    const int b = t * 16 + tok, n = n0 + f;
    if (b >= a.B || n >= a.N) continue;
    float v = 0.f, v2 = 0.f;
#pragma unroll
    for (int w = 0; w < KW; ++w) {
      v += red[((w * NBT + t) * 16 + tok) * 16 + f];
      if (NMAT == 2) v2 += red[(((KW + w) * NBT + t) * 16 + tok) * 16 + f];
    }
    if (EPI == EPI_SWIGLU) v = (v / (1.0f + expf(-v))) * v2;
    if (EPI == EPI_RESID) v += a.resid[(size_t)b * a.ldr + n];
    a.y[(size_t)b * a.ldy + n] = v;
  }
}

template <int NBT, int EPI>
bool launch_gemv_f32(hipStream_t s, const PcyF32GemvArgs& a) {
  static PcyLdsAttr attr;
  constexpr int CH = (EPI == EPI_SWIGLU ? G_NW / 2 : G_NW) * G_U * 16;
  const size_t smem = (size_t)16 * NBT * (CH + 4) * sizeof(float);
  static_assert((size_t)16 * 2 * (G_NW * G_U * 16 + 4) * sizeof(float) <= LDS_MAX, "two x tiles of a window must fit the LDS of a CU");
  static_assert((size_t)G_NW * 2 * 256 <= (size_t)16 * (G_NW / 2 * G_U * 16 + 4), "the waves' partial sums reuse the x window");
  if (!attr.ensure(gemv_f32_kernel<NBT, EPI>, smem)) return false;
  hipLaunchKernelGGL((gemv_f32_kernel<NBT, EPI>), dim3((a.N + G_ROWS - 1) / G_ROWS), dim3(G_NT), smem, s, a);
  return true;
}
template <int NBT>
bool launch_gemv_f32_epi(hipStream_t s, const PcyF32GemvArgs& a) {
  switch (a.epi) {
    case EPI_STORE: return launch_gemv_f32<NBT, EPI_STORE>(s, a);
    case EPI_RESID: return launch_gemv_f32<NBT, EPI_RESID>(s, a);
    case EPI_SWIGLU: return launch_gemv_f32<NBT, EPI_SWIGLU>(s, a);
  }
  return false;
}

// ------------------------------------------------------------------------------------------------ decode attention, position on the device
constexpr int A_NW = 8, A_NT = A_NW * 64;

template <int GT, int DH>
__device__ __forceinline__ void qk_dots(const float* __restrict__ kr, const float* __restrict__ qs, float (&s)[GT]) {
#pragma unroll
  for (int g = 0; g < GT; ++g) s[g] = 0.f;
#pragma unroll 4
  for (int e = 0; e < DH; e += 4) {
    const float4 kv = *reinterpret_cast<const float4*>(kr + e);
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      const float4 q = *reinterpret_cast<const float4*>(qs + g * DH + e);
      s[g] = fmaf(q.x, kv.x, s[g]); s[g] = fmaf(q.y, kv.y, s[g]); s[g] = fmaf(q.z, kv.z, s[g]); s[g] = fmaf(q.w, kv.w, s[g]);
    }
  }
}

// grid (Hkv * (G / GT), B): workgroup (kv head hk, sub) serves query heads hk * G + sub * GT .. + GT - 1 of row b; sub 0 appends K / V
template <int GT, int DH>
__global__ __launch_bounds__(A_NT) void attn_pos_f32_kernel(const float* __restrict__ qkv, int ld, float* __restrict__ kc, float* __restrict__ vc, int ldkv,
                                                            int Tmax, float* __restrict__ o, int ldo, const int32_t* __restrict__ pos,
                                                            const float* __restrict__ cos_t, const float* __restrict__ sin_t, int H, int Hkv,
                                                            float scale) {
  extern __shared__ __attribute__((aligned(16))) float a_smem[];
  const int t = *pos;
  if (t < 0 || t >= Tmax) return;             // (uniform: nothing is written)
  float* qs = a_smem;                         // [GT][DH] roped queries
  float* kn = qs + GT * DH;                   // [DH] roped new key
  float* vn = kn + DH;                        // [DH] new value
  float* part = vn + DH;                      // [A_NW][GT][DH] partial o per wave
  float* red = part + A_NW * GT * DH;         // [64]
  float* sc = red + 64;                       // [GT][Tmax] scores, then exp(s - max)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = H / Hkv, nsub = G / GT;
  const int hk = blockIdx.x / nsub, sub = blockIdx.x - hk * nsub, b = blockIdx.y;
  const int h0 = hk * G + sub * GT;
  const float* row = qkv + (size_t)b * ld;
  float* kb = kc + (size_t)b * Tmax * ldkv + hk * DH;
  float* vb = vc + (size_t)b * Tmax * ldkv + hk * DH;
  constexpr int half = DH / 2;
  for (int i = tid; i < (GT + 1) * half; i += A_NT) {
    const int hh = i / half, e = i - hh * half;
    const float* src = hh < GT ? row + (size_t)(h0 + hh) * DH : row + (size_t)(H + hk) * DH;
    const float x1 = src[e], x2 = src[e + half];
    const float c1 = cos_t[(size_t)t * DH + e], s1 = sin_t[(size_t)t * DH + e];
    const float c2 = cos_t[(size_t)t * DH + e + half], s2 = sin_t[(size_t)t * DH + e + half];
    const float y1 = x1 * c1 + (-x2) * s1, y2 = x2 * c2 + x1 * s2;      // (pcy_f32_rope's formula)
    float* dst = hh < GT ? qs + hh * DH : kn;
    dst[e] = y1; dst[e + half] = y2;
    if (hh == GT && sub == 0) { kb[(size_t)t * ldkv + e] = y1; kb[(size_t)t * ldkv + e + half] = y2; }
  }
  for (int e = tid; e < DH; e += A_NT) {
    const float v = row[(size_t)(H + Hkv + hk) * DH + e];
    vn[e] = v;
    if (sub == 0) vb[(size_t)t * ldkv + e] = v;
  }
  __syncthreads();
  // scores: a thread per key, the GT heads against one read of the key; slot t comes from LDS (never read back from the cache)
  float mx[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) mx[g] = -INFINITY;
  for (int j = tid; j <= t; j += A_NT) {
    float s[GT];
    if (j < t) qk_dots<GT, DH>(kb + (size_t)j * ldkv, qs, s);
    else qk_dots<GT, DH>(kn, qs, s);
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      const float v = s[g] * scale;
      sc[(size_t)g * Tmax + j] = v;
      mx[g] = fmaxf(mx[g], v);
    }
  }
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    const float m = wave_max(mx[g]);
    if (lane == 0) red[g * A_NW + wave] = m;
  }
  __syncthreads();
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    float m = red[g * A_NW];
#pragma unroll
    for (int w = 1; w < A_NW; ++w) m = fmaxf(m, red[g * A_NW + w]);
    mx[g] = m;
  }
  __syncthreads();
  float sum[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) sum[g] = 0.f;
  for (int j = tid; j <= t; j += A_NT) {
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      const float p = expf(sc[(size_t)g * Tmax + j] - mx[g]);
      sc[(size_t)g * Tmax + j] = p;
      sum[g] += p;
    }
  }
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    const float s = wave_sum(sum[g]);
    if (lane == 0) red[g * A_NW + wave] = s;
  }
  __syncthreads();
  float inv[GT];
#pragma unroll
  for (int g = 0; g < GT; ++g) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < A_NW; ++w) s += red[g * A_NW + w];
    inv[g] = 1.0f / s;
  }
  // P.V: wave w takes keys w, w + A_NW, ...; a lane owns features lane (+ 64)
  constexpr int EPL = DH > 64 ? DH / 64 : 1;
  float acc[GT][EPL];
#pragma unroll
  for (int g = 0; g < GT; ++g)
#pragma unroll
    for (int i = 0; i < EPL; ++i) acc[g][i] = 0.f;
  const bool live = DH >= 64 || lane < DH;
  if (live) {
#pragma unroll 4
    for (int j = wave; j < t; j += A_NW) {
      float v[EPL];
#pragma unroll
      for (int i = 0; i < EPL; ++i) v[i] = vb[(size_t)j * ldkv + lane + 64 * i];
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        const float p = sc[(size_t)g * Tmax + j] * inv[g];
#pragma unroll
        for (int i = 0; i < EPL; ++i) acc[g][i] = fmaf(p, v[i], acc[g][i]);
      }
    }
    if (t % A_NW == wave) {
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        const float p = sc[(size_t)g * Tmax + t] * inv[g];
#pragma unroll
        for (int i = 0; i < EPL; ++i) acc[g][i] = fmaf(p, vn[lane + 64 * i], acc[g][i]);
      }
    }
#pragma unroll
    for (int g = 0; g < GT; ++g)
#pragma unroll
      for (int i = 0; i < EPL; ++i) part[(wave * GT + g) * DH + lane + 64 * i] = acc[g][i];
  }
  __syncthreads();
  for (int idx = tid; idx < GT * DH; idx += A_NT) {
    const int g = idx / DH, e = idx - g * DH;
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < A_NW; ++w) v += part[(w * GT + g) * DH + e];
    o[(size_t)b * ldo + (size_t)(h0 + g) * DH + e] = v;
  }
}

inline int attn_pos_gt(int G) { return G % 4 == 0 ? 4 : G % 2 == 0 ? 2 : 1; }

template <int GT, int DH>
bool launch_attn_pos(hipStream_t s, size_t smem, const float* qkv, int ld, float* kc, float* vc, int ldkv, int Tmax, float* o, int ldo, const int32_t* pos,
                     const float* cos_t, const float* sin_t, int B, int H, int Hkv, float scale) {
  static PcyLdsAttr attr;
  if (!attr.ensure(attn_pos_f32_kernel<GT, DH>, smem)) return false;
  hipLaunchKernelGGL((attn_pos_f32_kernel<GT, DH>), dim3(Hkv * (H / Hkv / GT), B), dim3(A_NT), smem, s, qkv, ld, kc, vc, ldkv, Tmax, o, ldo, pos, cos_t,
                     sin_t, H, Hkv, scale);
  return true;
}
template <int DH, typename... Args>
bool launch_attn_pos_g(int gt, Args... args) {
  return gt == 4 ? launch_attn_pos<4, DH>(args...) : gt == 2 ? launch_attn_pos<2, DH>(args...) : launch_attn_pos<1, DH>(args...);
}

// ------------------------------------------------------------------------------------------------ the step's small kernels
constexpr int E_NT = 256;
__global__ __launch_bounds__(E_NT) void embed_dev_f32_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids, float* __restrict__ out, int d) {
  const float* src = table + (size_t)ids[blockIdx.x] * d;
  for (int k = threadIdx.x; k < d; k += E_NT) out[(size_t)blockIdx.x * d + k] = src[k];
}
// HF's order: w * (x * rsqrt(mean(x^2) + eps))
__global__ __launch_bounds__(E_NT) void rmsnorm_stream_f32_kernel(const float* __restrict__ x, const float* __restrict__ w, float* __restrict__ y, int d,
                                                                  float eps) {
  __shared__ float red[E_NT / 64];
  const float* xr = x + (size_t)blockIdx.x * d;
  float s = 0.f;
  for (int k = threadIdx.x; k < d; k += E_NT) s += xr[k] * xr[k];
  const float r = rsqrtf(block_sum<E_NT>(s, red) / (float)d + eps);
  float* yr = y + (size_t)blockIdx.x * d;
  for (int k = threadIdx.x; k < d; k += E_NT) yr[k] = w[k] * (xr[k] * r);
}
// row (*step, b) of the record <- the step's logits
__global__ __launch_bounds__(E_NT) void record_f32_kernel(const float* __restrict__ logits, float* __restrict__ all, const int32_t* __restrict__ step_dev,
                                                          int B, int V, int ld, const int32_t* __restrict__ done) {
  if (done && *done) return;   // EOS stop: a launch behind *done changes nothing (written by the advance launch only)
  const int b = blockIdx.y;
  const float* src = logits + (size_t)b * V;
  float* dst = all + ((size_t)(*step_dev) * B + b) * ld;
  for (int i = blockIdx.x * E_NT + threadIdx.x; i < V; i += gridDim.x * E_NT) dst[i] = src[i];
}
constexpr int P_NT = 1024;
// one workgroup per row: argmax (lowest index on ties), sum exp(x - max), logprob += (x[tok] - max) - log(sum)
__global__ __launch_bounds__(P_NT) void pick_f32_kernel(const float* __restrict__ logits, int V, int32_t* __restrict__ next_tok, int32_t* __restrict__ tokens_out,
                                                        int max_steps, float* __restrict__ logprob, const int32_t* __restrict__ step_dev, PcyStop stop) {
  __shared__ float redv[P_NT / 64];
  __shared__ int redi[P_NT / 64];
  __shared__ float red[P_NT / 64];
  const int b = blockIdx.x;
  // EOS stop (pcy.h; workgroup-uniform, both words are written behind this point of the step only): nothing once *done is set; a finished
  // row emits eos_id, keeps its logprob and does not read its logits
  if (stop.finished) {
    if (*stop.done) return;
    if (stop.finished[b]) {
      if (threadIdx.x == 0) { next_tok[b] = stop.eos_id; tokens_out[(size_t)b * max_steps + *step_dev] = stop.eos_id; }
      return;
    }
  }
  const float* lg = logits + (size_t)b * V;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < V; i += P_NT) {
    const float v = lg[i];
    if (v > best || (v == best && i < bi)) { best = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { redv[w] = best; redi[w] = bi; }
  __syncthreads();
  best = redv[0]; bi = redi[0];
  for (int i = 1; i < P_NT / 64; ++i)
    if (redv[i] > best || (redv[i] == best && redi[i] < bi)) { best = redv[i]; bi = redi[i]; }
  float se = 0.f;
  for (int i = threadIdx.x; i < V; i += P_NT) se += expf(lg[i] - best);
  se = block_sum<P_NT>(se, red);
  if (threadIdx.x == 0) {
    logprob[b] += (lg[bi] - best) - logf(se);
    next_tok[b] = bi;
    tokens_out[(size_t)b * max_steps + *step_dev] = bi;
    if (stop.finished && bi == stop.eos_id) stop.finished[b] = 1;
  }
}
// (with an EOS stop: behind the picks of every row -- the count of the rows of [0, B) still unfinished raises *done at zero)
// One thread without a stop; with one, a wave: lane l counts rows l, l + 64, ..., lane 0 writes.
__global__ void advance_f32_kernel(int32_t* step_dev, int32_t* pos_dev, int advance_pos, PcyStop stop, int B) {
  int unfinished = 0;
  if (stop.finished) {
    if (*stop.done) return;   // (uniform: lane 0 writes the word at the end only)
    for (int b = threadIdx.x; b < B; b += 64) unfinished += stop.finished[b] == 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) unfinished += __shfl_xor(unfinished, o, 64);
  }
  if (threadIdx.x != 0) return;
  const int step = *step_dev + 1;
  *step_dev = step;
  if (advance_pos) *pos_dev += 1;
  if (stop.finished) {
    if (unfinished == 0) {
      if (stop.n_steps_run) *stop.n_steps_run = step;
      *stop.done = 1;
    }
  }
}

int launch_ok(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { pcy_set_error("kernel launch failed in %s: %s", what, hipGetErrorString(e)); return 3; }
  return 0;
}

}  // namespace

bool pcy_launch_f32_gemv(hipStream_t s, const PcyF32GemvArgs& a0) {
  for (int b0 = 0; b0 < a0.B; b0 += 32) {
    PcyF32GemvArgs a = a0;
    a.B = a0.B - b0 < 32 ? a0.B - b0 : 32;
    a.x = a0.x + (size_t)b0 * a0.ldx;
    a.y = a0.y + (size_t)b0 * a0.ldy;
    if (a0.resid) a.resid = a0.resid + (size_t)b0 * a0.ldr;
    if (!(a.B > 16 ? launch_gemv_f32_epi<2>(s, a) : launch_gemv_f32_epi<1>(s, a))) return false;
  }
  return true;
}

size_t pcy_f32_attn_pos_lds(int H, int Hkv, int dh, int Tmax) {
  const size_t gt = (size_t)attn_pos_gt(H / Hkv);
  return (gt * ((size_t)Tmax + (size_t)(1 + A_NW) * dh) + 2 * (size_t)dh + 64) * sizeof(float);
}

bool pcy_launch_f32_attn_decode_pos(hipStream_t s, const float* qkv, int ld, float* kc, float* vc, int ldkv, int Tmax, float* o, int ldo,
                                    const int32_t* pos, const float* cos_t, const float* sin_t, int B, int H, int Hkv, int dh, float scale) {
  const int gt = attn_pos_gt(H / Hkv);
  const size_t smem = pcy_f32_attn_pos_lds(H, Hkv, dh, Tmax);
  switch (dh) {
    case 16: return launch_attn_pos_g<16>(gt, s, smem, qkv, ld, kc, vc, ldkv, Tmax, o, ldo, pos, cos_t, sin_t, B, H, Hkv, scale);
    case 64: return launch_attn_pos_g<64>(gt, s, smem, qkv, ld, kc, vc, ldkv, Tmax, o, ldo, pos, cos_t, sin_t, B, H, Hkv, scale);
    case 128: return launch_attn_pos_g<128>(gt, s, smem, qkv, ld, kc, vc, ldkv, Tmax, o, ldo, pos, cos_t, sin_t, B, H, Hkv, scale);
  }
  return false;
}

void pcy_launch_f32_embed_dev(hipStream_t s, const float* table, const int32_t* ids, float* out, int rows, int d) {
  hipLaunchKernelGGL(embed_dev_f32_kernel, dim3(rows), dim3(E_NT), 0, s, table, ids, out, d);
}
void pcy_launch_f32_rmsnorm(hipStream_t s, const float* x, const float* w, float* y, int rows, int d, float eps) {
  hipLaunchKernelGGL(rmsnorm_stream_f32_kernel, dim3(rows), dim3(E_NT), 0, s, x, w, y, d, eps);
}
void pcy_launch_f32_record(hipStream_t s, const float* logits, float* logits_all, const int32_t* step_dev, int B, int V, int ld, const int32_t* done) {
  if (!logits_all) return;
  int nb = (V + E_NT - 1) / E_NT;
  nb = nb < 64 ? nb : 64;
  hipLaunchKernelGGL(record_f32_kernel, dim3(nb, B), dim3(E_NT), 0, s, logits, logits_all, step_dev, B, V, ld > 0 ? ld : V, done);
}
void pcy_launch_f32_advance(hipStream_t s, int32_t* step_dev, int32_t* pos_dev, int advance_pos, const PcyStop& stop, int B) {
  hipLaunchKernelGGL(advance_f32_kernel, dim3(1), dim3(stop.finished ? 64 : 1), 0, s, step_dev, pos_dev, advance_pos, stop, B);
}
void pcy_launch_f32_pick(hipStream_t s, const float* logits, int B, int V, int32_t* next_tok, int32_t* tokens_out, int max_steps, float* logprob,
                         int32_t* pos_dev, int32_t* step_dev, int advance_pos, float* logits_all, int logits_all_ld, const PcyStop& stop) {
  pcy_launch_f32_record(s, logits, logits_all, step_dev, B, V, logits_all_ld, stop.finished ? stop.done : nullptr);
  hipLaunchKernelGGL(pick_f32_kernel, dim3(B), dim3(P_NT), 0, s, logits, V, next_tok, tokens_out, max_steps, logprob, step_dev, stop);
  pcy_launch_f32_advance(s, step_dev, pos_dev, advance_pos, stop, B);
}

extern "C" {

int pcy_f32_gemv(pcy_ctx* c, const float* W, const float* W2, const float* x, int ldx, const float* resid, int ldr, float* y, int ldy, int N, int K,
                 int B, int epi) {
  if (epi != EPI_STORE && epi != EPI_RESID && epi != EPI_SWIGLU) { pcy_set_error("pcy_f32_gemv: epi=%d (0 STORE, 1 RESID, 4 SWIGLU)", epi); return 1; }
  if (!W || !x || !y) { pcy_set_error("pcy_f32_gemv: W, x or y is NULL"); return 1; }
  if (epi == EPI_SWIGLU && !W2) { pcy_set_error("pcy_f32_gemv: SWIGLU needs the up matrix W2"); return 1; }
  if (epi == EPI_RESID && !resid) { pcy_set_error("pcy_f32_gemv: RESID needs resid"); return 1; }
  if (B < 1 || N < 1 || K < 4 || K % 4) { pcy_set_error("pcy_f32_gemv: B=%d N=%d K=%d (B, N >= 1, K a positive multiple of 4)", B, N, K); return 1; }
  if (ldx < K || ldx % 4 || ldy < N || (epi == EPI_RESID && ldr < N)) {
    pcy_set_error("pcy_f32_gemv: ldx=%d ldy=%d ldr=%d (rows must hold K / N floats, ldx %% 4 == 0)", ldx, ldy, ldr); return 1;
  }
  if (((reinterpret_cast<uintptr_t>(W) | reinterpret_cast<uintptr_t>(x) | (epi == EPI_SWIGLU ? reinterpret_cast<uintptr_t>(W2) : 0)) & 15) != 0) {
    pcy_set_error("pcy_f32_gemv: W, W2 and x must be 16-byte aligned"); return 1;
  }
  PcyF32GemvArgs a{};
  a.W = W; a.W2 = epi == EPI_SWIGLU ? W2 : nullptr; a.x = x; a.resid = epi == EPI_RESID ? resid : nullptr; a.y = y;
  a.N = N; a.K = K; a.B = B; a.ldx = ldx; a.ldr = ldr; a.ldy = ldy; a.epi = epi;
  if (!pcy_launch_f32_gemv(pcy_ctx_stream(c), a)) { pcy_set_error("pcy_f32_gemv: the device refused the LDS size"); return 1; }
  return launch_ok("pcy_f32_gemv");
}

int pcy_f32_attn_decode_pos(pcy_ctx* c, const float* qkv, int ld, float* kcache, float* vcache, int ldkv, int Tmax, float* o, int ldo,
                            const int32_t* pos, const float* cos_t, const float* sin_t, int B, int H, int Hkv, int dh, float scale) {
  if (!qkv || !kcache || !vcache || !o || !pos || !cos_t || !sin_t) { pcy_set_error("pcy_f32_attn_decode_pos: a NULL pointer"); return 1; }
  if (B < 1 || B > 65535 || Tmax < 1) { pcy_set_error("pcy_f32_attn_decode_pos: B=%d Tmax=%d", B, Tmax); return 1; }
  if (dh != 16 && dh != 64 && dh != 128) { pcy_set_error("pcy_f32_attn_decode_pos: head_dim %d (16, 64 or 128)", dh); return 1; }
  if (Hkv < 1 || H < 1 || H % Hkv) { pcy_set_error("pcy_f32_attn_decode_pos: H=%d Hkv=%d (Hkv | H required)", H, Hkv); return 1; }
  if (ld < (H + 2 * Hkv) * dh || ldkv < Hkv * dh || ldo < H * dh || ld % 4 || ldkv % 4 || ldo % 4) {
    pcy_set_error("pcy_f32_attn_decode_pos: ld=%d ldkv=%d ldo=%d (rows must hold their heads, multiples of 4 floats)", ld, ldkv, ldo); return 1;
  }
  if (((reinterpret_cast<uintptr_t>(qkv) | reinterpret_cast<uintptr_t>(kcache) | reinterpret_cast<uintptr_t>(vcache)) & 15) != 0) {
    pcy_set_error("pcy_f32_attn_decode_pos: qkv and the caches must be 16-byte aligned"); return 1;
  }
  if (pcy_f32_attn_pos_lds(H, Hkv, dh, Tmax) > LDS_MAX - 1024) { pcy_set_error("pcy_f32_attn_decode_pos: %d slots exceed the LDS score buffer", Tmax); return 1; }
  if (!pcy_launch_f32_attn_decode_pos(pcy_ctx_stream(c), qkv, ld, kcache, vcache, ldkv, Tmax, o, ldo, pos, cos_t, sin_t, B, H, Hkv, dh, scale)) {
    pcy_set_error("pcy_f32_attn_decode_pos: the device refused the LDS size"); return 1;
  }
  return launch_ok("pcy_f32_attn_decode_pos");
}

}  // extern "C"
