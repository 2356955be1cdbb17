// Weight-only fp8 (W8A16) streaming GEMV for gfx950: the decode step that streams e4m3 weights.
//
//   y[b][n] = epilogue( (sum_k x[b][k] * f32(q[n][k])) * s[n] ),  b < B <= 8, q in nn.Linear layout [N,K] as OCP e4m3 codes,
//   s[n] the per-output-channel power-of-two scale of pcy_quant_rows_fp8.
//
// The activations stay bf16 and nothing is quantised per call.  Built in the mould of gemv_stream_kernel (pcy_gemv.hip):
//   * persistent waves; a "unit" = R output rows (R features = 2R weight rows for SwiGLU); wave w handles units w, w + n_waves, ...
//   * every lane loads 16 B = 16 codes per row and k-iteration with non-temporal loads (64 lanes x 16 B = 1 KiB contiguous per row);
//     two batches of 16 such loads are in flight per lane, both issued BEFORE the x-staging / RMSNorm prologue
//   * x is staged once per workgroup in LDS as bf16 (optionally RMS-normalised with the reference's rounding points)
//   * codes -> fp32 in hardware (v_cvt_pk_f32_fp8: gfx950 converts OCP e4m3fn, the quantiser's format), fp32 FMAs (two per v_pk_fma_f32),
//     one xor-shuffle tree per output, the scale ONCE on the finished sum, then pcy_gemv's bf16 rounding points
//   * the order of a (row, output) sum is a function of the output row and K alone: lane l owns elements [16 l, 16 l + 16) of every
//     1024-element k-iteration, the iterations of output row r are walked rotated by (r / 4) % (K / 1024) when K % 1024 == 0 (all waves of
//     the chip otherwise read the same 1 KiB window of their rows at the same moment, and K = 4096 makes the row stride a power of two
//     again), and neither depends on B or on what the other rows of the call hold.
#include "pcy_internal.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float w8_f32x2;

constexpr int W8_MAX_WAVES = 2048;   // 256 CUs x 2 waves/SIMD x 4 SIMDs
constexpr int W8_CUS = 256;
constexpr size_t W8_LDS_MAX = 160 * 1024;   // LDS of a gfx950 CU; x rows + the reduction words must fit

// 16 codes x 16 bf16 -> two fp32 partial sums (even / odd elements), added onto acc.  xa = elements 0..7, xb = 8..15 of the lane's piece.
__device__ __forceinline__ w8_f32x2 dot16_w8(const uint4& w, const uint4& xa, const uint4& xb, w8_f32x2 acc) {
  const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
  const uint32_t xw[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const w8_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)ww[j], false);   // codes 4j, 4j + 1
    const w8_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)ww[j], true);    // codes 4j + 2, 4j + 3
    const w8_f32x2 x0 = {lo_bf(xw[2 * j]), hi_bf(xw[2 * j])};
    const w8_f32x2 x1 = {lo_bf(xw[2 * j + 1]), hi_bf(xw[2 * j + 1])};
    acc = __builtin_elementwise_fma(lo, x0, acc);
    acc = __builtin_elementwise_fma(hi, x1, acc);
  }
  return acc;
}

typedef const __attribute__((address_space(1))) u32x4_t* w8_gptr;
__device__ __forceinline__ uint4 ldg_nt_w8(const uint8_t* p) {
  const u32x4_t v = __builtin_nontemporal_load((w8_gptr)(p));
  return make_uint4(v[0], v[1], v[2], v[3]);
}

template <int NB, int EPI, bool RMS, int R>
__global__ __launch_bounds__(512) void gemv_w8_kernel(PcyGemvW8Args a, int units) {
  constexpr int RW = (EPI == EPI_SWIGLU) ? 2 * R : R;
  constexpr int UN = 16 / RW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* xs = reinterpret_cast<bf16_t*>(smem);                          // [NB][K]
  float* red = reinterpret_cast<float*>(smem + (size_t)NB * a.K * 2);    // [waves per block]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int K = a.K;
  const int nit = (K + 1023) >> 10;   // 1024 elements per wave-iteration
  const int wpb = blockDim.x >> 6;
  const int nw = gridDim.x * wpb;
  const int nthr = blockDim.x;
  const int nrows = (EPI == EPI_SWIGLU) ? 2 * a.N : a.N;

  // weight row i of unit u (clamped into the matrix)
  auto row_of = [&](int u, int i) -> int {
    if (EPI == EPI_SWIGLU) {
      const int f = u * R + (i % R);
      const int fc = f < a.N ? f : a.N - 1;
      return (fc >> 4) * 32 + (fc & 15) + (i >= R ? 16 : 0);
    }
    const int r = u * R + i;
    return r < nrows ? r : nrows - 1;
  };
  const bool krot = (K & 1023) == 0;
  auto rot = [&](int u, int it) { if (!krot) return it; const int r = it + ((u * R) >> 2) % nit; return r >= nit ? r - nit : r; };
  auto issue = [&](int u, int it0, uint4 (&wv)[UN][RW]) {
#pragma unroll
    for (int un = 0; un < UN; ++un) {
      const bool ok = it0 + un < nit;
      const int k = ok ? (rot(u, it0 + un) * 64 + lane) * 16 : 0;
#pragma unroll
      for (int i = 0; i < RW; ++i)
        wv[un][i] = (ok && k < K) ? ldg_nt_w8(a.W + (size_t)row_of(u, i) * K + k) : make_uint4(0, 0, 0, 0);
    }
  };
  w8_f32x2 acc[RW][NB];
  auto zero_acc = [&]() {
#pragma unroll
    for (int i = 0; i < RW; ++i)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[i][b] = (w8_f32x2){0.f, 0.f};
  };
  auto compute = [&](int u, int it0, const uint4 (&wv)[UN][RW]) {
#pragma unroll
    for (int un = 0; un < UN; ++un) {
      if (it0 + un < nit) {
        const int k = (rot(u, it0 + un) * 64 + lane) * 16;
        if (k < K) {
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const uint4 xa = *reinterpret_cast<const uint4*>(xs + (size_t)b * K + k);
            const uint4 xb = *reinterpret_cast<const uint4*>(xs + (size_t)b * K + k + 8);
#pragma unroll
            for (int i = 0; i < RW; ++i) acc[i][b] = dot16_w8(wv[un][i], xa, xb, acc[i][b]);
          }
        }
      }
    }
  };
  auto finish = [&](int u) {
    float sum[RW][NB];
#pragma unroll
    for (int i = 0; i < RW; ++i)
#pragma unroll
      for (int b = 0; b < NB; ++b) sum[i][b] = wave_sum(acc[i][b][0] + acc[i][b][1]);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int n = u * R + i;
        if (n >= a.N) continue;
        const float s0 = a.scale[row_of(u, i)];
        const float s1 = EPI == EPI_SWIGLU ? a.scale[row_of(u, i + R)] : 0.f;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          float v;
          if (EPI == EPI_SWIGLU) {
            const float g = rbf(sum[i][b] * s0), up = rbf(sum[(EPI == EPI_SWIGLU) ? i + R : i][b] * s1);
            v = rbf(silu_f(g)) * up;
          } else {
            v = rbf(sum[i][b] * s0);
            if (EPI == EPI_RESID) v = rbf(v + bf2f(a.resid[(size_t)b * a.ldy + n]));
          }
          a.y[(size_t)b * a.ldy + n] = f2bf(v);
        }
      }
    }
    zero_acc();
  };

  uint4 wa[UN][RW], wb[UN][RW];
  int u = blockIdx.x * wpb + wave;
  int it0 = 0;
  bool have = u < units;
  // position of the batch after (cu, cit)
  auto next_pos = [&](int cu, int cit, int& nu_, int& nit_) {
    nit_ = cit + UN; nu_ = cu;
    if (nit_ >= nit) { nit_ = 0; nu_ = cu + nw; }
  };
  // two weight batches (32 x 16 B per lane) go out before anything else
  int u1, it1;
  if (have) issue(u, 0, wa);
  next_pos(u, 0, u1, it1);
  bool have1 = have && u1 < units;
  if (have1) issue(u1, it1, wb);

  // ---- prologue: x (optionally RMS-normalised) -> LDS, while the weights stream ----
  float rstd[NB];
  if (RMS) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float ss = 0.f;
      for (int k = threadIdx.x * 8; k < K; k += nthr * 8) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.x + (size_t)b * a.ldx + k);
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) { const float f0 = lo_bf(w4[j]), f1 = hi_bf(w4[j]); ss += f0 * f0 + f1 * f1; }
      }
      ss = block_sum_rt(ss, red, wpb);
      rstd[b] = rsqrtf(ss / (float)K + a.rms_eps);
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    for (int k = threadIdx.x * 8; k < K; k += nthr * 8) {
      uint4 v = *reinterpret_cast<const uint4*>(a.x + (size_t)b * a.ldx + k);
      if (RMS) {
        const uint4 g = *reinterpret_cast<const uint4*>(a.rms_w + k);
        const uint32_t xin[4] = {v.x, v.y, v.z, v.w}, gin[4] = {g.x, g.y, g.z, g.w};
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float x0 = lo_bf(xin[j]) * rstd[b], x1 = hi_bf(xin[j]) * rstd[b];
          if (a.rms_cast == 0) { x0 = rbf(x0); x1 = rbf(x1); }
          o[j] = pack_bf(lo_bf(gin[j]) * x0, hi_bf(gin[j]) * x1);
        }
        v = make_uint4(o[0], o[1], o[2], o[3]);
      }
      *reinterpret_cast<uint4*>(xs + (size_t)b * K + k) = v;
    }
  }
  __syncthreads();
  zero_acc();

  // ---- steady state, two batches deep: batch i sits in CUR, batch i+1 is on its way into NXT; after consuming i its registers take i+2 ----
#define PCY_W8_STEP(CUR)                                         \
  {                                                              \
    compute(u, it0, CUR);                                        \
    if (it0 + UN >= nit) finish(u);                              \
    int u2, it2;                                                 \
    next_pos(u1, it1, u2, it2);                                  \
    const bool have2 = have1 && u2 < units;                      \
    if (have2) issue(u2, it2, CUR);                              \
    u = u1; it0 = it1; have = have1;                             \
    u1 = u2; it1 = it2; have1 = have2;                           \
  }
  while (have) {
    PCY_W8_STEP(wa)
    if (!have) break;
    PCY_W8_STEP(wb)
  }
#undef PCY_W8_STEP
}

// Grid shape (pick_grid of pcy_gemv.hip): a multiple of the CU count with 4..8 waves per workgroup, chosen so that every CU streams the same
// number of rows; one workgroup per CU when two would not fit its LDS.  A function of (N, K) and the rows per pass only.
inline void pick_grid_w8(int units, bool one_per_cu, int& blocks, int& wpb) {
  double best = 1e30;
  blocks = W8_CUS; wpb = 4;
  for (int bl = W8_CUS; bl <= (one_per_cu ? 1 : 2) * W8_CUS; bl += W8_CUS)
    for (int w = 4; w <= 8; ++w) {
      const int waves = bl * w;
      if (waves > W8_MAX_WAVES) continue;
      const int per = (units + waves - 1) / waves;
      const double cost = (double)per * waves / units + 1e-3 * (W8_MAX_WAVES - waves) / W8_MAX_WAVES;
      if (cost < best) { best = cost; blocks = bl; wpb = w; }
    }
  if (units < W8_CUS * 4) { blocks = (units + 3) / 4; wpb = 4; }
}

template <int NB, int EPI, bool RMS, int R>
bool launch_w8_r(hipStream_t s, const PcyGemvW8Args& a) {
  static PcyLdsAttr attr;
  const int units = (a.N + R - 1) / R;
  const size_t smem = (size_t)NB * a.K * 2 + 64;
  if (!attr.ensure(gemv_w8_kernel<NB, EPI, RMS, R>, smem)) return false;
  int blocks, wpb;
  pick_grid_w8(units, 2 * smem > W8_LDS_MAX, blocks, wpb);
  hipLaunchKernelGGL((gemv_w8_kernel<NB, EPI, RMS, R>), dim3(blocks), dim3(wpb * 64), smem, s, a, units);
  return true;
}
template <int NB, int EPI, bool RMS>
bool launch_w8_nb(hipStream_t s, const PcyGemvW8Args& a) {
  // few rows -> 2-row units so that the launch still spreads over ~2k waves (a function of N alone: a row's bits do not depend on B).
  // SwiGLU: always 2 features = 4 weight rows per unit (8 weight rows x 4 batch rows of accumulators beside the two weight batches spill).
  if (EPI == EPI_SWIGLU || (a.N + 3) / 4 < W8_MAX_WAVES) return launch_w8_r<NB, EPI, RMS, 2>(s, a);
  return launch_w8_r<NB, EPI, RMS, (EPI == EPI_SWIGLU ? 2 : 4)>(s, a);
}
template <int NB>
bool launch_w8_epi(hipStream_t s, const PcyGemvW8Args& a) {
  const bool rms = a.rms_w != nullptr;
  switch (a.epi) {
    case EPI_STORE: return rms ? launch_w8_nb<NB, EPI_STORE, true>(s, a) : launch_w8_nb<NB, EPI_STORE, false>(s, a);
    case EPI_RESID: return launch_w8_nb<NB, EPI_RESID, false>(s, a);
    case EPI_SWIGLU: return rms ? launch_w8_nb<NB, EPI_SWIGLU, true>(s, a) : launch_w8_nb<NB, EPI_SWIGLU, false>(s, a);
  }
  return false;
}

}  // namespace

int pcy_gemv_w8_rows_per_pass(int K) {
  const size_t per_row = (size_t)K * 2;
  const size_t fit = K > 0 ? (W8_LDS_MAX - 64) / per_row : 0;
  return fit >= 4 ? 4 : (int)fit;
}

bool pcy_launch_gemv_w8(hipStream_t s, const PcyGemvW8Args& a0) {
  const int per = pcy_gemv_w8_rows_per_pass(a0.K);
  if (per < 1) return false;
  for (int b0 = 0; b0 < a0.B; b0 += per) {
    PcyGemvW8Args a = a0;
    a.B = (a0.B - b0) < per ? (a0.B - b0) : per;
    a.x = a0.x + (size_t)b0 * a0.ldx;
    a.y = a0.y + (size_t)b0 * a0.ldy;
    if (a0.resid) a.resid = a0.resid + (size_t)b0 * a0.ldy;
    bool ok = false;
    switch (a.B) {
      case 1: ok = launch_w8_epi<1>(s, a); break;
      case 2: ok = launch_w8_epi<2>(s, a); break;
      case 3: ok = launch_w8_epi<3>(s, a); break;
      default: ok = launch_w8_epi<4>(s, a); break;
    }
    if (!ok) return false;
  }
  return true;
}
