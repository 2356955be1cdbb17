// The main loop of the fp32 Linear (pcy_f32.hip), shared by linear_f32_kernel and the fused lm_head x cross-entropy kernel
// (f32_xent_partial_kernel) so that both produce the same accumulator bits: v_mfma_f32_16x16x4_f32 on exact fp32 products, fp32
// accumulation in ascending k (== an fmaf chain), 128 x 128 x 16 tiles, register-staged double buffer.  Operands are fed swapped (W rows as
// the MFMA A operand), so a lane ends up with 4 consecutive output features of one token.
#pragma once
#include "pcy_common.h"

constexpr int F_NT = 256;                                             // 2 x 2 waves of 64 tokens x 64 features
constexpr int F_TM = 128, F_TN = 128, F_BK = 16, F_LD = F_BK + 1;     // LDS row stride 17 floats: conflict-free ds_read_b32 fragments
constexpr int F_TILE_LDS = 2 * F_TM * F_LD;                           // floats per operand (two buffers)

// acc[i][j] <- A[m0.., :K] . W[n0.., :K]^T for the 128 x 128 tile at (m0, n0); rows >= M / >= N are clamped on load (their products land
// in accumulators the caller masks).  As / Ws: F_TILE_LDS floats each.  Ends behind a barrier: the buffers are free on return.
// On return lane (fr = lane & 15, fq = lane >> 4) of wave (wm, wn) holds D[feature n0 + wn*64 + i*16 + fq*4 + r][token m0 + wm*64 + j*16 + fr]
// in acc[i][j][r].
__device__ __forceinline__ void f32_tile_mainloop(const float* __restrict__ A, int lda, const float* __restrict__ W, int M, int N, int K, int m0,
                                                  int n0, float* As, float* Ws, f32x4 (&acc)[4][4]) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // staging: 128 rows x 16 floats = 512 float4 per operand, two per thread
  const int sr = tid >> 2, sc = (tid & 3) * 4;              // rows sr and sr + 64, columns sc .. sc+3
  const float* ap[2]; const float* wp[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int ra = m0 + sr + 64 * i; ra = ra < M ? ra : M - 1;
    int rw = n0 + sr + 64 * i; rw = rw < N ? rw : N - 1;
    ap[i] = A + (size_t)ra * lda + sc;
    wp[i] = W + (size_t)rw * K + sc;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float4 ra[2], rw[2];
  auto gload = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) { ra[i] = *reinterpret_cast<const float4*>(ap[i] + k0); rw[i] = *reinterpret_cast<const float4*>(wp[i] + k0); }
  };
  auto sstore = [&](int b) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float* a = &As[b * (F_TM * F_LD) + (sr + 64 * i) * F_LD + sc];
      float* w = &Ws[b * (F_TN * F_LD) + (sr + 64 * i) * F_LD + sc];
      a[0] = ra[i].x; a[1] = ra[i].y; a[2] = ra[i].z; a[3] = ra[i].w;
      w[0] = rw[i].x; w[1] = rw[i].y; w[2] = rw[i].z; w[3] = rw[i].w;
    }
  };
  const int nk = K / F_BK;
  gload(0);
  sstore(0);
  __syncthreads();
  const int fr = lane & 15, fq = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int b = kt & 1;
    const float* Ab = As + b * (F_TM * F_LD);
    const float* Wb = Ws + b * (F_TN * F_LD);
    if (kt + 1 < nk) gload((kt + 1) * F_BK);
#pragma unroll
    for (int k4 = 0; k4 < F_BK / 4; ++k4) {
      float xf[4], wf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) xf[j] = Ab[(wm * 64 + j * 16 + fr) * F_LD + k4 * 4 + fq];
#pragma unroll
      for (int i = 0; i < 4; ++i) wf[i] = Wb[(wn * 64 + i * 16 + fr) * F_LD + k4 * 4 + fq];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i], xf[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) sstore(b ^ 1);
    __syncthreads();
  }
}
