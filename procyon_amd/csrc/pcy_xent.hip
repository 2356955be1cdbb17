// lm_head x cross-entropy for teacher-forced scoring (pcy_lm_head_xent, pcy_llama_score): per token row m
//
//   nll[m] = logsumexp_n( bf16(x[m] . W[n]) ) - bf16(x[m] . W[targets[m]])
//
// which is HF's causal-LM loss per labelled token (`logits = bf16(acc)`, `logits.float()`, fp32 cross_entropy) -- without the
// [M, V] logits ever reaching memory: the row statistics are taken in the epilogue of the GEMM, on the accumulators.
//
//   * main loop: the 128-column tile loop of gemm_kernel (pcy_gemm.hip) -- same loaders, same fragment layout (pcy_gemm_tile.h), same
//     k order per element -- so the rounded logit of (m, n) is bit-equal to what pcy_gemm(x, W, EPI_STORE) stores, whichever of its
//     non-split-K kernels runs.  Row tile 32 / 64 / 128 tokens by M (2 x 2 waves, WTM = 1 / 2 / 4 MFMA tiles per wave along tokens).
//   * a workgroup walks the xent_cb(V) consecutive 128-column tiles of ONE column block and carries (max, sum exp) per lane and token
//     across them (online rescale); the lane layout is D[n = fq*4 + r][m = fr], so a lane's 16 values per tile and token are columns
//     i*16 + fq*4 + r.  Columns >= V contribute nothing (W rows are clamped on load, masked here).  At the end of the block: merge over
//     the four fq lane groups (xor 16, 32), then over the two waves along N through LDS, and ONE (max, sumexp) pair per (column block,
//     row) goes to the workspace part[cb][m] as a plain 8-byte store.  The one lane that holds column targets[m] stores label[m].
//   * finish kernel: one wave per row merges the column-block partials -- lane l takes blocks l, l + 64, ... in order, then a xor
//     butterfly -- and writes lse, row_max, nll.
//   * no atomics; the column partition and every merge order are functions of V alone, so a row's nll / lse / label bits do not depend
//     on M or on which other rows are scored.  Every merge is written symmetrically ((a, b) and (b, a) give the same bits).
//   * rows are scored in chunks of XENT_MCHUNK, so the workspace is min(M, XENT_MCHUNK) x (n_col_blocks x 8 + 4) bytes.
#include <math.h>
#include "pcy_internal.h"
#include "pcy_gemm_tile.h"

namespace {

constexpr int XENT_THREADS = 256, XENT_BN = 128, XENT_BK = 64;
constexpr int XENT_MCHUNK = 1024;

// 128-column tiles per column block: at most 512 column blocks (two workgroups per CU on 256 CUs for ONE row tile), a function of V only
inline int xent_cb(int V) {
  const int tiles_n = (V + XENT_BN - 1) / XENT_BN;
  return (tiles_n + 511) / 512;
}
inline int xent_ncb(int V) {
  const int tiles_n = (V + XENT_BN - 1) / XENT_BN, cb = xent_cb(V);
  return (tiles_n + cb - 1) / cb;
}

struct XentKArgs {
  const bf16_t* x; int ldx;     // [M, d] rows of this chunk
  const bf16_t* W;              // [V, d]
  const int32_t* targets;       // [M]
  int M, V, d, cb, ncb, stride; // stride = rows of the partial buffer
  float2* part;                 // [ncb][stride] (max, sumexp)
  float* label;                 // [M] bf16-rounded logit of the target column
};

// (m, s) <- merge of (m, s) and (om, os): s counts exp(. - m).  Symmetric in its two arguments; an empty side is (-inf, 0).
__device__ __forceinline__ void xent_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  const float a = (m == nm) ? s : s * expf(m - nm);
  const float b = (om == nm) ? os : os * expf(om - nm);
  m = nm;
  s = a + b;
}

template <int WTM>
__global__ __launch_bounds__(XENT_THREADS) void xent_partial_kernel(XentKArgs a) {
  constexpr int BK = XENT_BK, TM = 2 * WTM * 16, TN = XENT_BN, WTN = 4;
  constexpr int TILE_A = TM * BK * 2, TILE_W = TN * BK * 2;
  __shared__ __attribute__((aligned(1024))) char smem[2 * (TILE_A + TILE_W)];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  // XCD-aware order (as gemm_kernel): every XCD takes a contiguous run of the logical order, in which the row tiles of a column
  // block are neighbours -- they stream the same W panels through one L2
  const int nwg = gridDim.x, bid = blockIdx.x;
  const int xq = nwg >> 3, xr = nwg & 7, xcd = bid & 7;
  const int t = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (bid >> 3);
  const int tiles_m = (a.M + TM - 1) / TM;
  const int cblk = t / tiles_m, m0 = (t - cblk * tiles_m) * TM;
  const int nk = a.d / BK;
  const float NEG_INF = -__builtin_inff();

  int tg[WTM];
  float mx[WTM], sm[WTM], lab[WTM];
  unsigned found = 0;
#pragma unroll
  for (int j = 0; j < WTM; ++j) {
    const int m = m0 + wm * WTM * 16 + j * 16 + fr;
    tg[j] = a.targets[m < a.M ? m : a.M - 1];
    mx[j] = NEG_INF; sm[j] = 0.f; lab[j] = 0.f;
  }

  for (int ct = 0; ct < a.cb; ++ct) {
    const int n0 = (cblk * a.cb + ct) * TN;
    if (n0 >= a.V) break;   // (uniform: the last column block may hold fewer tiles)
    f32x4 acc[WTN][WTM];
#pragma unroll
    for (int i = 0; i < WTN; ++i)
#pragma unroll
      for (int j = 0; j < WTM; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    stage_tile<BK, TM, 4, 0, 1>(a.x, a.ldx, m0, a.M, 0, smem, wave, lane);
    stage_tile<BK, TN, 4, 0, 1>(a.W, a.d, n0, a.V, 0, smem + TILE_A, wave, lane);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
      const int cur = kt & 1;
      const char* Acur = smem + cur * (TILE_A + TILE_W);
      const char* Wcur = Acur + TILE_A;
      if (kt + 1 < nk) {
        char* Anext = smem + (cur ^ 1) * (TILE_A + TILE_W);
        stage_tile<BK, TM, 4, 0, 1>(a.x, a.ldx, m0, a.M, (kt + 1) * BK, Anext, wave, lane);
        stage_tile<BK, TN, 4, 0, 1>(a.W, a.d, n0, a.V, (kt + 1) * BK, Anext + TILE_A, wave, lane);
      }
#pragma unroll
      for (int kb = 0; kb < BK / 32; ++kb) {
        bf16x8 xf[WTM], wf[WTN];
#pragma unroll
        for (int j = 0; j < WTM; ++j) xf[j] = lds_frag<BK>(Acur, wm * WTM * 16 + j * 16 + fr, kb * 4 + fq);
#pragma unroll
        for (int i = 0; i < WTN; ++i) wf[i] = lds_frag<BK>(Wcur, wn * WTN * 16 + i * 16 + fr, kb * 4 + fq);
#pragma unroll
        for (int i = 0; i < WTN; ++i)
#pragma unroll
          for (int j = 0; j < WTM; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], xf[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
    // row statistics of this tile on the ROUNDED logits (rbf(acc + 0) is gemm_epilogue's value without a bias)
    const int nb = n0 + wn * 64 + fq * 4;
#pragma unroll
    for (int j = 0; j < WTM; ++j) {
      float v[WTN][4];
      float tmax = NEG_INF;
#pragma unroll
      for (int i = 0; i < WTN; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = nb + i * 16 + r;
          const float l = rbf(acc[i][j][r] + 0.f);
          if (n == tg[j]) { lab[j] = l; found |= 1u << j; }
          v[i][r] = n < a.V ? l : NEG_INF;
          tmax = fmaxf(tmax, v[i][r]);
        }
      const float nm = fmaxf(mx[j], tmax);
      float s = (mx[j] == nm) ? sm[j] : sm[j] * expf(mx[j] - nm);
#pragma unroll
      for (int i = 0; i < WTN; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) s += v[i][r] > NEG_INF ? expf(v[i][r] - nm) : 0.f;
      mx[j] = nm; sm[j] = s;
    }
  }

  // the four fq groups hold disjoint columns of the same tokens
#pragma unroll
  for (int j = 0; j < WTM; ++j) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float om = __shfl_xor(mx[j], off), os = __shfl_xor(sm[j], off);
      xent_merge(mx[j], sm[j], om, os);
    }
  }
  // the two waves along N: through LDS (the tile buffers are dead behind the k-loop's last barrier)
  float2* red = reinterpret_cast<float2*>(smem);
  if (wn == 1 && fq == 0) {
#pragma unroll
    for (int j = 0; j < WTM; ++j) red[wm * WTM * 16 + j * 16 + fr] = make_float2(mx[j], sm[j]);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < WTM; ++j) {
    const int ml = wm * WTM * 16 + j * 16 + fr, m = m0 + ml;
    if (m >= a.M) continue;
    if (wn == 0 && fq == 0) {
      const float2 o = red[ml];
      xent_merge(mx[j], sm[j], o.x, o.y);
      a.part[(size_t)cblk * a.stride + m] = make_float2(mx[j], sm[j]);
    }
    if (found & (1u << j)) a.label[m] = lab[j];
  }
}

// one wave per row
__global__ __launch_bounds__(256) void xent_finish_kernel(const float2* __restrict__ part, int ncb, int stride, int M, const int32_t* __restrict__ targets,
                                                          int V, const float* __restrict__ label, float* nll, float* lse_out, float* max_out,
                                                          float* label_out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  float m = -__builtin_inff(), s = 0.f;
  for (int cb = lane; cb < ncb; cb += 64) {
    const float2 p = part[(size_t)cb * stride + row];
    xent_merge(m, s, p.x, p.y);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float om = __shfl_xor(m, off), os = __shfl_xor(s, off);
    xent_merge(m, s, om, os);
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

template <int WTM>
void launch_partial(hipStream_t s, const XentKArgs& k) {
  constexpr int TM = 2 * WTM * 16;
  const int tiles_m = (k.M + TM - 1) / TM;
  hipLaunchKernelGGL((xent_partial_kernel<WTM>), dim3(tiles_m * k.ncb), dim3(XENT_THREADS), 0, s, k);
}

}  // namespace

int pcy_xent_col_blocks(int V) { return xent_ncb(V); }

size_t pcy_xent_ws_bytes(int M, int V) {
  const size_t mc = (size_t)(M < XENT_MCHUNK ? M : XENT_MCHUNK);
  return ((mc * xent_ncb(V) * 8 + 255) / 256 * 256) + ((mc * 4 + 255) / 256 * 256);
}

void pcy_launch_lm_head_xent(hipStream_t s, const PcyXentArgs& a) {
  if (a.M <= 0) return;
  const int ncb = xent_ncb(a.V);
  const int stride = a.M < XENT_MCHUNK ? a.M : XENT_MCHUNK;
  float2* part = reinterpret_cast<float2*>(a.ws);
  float* label = reinterpret_cast<float*>(reinterpret_cast<char*>(a.ws) + ((size_t)stride * ncb * 8 + 255) / 256 * 256);
  for (int r0 = 0; r0 < a.M; r0 += XENT_MCHUNK) {
    const int mc = a.M - r0 < XENT_MCHUNK ? a.M - r0 : XENT_MCHUNK;
    XentKArgs k;
    k.x = a.x + (size_t)r0 * a.ldx; k.ldx = a.ldx; k.W = a.W; k.targets = a.targets + r0;
    k.M = mc; k.V = a.V; k.d = a.d; k.cb = xent_cb(a.V); k.ncb = ncb; k.stride = stride; k.part = part; k.label = label;
    if (mc <= 32) launch_partial<1>(s, k);
    else if (mc <= 64) launch_partial<2>(s, k);
    else launch_partial<4>(s, k);
    hipLaunchKernelGGL(xent_finish_kernel, dim3((mc + 3) / 4), dim3(256), 0, s, part, ncb, stride, mc, a.targets + r0, a.V, label, a.nll + r0,
                       a.lse ? a.lse + r0 : nullptr, a.row_max ? a.row_max + r0 : nullptr, a.label_logit ? a.label_logit + r0 : nullptr);
  }
  ++g_pcy_dispatch[PCY_DISPATCH_XENT];
}
