// Window attention (pcy_attn_window): W consecutive tokens of ONE cache row -- a lookahead pass -- against the keys the cache
// already holds plus their own, with the past cut into key chunks across workgroups and the position read from device memory.
//
// The arithmetic is attn_ext_kernel's (pcy_attn_ext.hip), rounding point for rounding point:
//   S = bf16(Q.K^T) ; S = bf16(S * scale) ; P = bf16(softmax_fp32(S)) normalised BEFORE the rounding ; O = bf16(P.V)
// with the same MFMA operand layout (S^T = K.Q^T, a lane ends with 8 consecutive keys of one query), the same XOR-swizzled K image and the
// same ds_read_b64_tr_b16 V path.  What differs is the work split (design (a) of the issue: a global (m, l), p normalised before P.V):
//   win_prologue_kernel   one wave per (window row i, head): rope q -> workspace, rope k -> cache slot *pos + i, v -> cache slot *pos + i
//   attn_win_kernel<.,0>  workgroup (chunk c, kv head g, 64 packed queries): the chunk's (row max, sum of exp2) per query -> workspace
//   attn_win_kernel<.,1>  the same workgroup recomputes the chunk's scores (same bits), combines the (m, l) of the query's chunks IN CHUNK
//                         ORDER, and leaves the chunk's fp32 P.V in the workspace
//   win_combine_kernel    o = bf16(sum of the chunks' partial sums, in chunk order)
// No atomics, no flags: the launches order the phases.  A chunk is PCY_WIN_CHUNK keys, a constant; the grid is sized from the cache capacity
// and a workgroup whose chunk starts at or beyond *pos + W returns before any write, so nothing a live workgroup computes depends on the
// capacity.  *pos < 0 or *pos + W > Tmax: every workgroup of every launch returns at once.
//
// The W * G queries of a kv head (G = H / Hkv) are packed i-major, packed index = i * G + hg, into 16-wide MFMA tiles; a wave owns one tile,
// a workgroup four.  Every 32-key K tile and V tile of the chunk is staged once for the workgroup's tiles.
//
// What a query may see.  Query i sits at slot *pos + i and attends slots [0, *pos + i].  A key beyond that is masked by SELECT (-inf score,
// p = +0), and rows beyond *pos + W - 1 are never loaded (the staging clamps the slot).  That covers K; for V a zero probability is not
// enough, 0 * NaN = NaN inside the MFMA.  So a block that holds window slots runs P.V once per window row ii present in the tile: the
// probabilities of the other rows' queries and the V rows above slot *pos + ii are replaced by zeros, and the product is added to the
// accumulators of row ii's queries only (again by select).  Nothing that a later draft's row holds -- q, k or v, NaN included -- reaches an
// earlier row's output.
#include "pcy_internal.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short win_s16x4;
typedef __attribute__((ext_vector_type(8))) short win_s16x8;

constexpr int WIN_C = PCY_WIN_CHUNK;
static_assert(WIN_C % 32 == 0 && WIN_C >= 32, "a chunk is a whole number of 32-key blocks");

__device__ __forceinline__ bool win_pos_ok(int pos, int W, int Tmax) { return pos >= 0 && pos <= Tmax - W; }

// one wave per (window row, head of qkv).  Rope: every product a bf16 tensor (rope_row, mode 0, pcy_elem.hip): the bits pcy_attn_extend appends.
__global__ __launch_bounds__(64) void win_prologue_kernel(PcyWinAttnArgs a) {
  const int pos = *a.pos_dev;
  if (!win_pos_ok(pos, a.W, a.Tmax)) return;
  const int i = blockIdx.x, h = blockIdx.y, p = pos + i, dh = a.dh, half = dh >> 1;
  const bf16_t* x = a.qkv + (size_t)i * a.ld + h * dh;
  if (h >= a.H + a.Hkv) {                      // a v head: a copy
    bf16_t* dst = a.vcache + ((size_t)(h - a.H - a.Hkv) * a.Tmax + p) * dh;
    for (int j = threadIdx.x; j < dh; j += 64) dst[j] = x[j];
    return;
  }
  const bf16_t* c = a.cos_t + (size_t)p * dh;
  const bf16_t* s = a.sin_t + (size_t)p * dh;
  bf16_t* dst = h < a.H ? a.qr + (size_t)i * a.H * dh + h * dh : a.kcache + ((size_t)(h - a.H) * a.Tmax + p) * dh;
  for (int j = threadIdx.x; j < half; j += 64) {
    const float x1 = bf2f(x[j]), x2 = bf2f(x[j + half]);
    dst[j] = f2bf(rbf(rbf(x1 * bf2f(c[j])) + rbf(-x2 * bf2f(s[j]))));
    dst[j + half] = f2bf(rbf(rbf(x2 * bf2f(c[j + half])) + rbf(x1 * bf2f(s[j + half]))));
  }
}

// PHASE 0: the chunk's (m, l) of every query.  PHASE 1: the chunk's P.V under the global (m, l).
template <int DH, int PHASE>
__global__ __launch_bounds__(256) void attn_win_kernel(PcyWinAttnArgs a) {
  constexpr int KB = DH / 32, NT = DH / 16;
  constexpr int KCH = DH / 8;                  // 16-B chunks per K / V row
  constexpr int NLD = (32 * KCH) / 256;        // chunks per thread and tile
  constexpr int KTILE = 32 * DH * 2;
  constexpr int VSTR = DH * 2 + 32;
  constexpr int VTILE = PHASE ? 32 * VSTR : 0;
  __shared__ __attribute__((aligned(16))) char smem[2 * (KTILE + VTILE)];
  const int pos = *a.pos_dev;
  const int W = a.W;
  if (!win_pos_ok(pos, W, a.Tmax)) return;     // (uniform for the whole launch)
  const int nk = pos + W;                      // keys of the row after the append
  const int c = blockIdx.x, k0 = c * WIN_C;
  if (k0 >= nk) return;                        // a chunk beyond the live range: workgroup-uniform, nothing written
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int g = blockIdx.y;
  const int G = a.H / a.Hkv, gs = __ffs(G) - 1;   // (G is 1, 2, 4 or 8)
  const int total = W * G;                     // packed queries of this kv head
  const int iw0 = (blockIdx.z * 4 + wave) * 16;
  const bool active = iw0 < total;             // wave-uniform
  constexpr float LOG2E = 1.4426950408889634f;
  // this lane's query (slots beyond the last packed query repeat it: finite statistics, never stored)
  int idx = iw0 + fr;
  idx = idx < total ? idx : total - 1;
  const int qi = idx >> gs, qh = idx & (G - 1);
  const int qpos = pos + qi;                   // the query's slot = its last allowed key
  const bool q_live = (iw0 + fr) < total && k0 <= qpos;   // the chunk holds a key of this query
  const bf16_t* kc = a.kcache + (size_t)g * a.Tmax * DH;
  const bf16_t* vc = a.vcache + (size_t)g * a.Tmax * DH;
  const int kend = (k0 + WIN_C) < nk ? (k0 + WIN_C) : nk;

  bf16x8 qf[KB];
  {
    const bf16_t* qp = a.qr + (size_t)qi * a.H * DH + (g * G + qh) * DH + fq * 8;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) qf[kb] = *reinterpret_cast<const bf16x8*>(qp + kb * 32);
  }
  auto kswz = [](int row) __attribute__((always_inline)) { return DH == 64 ? (row & 7) : (row & 15); };
  struct Regs { uint4 v[NLD]; };
  // rows of key block kb0; slots beyond the row's range are clamped to its last key (never loaded, never skipped)
  auto fetch = [&](const bf16_t* base, int kb0) __attribute__((always_inline)) {
    Regs rr;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int ch = tid + i * 256, key = ch / KCH, cc = ch % KCH;
      int j = kb0 + key;
      j = j < nk ? j : nk - 1;
      rr.v[i] = *reinterpret_cast<const uint4*>(base + (size_t)j * DH + cc * 8);
    }
    return rr;
  };
  auto put_k = [&](char* buf, const Regs& rr) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int ch = tid + i * 256, key = ch / KCH, cc = ch % KCH;
      *reinterpret_cast<uint4*>(buf + (key * KCH + (cc ^ kswz(key))) * 16) = rr.v[i];
    }
  };
  auto put_v = [&](char* buf, const Regs& rr) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int ch = tid + i * 256, key = ch / KCH, cc = ch % KCH;
      *reinterpret_cast<uint4*>(buf + key * VSTR + cc * 16) = rr.v[i];
    }
  };
  const int krow_a = (fr >> 2) * 8 + (fr & 3);
  auto kfrag = [&](const char* buf, int tile, int kb) __attribute__((always_inline)) {
    const int row = krow_a + tile * 4;
    return *reinterpret_cast<const bf16x8*>(buf + (row * KCH + ((kb * 4 + fq) ^ kswz(row))) * 16);
  };
  // B operand of P.V for output columns n*16 .. +16: this lane's dh column n*16 + fr, keys fq*8 .. +8 of the block
  const int vlane = (fq * 8 + (fr >> 2)) * VSTR + (fr & 3) * 8;
  auto vfrag = [&](const char* buf, int n) __attribute__((always_inline)) {
    typedef __attribute__((address_space(3))) win_s16x4* tr_ptr_t;
    const char* p = buf + vlane + n * 32;
    const win_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(p));
    const win_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(p + 4 * VSTR));
    return __builtin_bit_cast(bf16x8, (win_s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
  };
  // scores of this lane's 8 keys (kb0 + fq*8 ..) for its query, in the exp2 domain; a key the query may not see: -inf, by select
  auto scores = [&](const char* kbuf, int kb0, float (&s)[8]) __attribute__((always_inline)) {
    f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kbuf, 0, kb), qf[kb], sa, 0, 0, 0);
      sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kbuf, 1, kb), qf[kb], sb, 0, 0, 0);
    }
    const bool interior = kb0 + 31 < pos;      // every key below the window: allowed for every query; workgroup-uniform
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int j = kb0 + fq * 8 + r;
      float v = rbf(r < 4 ? sa[r & 3] : sb[r & 3]);
      v = rbf(v * a.scale);
      s[r] = (interior || j <= qpos) ? v * LOG2E : -INFINITY;
    }
  };
  float2* stats = a.stats + ((size_t)g * total);   // chunk c' of this kv head: + c' * Hkv * total
  const size_t stat_step = (size_t)a.Hkv * total;

  char* kb_base = smem;
  char* vb_base = smem + 2 * KTILE;
  if constexpr (PHASE == 0) {
    float m = -INFINITY, l = 0.f;
    Regs ka = fetch(kc, k0);
    put_k(kb_base, ka);
    __syncthreads();
    int cur = 0;
    for (int kb0 = k0; kb0 < kend; kb0 += 32, cur ^= 1) {
      const bool more = kb0 + 32 < kend;       // uniform
      if (more) ka = fetch(kc, kb0 + 32);
      if (active) {
        float s[8];
        scores(kb_base + cur * KTILE, kb0, s);
        float bm = s[0];
#pragma unroll
        for (int r = 1; r < 8; ++r) bm = fmaxf(bm, s[r]);
        bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float mn = fmaxf(m, bm);
        const float ms = mn == -INFINITY ? 0.f : mn;   // (a query without a key in this chunk: every term exp2(-inf) = 0, never stored)
        float bs = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) bs += __builtin_amdgcn_exp2f(s[r] - ms);
        bs += __shfl_xor(bs, 16, 64);
        bs += __shfl_xor(bs, 32, 64);
        l = l * __builtin_amdgcn_exp2f(m - ms) + bs;
        m = mn;
      }
      if (more) put_k(kb_base + (cur ^ 1) * KTILE, ka);
      __syncthreads();
    }
    if (active && q_live && fq == 0) stats[(size_t)c * stat_step + iw0 + fr] = make_float2(m, l);
  } else {
    // the query's (m, l) over all its chunks, in chunk order: every workgroup of the query computes the same bits
    float m = -INFINITY, l = 0.f;
    if (active) {
      const int nch = qpos / WIN_C + 1;
      const float2* sp = stats + idx;
      for (int cc = 0; cc < nch; ++cc) m = fmaxf(m, sp[(size_t)cc * stat_step].x);
      for (int cc = 0; cc < nch; ++cc) {
        const float2 t = sp[(size_t)cc * stat_step];
        l += t.y * __builtin_amdgcn_exp2f(t.x - m);
      }
    }
    const float rl = 1.0f / l;
    // window rows with a query in this wave's tile (wave-uniform)
    const int wlast = (iw0 + 15) < total ? (iw0 + 15) : total - 1;
    const int ii_lo = (iw0 < total ? iw0 : total - 1) >> gs, ii_hi = wlast >> gs;
    f32x4 oacc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) oacc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    Regs ka = fetch(kc, k0), va = fetch(vc, k0);
    put_k(kb_base, ka); put_v(vb_base, va);
    __syncthreads();
    int cur = 0;
    for (int kb0 = k0; kb0 < kend; kb0 += 32, cur ^= 1) {
      const bool more = kb0 + 32 < kend;
      if (more) { ka = fetch(kc, kb0 + 32); va = fetch(vc, kb0 + 32); }
      if (active) {                            // wave-uniform: all 64 lanes take the transposed reads together
        float s[8];
        scores(kb_base + cur * KTILE, kb0, s);
        bf16x8 pf;
#pragma unroll
        for (int r = 0; r < 8; ++r) pf[r] = (short)f2bf(__builtin_amdgcn_exp2f(s[r] - m) * rl);   // (a masked key: exp2(-inf) * rl = +0)
        const char* vbuf = vb_base + cur * VTILE;
        if (kb0 + 31 < pos) {                  // no window slot in the block (workgroup-uniform)
#pragma unroll
          for (int n = 0; n < NT; ++n) oacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vfrag(vbuf, n), oacc[n], 0, 0, 0);
        } else {
          for (int ii = ii_lo; ii <= ii_hi; ++ii) {
            const int lim = pos + ii - kb0 - fq * 8;   // element r of this lane's fragments is a key row ii may see iff r <= lim
            bf16x8 pi;
#pragma unroll
            for (int r = 0; r < 8; ++r) pi[r] = qi == ii ? pf[r] : (short)0;
#pragma unroll
            for (int n = 0; n < NT; ++n) {
              bf16x8 vf = vfrag(vbuf, n);
#pragma unroll
              for (int r = 0; r < 8; ++r) vf[r] = r <= lim ? vf[r] : (short)0;
              const f32x4 t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pi, vf, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int oq = iw0 + fq * 4 + r;
                oacc[n][r] = (oq >> gs) == ii ? oacc[n][r] + t[r] : oacc[n][r];
              }
            }
          }
        }
      }
      if (more) { put_k(kb_base + (cur ^ 1) * KTILE, ka); put_v(vb_base + (cur ^ 1) * VTILE, va); }
      __syncthreads();
    }
    if (!active) return;
    // partial O[packed query iw0 + fq*4 + r][d = n*16 + fr] of chunk c
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int oq = iw0 + fq * 4 + r;
      if (oq >= total) continue;
      const int oi = oq >> gs, oh = oq & (G - 1);
      if (k0 > pos + oi) continue;             // the chunk holds no key of this query: the combine does not read it
      float* op = a.part + ((size_t)c * W + oi) * a.H * DH + (g * G + oh) * DH + fr;
#pragma unroll
      for (int n = 0; n < NT; ++n) op[n * 16] = oacc[n][r];
    }
  }
}

// o[i] = bf16(sum over the chunks of query i, in chunk order); a lane owns 4 columns, a wave 256
__global__ __launch_bounds__(64) void win_combine_kernel(PcyWinAttnArgs a) {
  const int pos = *a.pos_dev;
  if (!win_pos_ok(pos, a.W, a.Tmax)) return;
  const int i = blockIdx.x, hd = a.H * a.dh;
  const int e = (blockIdx.y * 64 + threadIdx.x) * 4;
  if (e >= hd) return;
  const int nch = (pos + i) / WIN_C + 1;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c = 0; c < nch; ++c) {
    const float4 t = *reinterpret_cast<const float4*>(a.part + ((size_t)c * a.W + i) * hd + e);
    acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
  }
  *reinterpret_cast<uint2*>(a.o + (size_t)i * a.ldo + e) = make_uint2(pack_bf(acc.x, acc.y), pack_bf(acc.z, acc.w));
}

}  // namespace

int pcy_attn_win_chunk() { return WIN_C; }

bool pcy_attn_win_covers(int W, int H, int Hkv, int dh) {
  if (W < 2 || W > 32 || (dh != 64 && dh != 128) || Hkv < 1 || H % Hkv) return false;
  const int G = H / Hkv;
  return G == 1 || G == 2 || G == 4 || G == 8;
}

PcyWinPlan pcy_attn_win_plan(int W, int H, int Hkv, int dh, int Tmax) {
  PcyWinPlan p{};
  p.nchunk = (Tmax + WIN_C - 1) / WIN_C;
  p.qr_bytes = (size_t)W * H * dh * sizeof(bf16_t);
  p.stats_bytes = (size_t)p.nchunk * W * H * sizeof(float2);
  p.part_bytes = (size_t)p.nchunk * W * H * dh * sizeof(float);
  return p;
}

bool pcy_launch_attn_window(hipStream_t s, const PcyWinAttnArgs& a) {
  if (!pcy_attn_win_covers(a.W, a.H, a.Hkv, a.dh) || a.Tmax < a.W || a.nchunk != (a.Tmax + WIN_C - 1) / WIN_C) return false;
  hipLaunchKernelGGL(win_prologue_kernel, dim3(a.W, a.H + 2 * a.Hkv), dim3(64), 0, s, a);
  const dim3 grid(a.nchunk, a.Hkv, (a.W * (a.H / a.Hkv) + 63) / 64);
  if (a.dh == 64) {
    hipLaunchKernelGGL((attn_win_kernel<64, 0>), grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL((attn_win_kernel<64, 1>), grid, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL((attn_win_kernel<128, 0>), grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL((attn_win_kernel<128, 1>), grid, dim3(256), 0, s, a);
  }
  hipLaunchKernelGGL(win_combine_kernel, dim3(a.W, (a.H * a.dh + 255) / 256), dim3(64), 0, s, a);
  return true;
}
