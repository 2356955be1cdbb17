// Many-queries decode attention on a shared-prefix cache: the decode attention's operator -- one new token per row, rope,
// append, exact softmax rounding (pcy_attn_dec.h) -- with the prefix of a prompt staged ONCE for all rows x G queries that read it.
//
// Logical slot j < Tp of row b is prefix[b / rows_per_prefix][j], slot j >= Tp is the row's own panel at j - Tp; the new token sits at t = *pos.
// Four launches, each a function of the call's shape only:
//   attn_mq_score_kernel  (key chunk x query tile, kv head, prompt): ropes its 64 packed queries (row r, head hg -> r * G + hg) straight into
//                         MFMA fragments, stages the [32 keys][DH] K tiles of its chunk of the prefix once (the XOR-swizzled image of
//                         pcy_attn_ext.hip) and writes s = bf16(bf16(q.k) * scale), masked s = PCY_BF16_MIN, to the score rows [B*H][lds].
//   attn_mq_row_kernel    (kv head, row): ropes the row's G heads and its new key, appends K / V at suffix slot t - Tp, scores the row's own
//                         slots [Tp, t], takes (m, l) over ALL t + 1 scores of a query, turns the score row into p = bf16(exp(s - m) / l) in
//                         place (zeros in the row's padding up to lds) and adds up P.V of the own slots in slot order (fp32).
//   attn_mq_pv_kernel     (key chunk x query tile, kv head, prompt): stages the V tiles of its chunk once, P.V for the 64 packed queries by MFMA
//                         with V in place (ds_read_b64_tr_b16), fp32 partial o per chunk.
//   attn_mq_combine_kernel: o = bf16(chunk 0 + chunk 1 + ... + own slots), added in that order, rounded once.
// p is normalised with the query's global (m, l) BEFORE P.V, so the partial sums need no rescaling and no atomics: the order of every sum is
// fixed by (B, rows_per_prefix, Tp, t, geometry).  An MFMA output element depends on its own row and column only, so a query's bits do not
// depend on its slot in a tile or on its prompt mates.  Rows beyond the prefix are clamped to its last key when a tile is staged (their p is
// exactly 0), never skipped.  The prefix panels are only read; of the own panels only slot t - Tp is written.
// t < Tp or t >= Tp + Town: every workgroup of every launch leaves without writing.
#include "pcy_internal.h"
#include "pcy_attn_dec.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short mq_s16x4;
typedef __attribute__((ext_vector_type(8))) short mq_s16x8;

// what the score and the P.V launch share: the workgroup's place in the grid and its lane's packed query
struct MqTile {
  int chunk, g, p, row0, total, iw0, qb, qh, kb_lo, kb_hi;
  bool live, active;
};
__device__ __forceinline__ MqTile mq_tile(const PcyMqAttnArgs& a, int G) {
  MqTile m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fr = lane & 15;
  m.chunk = blockIdx.x / a.ntiles;
  const int tile = blockIdx.x - m.chunk * a.ntiles;
  m.g = blockIdx.y; m.p = blockIdx.z;
  m.row0 = m.p * a.rows_per_prefix;                                  // (< B by the grid)
  const int rows = (a.B - m.row0) < a.rows_per_prefix ? (a.B - m.row0) : a.rows_per_prefix;   // the last prompt may be short of rows
  m.total = rows * G;
  const int i0 = tile * 64;
  m.live = i0 < m.total;                                             // workgroup-uniform
  m.iw0 = i0 + wave * 16;
  m.active = m.iw0 < m.total;                                        // wave-uniform
  int idx = m.iw0 + fr;
  idx = idx < m.total ? idx : m.total - 1;                           // (slots beyond the last query repeat it; never stored)
  m.qb = m.row0 + idx / G; m.qh = idx % G;
  const int nblk = (a.Tp + 31) >> 5;
  m.kb_lo = m.chunk * a.cblocks * 32;
  const int hi = (m.chunk + 1) * a.cblocks;
  m.kb_hi = (hi < nblk ? hi : nblk) * 32;
  return m;
}
__device__ __forceinline__ bool mq_pos_ok(const PcyMqAttnArgs& a, int t) { return t >= a.Tp && t < a.Tp + a.Town; }

template <int DH>
__global__ __launch_bounds__(256) void attn_mq_score_kernel(PcyMqAttnArgs a) {
  constexpr int KB = DH / 32, KCH = DH / 8, NLD = (32 * KCH) / 256, KTILE = 32 * DH * 2;
  __shared__ __attribute__((aligned(16))) char smem[2 * KTILE];
  const int t = *a.pos_dev;
  if (!mq_pos_ok(a, t)) return;
  const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
  const int G = a.H / a.Hkv, Tp = a.Tp;
  const MqTile m = mq_tile(a, G);
  if (!m.live) return;
  const int h = m.g * G + m.qh;
  const uint8_t* keep = a.keep ? a.keep + (size_t)m.qb * a.ld_keep : nullptr;   // per lane: the query's own row
  const bf16_t* k_pre = a.k_pre + ((size_t)m.p * a.Hkv + m.g) * Tp * DH;

  bf16x8 qf[KB];
  {
    const bf16_t* qp = a.qkv + (size_t)m.qb * a.ld + h * DH;
    const bf16_t* cs = a.cos_t + (size_t)t * DH;
    const bf16_t* sn = a.sin_t + (size_t)t * DH;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      float r[8];
      rope8<DH>(qp, cs, sn, kb * 32 + fq * 8, r);
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[kb][e] = (short)f2bf(r[e]);
    }
  }
  auto kswz = [](int row) __attribute__((always_inline)) { return DH == 64 ? (row & 7) : (row & 15); };
  struct Regs { uint4 v[NLD]; };
  auto fetch = [&](int kb0) __attribute__((always_inline)) {
    Regs rr;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
      int j = kb0 + key;
      j = j < Tp ? j : Tp - 1;
      rr.v[i] = *reinterpret_cast<const uint4*>(k_pre + (size_t)j * DH + ch * 8);
    }
    return rr;
  };
  auto put_k = [&](char* buf, const Regs& rr) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
      *reinterpret_cast<uint4*>(buf + (key * KCH + (ch ^ kswz(key))) * 16) = rr.v[i];
    }
  };
  const int krow_a = (fr >> 2) * 8 + (fr & 3);
  auto kfrag = [&](const char* buf, int tile, int kb) __attribute__((always_inline)) {
    const int row = krow_a + tile * 4;
    return *reinterpret_cast<const bf16x8*>(buf + (row * KCH + ((kb * 4 + fq) ^ kswz(row))) * 16);
  };
  bf16_t* srow = a.sc + ((size_t)m.qb * a.H + h) * a.lds;
  const bool store = m.active && (m.iw0 + fr) < m.total;

  Regs ka = fetch(m.kb_lo);
  put_k(smem, ka);
  __syncthreads();
  int cur = 0;
  for (int kb0 = m.kb_lo; kb0 < m.kb_hi; kb0 += 32, cur ^= 1) {
    const bool more = kb0 + 32 < m.kb_hi;      // uniform
    if (more) ka = fetch(kb0 + 32);
    if (m.active) {
      const char* kbuf = smem + cur * KTILE;
      f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) {
        sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kbuf, 0, kb), qf[kb], sa, 0, 0, 0);
        sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kbuf, 1, kb), qf[kb], sb, 0, 0, 0);
      }
      // this lane: keys kb0 + fq*8 .. +8 of query fr
      bf16x8 sv;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int j = kb0 + fq * 8 + r;
        float v = rbf(rbf(r < 4 ? sa[r & 3] : sb[r & 3]) * a.scale);
        if (keep && j < Tp && keep[j] == 0) v = PCY_BF16_MIN;
        sv[r] = (short)f2bf(v);
      }
      if (store) *reinterpret_cast<bf16x8*>(srow + kb0 + fq * 8) = sv;
    }
    if (more) put_k(smem + (cur ^ 1) * KTILE, ka);
    __syncthreads();
  }
}

// dynamic LDS: [(G + 1)][DH] bf16 roped q heads and new key | [G][Town] fp32 scores / probabilities of the own slots | [4][G] wave partials
template <int DH, int G>
__global__ __launch_bounds__(256) void attn_mq_row_kernel(PcyMqAttnArgs a) {
  constexpr int NT = 256, NWV = 4;
  extern __shared__ __attribute__((aligned(16))) char smem_dyn[];
  const int t = *a.pos_dev;
  if (!mq_pos_ok(a, t)) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kvh = blockIdx.x, b = blockIdx.y;
  const int Tp = a.Tp, Town = a.Town;
  const int ns = t - Tp + 1;                                 // own slots, the new one included (<= Town)
  bf16_t* qk = reinterpret_cast<bf16_t*>(smem_dyn);
  float* ss = reinterpret_cast<float*>(smem_dyn + (G + 1) * DH * 2);
  float* wred = ss + (size_t)G * Town;
  const bf16_t* row = a.qkv + (size_t)b * a.ld;
  bf16_t* kc = a.k_own + ((size_t)b * a.Hkv + kvh) * Town * DH;
  bf16_t* vc = a.v_own + ((size_t)b * a.Hkv + kvh) * Town * DH;
  const bf16_t* vrow = row + (a.H + a.Hkv + kvh) * DH;
  const uint8_t* keep = a.keep ? a.keep + (size_t)b * a.ld_keep : nullptr;

  static_assert((G + 1) * (DH / 8) <= NT - DH / 8, "one rope item or one V chunk per thread");
  if (tid < (G + 1) * (DH / 8)) {
    const int hh = tid / (DH / 8), ch = tid % (DH / 8);
    const bf16_t* src = hh < G ? row + (kvh * G + hh) * DH : row + (a.H + kvh) * DH;
    float r[8];
    rope8<DH>(src, a.cos_t + (size_t)t * DH, a.sin_t + (size_t)t * DH, ch * 8, r);
    const uint4 w = make_uint4(pack_bf(r[0], r[1]), pack_bf(r[2], r[3]), pack_bf(r[4], r[5]), pack_bf(r[6], r[7]));
    *reinterpret_cast<uint4*>(qk + hh * DH + ch * 8) = w;
    if (hh == G) *reinterpret_cast<uint4*>(kc + (size_t)(t - Tp) * DH + ch * 8) = w;   // append the new token's K
  }
  if (tid >= NT - DH / 8) {                                                          // ... and its V
    const int ch = tid - (NT - DH / 8);
    *reinterpret_cast<uint4*>(vc + (size_t)(t - Tp) * DH + ch * 8) = *reinterpret_cast<const uint4*>(vrow + ch * 8);
  }
  lds_barrier();

  // scores of the own slots: slot t from the roped key in LDS, the older ones from the row's panel
  for (int i = tid; i < G * ns; i += NT) {
    const int g = i / ns, jj = i - g * ns;
    const bool is_new = jj == ns - 1;
    float acc = 0.f;
#pragma unroll 4
    for (int ch = 0; ch < DH / 8; ++ch) {
      const uint4 kw = is_new ? *reinterpret_cast<const uint4*>(qk + G * DH + ch * 8) : *reinterpret_cast<const uint4*>(kc + (size_t)jj * DH + ch * 8);
      const uint4 qw = *reinterpret_cast<const uint4*>(qk + g * DH + ch * 8);
      acc += lo_bf(qw.x) * lo_bf(kw.x); acc += hi_bf(qw.x) * hi_bf(kw.x);
      acc += lo_bf(qw.y) * lo_bf(kw.y); acc += hi_bf(qw.y) * hi_bf(kw.y);
      acc += lo_bf(qw.z) * lo_bf(kw.z); acc += hi_bf(qw.z) * hi_bf(kw.z);
      acc += lo_bf(qw.w) * lo_bf(kw.w); acc += hi_bf(qw.w) * hi_bf(kw.w);
    }
    const bool kept = (keep && !is_new) ? keep[Tp + jj] != 0 : true;
    ss[g * Town + jj] = kept ? rbf(rbf(acc) * a.scale) : PCY_BF16_MIN;
  }
  lds_barrier();

  // (m, l) over all t + 1 keys of every query, then p in place
  float mx[G], li[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const bf16_t* sp = a.sc + ((size_t)b * a.H + kvh * G + g) * a.lds;
    float v = -INFINITY;
    for (int j = tid; j < Tp; j += NT) v = fmaxf(v, bf2f(sp[j]));
    for (int jj = tid; jj < ns; jj += NT) v = fmaxf(v, ss[g * Town + jj]);
    v = wave_max_dpp(v);
    if (lane == 0) wred[wave * G + g] = v;
  }
  lds_barrier();
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const bf16_t* sp = a.sc + ((size_t)b * a.H + kvh * G + g) * a.lds;
    float v = wred[g];
#pragma unroll
    for (int w = 1; w < NWV; ++w) v = fmaxf(v, wred[w * G + g]);
    mx[g] = v;
    float se = 0.f;
    for (int j = tid; j < Tp; j += NT) se += expf(bf2f(sp[j]) - v);
    for (int jj = tid; jj < ns; jj += NT) se += expf(ss[g * Town + jj] - v);
    li[g] = wave_sum_dpp(se);
  }
  lds_barrier();
#pragma unroll
  for (int g = 0; g < G; ++g) if (lane == 0) wred[wave * G + g] = li[g];
  lds_barrier();
#pragma unroll
  for (int g = 0; g < G; ++g) {
    bf16_t* sp = a.sc + ((size_t)b * a.H + kvh * G + g) * a.lds;
    float l = wred[g];
#pragma unroll
    for (int w = 1; w < NWV; ++w) l += wred[w * G + g];
    for (int j = tid; j < a.lds; j += NT) sp[j] = j < Tp ? f2bf(expf(bf2f(sp[j]) - mx[g]) / l) : (bf16_t)0;
    for (int jj = tid; jj < ns; jj += NT) ss[g * Town + jj] = rbf(expf(ss[g * Town + jj] - mx[g]) / l);
  }
  lds_barrier();

  // P.V of the own slots in slot order; slot t straight from the projection
  float* part = a.part + ((size_t)a.nchunk * a.B + b) * a.H * DH + (size_t)kvh * G * DH;
  for (int i = tid; i < G * DH; i += NT) {
    const int g = i / DH, d = i - g * DH;
    float acc = 0.f;
    for (int jj = 0; jj < ns - 1; ++jj) acc += ss[g * Town + jj] * bf2f(vc[(size_t)jj * DH + d]);
    acc += ss[g * Town + ns - 1] * bf2f(vrow[d]);
    part[i] = acc;
  }
}

template <int DH>
__global__ __launch_bounds__(256) void attn_mq_pv_kernel(PcyMqAttnArgs a) {
  constexpr int NTL = DH / 16, KCH = DH / 8, NLD = (32 * KCH) / 256;
  constexpr int VSTR = DH * 2 + 32;            // V tile row stride in bytes: the 4 key rows of a transposed read fall on distinct banks
  constexpr int VTILE = 32 * VSTR;
  __shared__ __attribute__((aligned(16))) char smem[2 * VTILE];
  const int t = *a.pos_dev;
  if (!mq_pos_ok(a, t)) return;
  const int tid = threadIdx.x, lane = tid & 63, fr = lane & 15, fq = lane >> 4;
  const int G = a.H / a.Hkv, Tp = a.Tp;
  const MqTile m = mq_tile(a, G);
  if (!m.live) return;
  const bf16_t* v_pre = a.v_pre + ((size_t)m.p * a.Hkv + m.g) * Tp * DH;
  const bf16_t* prow = a.sc + ((size_t)m.qb * a.H + m.g * G + m.qh) * a.lds + fq * 8;   // A operand: 8 consecutive keys of query fr

  struct Regs { uint4 v[NLD]; };
  auto fetch = [&](int kb0) __attribute__((always_inline)) {
    Regs rr;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
      int j = kb0 + key;
      j = j < Tp ? j : Tp - 1;
      rr.v[i] = *reinterpret_cast<const uint4*>(v_pre + (size_t)j * DH + ch * 8);
    }
    return rr;
  };
  auto put_v = [&](char* buf, const Regs& rr) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
      *reinterpret_cast<uint4*>(buf + key * VSTR + ch * 16) = rr.v[i];
    }
  };
  // B operand for output columns n*16 .. +16: this lane's dh column n*16 + fr, keys fq*8 .. +8 of the block (pcy_attn_ext.hip)
  const int vlane = (fq * 8 + (fr >> 2)) * VSTR + (fr & 3) * 8;
  auto vfrag = [&](const char* buf, int n) __attribute__((always_inline)) {
    typedef __attribute__((address_space(3))) mq_s16x4* tr_ptr_t;
    const char* pp = buf + vlane + n * 32;
    const mq_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(pp));
    const mq_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(pp + 4 * VSTR));
    return __builtin_bit_cast(bf16x8, (mq_s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
  };

  f32x4 oacc[NTL];
#pragma unroll
  for (int n = 0; n < NTL; ++n) oacc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  Regs va = fetch(m.kb_lo);
  bf16x8 pf = *reinterpret_cast<const bf16x8*>(prow + m.kb_lo), pn = pf;
  put_v(smem, va);
  __syncthreads();
  int cur = 0;
  for (int kb0 = m.kb_lo; kb0 < m.kb_hi; kb0 += 32, cur ^= 1) {
    const bool more = kb0 + 32 < m.kb_hi;      // uniform
    if (more) { va = fetch(kb0 + 32); pn = *reinterpret_cast<const bf16x8*>(prow + kb0 + 32); }
    if (m.active) {                            // wave-uniform: all 64 lanes take the transposed reads together
      const char* vbuf = smem + cur * VTILE;
#pragma unroll
      for (int n = 0; n < NTL; ++n) oacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vfrag(vbuf, n), oacc[n], 0, 0, 0);
    }
    if (more) put_v(smem + (cur ^ 1) * VTILE, va);
    pf = pn;
    __syncthreads();
  }
  if (!m.active) return;
  // O[packed query iw0 + fq*4 + r][d = n*16 + fr]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = m.iw0 + fq * 4 + r;
    if (qi >= m.total) continue;
    float* op = a.part + ((size_t)m.chunk * a.B + m.row0 + qi / G) * a.H * DH + (size_t)(m.g * G + qi % G) * DH + fr;
#pragma unroll
    for (int n = 0; n < NTL; ++n) op[n * 16] = oacc[n][r];
  }
}

// o[b][c .. c+4] = bf16(part[0] + part[1] + ... + part[nchunk]) -- chunk order, the own slots last, rounded once
__global__ __launch_bounds__(256) void attn_mq_combine_kernel(PcyMqAttnArgs a) {
  const int t = *a.pos_dev;
  if (!mq_pos_ok(a, t)) return;
  const int HD = a.H * a.dh;
  const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= (size_t)a.B * HD) return;
  const int b = (int)(i / HD), c = (int)(i - (size_t)b * HD);
  float4 s = *reinterpret_cast<const float4*>(a.part + i);
  for (int ch = 1; ch <= a.nchunk; ++ch) {
    const float4 v = *reinterpret_cast<const float4*>(a.part + (size_t)ch * a.B * HD + i);
    s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
  }
  *reinterpret_cast<uint2*>(a.o + (size_t)b * a.ldo + c) = make_uint2(pack_bf(s.x, s.y), pack_bf(s.z, s.w));
}

size_t mq_row_smem(int G, int dh, int Town) { return (size_t)(G + 1) * dh * 2 + sizeof(float) * ((size_t)G * Town + 4 * G + 8); }

template <int DH>
void mq_launch_row(hipStream_t s, const PcyMqAttnArgs& a, int G, dim3 grid, size_t smem) {
  switch (G) {
    case 1: hipLaunchKernelGGL((attn_mq_row_kernel<DH, 1>), grid, dim3(256), smem, s, a); break;
    case 2: hipLaunchKernelGGL((attn_mq_row_kernel<DH, 2>), grid, dim3(256), smem, s, a); break;
    case 4: hipLaunchKernelGGL((attn_mq_row_kernel<DH, 4>), grid, dim3(256), smem, s, a); break;
    default: hipLaunchKernelGGL((attn_mq_row_kernel<DH, 8>), grid, dim3(256), smem, s, a); break;
  }
}

}  // namespace

PcyMqPlan pcy_attn_mq_plan(int B, int rows_per_prefix, int H, int Hkv, int dh, int Tp) {
  PcyMqPlan p{};
  const int G = H / Hkv;
  const int rows = B < rows_per_prefix ? B : rows_per_prefix;
  const int prompts = (B + rows_per_prefix - 1) / rows_per_prefix;
  p.ntiles = (rows * G + 63) / 64;
  const int nblk = (Tp + 31) / 32;
  // key chunks: enough workgroups for two per CU of a 256-CU chip, at most 16 (each chunk costs a partial o per query)
  const long wgs = (long)prompts * Hkv * p.ntiles;
  long want = (512 + wgs - 1) / wgs;
  want = want < 1 ? 1 : want > 16 ? 16 : want;
  want = want > nblk ? nblk : want;
  p.cblocks = (nblk + (int)want - 1) / (int)want;
  p.nchunk = (nblk + p.cblocks - 1) / p.cblocks;
  p.lds = nblk * 32;
  p.sc_bytes = (size_t)B * H * p.lds * sizeof(bf16_t);
  p.part_bytes = (size_t)(p.nchunk + 1) * B * H * dh * sizeof(float);
  return p;
}

bool pcy_attn_mq_covers(int H, int Hkv, int dh, int Town) {
  if (dh != 64 && dh != 128) return false;
  if (Hkv < 1 || H % Hkv) return false;
  const int G = H / Hkv;
  if (!(G == 1 || G == 2 || G == 4 || G == 8)) return false;
  return Town >= 1 && mq_row_smem(G, dh, Town) <= 64 * 1024;
}

bool pcy_launch_attn_mq(hipStream_t s, const PcyMqAttnArgs& a) {
  if (a.B <= 0) return true;
  if (!pcy_attn_mq_covers(a.H, a.Hkv, a.dh, a.Town) || a.Tp < 1 || a.rows_per_prefix < 1) return false;
  const int G = a.H / a.Hkv;
  const int prompts = (a.B + a.rows_per_prefix - 1) / a.rows_per_prefix;
  const dim3 tiles((unsigned)(a.ntiles * a.nchunk), a.Hkv, prompts), rows(a.Hkv, a.B);
  const size_t smem = mq_row_smem(G, a.dh, a.Town);
  if (a.dh == 64) {
    hipLaunchKernelGGL((attn_mq_score_kernel<64>), tiles, dim3(256), 0, s, a);
    mq_launch_row<64>(s, a, G, rows, smem);
    hipLaunchKernelGGL((attn_mq_pv_kernel<64>), tiles, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL((attn_mq_score_kernel<128>), tiles, dim3(256), 0, s, a);
    mq_launch_row<128>(s, a, G, rows, smem);
    hipLaunchKernelGGL((attn_mq_pv_kernel<128>), tiles, dim3(256), 0, s, a);
  }
  const size_t quads = (size_t)a.B * a.H * a.dh / 4;
  hipLaunchKernelGGL(attn_mq_combine_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, a);
  return true;
}
