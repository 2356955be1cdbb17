// Split-key decode attention on a shared-prefix cache: the operator of pcy_attn_mq.hip -- one new token per row, rope, append,
// logical slot j < Tp of row b from prefix[b / rows_per_prefix][j], slot j >= Tp from the row's own panel at j - Tp, the new token at t = *pos --
// with the softmax statistics kept PER KEY CHUNK, so that no score row and no probability ever leaves the chip.  Two launches, each a function
// of the call's shape only (never of t: a captured launch is valid at every position):
//   attn_split_partial_kernel: one grid, two kinds of workgroup, told apart by blockIdx.x alone (workgroup-uniform):
//     row workgroups    (kv head, row): rope the row's G heads and its new key, append K / V at suffix slot t - Tp, score the row's own slots
//                       [Tp, t] and reduce them as the LAST chunk.
//     prefix workgroups (key chunk x 64-query tile, kv head, prompt): rope their 64 packed queries (row r, head hg -> r * G + hg) into MFMA
//                       fragments, stage every [32 keys][DH] K tile of their chunk once (the XOR-swizzled image of pcy_attn_mq.hip), S by
//                       MFMA into registers; then every V tile once, P.V by MFMA with V read in place (ds_read_b64_tr_b16).
//     Both write, per (chunk c, query): m_c = max s_j, l_c = sum e_j and the fp32 o_c = sum p_j * v_j, where
//                       s_j = bf16(bf16(q.k) * scale), masked s_j = PCY_BF16_MIN, e_j = exp(s_j - m_c) in fp32, p_j = bf16(e_j).
//   attn_split_combine_kernel: m = max_c m_c, w_c = exp(m_c - m), o = bf16((sum_c w_c * o_c) / (sum_c w_c * l_c)), both sums in chunk order
//                       with the own slots last, rounded once.
// A chunk in which every key of a query is masked has m_c = PCY_BF16_MIN and finite l_c, o_c; slot t is never masked, so m is a real score and
// w_c = exp(PCY_BF16_MIN - m) is exactly 0: the chunk drops out, without NaN or Inf.
//
// Promises:
//   - a query's bits depend only on its own row's logical contents (qkv row, prefix row, own slots below t, mask row) and on the call's shape
//     (B, rows_per_prefix, H, Hkv, dh, Tp -- they fix the chunk plan): an MFMA output element depends on its own row and column only, every
//     sum has a fixed order, there are no atomics and no workgroup waits for another;
//   - equal calls give equal bits; equal rows in other tiles or prompts give equal bits;
//   - the prefix panels are only read; of the own panels only slot t - Tp is written (the bits pcy_attn_decode appends);
//   - slots above t never reach a result (rows of a staged tile beyond the prefix repeat its last key and get e = 0);
//   - t < Tp or t >= Tp + Town: every workgroup of both launches leaves without writing.
// NOT promised: the bits of pcy_attn_decode or pcy_attn_decode_shared -- their p = bf16(exp(s - m) / l) is rounded under the global (m, l).
#include "pcy_internal.h"
#include "pcy_attn_dec.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short sp_s16x4;
typedef __attribute__((ext_vector_type(8))) short sp_s16x8;

constexpr int SP_MAXCB = 4;   // 32-key blocks per chunk at most: the chunk's scores wait in registers (8 per lane and block) for its maximum

__device__ __forceinline__ bool sp_pos_ok(const PcySplitAttnArgs& a, int t) { return t >= a.Tp && t < a.Tp + a.Town; }

// row workgroup.  LDS: [(G + 1)][DH] bf16 roped q heads and new key | [G][Town] fp32 scores, then probabilities, of the own slots
template <int DH>
__device__ __forceinline__ void sp_row_role(const PcySplitAttnArgs& a, char* smem, int t, int kvh, int b) {
  constexpr int NT = 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int G = a.H / a.Hkv, Tp = a.Tp, Town = a.Town;
  const int ns = t - Tp + 1;                                 // own slots, the new one included (<= Town)
  bf16_t* qk = reinterpret_cast<bf16_t*>(smem);
  float* ss = reinterpret_cast<float*>(smem + (G + 1) * DH * 2);
  const bf16_t* row = a.qkv + (size_t)b * a.ld;
  bf16_t* kc = a.k_own + ((size_t)b * a.Hkv + kvh) * Town * DH;
  bf16_t* vc = a.v_own + ((size_t)b * a.Hkv + kvh) * Town * DH;
  const bf16_t* vrow = row + (a.H + a.Hkv + kvh) * DH;
  const uint8_t* keep = a.keep ? a.keep + (size_t)b * a.ld_keep : nullptr;

  static_assert(9 * (DH / 8) <= NT - DH / 8, "one rope item or one V chunk per thread");
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

  // (m, l) of the own slots, a wave per head; p = bf16(e) in place
  for (int g = wave; g < G; g += 4) {
    float* sg = ss + g * Town;
    float mx = -INFINITY;
    for (int jj = lane; jj < ns; jj += 64) mx = fmaxf(mx, sg[jj]);
    mx = wave_max_dpp(mx);
    float se = 0.f;
    for (int jj = lane; jj < ns; jj += 64) {
      const float e = expf(sg[jj] - mx);
      se += e;
      sg[jj] = rbf(e);
    }
    se = wave_sum_dpp(se);
    if (lane == 0) a.stat[((size_t)a.nchunk * a.B + b) * a.H + kvh * G + g] = make_float2(mx, se);
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

// prefix workgroup.  LDS: two K tiles [32][DH] (swizzled), then two V tiles [32][DH*2 + 32 bytes] in the same bytes
template <int DH>
__device__ __forceinline__ void sp_prefix_role(const PcySplitAttnArgs& a, char* smem, int t, int id) {
  constexpr int KB = DH / 32, KCH = DH / 8, NLD = (32 * KCH) / 256, KTILE = 32 * DH * 2, NTL = DH / 16;
  constexpr int VSTR = DH * 2 + 32;            // V tile row stride in bytes: the 4 key rows of a transposed read fall on distinct banks
  constexpr int VTILE = 32 * VSTR;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fq = lane >> 4;
  const int G = a.H / a.Hkv, Tp = a.Tp;
  // the workgroup's place: (chunk, tile) fastest, then kv head, then prompt
  const int per = a.ntiles * a.nchunk;
  const int ct = id % per, gp = id / per;
  const int chunk = ct / a.ntiles, tile = ct - chunk * a.ntiles;
  const int g = gp % a.Hkv, p = gp / a.Hkv;
  const int row0 = p * a.rows_per_prefix;                            // (< B by the grid)
  const int rows = (a.B - row0) < a.rows_per_prefix ? (a.B - row0) : a.rows_per_prefix;   // the last prompt may be short of rows
  const int total = rows * G;
  if (tile * 64 >= total) return;                                    // workgroup-uniform
  const int iw0 = tile * 64 + wave * 16;
  const bool active = iw0 < total;                                   // wave-uniform
  int idx = iw0 + fr;
  idx = idx < total ? idx : total - 1;                               // (slots beyond the last query repeat it; never stored)
  const int qb = row0 + idx / G, h = g * G + idx % G;
  const int nblk = (Tp + 31) >> 5;
  const int kb_lo = chunk * a.cblocks * 32;
  const int hi = (chunk + 1) * a.cblocks;
  const int kb_hi = (hi < nblk ? hi : nblk) * 32;
  const uint8_t* keep = a.keep ? a.keep + (size_t)qb * a.ld_keep : nullptr;   // per lane: the query's own row
  const bf16_t* k_pre = a.k_pre + ((size_t)p * a.Hkv + g) * Tp * DH;
  const bf16_t* v_pre = a.v_pre + ((size_t)p * a.Hkv + g) * Tp * DH;

  struct Regs { uint4 v[NLD]; };
  auto fetch = [&](const bf16_t* base, int kb0) __attribute__((always_inline)) {
    Regs rr;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
      int j = kb0 + key;
      j = j < Tp ? j : Tp - 1;
      rr.v[i] = *reinterpret_cast<const uint4*>(base + (size_t)j * DH + ch * 8);
    }
    return rr;
  };

  // ---- pass 1: S = bf16(bf16(q.k) * scale) of the chunk, into registers
  float sc[SP_MAXCB][8];
#pragma unroll
  for (int cb = 0; cb < SP_MAXCB; ++cb)
#pragma unroll
    for (int r = 0; r < 8; ++r) sc[cb][r] = -INFINITY;
  {
    bf16x8 qf[KB];
    const bf16_t* qp = a.qkv + (size_t)qb * a.ld + h * DH;
    const bf16_t* cs = a.cos_t + (size_t)t * DH;
    const bf16_t* sn = a.sin_t + (size_t)t * DH;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      float r[8];
      rope8<DH>(qp, cs, sn, kb * 32 + fq * 8, r);
#pragma unroll
      for (int e = 0; e < 8; ++e) qf[kb][e] = (short)f2bf(r[e]);
    }
    auto kswz = [](int row) __attribute__((always_inline)) { return DH == 64 ? (row & 7) : (row & 15); };
    auto put_k = [&](char* buf, const Regs& rr) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < NLD; ++i) {
        const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
        *reinterpret_cast<uint4*>(buf + (key * KCH + (ch ^ kswz(key))) * 16) = rr.v[i];
      }
    };
    const int krow_a = (fr >> 2) * 8 + (fr & 3);
    auto kfrag = [&](const char* buf, int tl, int kb) __attribute__((always_inline)) {
      const int row = krow_a + tl * 4;
      return *reinterpret_cast<const bf16x8*>(buf + (row * KCH + ((kb * 4 + fq) ^ kswz(row))) * 16);
    };
    Regs ka = fetch(k_pre, kb_lo);
    put_k(smem, ka);
    __syncthreads();
#pragma unroll
    for (int cb = 0; cb < SP_MAXCB; ++cb) {
      const int kb0 = kb_lo + cb * 32;
      if (kb0 < kb_hi) {                          // uniform
        const bool more = kb0 + 32 < kb_hi;       // uniform
        if (more) ka = fetch(k_pre, kb0 + 32);
        if (active) {
          const char* kbuf = smem + (cb & 1) * KTILE;
          f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kb = 0; kb < KB; ++kb) {
            sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kbuf, 0, kb), qf[kb], sa, 0, 0, 0);
            sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kbuf, 1, kb), qf[kb], sb, 0, 0, 0);
          }
          // this lane: keys kb0 + fq*8 .. +8 of query fr
#pragma unroll
          for (int r = 0; r < 8; ++r) {
            const int j = kb0 + fq * 8 + r;
            float v = rbf(rbf(r < 4 ? sa[r & 3] : sb[r & 3]) * a.scale);
            if (keep && j < Tp && keep[j] == 0) v = PCY_BF16_MIN;
            sc[cb][r] = j < Tp ? v : -INFINITY;   // (a tile row beyond the prefix: e = 0)
          }
        }
        if (more) put_k(smem + ((cb & 1) ^ 1) * KTILE, ka);
        __syncthreads();
      }
    }
  }

  // ---- the chunk's (m, l) of query fr: over this lane's keys, then over the four lanes that hold the query; p = bf16(e)
  float mc = -INFINITY;
#pragma unroll
  for (int cb = 0; cb < SP_MAXCB; ++cb)
#pragma unroll
    for (int r = 0; r < 8; ++r) mc = fmaxf(mc, sc[cb][r]);
  mc = fmaxf(mc, __shfl_xor(mc, 16));
  mc = fmaxf(mc, __shfl_xor(mc, 32));
  float lc = 0.f;
  bf16x8 pf[SP_MAXCB];
#pragma unroll
  for (int cb = 0; cb < SP_MAXCB; ++cb)
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const float e = active ? expf(sc[cb][r] - mc) : 0.f;   // (the chunk holds a key below Tp: mc is finite in an active wave)
      lc += e;
      pf[cb][r] = (short)f2bf(e);
    }
  lc += __shfl_xor(lc, 16);
  lc += __shfl_xor(lc, 32);

  // ---- pass 2: o_c = P.V, V in place
  auto put_v = [&](char* buf, const Regs& rr) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
      *reinterpret_cast<uint4*>(buf + key * VSTR + ch * 16) = rr.v[i];
    }
  };
  // B operand for output columns n*16 .. +16: this lane's dh column n*16 + fr, keys fq*8 .. +8 of the block (pcy_attn_mq.hip)
  const int vlane = (fq * 8 + (fr >> 2)) * VSTR + (fr & 3) * 8;
  auto vfrag = [&](const char* buf, int n) __attribute__((always_inline)) {
    typedef __attribute__((address_space(3))) sp_s16x4* tr_ptr_t;
    const char* pp = buf + vlane + n * 32;
    const sp_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(pp));
    const sp_s16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(pp + 4 * VSTR));
    return __builtin_bit_cast(bf16x8, (sp_s16x8){lo[0], lo[1], lo[2], lo[3], hi4[0], hi4[1], hi4[2], hi4[3]});
  };
  f32x4 oacc[NTL];
#pragma unroll
  for (int n = 0; n < NTL; ++n) oacc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  Regs va = fetch(v_pre, kb_lo);
  put_v(smem, va);                                // (the last K tile was read before pass 1's closing barrier)
  __syncthreads();
#pragma unroll
  for (int cb = 0; cb < SP_MAXCB; ++cb) {
    const int kb0 = kb_lo + cb * 32;
    if (kb0 < kb_hi) {                            // uniform
      const bool more = kb0 + 32 < kb_hi;         // uniform
      if (more) va = fetch(v_pre, kb0 + 32);
      if (active) {                               // wave-uniform: all 64 lanes take the transposed reads together
        const char* vbuf = smem + (cb & 1) * VTILE;
#pragma unroll
        for (int n = 0; n < NTL; ++n) oacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf[cb], vfrag(vbuf, n), oacc[n], 0, 0, 0);
      }
      if (more) put_v(smem + ((cb & 1) ^ 1) * VTILE, va);
      __syncthreads();
    }
  }
  if (!active) return;
  if (fq == 0 && iw0 + fr < total) a.stat[((size_t)chunk * a.B + qb) * a.H + h] = make_float2(mc, lc);
  // O[packed query iw0 + fq*4 + r][d = n*16 + fr]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = iw0 + fq * 4 + r;
    if (qi >= total) continue;
    float* op = a.part + ((size_t)chunk * a.B + row0 + qi / G) * a.H * DH + (size_t)(g * G + qi % G) * DH + fr;
#pragma unroll
    for (int n = 0; n < NTL; ++n) op[n * 16] = oacc[n][r];
  }
}

// grid.x = Hkv * B row workgroups, then ntiles * nchunk * Hkv * prompts prefix workgroups
template <int DH>
__global__ __launch_bounds__(256) void attn_split_partial_kernel(PcySplitAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char sp_smem[];
  const int t = *a.pos_dev;
  if (!sp_pos_ok(a, t)) return;
  const int nrow = a.Hkv * a.B;
  if ((int)blockIdx.x < nrow) sp_row_role<DH>(a, sp_smem, t, blockIdx.x % a.Hkv, blockIdx.x / a.Hkv);
  else sp_prefix_role<DH>(a, sp_smem, t, blockIdx.x - nrow);
}

// four output elements of one (row, head) per thread.  The chunks are ADDED in chunk order, but their loads are issued SP_CU at a time: a
// thread that waited for each chunk in turn spent 11 us on 17 chunks.
constexpr int SP_CT = 64, SP_CU = 8;
__global__ __launch_bounds__(SP_CT) void attn_split_combine_kernel(PcySplitAttnArgs a) {
  const int t = *a.pos_dev;
  if (!sp_pos_ok(a, t)) return;
  const int HD = a.H * a.dh;
  const size_t i = ((size_t)blockIdx.x * SP_CT + threadIdx.x) * 4;
  if (i >= (size_t)a.B * HD) return;
  const int b = (int)(i / HD), c = (int)(i - (size_t)b * HD), h = c / a.dh;
  const size_t nq = (size_t)a.B * a.H, np = (size_t)a.B * HD;
  const float2* st = a.stat + (size_t)b * a.H + h;
  const float* pt = a.part + i;
  const int last = a.nchunk;
  float m = -INFINITY;
  for (int c0 = 0; c0 <= last; c0 += SP_CU) {
    float mc[SP_CU];
#pragma unroll
    for (int u = 0; u < SP_CU; ++u) mc[u] = st[(size_t)(c0 + u <= last ? c0 + u : last) * nq].x;   // (beyond the last chunk: the last again)
#pragma unroll
    for (int u = 0; u < SP_CU; ++u) m = fmaxf(m, mc[u]);
  }
  float4 s = {0.f, 0.f, 0.f, 0.f};
  float den = 0.f;
  for (int c0 = 0; c0 <= last; c0 += SP_CU) {
    float2 ml[SP_CU];
    float4 v[SP_CU];
#pragma unroll
    for (int u = 0; u < SP_CU; ++u) {
      const int ch = c0 + u <= last ? c0 + u : last;
      ml[u] = st[(size_t)ch * nq];
      v[u] = *reinterpret_cast<const float4*>(pt + (size_t)ch * np);
    }
#pragma unroll
    for (int u = 0; u < SP_CU; ++u) {
      if (c0 + u > last) break;
      const float w = expf(ml[u].x - m);
      s.x += w * v[u].x; s.y += w * v[u].y; s.z += w * v[u].z; s.w += w * v[u].w;
      den += w * ml[u].y;
    }
  }
  *reinterpret_cast<uint2*>(a.o + (size_t)b * a.ldo + c) = make_uint2(pack_bf(s.x / den, s.y / den), pack_bf(s.z / den, s.w / den));
}

size_t sp_smem_bytes(int G, int dh, int Town) {
  const size_t row = (size_t)(G + 1) * dh * 2 + sizeof(float) * (size_t)G * Town;
  const size_t pre = (size_t)2 * 32 * (dh * 2 + 32);
  return row > pre ? row : pre;
}

}  // namespace

PcySplitPlan pcy_attn_split_plan(int B, int rows_per_prefix, int H, int Hkv, int dh, int Tp) {
  PcySplitPlan p{};
  const int G = H / Hkv;
  const int rows = B < rows_per_prefix ? B : rows_per_prefix;
  const int prompts = (B + rows_per_prefix - 1) / rows_per_prefix;
  p.ntiles = (rows * G + 63) / 64;
  const int nblk = (Tp + 31) / 32;
  // key chunks: 64 prefix workgroups where the prefix is long enough; a chunk holds at most SP_MAXCB blocks (its scores wait in registers).
  // Measured at 1 x 10 and 1 x 32 rows, T = 512: a chunk costs a partial o per query each way and a term of the combine, so
  // 256 / 128 workgroups lost 2-3 % of a step to 64; 32 was level with 64; 8 blocks per chunk (127 VGPRs) lost 1-4 %.
  const long wgs = (long)prompts * Hkv * p.ntiles;
  long want = (64 + wgs - 1) / wgs;
  want = want < 1 ? 1 : want > nblk ? nblk : want;
  int cb = (nblk + (int)want - 1) / (int)want;
  p.cblocks = cb > SP_MAXCB ? SP_MAXCB : cb;
  p.nchunk = (nblk + p.cblocks - 1) / p.cblocks;
  p.part_bytes = (size_t)(p.nchunk + 1) * B * H * dh * sizeof(float);
  p.stat_bytes = (size_t)(p.nchunk + 1) * B * H * sizeof(float2);
  return p;
}

bool pcy_attn_split_covers(int H, int Hkv, int dh, int Town) { return pcy_attn_mq_covers(H, Hkv, dh, Town); }

bool pcy_launch_attn_split(hipStream_t s, const PcySplitAttnArgs& a) {
  if (a.B <= 0) return true;
  if (!pcy_attn_split_covers(a.H, a.Hkv, a.dh, a.Town) || a.Tp < 1 || a.rows_per_prefix < 1) return false;
  const int G = a.H / a.Hkv;
  const int prompts = (a.B + a.rows_per_prefix - 1) / a.rows_per_prefix;
  const dim3 grid((unsigned)(a.Hkv * a.B + a.ntiles * a.nchunk * a.Hkv * prompts));
  const size_t smem = sp_smem_bytes(G, a.dh, a.Town);
  if (a.dh == 64) hipLaunchKernelGGL((attn_split_partial_kernel<64>), grid, dim3(256), smem, s, a);
  else hipLaunchKernelGGL((attn_split_partial_kernel<128>), grid, dim3(256), smem, s, a);
  const size_t quads = (size_t)a.B * a.H * a.dh / 4;
  hipLaunchKernelGGL(attn_split_combine_kernel, dim3((unsigned)((quads + SP_CT - 1) / SP_CT)), dim3(SP_CT), 0, s, a);
  return true;
}
