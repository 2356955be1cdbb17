// Extension attention: S new query rows per batch row against keys that already sit in the KV cache (plain or shared-prefix).
//
// attn_ext_kernel<DH> is the multi-query sibling of the decode attention and the cache-reading sibling of attn_lds_kernel
// (pcy_attn.hip): the same exact-rounding two-pass arithmetic --
//   S = bf16(Q.K^T) ; S = bf16(S * scale) ; masked keys -2^126, keys beyond the row's range -inf ;
//   P = bf16(softmax_fp32(S)) normalised BEFORE the rounding (pass 1: row max / sum, pass 2: P.V) ; O = bf16(P.V)
// -- with the same MFMA operand layout (S^T = K.Q^T with the keys of a 32-key block permuted over the two 16-row tiles, so that a
// lane ends with 8 CONSECUTIVE keys of one query = its A fragment of P.V).  What differs is where the operands come from:
//   * keys are walked by LOGICAL slot j in [0, t_past + S): the K / V row of slot j is `prefix panel + j * dh` for j < prefix_T
//     (the panel of prompt b / rows_per_prefix) and `own panel + (j - prefix_T) * dh` otherwise.  Only the address depends on the
//     cache kind: a shared-prefix cache and a plain cache with the same logical contents give the same bits.
//   * V is read where the cache holds it, [slot][dh] rows -- no transposed copy (a per-row transposed prefix would undo the
//     sharing).  The workgroup stages a [32 keys][DH] tile in LDS and the B operand of P.V (8 consecutive keys of ONE dh column
//     per lane) comes from two ds_read_b64_tr_b16 (lane map: tools/probes/tr_read_map.hip): the 16 lanes of a fragment group
//     address the [4 keys][16 dh] block of their key quad and lane i receives column i.  Every lane of the wave issues the reads
//     with an in-bounds, 8-byte aligned address (rows are clamped at staging time, never skipped), whole waves skip them only
//     on wave-uniform conditions: EXEC is all ones at the transposed reads.
//   * K rows ([slot][dh], contiguous) are staged next to it in the XOR-swizzled image of attn_lds_kernel and read back as
//     16-byte fragments.
// Workgroup = 4 waves = 64 query rows of one (row b, head h); a wave owns 16 of them; the waves walk the key blocks together
// (double-buffered tiles, one barrier per block).  The key range of a workgroup is causal: [0, t_past + its last query row].
// A query row whose allowed-key set is empty (a pad query) gets the reference's uniform softmax over ALL t_past + S keys, future
// ones included: the workgroup then repeats pass 1 over the full range, as attn_lds_kernel does.
// A row's bits depend on nothing but its own row of the batch: B rows at once = each row alone.
// Both kernels have a GROUPED mode (PcyExtAttnArgs::g_*): the prefix row, the split point between the two panels and the
// past length come from per-group device tables instead of (rows_per_prefix, Tp, t_past).  The walk over logical slots is the same, so a
// row of a grouped call has the bits of that row alone on a plain cache.
#include "pcy_internal.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short ext_s16x4;
typedef __attribute__((ext_vector_type(8))) short ext_s16x8;

__global__ void ext_pos_kernel(int32_t* __restrict__ pos, int n, int S, int t_past) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pos[i] = t_past + i % S;
}
__global__ void ext_pos_grouped_kernel(int32_t* __restrict__ pos, int n, int S, int t_own, const int32_t* __restrict__ g_len,
                                       const int32_t* __restrict__ g_row_grp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pos[i] = g_len[g_row_grp[i / S]] + t_own + i % S;
}

// GROUPED (pcy_attn_extend_grouped): row b belongs to group grp = g_row_grp[b]; the split point between the prefix panel (of prefix row grp,
// panel stride a.Tp) and the row's own panel is g_len[grp], and the row's past length is g_len[grp] + a.t_past.  Nothing else changes: the
// walk over logical slots, the blocks and the arithmetic are those of a one-row plain cache with the same logical contents.
template <int DH, bool GROUPED>
__global__ __launch_bounds__(256) void attn_ext_kernel(PcyExtAttnArgs a) {
  constexpr int KB = DH / 32, NT = DH / 16;
  constexpr int KCH = DH / 8;                  // 16-B chunks per K / V row
  constexpr int NLD = (32 * KCH) / 256;        // chunks per thread and tile (1 for DH = 64, 2 for DH = 128)
  constexpr int KTILE = 32 * DH * 2;
  constexpr int VSTR = DH * 2 + 32;            // V tile row stride in bytes: the 4 key rows of a transposed read fall on 4 x 8 distinct banks
  constexpr int VTILE = 32 * VSTR;
  __shared__ __attribute__((aligned(16))) char smem[2 * (KTILE + VTILE)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  int grp = 0, glen = 0;                       // (GROUPED only; workgroup-uniform)
  if constexpr (GROUPED) { grp = a.g_row_grp[b]; glen = a.g_len[grp]; }
  const int S = a.S, t_past = GROUPED ? glen + a.t_past : a.t_past;
  const int nk = t_past + S;                   // keys of the row after the append
  const int bq0 = blockIdx.x * 64;             // (< S by the grid)
  const int qr0 = bq0 + wave * 16;
  const bool active = qr0 < S;                 // wave-uniform
  const int G = a.H / a.Hkv;
  const int kvh = h / G;
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr float MASKZ = -0x1p126f;
  const uint8_t* keep = a.keep ? a.keep + (size_t)b * a.ld_keep : nullptr;

  // logical slot -> row address: the prompt's prefix panel below Tp, the row's own panel above
  const int Tp = GROUPED ? glen : (a.k_pre ? a.Tp : 0);
  const size_t own_off = ((size_t)b * a.Hkv + kvh) * a.Town * DH;
  const size_t pre_off = GROUPED ? ((size_t)grp * a.Hkv + kvh) * a.Tp * DH
                                 : (a.k_pre ? ((size_t)(b / a.rows_per_prefix) * a.Hkv + kvh) * Tp * DH : 0);
  const bf16_t* k_own = a.k_own + own_off;
  const bf16_t* v_own = a.v_own + own_off;
  const bf16_t* k_pre = a.k_pre ? a.k_pre + pre_off : nullptr;
  const bf16_t* v_pre = a.k_pre ? a.v_pre + pre_off : nullptr;

  bf16x8 qf[KB];
  {
    int qrow = qr0 + fr;
    qrow = qrow < S ? qrow : S - 1;
    const bf16_t* qp = a.q + (size_t)(b * S + qrow) * a.ldq + h * DH + fq * 8;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) qf[kb] = *reinterpret_cast<const bf16x8*>(qp + kb * 32);
  }
  auto kswz = [](int row) __attribute__((always_inline)) { return DH == 64 ? (row & 7) : (row & 15); };
  // cooperative fetch of the K (or V) rows of key block kb0: slots beyond the row's range are clamped to its last key (finite
  // values whose probability is exactly 0)
  struct Regs { uint4 v[NLD]; };
  auto fetch = [&](const bf16_t* own, const bf16_t* pre, int kb0) __attribute__((always_inline)) {
    Regs rr;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
      int j = kb0 + key;
      j = j < nk ? j : nk - 1;
      const bf16_t* row = j < Tp ? pre + (size_t)j * DH : own + (size_t)(j - Tp) * DH;
      rr.v[i] = *reinterpret_cast<const uint4*>(row + ch * 8);
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
  auto put_v = [&](char* buf, const Regs& rr) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
      *reinterpret_cast<uint4*>(buf + key * VSTR + ch * 16) = rr.v[i];
    }
  };
  const int krow_a = (fr >> 2) * 8 + (fr & 3);
  auto kfrag = [&](const char* buf, int tile, int kb) __attribute__((always_inline)) {
    const int row = krow_a + tile * 4;
    return *reinterpret_cast<const bf16x8*>(buf + (row * KCH + ((kb * 4 + fq) ^ kswz(row))) * 16);
  };
  // B operand of P.V for output columns n*16 .. +16: this lane's dh column n*16 + fr, keys fq*8 .. +8 of the block.
  // The lane's own address: key fq*8 + (fr >> 2) (+ 4 for the second read), dh n*16 + 4 (fr & 3) .. +4.
  const int vlane = (fq * 8 + (fr >> 2)) * VSTR + (fr & 3) * 8;
  auto vfrag = [&](const char* buf, int n) __attribute__((always_inline)) {
    typedef __attribute__((address_space(3))) ext_s16x4* tr_ptr_t;
    const char* p = buf + vlane + n * 32;
    const ext_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(p));
    const ext_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(p + 4 * VSTR));
    return __builtin_bit_cast(bf16x8, (ext_s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
  };
  // scores of this lane's 8 keys (kb0 + fq*8 ..) for query qr0 + fr, in the exp2 domain; masked MASKZ, out of range -inf
  const int qpos = t_past + qr0 + fr;          // logical slot of the query = its last allowed key
  auto scores = [&](const char* kbuf, int kb0, float (&s)[8]) __attribute__((always_inline)) {
    f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kbuf, 0, kb), qf[kb], sa, 0, 0, 0);
      sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kbuf, 1, kb), qf[kb], sb, 0, 0, 0);
    }
    const bool interior = !keep && (kb0 + 31 <= t_past + qr0);   // (then also kb0 + 32 <= nk); wave-uniform
    if (interior) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        float v = rbf(r < 4 ? sa[r & 3] : sb[r & 3]);
        v = rbf(v * a.scale);
        s[r] = v * LOG2E;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int j = kb0 + fq * 8 + r;
        float v = rbf(r < 4 ? sa[r & 3] : sb[r & 3]);
        v = rbf(v * a.scale);
        bool allowed = j <= qpos;
        if (keep && j < nk) allowed = allowed && (keep[j] != 0);
        s[r] = j < nk ? (allowed ? v * LOG2E : MASKZ) : -INFINITY;
      }
    }
  };

  char* kb_base = smem;
  char* vb_base = smem + 2 * KTILE;
  // key range of the WORKGROUP (uniform): up to its last query row
  int kend = t_past + ((bq0 + 64) < S ? (bq0 + 64) : S);
  float m = -INFINITY, l = 0.f;
  for (int attempt = 0; attempt < 2; ++attempt) {
    m = -INFINITY; l = 0.f;
    Regs ka = fetch(k_own, k_pre, 0);
    __syncthreads();                           // previous readers of buffer 0 are done
    put_k(kb_base, ka);
    __syncthreads();
    int cur = 0;
    for (int kb0 = 0; kb0 < kend; kb0 += 32, cur ^= 1) {
      const bool more = kb0 + 32 < kend;       // uniform
      if (more) ka = fetch(k_own, k_pre, kb0 + 32);
      if (active) {
        float s[8];
        scores(kb_base + cur * KTILE, kb0, s);
        float bm = s[0];
#pragma unroll
        for (int r = 1; r < 8; ++r) bm = fmaxf(bm, s[r]);
        bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float mn = fmaxf(m, bm);         // (finite from the first block on: key 0 is in range for every row)
        float bs = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) bs += __builtin_amdgcn_exp2f(s[r] - mn);
        bs += __shfl_xor(bs, 16, 64);
        bs += __shfl_xor(bs, 32, 64);
        l = l * __builtin_amdgcn_exp2f(m - mn) + bs;
        m = mn;
      }
      if (more) put_k(kb_base + (cur ^ 1) * KTILE, ka);
      __syncthreads();
    }
    const bool empty_row = active && (m == MASKZ) && (qr0 + fr) < S;
    // workgroup-uniform decision (every wave must walk the same key blocks)
    if (attempt == 0 && kend < nk && __syncthreads_or(empty_row ? 1 : 0)) { kend = nk; continue; }
    break;
  }

  const float rl = 1.0f / l;
  f32x4 oacc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) oacc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    Regs ka = fetch(k_own, k_pre, 0), va = fetch(v_own, v_pre, 0);
    __syncthreads();
    put_k(kb_base, ka); put_v(vb_base, va);
    __syncthreads();
    int cur = 0;
    for (int kb0 = 0; kb0 < kend; kb0 += 32, cur ^= 1) {
      const bool more = kb0 + 32 < kend;
      if (more) { ka = fetch(k_own, k_pre, kb0 + 32); va = fetch(v_own, v_pre, kb0 + 32); }
      if (active) {                            // wave-uniform: all 64 lanes take the transposed reads together
        float s[8];
        scores(kb_base + cur * KTILE, kb0, s);
        bf16x8 pf;
#pragma unroll
        for (int r = 0; r < 8; ++r) pf[r] = (short)f2bf(__builtin_amdgcn_exp2f(s[r] - m) * rl);
        const char* vbuf = vb_base + cur * VTILE;
#pragma unroll
        for (int n = 0; n < NT; ++n) oacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vfrag(vbuf, n), oacc[n], 0, 0, 0);
      }
      if (more) { put_k(kb_base + (cur ^ 1) * KTILE, ka); put_v(vb_base + (cur ^ 1) * VTILE, va); }
      __syncthreads();
    }
  }
  if (!active) return;
  // O[q = fq*4 + r][d = n*16 + fr]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qq = qr0 + fq * 4 + r;
    if (qq >= S) continue;
    bf16_t* op = a.o + (size_t)(b * S + qq) * a.ldo + h * DH + fr;
#pragma unroll
    for (int n = 0; n < NT; ++n) op[n * 16] = f2bf(oacc[n][r]);
  }
}

// attn_ext_packed_kernel<DH>: the same arithmetic with the 64 query slots of a workgroup PACKED over the rows of one prompt and the G query
// heads of one kv head.  Workgroup (tile, kv head g, prompt p); packed query index ((r * G + hg) * S + s), r over the rows of prompt p
// that the call holds (a plain cache: every row is its own prompt, Tp = 0, one row -- GQA packing only); a wave owns 16 packed slots.
//   shared phase: key blocks [0, 32 * (Tp / 32)) come from the prompt's prefix panel, are staged ONCE per tile and scored for all 64
//                 packed queries;
//   own phase:    for every row rho with a query in the tile (a workgroup-uniform loop) the blocks from 32 * (Tp / 32) to t_past + S,
//                 staged with the logical-slot addressing above (the block that straddles Tp reads both panels).  Lanes whose query
//                 belongs to another row take no part: no update of (m, l), P = 0 exactly; a wave without a query of rho skips the
//                 block's arithmetic (wave-uniform) but stages and synchronises with the others.
// Every row is walked to nk = t_past + S: the keys beyond a query's own position score -2^126 and contribute exactly 0, and a query
// without any allowed key gets the uniform softmax over all nk keys in the first walk (attn_ext_kernel's second attempt).
// Bits: a query meets the same 32-key blocks in the same order as in attn_ext_kernel; an MFMA output element depends on its own row
// and column only; a foreign block adds P = 0 times finite V; blocks beyond attn_ext_kernel's causal range add exp2(-2^126 - m) = 0.
// So the output equals attn_ext_kernel's bit for bit, and a query's bits depend on its own row of the batch only.
// GROUPED: the workgroup's "prompt" p is group p of the table -- row0 / rows from g_row0, the split point Tp = g_len[p] (panel stride a.Tp),
// t_past = g_len[p] + a.t_past.  The grid is sized for the largest group; everything below is written in terms of (row0, rows, Tp, t_past).
template <int DH, bool GROUPED>
__global__ __launch_bounds__(256) void attn_ext_packed_kernel(PcyExtAttnArgs a) {
  constexpr int KB = DH / 32, NT = DH / 16;
  constexpr int KCH = DH / 8;
  constexpr int NLD = (32 * KCH) / 256;
  constexpr int KTILE = 32 * DH * 2;
  constexpr int VSTR = DH * 2 + 32;
  constexpr int VTILE = 32 * VSTR;
  __shared__ __attribute__((aligned(16))) char smem[2 * (KTILE + VTILE)];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fq = lane >> 4;
  const int g = blockIdx.y, p = blockIdx.z;
  int g_r0 = 0, g_rows = 0, glen = 0;          // (GROUPED only; workgroup-uniform)
  if constexpr (GROUPED) { g_r0 = a.g_row0[p]; g_rows = a.g_row0[p + 1] - g_r0; glen = a.g_len[p]; }
  const int S = a.S, t_past = GROUPED ? glen + a.t_past : a.t_past;
  const int nk = t_past + S;
  const int G = a.H / a.Hkv, GS = G * S;
  const int Tp = GROUPED ? glen : (a.k_pre ? a.Tp : 0);
  const int rpp = a.k_pre ? a.rows_per_prefix : 1;
  const int row0 = GROUPED ? g_r0 : p * rpp;   // (< B by the grid)
  const int rows = GROUPED ? g_rows : ((a.B - row0) < rpp ? (a.B - row0) : rpp);   // the last prompt may be short of rows
  const int total = rows * GS;                 // packed queries of this (prompt, kv head)
  const int i0 = blockIdx.x * 64;
  if (i0 >= total) return;                     // workgroup-uniform (the grid is sized for a full prompt / the largest group)
  const int iw0 = i0 + wave * 16;
  const bool active = iw0 < total;             // wave-uniform
  constexpr float LOG2E = 1.4426950408889634f;
  constexpr float MASKZ = -0x1p126f;
  // this lane's query (slots beyond the last packed query repeat it: finite statistics, never stored)
  int idx = iw0 + fr;
  idx = idx < total ? idx : total - 1;
  const int qrow_r = idx / GS;
  const int qh = (idx - qrow_r * GS) / S, qs = idx - qrow_r * GS - qh * S;
  const int qb = row0 + qrow_r;
  const int qpos = t_past + qs;                // logical slot of the query = its last allowed key
  const uint8_t* keep = a.keep ? a.keep + (size_t)qb * a.ld_keep : nullptr;   // per lane: the query's own row
  // rows with a query in the tile / in this wave
  const int last_i = (i0 + 63) < total ? (i0 + 63) : total - 1;
  const int r_lo = i0 / GS, r_hi = last_i / GS;
  const int wlast_i = (iw0 + 15) < total ? (iw0 + 15) : total - 1;
  const int wr_lo = (iw0 < total ? iw0 : total - 1) / GS, wr_hi = wlast_i / GS;
  const int Tps = Tp & ~31;                    // keys of the shared phase

  const size_t panel = (size_t)a.Town * DH;
  const bf16_t* k_own0 = a.k_own + ((size_t)row0 * a.Hkv + g) * panel;   // row r of the prompt: + r * Hkv * panel
  const bf16_t* v_own0 = a.v_own + ((size_t)row0 * a.Hkv + g) * panel;
  const size_t row_step = (size_t)a.Hkv * panel;
  const size_t pre_off = a.k_pre ? ((size_t)p * a.Hkv + g) * (GROUPED ? a.Tp : Tp) * DH : 0;
  const bf16_t* k_pre = a.k_pre ? a.k_pre + pre_off : nullptr;
  const bf16_t* v_pre = a.k_pre ? a.v_pre + pre_off : nullptr;

  bf16x8 qf[KB];
  {
    const bf16_t* qp = a.q + (size_t)(qb * S + qs) * a.ldq + (g * G + qh) * DH + fq * 8;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) qf[kb] = *reinterpret_cast<const bf16x8*>(qp + kb * 32);
  }
  auto kswz = [](int row) __attribute__((always_inline)) { return DH == 64 ? (row & 7) : (row & 15); };
  struct Regs { uint4 v[NLD]; };
  // rows of key block kb0 as row `rho` of the prompt sees them (slots beyond the range are clamped to the last key, never skipped)
  auto fetch = [&](const bf16_t* own0, const bf16_t* pre, int rho, int kb0) __attribute__((always_inline)) {
    Regs rr;
    const bf16_t* own = own0 + (size_t)(rho < 0 ? r_lo : rho) * row_step;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
      int j = kb0 + key;
      j = j < nk ? j : nk - 1;
      const bf16_t* row = j < Tp ? pre + (size_t)j * DH : own + (size_t)(j - Tp) * DH;
      rr.v[i] = *reinterpret_cast<const uint4*>(row + ch * 8);
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
  auto put_v = [&](char* buf, const Regs& rr) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int c = tid + i * 256, key = c / KCH, ch = c % KCH;
      *reinterpret_cast<uint4*>(buf + key * VSTR + ch * 16) = rr.v[i];
    }
  };
  const int krow_a = (fr >> 2) * 8 + (fr & 3);
  auto kfrag = [&](const char* buf, int tile, int kb) __attribute__((always_inline)) {
    const int row = krow_a + tile * 4;
    return *reinterpret_cast<const bf16x8*>(buf + (row * KCH + ((kb * 4 + fq) ^ kswz(row))) * 16);
  };
  const int vlane = (fq * 8 + (fr >> 2)) * VSTR + (fr & 3) * 8;
  auto vfrag = [&](const char* buf, int n) __attribute__((always_inline)) {
    typedef __attribute__((address_space(3))) ext_s16x4* tr_ptr_t;
    const char* pp = buf + vlane + n * 32;
    const ext_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(pp));
    const ext_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((tr_ptr_t)(pp + 4 * VSTR));
    return __builtin_bit_cast(bf16x8, (ext_s16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
  };
  auto scores = [&](const char* kbuf, int kb0, float (&s)[8]) __attribute__((always_inline)) {
    f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kbuf, 0, kb), qf[kb], sa, 0, 0, 0);
      sb = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(kbuf, 1, kb), qf[kb], sb, 0, 0, 0);
    }
    const bool interior = !a.keep && (kb0 + 31 <= t_past);   // every key allowed for every query; workgroup-uniform
    if (interior) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        float v = rbf(r < 4 ? sa[r & 3] : sb[r & 3]);
        v = rbf(v * a.scale);
        s[r] = v * LOG2E;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int j = kb0 + fq * 8 + r;
        float v = rbf(r < 4 ? sa[r & 3] : sb[r & 3]);
        v = rbf(v * a.scale);
        bool allowed = j <= qpos;
        if (keep && j < nk) allowed = allowed && (keep[j] != 0);
        s[r] = j < nk ? (allowed ? v * LOG2E : MASKZ) : -INFINITY;
      }
    }
  };
  // the walk: (rho, kb0) = (-1, 0), (-1, 32) .. (-1, Tps - 32), then for rho = r_lo .. r_hi: (rho, Tps), (rho, Tps + 32) .. below nk
  const int rho_first = Tps > 0 ? -1 : r_lo;
  struct Step { int rho, kb0; };
  auto advance = [=](Step c) __attribute__((always_inline)) {
    const int kb1 = c.kb0 + 32;
    Step n;
    if (c.rho < 0) { n.rho = kb1 >= Tps ? r_lo : -1; n.kb0 = kb1; }          // (kb1 == Tps at the change)
    else if (kb1 >= nk) { n.rho = c.rho + 1; n.kb0 = Tps; }
    else { n.rho = c.rho; n.kb0 = kb1; }
    return n;
  };
  // wave-uniform: does this wave hold a query that meets the block of row rho
  auto takes_part = [&](int rho) __attribute__((always_inline)) { return active && (rho < 0 || (rho >= wr_lo && rho <= wr_hi)); };

  char* kb_base = smem;
  char* vb_base = smem + 2 * KTILE;
  float m = -INFINITY, l = 0.f;
  {
    int rho = rho_first, kb0 = 0;
    Regs ka = fetch(k_own0, k_pre, rho, kb0);
    put_k(kb_base, ka);
    __syncthreads();
    int cur = 0;
    while (rho <= r_hi) {
      const Step nx = advance(Step{rho, kb0});
      const int nrho = nx.rho, nkb0 = nx.kb0;
      const bool more = nrho <= r_hi;           // uniform
      if (more) ka = fetch(k_own0, k_pre, nrho, nkb0);
      if (takes_part(rho)) {
        const bool mine = rho < 0 || qrow_r == rho;   // the same for the 4 lanes of a query
        float s[8];
        scores(kb_base + cur * KTILE, kb0, s);
        float bm = s[0];
#pragma unroll
        for (int r = 1; r < 8; ++r) bm = fmaxf(bm, s[r]);
        bm = fmaxf(bm, __shfl_xor(bm, 16, 64));
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float mn = fmaxf(m, bm);         // finite: every block holds a key below nk (so never -inf - -inf below)
        float bs = 0.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) bs += __builtin_amdgcn_exp2f(s[r] - mn);
        bs += __shfl_xor(bs, 16, 64);
        bs += __shfl_xor(bs, 32, 64);
        const float nl = l * __builtin_amdgcn_exp2f(m - mn) + bs;
        l = mine ? nl : l;
        m = mine ? mn : m;
      }
      if (more) put_k(kb_base + (cur ^ 1) * KTILE, ka);
      __syncthreads();
      rho = nrho; kb0 = nkb0; cur ^= 1;
    }
  }

  const float rl = 1.0f / l;
  f32x4 oacc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) oacc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
  {
    int rho = rho_first, kb0 = 0;
    Regs ka = fetch(k_own0, k_pre, rho, kb0), va = fetch(v_own0, v_pre, rho, kb0);
    __syncthreads();
    put_k(kb_base, ka); put_v(vb_base, va);
    __syncthreads();
    int cur = 0;
    while (rho <= r_hi) {
      const Step nx = advance(Step{rho, kb0});
      const int nrho = nx.rho, nkb0 = nx.kb0;
      const bool more = nrho <= r_hi;
      if (more) { ka = fetch(k_own0, k_pre, nrho, nkb0); va = fetch(v_own0, v_pre, nrho, nkb0); }
      if (takes_part(rho)) {                   // wave-uniform: all 64 lanes take the transposed reads together
        const bool mine = rho < 0 || qrow_r == rho;
        float s[8];
        scores(kb_base + cur * KTILE, kb0, s);
        bf16x8 pf;
#pragma unroll
        for (int r = 0; r < 8; ++r) pf[r] = mine ? (short)f2bf(__builtin_amdgcn_exp2f(s[r] - m) * rl) : (short)0;   // (m is finite)
        const char* vbuf = vb_base + cur * VTILE;
#pragma unroll
        for (int n = 0; n < NT; ++n) oacc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, vfrag(vbuf, n), oacc[n], 0, 0, 0);
      }
      if (more) { put_k(kb_base + (cur ^ 1) * KTILE, ka); put_v(vb_base + (cur ^ 1) * VTILE, va); }
      __syncthreads();
      rho = nrho; kb0 = nkb0; cur ^= 1;
    }
  }
  if (!active) return;
  // O[packed query iw0 + fq*4 + r][d = n*16 + fr]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = iw0 + fq * 4 + r;
    if (qi >= total) continue;
    const int orow = qi / GS, oh = (qi - orow * GS) / S, os = qi - orow * GS - oh * S;
    bf16_t* op = a.o + (size_t)((row0 + orow) * S + os) * a.ldo + (g * G + oh) * DH + fr;
#pragma unroll
    for (int n = 0; n < NT; ++n) op[n * 16] = f2bf(oacc[n][r]);
  }
}

}  // namespace

void pcy_launch_ext_pos(hipStream_t s, int32_t* pos, int B, int S, int t_past) {
  const int n = B * S;
  if (n > 0) hipLaunchKernelGGL(ext_pos_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pos, n, S, t_past);
}
void pcy_launch_ext_pos_grouped(hipStream_t s, int32_t* pos, int B, int S, int t_own, const int32_t* g_len, const int32_t* g_row_grp) {
  const int n = B * S;
  if (n > 0) hipLaunchKernelGGL(ext_pos_grouped_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pos, n, S, t_own, g_len, g_row_grp);
}

bool pcy_launch_attn_extend(hipStream_t s, const PcyExtAttnArgs& a) {
  if (a.B <= 0 || a.S <= 0) return true;
  const dim3 grid((a.S + 63) / 64, a.H, a.B);
  if (a.dh != 64 && a.dh != 128) return false;
  if (a.g_row_grp) {   // grouped mode: the tables say which prefix row and which split point a row has
    if (a.dh == 64) hipLaunchKernelGGL((attn_ext_kernel<64, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attn_ext_kernel<128, true>), grid, dim3(256), 0, s, a);
  } else {
    if (a.dh == 64) hipLaunchKernelGGL((attn_ext_kernel<64, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attn_ext_kernel<128, false>), grid, dim3(256), 0, s, a);
  }
  return true;
}

bool pcy_launch_attn_extend_packed(hipStream_t s, const PcyExtAttnArgs& a) {
  if (a.B <= 0 || a.S <= 0) return true;
  if (a.dh != 64 && a.dh != 128) return false;
  if (a.g_row0) {      // grouped mode: one grid layer per group, sized for the largest one (a smaller group's spare tiles return at once)
    const long total = (long)a.g_max_rows * (a.H / a.Hkv) * a.S;
    const dim3 grid((unsigned)((total + 63) / 64), a.Hkv, a.n_groups);
    if (a.dh == 64) hipLaunchKernelGGL((attn_ext_packed_kernel<64, true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((attn_ext_packed_kernel<128, true>), grid, dim3(256), 0, s, a);
    return true;
  }
  const int rpp = a.k_pre ? a.rows_per_prefix : 1;
  const int rows = a.B < rpp ? a.B : rpp;
  const long total = (long)rows * (a.H / a.Hkv) * a.S;
  const dim3 grid((unsigned)((total + 63) / 64), a.Hkv, (a.B + rpp - 1) / rpp);
  if (a.dh == 64) hipLaunchKernelGGL((attn_ext_packed_kernel<64, false>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((attn_ext_packed_kernel<128, false>), grid, dim3(256), 0, s, a);
  return true;
}
