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
#include "pcy_internal.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short ext_s16x4;
typedef __attribute__((ext_vector_type(8))) short ext_s16x8;

__global__ void ext_pos_kernel(int32_t* __restrict__ pos, int n, int S, int t_past) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) pos[i] = t_past + i % S;
}

template <int DH>
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
  const int S = a.S, t_past = a.t_past;
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
  const int Tp = a.k_pre ? a.Tp : 0;
  const size_t own_off = ((size_t)b * a.Hkv + kvh) * a.Town * DH;
  const size_t pre_off = a.k_pre ? ((size_t)(b / a.rows_per_prefix) * a.Hkv + kvh) * Tp * DH : 0;
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

}  // namespace

void pcy_launch_ext_pos(hipStream_t s, int32_t* pos, int B, int S, int t_past) {
  const int n = B * S;
  if (n > 0) hipLaunchKernelGGL(ext_pos_kernel, dim3((n + 255) / 256), dim3(256), 0, s, pos, n, S, t_past);
}

bool pcy_launch_attn_extend(hipStream_t s, const PcyExtAttnArgs& a) {
  if (a.B <= 0 || a.S <= 0) return true;
  const dim3 grid((a.S + 63) / 64, a.H, a.B);
  if (a.dh == 64) hipLaunchKernelGGL(attn_ext_kernel<64>, grid, dim3(256), 0, s, a);
  else if (a.dh == 128) hipLaunchKernelGGL(attn_ext_kernel<128>, grid, dim3(256), 0, s, a);
  else return false;
  return true;
}
