// Tile staging (global -> LDS DMA) and fragment reads of the bf16 MFMA GEMMs: shared by pcy_gemm.hip and pcy_xent.hip, so that every kernel
// built on them walks k in the same order per output element (same bits).
#pragma once
#include "pcy_common.h"

namespace {

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gptr_t;

// stage a [128 rows][BK k] bf16 tile with 1-KiB wave-instructions (LDS image lane-linear).  A row holds CPR = BK/8
// 16-byte chunks; LDS chunk position c' of row r holds global chunk c' ^ swz(r), the same XOR is applied on the read side:
//   BK=64 (128-B rows): swz = r & 7        BK=32 (64-B rows): swz = (r >> 2) & 3      -> conflict-free ds_read_b128
// SW = 1 (BK = 64 only): the swizzle of a W tile whose rows are read in the PERMUTED order of the 256 x 256 kernels (wperm_row
// below: the 16 lanes fr of a fragment read hit rows a*8 + h*4 + b, a = fr >> 2, b = fr & 3) -- s(r) = 2*((r >> 3) & 3) + ((r >> 1) & 1)
// puts the 16 lanes of every ds_read_b128 lane group on 16 distinct 16-byte slots, as r & 7 does for 16 consecutive rows.
// SW = 2: the same for the SwiGLU row order (wperm_row_swiglu: a = bits 5 and 3 of the row).
template <int BK, int SW = 0>
__device__ __forceinline__ int swz(int r) {
  if (SW == 1) return (((r >> 3) & 3) << 1) | ((r >> 1) & 1);
  if (SW == 2) return (((r >> 5) & 1) << 2) | (((r >> 3) & 1) << 1) | ((r >> 1) & 1);
  return BK == 64 ? (r & 7) : ((r >> 2) & 3);
}

// STG = 1: the pieces go out as `buffer_load_dwordx4 ... offen lds` -- a buffer resource based at the tile's first row (wave-uniform,
// SGPRs), the lane's byte offset inside the tile (32 bits, the same for every k-step: computed once per tile) and the k offset as
// the instruction's SCALAR offset.  The global_load_lds form (STG = 0) carries a 64-bit address per lane and piece, which the k-loop
// re-forms with a v_lshl_add_u64 per piece; with the wave index read into an SGPR (readfirstlane) the LDS destination (M0) is
// scalar arithmetic as well instead of a VGPR add + v_readfirstlane per piece.
template <int BK, int ROWS = 128, int NW = 4, int SW = 0, int STG = 0>
__device__ __forceinline__ void stage_tile(const bf16_t* __restrict__ g, int ld, int row0, int nrows_valid, int k0,
                                           char* lds_tile, int wave, int lane) {
  constexpr int CPR = BK / 8, RPI = 64 / CPR, NINST = ROWS / RPI;
  if constexpr (STG >= 1) {
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(g + (size_t)row0 * ld), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int i = 0; i < NINST / NW; ++i) {
      const int inst = wave * (NINST / NW) + i;
      const int r = inst * RPI + lane / CPR;
      const int c = (lane % CPR) ^ swz<BK, SW>(r);
      const int rl = row0 + r < nrows_valid ? r : nrows_valid - 1 - row0;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_ptr_t)(lds_tile + inst * 1024), 16, (rl * ld + c * 8) * 2, k0 * 2, 0, 0);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < NINST / NW; ++i) {
    const int inst = wave * (NINST / NW) + i;
    const int r = inst * RPI + lane / CPR;
    const int cp = lane % CPR;
    const int c = cp ^ swz<BK, SW>(r);
    int gr = row0 + r;
    gr = gr < nrows_valid ? gr : nrows_valid - 1;
    const bf16_t* src = g + (size_t)gr * ld + k0 + c * 8;
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lds_ptr_t)(lds_tile + inst * 1024), 16, 0, 0);
  }
}

template <int BK, int SW = 0>
__device__ __forceinline__ bf16x8 lds_frag(const char* lds_tile, int row, int chunk) {
  return *reinterpret_cast<const bf16x8*>(lds_tile + row * (BK * 2) + ((chunk ^ swz<BK, SW>(row)) << 4));
}

}  // namespace
