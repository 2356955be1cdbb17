// The row merge of the greedy pick, shared by pick_stage2_kernel (pcy_elem.hip) and look_verify_kernel (pcy_lookahead.hip): one definition,
// so that a row's token and log-prob increment have the same bits whichever kernel commits it.
#pragma once
#include "pcy_common.h"

constexpr int PICK_NT = 256;
constexpr int PICK_NB = 64;    // chunks per row == lanes of the merging wave
struct PickPartial { float mx; int idx; float se; int pad; };   // per chunk: max, its lowest index, sum exp(x - max) (0 for an empty / all -inf chunk)

// One wave merges the PICK_NB partials of a row (lane l holds partial l) -> in every lane: the row's maximum, its lowest index, and
// sum exp(x - max) over the row.
__device__ __forceinline__ void pick_merge_row(const PickPartial pp, float& best, int& bi, float& se) {
  best = pp.mx;
  bi = pp.idx;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  se = pp.se * expf(pp.mx - best);   // empty chunks: mx = -inf -> exp(-inf) = 0
  se = wave_sum(se);
}
// log_softmax in model dtype at the picked token: bf16( x - max - log(sum exp(x - max)) ), x[tok] == max
__device__ __forceinline__ float pick_logprob(const bf16_t* __restrict__ row_logits, int bi, float best, float se) {
  return rbf((bf2f(row_logits[bi]) - best) - logf(se));
}
