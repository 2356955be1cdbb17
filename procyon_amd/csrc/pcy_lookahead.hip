// Greedy decoding with lookahead: the device-side steps between two W-row extension passes of one prompt.
//
//   pcy_look_draft   history -> window[1..W) by prompt lookup (the last g tokens are looked up in the prompt and the text so far; what followed
//                    their most recent earlier occurrence is the draft), then the W embedding rows of the window for the next pass
//   pcy_look_verify  logits [W, V] of the pass -> per row argmax + bf16 log-prob (the greedy pick's own code: pcy_pick.h and its stage-1 kernel),
//                    the leading drafts that were right, the commit (tokens, log-prob, history, position, step, counters), the logits record
//
// Nothing here touches the K / V cache: rows of rejected drafts leave their K / V in slots [*pos, *pos + W - 1 - accepted) behind the new
// *pos, and the next pass -- which always has W rows and starts at the new *pos -- rewrites every one of them before any query can read it
// (the extension attention of a query at slot p reads slots [0, p] only, and its own pass has written [*pos, p] by then).
//
// Every decision is taken by one thread over per-row results that a fixed partition of V produced (64 chunks per row, merged by one wave in
// lane order): no atomics, no dependence on scheduling.
#include "pcy_internal.h"
#include "pcy_pick.h"

namespace {

constexpr int LOOK_NT = 256;
constexpr int LOOK_WMAX = 32;    // rows of a pass (pcy.h: 2 <= W <= 32)
constexpr int LOOK_GMAX = 16;    // longest n-gram looked up

// The drafts of the window, computed by EVERY workgroup of the launch (the history is a few thousand ints in L2; a launch of its own for the
// gather would cost more than the repeated search): workgroup r then gathers embedding row r, workgroup 0 also stores window[1..W).
//   h = hist[0..n); for g = gmax .. gmin: the largest i with i + g < n and h[i..i+g) == h[n-g..n), every compared entry >= 0;
//   draft[j] = h[i+g+j] until the history ends or an entry is negative; the rest (all of them without a match) = h[n-1];
//   forced[step + j] >= 0 replaces draft j.
__global__ __launch_bounds__(LOOK_NT) void look_draft_kernel(PcyLookArgs a, const bf16_t* __restrict__ embed, int V, int d, bf16_t* __restrict__ out) {
  __shared__ int red[LOOK_NT / 64];
  __shared__ int suffix[LOOK_GMAX];
  __shared__ int draft[LOOK_WMAX];
  __shared__ int found_i, found_g;
  const int tid = threadIdx.x;
  const int* __restrict__ h = a.hist;
  int n = *a.n_hist;
  n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
  if (tid == 0) { found_i = -1; found_g = 0; }
  __syncthreads();
  for (int g = a.gmax; g >= a.gmin; --g) {
    if (g < 1 || g >= n) continue;                       // (uniform: needs an i >= 0 with i + g < n)
    if (tid < g) suffix[tid] = h[n - g + tid];
    __syncthreads();
    bool ok = true;
    for (int e = 0; e < g; ++e) ok = ok && suffix[e] >= 0;
    int best = -1;
    if (ok) {
      for (int i = tid; i + g < n; i += LOOK_NT) {      // ascending i per thread: the last hit is the thread's largest
        bool eq = true;
        for (int e = 0; e < g && eq; ++e) eq = h[i + e] == suffix[e];
        if (eq) best = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int ob = __shfl_xor(best, o, 64); best = ob > best ? ob : best; }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < LOOK_NT / 64; ++w) best = red[w] > best ? red[w] : best;
      if (best >= 0) { found_i = best; found_g = g; }
    }
    __syncthreads();
    if (found_i >= 0) break;                             // (uniform: read from LDS behind the barrier)
  }
  if (tid == 0) {
    const int filler = n > 0 ? h[n - 1] : a.window[0];
    const int step = *a.step;
    int p = found_i >= 0 ? found_i + found_g : n;        // first continuation slot (n: none)
    for (int j = 0; j < a.W - 1; ++j) {
      int t = filler;
      if (p < n && h[p] >= 0) { t = h[p]; ++p; } else p = n;
      if (a.forced && step + j >= 0 && step + j < a.max_steps && a.forced[step + j] >= 0) t = a.forced[step + j];
      draft[j] = t;
    }
  }
  __syncthreads();
  const int r = blockIdx.x;
  if (r == 0)
    for (int j = tid; j < a.W - 1; j += LOOK_NT) a.window[j + 1] = draft[j];
  const int tok = r == 0 ? a.window[0] : draft[r - 1];
  // a token outside the table (a caller's history may hold anything) reads row 0: wrong, but inside the table
  const bf16_t* src = embed + (size_t)((unsigned)tok < (unsigned)V ? tok : 0) * d;
  bf16_t* dst = out + (size_t)r * d;
  for (int c = tid * 8; c < d; c += LOOK_NT * 8) *reinterpret_cast<uint4*>(dst + c) = ldg16(src + c);   // (d % 8 == 0: checked by the entry)
}

// Rows 0..W-1 have their 64 chunk partials (pick_stage1_kernel); wave w merges rows w, w + 4, ... exactly as pick_stage2_kernel does, then one
// thread compares with the drafts and commits.
// EOS stop (stop.finished != nullptr; pcy.h): the commit ends with the first committed token that equals eos_id -- the rows behind it are
// treated as rejected drafts -- and raises *done; a launch that finds *done set commits nothing (last[1] = 0).
__global__ __launch_bounds__(LOOK_NT) void look_verify_kernel(PcyLookArgs a, const bf16_t* __restrict__ logits, int V, const PickPartial* __restrict__ part,
                                                              PcyStop stop) {
  __shared__ int tok[LOOK_WMAX];
  __shared__ float lsm[LOOK_WMAX];
  const int l = threadIdx.x & 63;
  for (int r = threadIdx.x >> 6; r < a.W; r += LOOK_NT / 64) {
    float best, se;
    int t;
    pick_merge_row(part[r * PICK_NB + l], best, t, se);
    if (l == 0) { tok[r] = t; lsm[r] = pick_logprob(logits + (size_t)r * V, t, best, se); }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int step = *a.step, pos = *a.pos;
  int nh = *a.n_hist;
  nh = nh < 0 ? 0 : (nh > a.cap ? a.cap : nh);
  int acc = 0;                                           // leading drafts that are right: draft j is window[j + 1], right when it is row j's argmax
  while (acc < a.W - 1 && a.window[acc + 1] == tok[acc]) ++acc;
  int n = a.max_steps - step;
  n = n < 0 ? 0 : (n > acc + 1 ? acc + 1 : n);
  bool eos = false;
  if (stop.finished) {
    if (*stop.done) n = 0;
    for (int i = 0; i < n && !eos; ++i)
      if (tok[i] == stop.eos_id) { n = i + 1; eos = true; }
  }
  float lp = a.logprob[0];
  for (int i = 0; i < n; ++i) {
    a.tokens_out[step + i] = tok[i];
    lp += lsm[i];                                        // in row order: the sum a step-by-step run forms
    if (nh + i < a.cap) a.hist[nh + i] = tok[i];
  }
  a.last[0] = acc; a.last[1] = n; a.last[2] = step; a.last[3] = pos;
  if (n == 0) return;
  a.logprob[0] = lp;
  a.next_tok[0] = tok[n - 1];
  a.window[0] = tok[n - 1];
  *a.pos = pos + n;
  *a.step = step + n;
  *a.n_hist = nh + n < a.cap ? nh + n : a.cap;
  a.counters[0] += 1;
  a.counters[1] += n;
  a.counters[2 + n - 1] += 1;
  if (eos) {
    stop.finished[0] = 1;
    if (stop.n_steps_run) *stop.n_steps_run = step + n;
    *stop.done = 1;
  }
}

// rows [0, last[1]) of the pass's logits -> rows last[2].. of the record (one prompt: row stride ld); `all` may be pinned host memory.
// 16-byte stores where the record allows them, as store_logits_kernel (pcy_engine.hip).
__global__ __launch_bounds__(LOOK_NT) void look_store_kernel(const bf16_t* __restrict__ logits, bf16_t* __restrict__ all, const int32_t* __restrict__ last,
                                                             int V, int ld) {
  const int n = last[1];
  const size_t step0 = (size_t)last[2];
  const int chunks = (V + 7) / 8;
  const bool vec = (ld % 8 == 0) && ((reinterpret_cast<uintptr_t>(all) & 15) == 0);
  for (size_t i = (size_t)blockIdx.x * LOOK_NT + threadIdx.x; i < (size_t)n * chunks; i += (size_t)gridDim.x * LOOK_NT) {
    const int r = (int)(i / chunks), c = (int)(i % chunks);
    const bf16_t* src = logits + (size_t)r * V + c * 8;
    bf16_t* dst = all + (step0 + r) * ld + c * 8;
    if (vec && c * 8 + 8 <= V) {
      const uint32_t w0 = src[0] | ((uint32_t)src[1] << 16), w1 = src[2] | ((uint32_t)src[3] << 16);
      const uint32_t w2 = src[4] | ((uint32_t)src[5] << 16), w3 = src[6] | ((uint32_t)src[7] << 16);
      *reinterpret_cast<uint4*>(dst) = make_uint4(w0, w1, w2, w3);
    } else {
      for (int e = 0; e < 8 && c * 8 + e < V; ++e) dst[e] = src[e];
    }
  }
}

}  // namespace

size_t pcy_look_verify_ws_bytes(int W) { return (size_t)W * PICK_NB * sizeof(PickPartial); }

void pcy_launch_look_draft(hipStream_t s, const PcyLookArgs& a, const bf16_t* embed, int V, int d, bf16_t* embeds_out) {
  hipLaunchKernelGGL(look_draft_kernel, dim3(a.W), dim3(LOOK_NT), 0, s, a, embed, V, d, embeds_out);
}

void pcy_launch_look_verify(hipStream_t s, const PcyLookArgs& a, const bf16_t* logits, int V, bf16_t* logits_all, int logits_all_ld, void* partials,
                            const PcyStop& stop) {
  pcy_launch_pick_stage1(s, logits, a.W, V, partials);
  hipLaunchKernelGGL(look_verify_kernel, dim3(1), dim3(LOOK_NT), 0, s, a, logits, V, reinterpret_cast<const PickPartial*>(partials), stop);
  if (logits_all)
    hipLaunchKernelGGL(look_store_kernel, dim3(a.W >= 8 ? 256 : 64), dim3(LOOK_NT), 0, s, logits, logits_all, a.last, V, logits_all_ld > 0 ? logits_all_ld : V);
}
