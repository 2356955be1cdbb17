// fp32 selection on the device: what stands between two steps of an fp32 generation besides the greedy pick --
//   the K / V reorder of a beam search on the token-major fp32 caches (and the row copy that replicates a B-row prefill into B * beam rows),
//   the sampling / nucleus step on fp32 logits.
// The fp32 beam step itself is the bf16 step's code on another logits type (pcy_elem.hip, pcy_launch_f32_beam_step).
// Nothing here uses a floating-point atomic: every sum that decides something is either a block reduction in a fixed order or a sum of
// 64-bit fixed-point values (integer addition is associative), so the result is a function of the inputs alone and an eager and a
// replayed run are bit-equal.
#include "pcy_common.h"
#include "pcy_internal.h"

namespace {

// ------------------------------------------------------------------------------------------------ K / V reorder and row copy
// Token-major caches [L][Bcache][Tmax][kw]: slots [t0, t) of a row are ONE contiguous span of (t - t0) * kw floats.
constexpr int R_NT = 256;

// grid (B, 2L, z).  to_tmp = 1: scratch row (lw, b) <- cache row rows[b]; to_tmp = 0: cache row b <- scratch row (lw, b).  Two launches, so
// every source is read before any destination is written: correct for any map (cycles, one source for many rows).  Rows that keep their
// place are skipped in both passes; a source outside the cache moves nothing.  Scratch rows are (Tmax - t0) * kw floats apart whatever t is.
__global__ __launch_bounds__(R_NT) void kv_reorder_f32_kernel(float* __restrict__ kbase, float* __restrict__ vbase, float* __restrict__ tmp,
                                                              const int32_t* __restrict__ rows, int B, int Bcache, int Tmax, int kw, int t0, int t,
                                                              const int32_t* __restrict__ t_dev, int to_tmp) {
  const int b = blockIdx.x, lw = blockIdx.y, l = lw >> 1;
  const int sb = rows[b];
  if (sb == b || sb < 0 || sb >= Bcache) return;
  if (t_dev) t = *t_dev;
  t = t < Tmax ? t : Tmax;
  if (t <= t0) return;
  float* cache = ((lw & 1) ? vbase : kbase) + (size_t)l * Bcache * Tmax * kw;
  float* scr = tmp + ((size_t)lw * B + b) * (size_t)(Tmax - t0) * kw;
  const float4* sp = reinterpret_cast<const float4*>(to_tmp ? cache + ((size_t)sb * Tmax + t0) * kw : scr);
  float4* dp = reinterpret_cast<float4*>(to_tmp ? scr : cache + ((size_t)b * Tmax + t0) * kw);
  const size_t n4 = (size_t)(t - t0) * kw / 4;
  for (size_t i = (size_t)blockIdx.z * R_NT + threadIdx.x; i < n4; i += (size_t)gridDim.z * R_NT) dp[i] = sp[i];
}

// grid (B, 2L, z): dst row r <- slots [0, t) of src row rows[r] (another cache: out of place)
__global__ __launch_bounds__(R_NT) void kv_copy_rows_f32_kernel(float* __restrict__ dk, float* __restrict__ dv, int Bdst, int Tdst,
                                                                const float* __restrict__ sk, const float* __restrict__ sv, int Bsrc, int Tsrc,
                                                                const int32_t* __restrict__ rows, int kw, int t) {
  const int r = blockIdx.x, lw = blockIdx.y, l = lw >> 1;
  const int sr = rows[r];
  if (sr < 0 || sr >= Bsrc) return;
  const float4* sp = reinterpret_cast<const float4*>(((lw & 1) ? sv : sk) + ((size_t)l * Bsrc + sr) * Tsrc * kw);
  float4* dp = reinterpret_cast<float4*>(((lw & 1) ? dv : dk) + ((size_t)l * Bdst + r) * Tdst * kw);
  const size_t n4 = (size_t)t * kw / 4;
  for (size_t i = (size_t)blockIdx.z * R_NT + threadIdx.x; i < n4; i += (size_t)gridDim.z * R_NT) dp[i] = sp[i];
}

int span_blocks(size_t n4) {   // workgroups along z for a span of n4 16-byte pieces: 4096 pieces (64 KB) each, at most 16
  const size_t z = (n4 + 4095) / 4096;
  return z < 1 ? 1 : z > 16 ? 16 : (int)z;
}

// ------------------------------------------------------------------------------------------------ sampling / nucleus step
// `_generate_sampling`'s selection (model_unified.py:896-906) on a row of fp32 logits x [V]:
//   p = softmax(x / temperature)            (nucleus: softmax(x), times the mask below)
//   nucleus mask: the tokens whose ascending cumulative probability has reached 1 - nucleus_p; equal probabilities in token order (a
//                 stable sort: the lower index is the smaller); not renormalised; nothing reaches the threshold: everything is kept
//   token = first i in vocabulary order with cdf_i > u * total;  logprob += log_softmax(x)[token]
// Three launches: chunk statistics (S_NCH chunks per row), the probabilities into a scratch row, and one 512-thread workgroup per row
// that selects.  A row of 128 263 fp32 probabilities does not fit the registers of that workgroup: it re-reads the 0.5 MB row from L2 in
// every pass (three radix passes + the CDF pass).
// Deterministic by construction: the chunk sums are block reductions in a fixed order, the partials are combined in chunk order, and
// every mass that decides something (bucket masses of the radix select, the kept total, the CDF) is a sum of fx(p) = trunc(p * 2^44) in
// 64 bits -- integer sums, whatever order the atomics of a histogram arrive in.  V <= 163840 < 2^18: a sum stays below 2^62, and the
// truncation loses less than V * 2^-44 < 2^-26 of mass over a row.
constexpr int S_NCH = 32, S_NT = 256;
constexpr int SEL_NT = 512, SEL_NW = SEL_NT / 64;      // (512: the 64-bit scans of four elements per thread want more than the 128 registers of a 1024-thread workgroup)
constexpr int RADIX_A = 12, RADIX_B = 12, RADIX_C = 8;      // bits of a probability's pattern per pass, from the top (the sign bit is 0)
constexpr int HIST_N = 1 << RADIX_A;

__device__ __forceinline__ unsigned long long fx(float p) { return (unsigned long long)(p * 17592186044416.0f); }   // p in [0, 1]: exact scaling, truncated

// max x, sum exp(x - max) and (temperature != 1) sum exp(x / T - max / T) of one chunk of every row: grid (S_NCH, B).  x / T is the
// correctly rounded fp32 quotient (monotonic in x: max / T is the maximum of the scaled chunk).  An empty chunk or one that holds only
// -inf gives (max = -inf, sums = 0), never a NaN.
__global__ __launch_bounds__(S_NT) void sample_stats_f32_kernel(const float* __restrict__ logits, int V, float temperature, float4* __restrict__ part) {
  __shared__ float red[S_NT / 64];
  const int c = blockIdx.x, b = blockIdx.y;
  const int chunk = (V + S_NCH - 1) / S_NCH;
  const int lo = c * chunk, hi = (lo + chunk) < V ? (lo + chunk) : V;
  const float* x = logits + (size_t)b * V;
  float m = -INFINITY;
  for (int v = lo + threadIdx.x; v < hi; v += S_NT) m = fmaxf(m, x[v]);
  m = block_max<S_NT>(m, red);
  const bool scaled = temperature != 1.0f;
  const float ms = m / temperature;
  float se = 0.f, ss = 0.f;
  if (m > -INFINITY) {
    for (int v = lo + threadIdx.x; v < hi; v += S_NT) {
      const float xv = x[v];
      se += expf(xv - m);
      if (scaled) ss += expf(xv / temperature - ms);
    }
  }
  se = block_sum<S_NT>(se, red);
  ss = scaled ? block_sum<S_NT>(ss, red) : se;
  if (threadIdx.x == 0) part[(size_t)b * S_NCH + c] = m > -INFINITY ? make_float4(m, se, ss, 0.f) : make_float4(-INFINITY, 0.f, 0.f, 0.f);
}

// the row statistics from the chunk partials, combined in chunk order: (max, sum exp(x - max), sum exp(x / T - max / T))
__device__ __forceinline__ void sample_row_stats(const float4* __restrict__ pp, float temperature, float& m, float& se, float& ss) {
  m = -INFINITY;
  for (int q = 0; q < S_NCH; ++q) m = fmaxf(m, pp[q].x);
  const float ms = m / temperature;
  se = 0.f; ss = 0.f;
  for (int q = 0; q < S_NCH; ++q) {
    if (!(pp[q].x > -INFINITY)) continue;
    se += pp[q].y * expf(pp[q].x - m);
    ss += pp[q].z * expf(pp[q].x / temperature - ms);
  }
}

// p[b][v] = exp(x / T - max / T) / sum: grid (S_NCH, B); rows of the scratch are Vp = V rounded up to 4 floats apart, the padding holds 0
__global__ __launch_bounds__(S_NT) void sample_probs_f32_kernel(const float* __restrict__ logits, int V, int Vp, float temperature,
                                                                const float4* __restrict__ part, float* __restrict__ pbuf) {
  const int c = blockIdx.x, b = blockIdx.y;
  float m, se, ss;
  sample_row_stats(part + (size_t)b * S_NCH, temperature, m, se, ss);
  const float ms = m / temperature;
  const int chunk = (V + S_NCH - 1) / S_NCH;
  const int lo = c * chunk, hi = (lo + chunk) < V ? (lo + chunk) : V;
  const float* x = logits + (size_t)b * V;
  float* p = pbuf + (size_t)b * Vp;
  for (int v = lo + threadIdx.x; v < hi; v += S_NT) p[v] = expf(x[v] / temperature - ms) / ss;
  if (c == S_NCH - 1 && threadIdx.x < Vp - V) p[V + threadIdx.x] = 0.f;
}

// inclusive scan over the workgroup, in thread order, of a 64-bit mass and a count; tot_*: the workgroup's totals
__device__ __forceinline__ void sel_scan(unsigned long long& a, unsigned& c, unsigned long long* red_a, unsigned* red_c, unsigned long long& tot_a,
                                         unsigned& tot_c) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long oa = __shfl_up(a, o, 64);
    const unsigned oc = __shfl_up(c, o, 64);
    if (lane >= o) { a += oa; c += oc; }
  }
  __syncthreads();            // (the words below may still be read from the previous scan)
  if (lane == 63) { red_a[w] = a; red_c[w] = c; }
  __syncthreads();
  unsigned long long pa = 0, ta = 0;
  unsigned pc = 0, tc = 0;
#pragma unroll
  for (int i = 0; i < SEL_NW; ++i) {
    const unsigned long long ra = red_a[i];
    const unsigned rc = red_c[i];
    if (i < w) { pa += ra; pc += rc; }
    ta += ra; tc += rc;
  }
  a += pa; c += pc; tot_a = ta; tot_c = tc;
}

struct SelShared {
  unsigned long long hist[HIST_N];
  unsigned long long red_a[SEL_NW];
  unsigned red_c[SEL_NW];
  unsigned long long below, total;
  unsigned bucket;
  int found, token, last;
};

// One pass of the radix select: the fixed-point mass of every probability whose pattern agrees with `prefix` above bit `shift + bits`,
// by its `bits` bits from `shift` up; then the bucket in which the ascending cumulative mass reaches `need` (> 0).  Returns whether one
// does (only the first pass can fail: the row's whole mass is below `need`); sh.bucket / sh.below (mass of the buckets in front of it) /
// sh.total (mass of all buckets) hold the result.  The truncation of fx loses less than one unit per token: a first pass whose total falls
// short of `need` by no more than that (a nucleus_p below about 2^-26) lowers `need` to the total -- the threshold is reached by the last
// token of the ascending order, as in the exact sum -- instead of reporting that nothing reaches it.
__device__ __forceinline__ bool radix_pass(SelShared& sh, const float4* __restrict__ p4, int n4, int shift, int bits, bool first, unsigned prefix,
                                           unsigned long long& need) {
  const int tid = threadIdx.x, nb = 1 << bits;
  for (int i = tid; i < nb; i += SEL_NT) sh.hist[i] = 0;
  if (tid == 0) sh.found = 0;
  __syncthreads();
  for (int i = tid; i < n4; i += SEL_NT) {
    const float4 v = p4[i];
    const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned key = __float_as_uint(e[j]);
      const unsigned long long q = fx(e[j]);
      if (q != 0 && (first || (key >> (shift + bits)) == prefix)) atomicAdd(&sh.hist[(key >> shift) & (unsigned)(nb - 1)], q);
    }
  }
  __syncthreads();
  const int per = nb >= SEL_NT ? nb / SEL_NT : 1;      // consecutive buckets per thread
  unsigned long long loc = 0;
  if (tid * per < nb)
    for (int j = 0; j < per; ++j) loc += sh.hist[tid * per + j];
  unsigned long long inc = loc, tot;
  unsigned cdummy = 0, ctot;
  sel_scan(inc, cdummy, sh.red_a, sh.red_c, tot, ctot);
  if (first && need > tot && need - tot <= 4ull * (unsigned long long)n4) need = tot;   // (uniform: tot is the workgroup's total)
  unsigned long long run = inc - loc;                  // mass in front of this thread's buckets
  if (run < need && need <= inc) {                     // (one thread at most: the cumulative mass never decreases)
    for (int j = 0; j < per; ++j) {
      const unsigned long long h = sh.hist[tid * per + j];
      if (need <= run + h) { sh.bucket = (unsigned)(tid * per + j); sh.below = run; sh.found = 1; break; }
      run += h;
    }
  }
  if (tid == 0) sh.total = tot;
  __syncthreads();
  const bool found = sh.found != 0;
  __syncthreads();                                     // (the next pass clears the word)
  return found;
}

// one workgroup per row: nucleus threshold by radix select over the probabilities' bit patterns, then the inverse CDF in vocabulary order
__global__ __launch_bounds__(SEL_NT) void sample_select_f32_kernel(const float* __restrict__ logits, int V, int Vp, float temperature, float nucleus_p,
                                                                   const float* __restrict__ uniforms, const float4* __restrict__ part,
                                                                   const float* __restrict__ pbuf, float* __restrict__ probs_out,
                                                                   int32_t* __restrict__ next_tok, int32_t* __restrict__ tokens_out, int max_steps,
                                                                   float* __restrict__ logprob, const int32_t* __restrict__ step_dev, int B,
                                                                   PcyStop stop) {
  __shared__ SelShared sh;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int step = *step_dev;
  if (step < 0 || step >= max_steps) return;             // outside tokens_out and the variates: nothing is written
  // EOS stop (pcy.h; workgroup-uniform, both words are written behind this point of the step only): nothing once *done is set; a finished
  // row emits eos_id, keeps its logprob and takes no pass over its probabilities unless they are recorded (probs_out) -- its variate
  // uniforms[step * B + b] is simply not read, the other rows' indices do not move
  bool was_finished = false;
  if (stop.finished) {
    if (*stop.done) return;
    was_finished = stop.finished[b] != 0;
    if (was_finished && !probs_out) {
      if (tid == 0) { next_tok[b] = stop.eos_id; tokens_out[(size_t)b * max_steps + step] = stop.eos_id; }
      return;
    }
  }
  const float4* p4 = reinterpret_cast<const float4*>(pbuf + (size_t)b * Vp);
  const int n4 = Vp / 4;
  // ---- what is kept: patterns above kstar, and of the tokens with pattern kstar (probability qstar in fixed point) the nstar-th in token
  // order and every later one.  Without a nucleus mask (or when nothing reaches the threshold): kstar = 0, qstar = 0 -- every positive
  // probability lies above, and a zero adds nothing.
  unsigned kstar = 0;
  unsigned long long qstar = 0, nstar = 1, total = 0;
  bool all = true;
  if (nucleus_p > 0.f) {
    double r = (1.0 - (double)nucleus_p) * 17592186044416.0;
    unsigned long long need = r < 1.0 ? 1ull : (unsigned long long)r;
    if (radix_pass(sh, p4, n4, 32 - RADIX_A, RADIX_A, true, 0u, need)) {
      all = false;
      total = sh.total;
      unsigned long long below = sh.below;
      unsigned prefix = sh.bucket;
      need -= sh.below;
      radix_pass(sh, p4, n4, RADIX_C, RADIX_B, false, prefix, need);
      prefix = (prefix << RADIX_B) | sh.bucket;
      below += sh.below; need -= sh.below;
      radix_pass(sh, p4, n4, 0, RADIX_C, false, prefix, need);
      kstar = (prefix << RADIX_C) | sh.bucket;
      below += sh.below; need -= sh.below;
      qstar = fx(__uint_as_float(kstar));                  // (> 0: its bucket holds at least `need` > 0 of mass)
      nstar = qstar ? (need + qstar - 1) / qstar : 1;
      total = total - below - (nstar - 1) * qstar;         // the kept mass
    } else {
      total = sh.total;
    }
  }
  if (all && !(nucleus_p > 0.f)) {                         // the row's mass (the first radix pass has it otherwise)
    unsigned long long loc = 0;
    for (int i = tid; i < n4; i += SEL_NT) {
      const float4 v = p4[i];
      loc += fx(v.x) + fx(v.y) + fx(v.z) + fx(v.w);
    }
    unsigned cdummy = 0, ctot;
    sel_scan(loc, cdummy, sh.red_a, sh.red_c, total, ctot);
  }
  // ---- inverse CDF in vocabulary order: cdf_i = (mass above kstar up to i) + qstar * (kept ties up to i); first i with cdf_i > u * total
  const double tg = (double)uniforms[(size_t)step * B + b] * (double)total;
  const unsigned long long target = tg > 0.0 ? (unsigned long long)tg : 0ull;
  if (tid == 0) { sh.found = 0; sh.token = 0; sh.last = -1; }
  __syncthreads();
  unsigned long long base_a = 0;
  unsigned base_c = 0;
  int last = -1;
  float* po = probs_out ? probs_out + (size_t)b * V : nullptr;
  for (int i0 = 0; i0 < n4; i0 += SEL_NT) {
    const int i = i0 + tid;
    float e[4] = {0.f, 0.f, 0.f, 0.f};
    if (i < n4) { const float4 v = p4[i]; e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w; }
    unsigned long long qa[4], la = 0;
    unsigned tie[4], lc = 0;
    bool above[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned key = __float_as_uint(e[j]);
      above[j] = key > kstar;
      qa[j] = above[j] ? fx(e[j]) : 0ull;
      tie[j] = (key == kstar && qstar != 0) ? 1u : 0u;
      la += qa[j]; lc += tie[j];
    }
    unsigned long long ia = la, ta;
    unsigned ic = lc, tc;
    sel_scan(ia, ic, sh.red_a, sh.red_c, ta, tc);
    unsigned long long ra = base_a + ia - la;            // mass above kstar in front of this thread's elements
    unsigned long long rc = (unsigned long long)base_c + ic - lc;   // ties in front of them
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned long long before = ra + (rc >= nstar ? (rc - nstar + 1) * qstar : 0ull);
      ra += qa[j]; rc += tie[j];
      const unsigned long long after = ra + (rc >= nstar ? (rc - nstar + 1) * qstar : 0ull);
      const bool kept = above[j] || (tie[j] && rc >= nstar);
      const int v = i * 4 + j;
      if (kept) last = v;
      if (before <= target && target < after) { sh.token = v; sh.found = 1; }
      if (po && v < V) po[v] = kept ? e[j] : 0.f;
    }
    base_a += ta; base_c += tc;
    __syncthreads();
    if (sh.found && !po) break;                            // (uniform: read behind the barrier)
  }
  if (!sh.found) {                                         // rounding (or a variate >= 1) pushed the draw past the end: the last kept token
    if (last >= 0) atomicMax(&sh.last, last);
    __syncthreads();
  }
  if (tid == 0 && was_finished) { next_tok[b] = stop.eos_id; tokens_out[(size_t)b * max_steps + step] = stop.eos_id; }
  if (tid == 0 && !was_finished) {
    int tok = sh.found ? sh.token : sh.last;
    tok = tok < 0 ? 0 : tok >= V ? V - 1 : tok;
    float m, se, ss;
    sample_row_stats(part + (size_t)b * S_NCH, 1.0f, m, se, ss);
    logprob[b] += (logits[(size_t)b * V + tok] - m) - logf(se);
    next_tok[b] = tok;
    tokens_out[(size_t)b * max_steps + step] = tok;
    if (stop.finished && tok == stop.eos_id) stop.finished[b] = 1;
  }
}

}  // namespace

size_t pcy_f32_kv_reorder_tmp_bytes(int L, int B, int Tmax, int t0, int kw) {
  return Tmax > t0 ? (size_t)2 * L * B * (size_t)(Tmax - t0) * kw * sizeof(float) : 0;
}
void pcy_launch_f32_kv_reorder(hipStream_t s, float* k, float* v, float* tmp, const int32_t* src_rows, int L, int B, int Bcache, int Tmax, int kw,
                               int t0, int t, const int32_t* t_dev) {
  const dim3 grid(B, 2 * L, span_blocks((size_t)((t_dev ? Tmax : t) - t0) * kw / 4));
  hipLaunchKernelGGL(kv_reorder_f32_kernel, grid, dim3(R_NT), 0, s, k, v, tmp, src_rows, B, Bcache, Tmax, kw, t0, t, t_dev, 1);
  hipLaunchKernelGGL(kv_reorder_f32_kernel, grid, dim3(R_NT), 0, s, k, v, tmp, src_rows, B, Bcache, Tmax, kw, t0, t, t_dev, 0);
}
void pcy_launch_f32_kv_copy_rows(hipStream_t s, float* dk, float* dv, int Bdst, int Tdst, const float* sk, const float* sv, int Bsrc, int Tsrc,
                                 const int32_t* src_rows, int L, int B, int kw, int t) {
  const dim3 grid(B, 2 * L, span_blocks((size_t)t * kw / 4));
  hipLaunchKernelGGL(kv_copy_rows_f32_kernel, grid, dim3(R_NT), 0, s, dk, dv, Bdst, Tdst, sk, sv, Bsrc, Tsrc, src_rows, kw, t);
}

size_t pcy_f32_sample_ws_bytes(int B, int V) {
  return ((size_t)B * S_NCH * sizeof(float4) + 255) / 256 * 256 + (size_t)B * ((V + 3) / 4 * 4) * sizeof(float) + 256;
}
void pcy_launch_f32_sample_step(hipStream_t s, const float* logits, int B, int V, float temperature, float nucleus_p, const float* uniforms,
                                float* probs_out, int32_t* next_tok, int32_t* tokens_out, int max_steps, float* logprob, const int32_t* step_dev,
                                void* ws, const PcyStop& stop) {
  const int Vp = (V + 3) / 4 * 4;
  float4* part = reinterpret_cast<float4*>(ws);
  float* pbuf = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + ((size_t)B * S_NCH * sizeof(float4) + 255) / 256 * 256);
  hipLaunchKernelGGL(sample_stats_f32_kernel, dim3(S_NCH, B), dim3(S_NT), 0, s, logits, V, temperature, part);
  hipLaunchKernelGGL(sample_probs_f32_kernel, dim3(S_NCH, B), dim3(S_NT), 0, s, logits, V, Vp, temperature, part, pbuf);
  hipLaunchKernelGGL(sample_select_f32_kernel, dim3(B), dim3(SEL_NT), 0, s, logits, V, Vp, temperature, nucleus_p, uniforms, part, pbuf, probs_out,
                     next_tok, tokens_out, max_steps, logprob, step_dev, B, stop);
}
