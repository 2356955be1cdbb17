// Run-time switches of libpcy.so, all read per call (tests flip them inside one process; a launch costs ~3.5 us, a getenv ~50 ns, and the
// replayed graphs of the decode step and of the short-input encoder read nothing at all).
//
// The decode path does not read the environment where it needs a value: every decode ABI entry takes ONE snapshot (PcySwitches, below)
// and hands it down, and a captured decode step and its hand-over slots are keyed on that snapshot BY VALUE -- two settings that resolve
// to different values never share a capture.  Defaults and clamps of the numeric switches below live in pcy_read_switches() and nowhere else.
//
//   PCY_DISABLE=a,b,...   switches OFF the named fused / alternative path (PCY_SWITCH_NAMES below is the whole list); each one has a slower
//                         twin with the same bits, and a test that compares the two  (decode_step / decode_layer also select the twins of the
//                         ProCyon-Split step, pcy_decode_mha.hip)
//                         (decode_nb: batches of 2..8 rows back on the round-4 launches -- another arithmetic, compared to bf16 noise)
//   PCY_NB_MAX=<rows>     largest batch on the small-batch decode step (default 6; 7, 8: tests, tools)
//   PCY_MB_MAX=<rows>     largest batch on the opt-in mid-batch decode step, 9..32 (default 0: off);  PCY_MB_ABL=<mask>  its timing ablations (tools)
//   PCY_ESM_ATTN=exact    the two-pass attention with the reference's bf16 rounding points (default: the single-pass kernel)
//   PCY_GEMM_PERM=<mask>  256 x 256 epilogues on the permuted W row order (1 STORE, 2 RESID, 4 ESM GELU, 8 SwiGLU, 16 fp8; default 7)
//   PCY_GEMM_MID=<cfg>    force a gemm_kernel_mid configuration (-1: the pre-round-4 kernels; "NxK=cfg,...": per shape)
//   PCY_AO_XMIN=<keys>    cache length from which the decode attention splits its keys across the slice workgroups (default 768 for one
//                         row, 1536 for 2 rows, 4096 for 3..8 rows; 0 = never)
//   PCY_NB_UB=1|2         k-iterations per weight batch of the small-batch decode step's MLP streams (measurement; default 2)
//   PCY_DEBUG_POISON_WS=1 fill the workspace with NaN patterns before every call;  PCY_MC_TRACE=1  in-kernel time stamps (tools)
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#define PCY_SWITCH_NAMES(X)                                                                                                                \
  X(attn_o) X(mlp_chain) X(decode_layer) X(decode_step) X(attn_qkv_finish) X(finish_norm) X(fp8_fused_norm) X(prefill_post_qkv) X(gemv_lds) \
  X(gemv_mfma4) X(fa_vrow) X(gelu_fast) X(esm_graph) X(lds_prefetch) X(decode_nb) X(decode_nb_step) X(beam_graph) X(kv_permute)             \
  X(decode_mb_step) X(beam_prefill_once) X(beam_kv_suffix) X(beam_kv_shared)
enum PcySwitch {
#define X(n) PCY_SW_##n,
  PCY_SWITCH_NAMES(X)
#undef X
  PCY_SW_COUNT
};
static_assert(PCY_SW_COUNT <= 32, "PcySwitches::off_mask holds one bit per name");

// whole-name match in a comma-separated list; pcy_off: in PCY_DISABLE (names outside the table are ignored)
inline bool pcy_list_has(const char* list, const char* name) {
  if (!list) return false;
  const size_t n = strlen(name);
  for (const char* p = list; (p = strstr(p, name)) != nullptr; p += n)
    if ((p == list || p[-1] == ',') && (p[n] == 0 || p[n] == ',')) return true;
  return false;
}
inline bool pcy_off(const char* name) { return pcy_list_has(getenv("PCY_DISABLE"), name); }

// What the decode path sees of the environment, taken once per ABI call.  Plain values, no padding: compared with == (memcmp).
struct PcySwitches {
  uint32_t off_mask;         // bit PCY_SW_<name>: the name stands in PCY_DISABLE
  int32_t nb_max, mb_max;    // PCY_NB_MAX (0..8), PCY_MB_MAX (0..32)
  int32_t xmin[3];           // PCY_AO_XMIN as it applies to a step of one row / 2 rows / 3 and more rows
  int32_t nb_ub;             // PCY_NB_UB: 1 or 2
  int32_t mb_abl;            // PCY_MB_ABL
  int32_t mc_trace;          // PCY_MC_TRACE is set
  bool off(PcySwitch s) const { return (off_mask >> s) & 1u; }
  int ao_xmin(int rows) const { return xmin[rows <= 1 ? 0 : rows == 2 ? 1 : 2]; }
  bool operator==(const PcySwitches& o) const { return memcmp(this, &o, sizeof(*this)) == 0; }
  bool operator!=(const PcySwitches& o) const { return !(*this == o); }
};

static_assert(std::has_unique_object_representations<PcySwitches>::value, "no padding: equal values <=> equal bytes");

inline PcySwitches pcy_read_switches() {
  static const char* const names[PCY_SW_COUNT] = {
#define X(n) #n,
      PCY_SWITCH_NAMES(X)
#undef X
  };
  auto num = [](const char* var, int unset) { const char* e = getenv(var); return e ? atoi(e) : unset; };
  auto clamp = [](int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; };
  PcySwitches s{};
  const char* off = getenv("PCY_DISABLE");
  for (int i = 0; i < PCY_SW_COUNT; ++i) s.off_mask |= pcy_list_has(off, names[i]) ? 1u << i : 0u;
  s.nb_max = clamp(num("PCY_NB_MAX", 6), 8);
  s.mb_max = clamp(num("PCY_MB_MAX", 0), 32);
  s.xmin[0] = num("PCY_AO_XMIN", 768);
  s.xmin[1] = num("PCY_AO_XMIN", 1536);
  s.xmin[2] = num("PCY_AO_XMIN", 4096);
  s.nb_ub = num("PCY_NB_UB", 2) == 1 ? 1 : 2;
  s.mb_abl = num("PCY_MB_ABL", 0);
  s.mc_trace = getenv("PCY_MC_TRACE") ? 1 : 0;
  return s;
}
