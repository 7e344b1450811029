// The library's process-wide tuning state, in one place: the option table of uvx_set_option (keys: uvx_option_t in include/uvx.h) and
// what the other probe setters write (uvx_gemm_force_variant, uvx_gemm_override_variant, uvx_attention_force_qt, uvx_probe_attn_timeline).
// Defined once, with its defaults, in api_core.hip next to those setters; every launcher reads it through uvx::g_tuning / uvx::opt().
// Plain ints, no lock: set before the first compute call, not concurrently with one (include/uvx.h "threading").
#pragma once
#include "../../include/uvx.h"

namespace uvx {

constexpr int kOptionSlots = 32;   // uvx_set_option accepts keys 1 .. 31; 27 .. 31 are unassigned (stored, read by nothing)
constexpr int kGemmOverrides = 32;

struct Tuning {
  int options[kOptionSlots];         // indexed by uvx_option_t; slot 0 unused
  int gemm_variant;                  // forced bf16 GEMM tile variant; -1 = automatic
  int gemm_split;                    // tail split of a partial last round of tiles (0: off, A/B probes)
  int gemm_ovr_n;                    // per-shape variant overrides {M, N, K, variant} (in-situ A/B of the tile choice inside bench.py)
  int gemm_ovr[kGemmOverrides][4];
  int attn_qt;                       // probes: force the attention forward kernel's q-tile count (0 = automatic)
  void* attn_tl;                     // probes build: stamp buffer of the fused attention backward kernel (uvx_probe_attn_timeline)
};
extern Tuning g_tuning;

inline int opt(uvx_option_t key) { return g_tuning.options[key]; }

}  // namespace uvx
