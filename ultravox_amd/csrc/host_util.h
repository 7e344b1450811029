// Host-side helpers of the orchestration files (model.hip, llm_stack.hip, generate.hip, wav2vec2.hip, enc_stack.hip): workspace carving, element
// addressing, error propagation, the configuration check, the plain linear's GEMM descriptor.
#pragma once
#include "common.h"
#include "kernels.h"
#include "tuning.h"

namespace uvx {

// Bump allocator over the caller's workspace (256-byte aligned slices).  base == NULL: a dry run that only measures.
struct Arena {
  char* base;
  size_t cap;
  size_t off = 0;
  Arena(void* b, size_t c) : base((char*)b), cap(c) {}
  void* take(size_t bytes) {
    const size_t a = (off + 255) & ~(size_t)255;
    off = a + bytes;
    return base ? (void*)(base + a) : nullptr;
  }
  bool fits() const { return !base || off <= cap; }
};

inline size_t esz(int dtype) { return dtype == DT_BF16 ? 2 : 4; }
inline int rup(int x, int m) { return (x + m - 1) / m * m; }
inline char* at(const void* p, size_t elems, int dtype) { return (char*)p + elems * esz(dtype); }

#define RC(expr)            \
  do {                      \
    int _rc = (expr);       \
    if (_rc) return _rc;    \
  } while (0)

inline int check_cfg(const uvx_config_t* c) {
  UVX_CHECK(c != nullptr, UVX_ERR_INVALID, "null config");
  UVX_CHECK(c->dtype == DT_BF16 || c->dtype == DT_F32, UVX_ERR_INVALID, "bad dtype %d", c->dtype);
  UVX_CHECK(c->llm_flavor >= UVX_LLM_LLAMA && c->llm_flavor <= UVX_LLM_GEMMA3, UVX_ERR_INVALID, "bad llm_flavor %d", c->llm_flavor);
  UVX_CHECK(c->llm_act >= UVX_ACT_SILU && c->llm_act <= UVX_ACT_GELU_ERF && (c->llm_flavor != UVX_LLM_LLAMA) == (c->llm_act != UVX_ACT_SILU),
            UVX_ERR_INVALID, "llm_act %d does not fit llm_flavor %d (Llama: SiLU; Gemma: tanh- or erf-GELU)", c->llm_act, c->llm_flavor);
  UVX_CHECK(c->llm_wt_stream == 0 || c->llm_wt_stream == 1, UVX_ERR_INVALID, "llm_wt_stream %d: 0 or 1", c->llm_wt_stream);
  UVX_CHECK(c->llm_qk_norm == 0 || (c->llm_qk_norm == 1 && c->llm_flavor != UVX_LLM_GEMMA), UVX_ERR_INVALID,
            "llm_qk_norm %d: 0 or 1 (Qwen3: Llama-flavoured; Gemma-3: Gemma-flavoured)", c->llm_qk_norm);
  UVX_CHECK((c->llm_flavor == UVX_LLM_GEMMA3) == (c->llm_qk_norm == 1 && c->llm_flavor == UVX_LLM_GEMMA3) && c->llm_attn_scale >= 0.f &&
            c->llm_window >= 0, UVX_ERR_INVALID, "Gemma-3 needs llm_qk_norm = 1; llm_attn_scale / llm_window must not be negative");
  return UVX_OK;
}

// y [M, N] = x [M, K] . W [N, K]^T
inline GemmDesc lin(const void* A, const void* W, void* C, int M, int N, int K) {
  GemmDesc g;
  g.A = A; g.B = W; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N;
  return g;
}

// Timing probe (tuning option 15, default 0): bit mask of kernel classes NOT launched - the step's results are then garbage, its
// time says what that class costs inside the overlapped schedule (bench.py --opt 15=<mask>; never set by the product).
// 1 LLM attention backward, 2 LLM attention forward, 4 SwiGLU backward, 8 RMSNorm backward, 16 RMSNorm forward, 32 RoPE forward,
// 64 attention forward of either audio tower's layer stack, 128 every LayerNorm forward inside that stack (enc_stack.hip: the layers' norms in
// the forward walks and their recomputes in the backward; not the towers' final LayerNorm)
inline bool probe_skip(int bit) { return (opt(UVX_OPT_PROBE_SKIP_MASK) & bit) != 0; }

}  // namespace uvx
