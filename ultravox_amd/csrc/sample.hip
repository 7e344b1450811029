// Sampled decoding in one launch per token: uvx_sample_select, the sampling counterpart of uvx_greedy_select (generate.hip).
//
// The warpers, the draw and the bookkeeping are sample.h's, instantiated here with the reader that takes the logits row as it lies
// (sample_penalized.hip reads the same body through the repetition penalty).
#include "sample.h"

namespace {
using namespace uvx;
using namespace uvx::sampler;

template <typename T>
__global__ void __launch_bounds__(NT) sample_select_k(const T* __restrict__ logits, int V, SampleArgs a, const int64_t* __restrict__ eos_ids, int n_eos,
                                                      int64_t pad, int32_t* __restrict__ unfinished, int64_t* __restrict__ next_tokens,
                                                      int64_t* __restrict__ sequences, long long stride, long long col,
                                                      const int32_t* __restrict__ pos0, int32_t* __restrict__ pos, int step,
                                                      int32_t* __restrict__ counter) {
  __shared__ Lds s;
  const int b = blockIdx.x;
  const int token = sample_row(PlainRow<T>{logits + (long long)b * V}, V, a, b, s);
  if (threadIdx.x != 0) return;
  select_bookkeeping(b, token, eos_ids, n_eos, pad, unfinished, next_tokens, sequences, stride, col, pos0, pos, step, counter);
}

}  // namespace

extern "C" int32_t uvx_sample_select(void* stream, int32_t logits_dtype, const void* logits, int32_t B, int32_t V, float temperature, int32_t top_k,
                                     float top_p, float min_p, int32_t min_keep, uint64_t seed, uint64_t offset, const float* uniforms,
                                     float* probs_out, const int64_t* eos_ids, int32_t n_eos, int64_t pad, int32_t* unfinished,
                                     int64_t* next_tokens, int64_t* sequences, int64_t stride, int64_t col, const int32_t* positions0,
                                     int32_t* positions, int32_t step, int32_t* counter) {
  UVX_CHECK(logits && unfinished && next_tokens && sequences && counter && (n_eos == 0 || eos_ids) && (!positions || positions0), UVX_ERR_INVALID,
            "sample_select: null argument");
  UVX_CHECK(logits_dtype == DT_BF16 || logits_dtype == DT_F32, UVX_ERR_INVALID, "sample_select: logits_dtype=%d", logits_dtype);
  UVX_CHECK(B >= 0 && V > 0 && V < (1 << 23) && n_eos >= 0 && step >= 0 && col >= 0 && col < stride, UVX_ERR_SHAPE,
            "sample_select: B=%d V=%d col=%lld stride=%lld", B, V, (long long)col, (long long)stride);
  UVX_CHECK(temperature > 0.f && top_k >= 0 && top_p > 0.f && top_p <= 1.f && min_p >= 0.f && min_p <= 1.f && min_keep >= 1, UVX_ERR_INVALID,
            "sample_select: temperature=%g top_k=%d top_p=%g min_p=%g min_keep=%d", (double)temperature, top_k, (double)top_p, (double)min_p, min_keep);
  if (B == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
  const SampleArgs a{temperature, top_p, min_p, top_k, min_keep, seed, offset, uniforms, probs_out};
  if (logits_dtype == DT_BF16) hipLaunchKernelGGL(sample_select_k<bf16_t>, dim3(B), dim3(NT), 0, st, (const bf16_t*)logits, V, a, eos_ids, n_eos, pad,
                                                       unfinished, next_tokens, sequences, (long long)stride, (long long)col, positions0, positions, step, counter);
  else hipLaunchKernelGGL(sample_select_k<float>, dim3(B), dim3(NT), 0, st, (const float*)logits, V, a, eos_ids, n_eos, pad, unfinished, next_tokens,
                          sequences, (long long)stride, (long long)col, positions0, positions, step, counter);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}
