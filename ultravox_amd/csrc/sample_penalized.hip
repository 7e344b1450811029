// Sampled decoding under a repetition penalty in one launch per token: uvx_sample_select_penalized.
//
// Reference: the reference's pipeline calls generate(do_sample = True, temperature = t, repetition_penalty = 1.1) when it is given a temperature
// (ultravox_pipeline.py:97-121), i.e. [3P] GenerationMixin._sample with a RepetitionPenaltyLogitsProcessor in front of the warpers: processors
// before warpers, so the penalty acts on the raw f32 logit and the temperature on the penalised score.  The sampler's body is sample.h's, its row
// reader penalty.h's over the `seen` bitmap of uvx_seen_mark; the token written then joins the bitmap as in greedy_select_penalized_k
// (penalized_select.hip).  One block of 1024 threads per row, no scratch buffer, no second launch.
#include "penalty.h"
#include "sample.h"

namespace {
using namespace uvx;
using namespace uvx::sampler;

template <typename T>
__global__ void __launch_bounds__(NT) sample_select_penalized_k(const T* __restrict__ logits, int V, float penalty, uint32_t* seen_all, int words, SampleArgs a,
                                                                const int64_t* __restrict__ eos_ids, int n_eos, int64_t pad, int32_t* __restrict__ unfinished,
                                                                int64_t* __restrict__ next_tokens, int64_t* __restrict__ sequences, long long stride,
                                                                long long col, const int32_t* __restrict__ pos0, int32_t* __restrict__ pos, int step,
                                                                int32_t* __restrict__ counter) {
  __shared__ Lds s;
  const int b = blockIdx.x;
  uint32_t* seen = seen_all + (long long)b * words;
  const int token = sample_row(PenalizedRow<T>{logits + (long long)b * V, seen, penalty}, V, a, b, s);
  __syncthreads();                                // every thread's bitmap reads - the probs_out pass and the draw's tail included - lie before this barrier
  if (threadIdx.x != 0) return;
  const int64_t tok = select_bookkeeping(b, token, eos_ids, n_eos, pad, unfinished, next_tokens, sequences, stride, col, pos0, pos, step, counter);
  // the token WRITTEN joins the row (HF's input_ids hold the pads of a finished row too); a pad outside the vocabulary (-1) has no bit.
  // Only this block touches the row's words, and all its reads are done: a plain read-modify-write.
  if (tok >= 0 && tok < V) seen[tok >> 5] |= 1u << (tok & 31);
}

}  // namespace

extern "C" int32_t uvx_sample_select_penalized(void* stream, int32_t logits_dtype, const void* logits, int32_t B, int32_t V, float penalty, uint32_t* seen,
                                               int32_t words, float temperature, int32_t top_k, float top_p, float min_p, int32_t min_keep, uint64_t seed,
                                               uint64_t offset, const float* uniforms, float* probs_out, const int64_t* eos_ids, int32_t n_eos, int64_t pad,
                                               int32_t* unfinished, int64_t* next_tokens, int64_t* sequences, int64_t stride, int64_t col,
                                               const int32_t* positions0, int32_t* positions, int32_t step, int32_t* counter) {
  // (null pointers first: a caller that passes zero words everywhere leaves the float arguments' registers undefined)
  UVX_CHECK(logits && seen && unfinished && next_tokens && sequences && counter && (n_eos == 0 || eos_ids) && (!positions || positions0), UVX_ERR_INVALID,
            "sample_select_penalized: null argument");
  UVX_CHECK(logits_dtype == DT_BF16 || logits_dtype == DT_F32, UVX_ERR_INVALID, "sample_select_penalized: logits_dtype=%d", logits_dtype);
  UVX_CHECK(B >= 0 && V > 0 && V < (1 << 23) && words >= (V + 31) / 32 && n_eos >= 0 && step >= 0 && col >= 0 && col < stride, UVX_ERR_SHAPE,
            "sample_select_penalized: B=%d V=%d words=%d col=%lld stride=%lld", B, V, words, (long long)col, (long long)stride);
  UVX_CHECK(penalty > 0.f && penalty <= 3.4028234663852886e38f, UVX_ERR_INVALID, "sample_select_penalized: penalty=%g has to be positive and finite",
            (double)penalty);
  UVX_CHECK(temperature > 0.f && top_k >= 0 && top_p > 0.f && top_p <= 1.f && min_p >= 0.f && min_p <= 1.f && min_keep >= 1, UVX_ERR_INVALID,
            "sample_select_penalized: temperature=%g top_k=%d top_p=%g min_p=%g min_keep=%d", (double)temperature, top_k, (double)top_p, (double)min_p,
            min_keep);
  if (B == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
  const SampleArgs a{temperature, top_p, min_p, top_k, min_keep, seed, offset, uniforms, probs_out};
  if (logits_dtype == DT_BF16)
    hipLaunchKernelGGL(sample_select_penalized_k<bf16_t>, dim3(B), dim3(NT), 0, st, (const bf16_t*)logits, V, penalty, seen, words, a, eos_ids, n_eos, pad,
                       unfinished, next_tokens, sequences, (long long)stride, (long long)col, positions0, positions, step, counter);
  else
    hipLaunchKernelGGL(sample_select_penalized_k<float>, dim3(B), dim3(NT), 0, st, (const float*)logits, V, penalty, seen, words, a, eos_ids, n_eos, pad,
                       unfinished, next_tokens, sequences, (long long)stride, (long long)col, positions0, positions, step, counter);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}
