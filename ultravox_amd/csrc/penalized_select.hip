// Greedy decoding under a repetition penalty in one launch per token: uvx_seen_mark + uvx_greedy_select_penalized.
//
// Reference: the reference's pipeline calls generate(do_sample = False, repetition_penalty = 1.1) (ultravox_pipeline.py:100-119), i.e.
// [3P] GenerationMixin._sample with a RepetitionPenaltyLogitsProcessor in front of the argmax.  "Has this id occurred in the row" is one bit per
// vocabulary entry (penalty.h): uvx_seen_mark sets the bits of the prompt once, the select kernel reads them next to the logits row and sets
// the bit of the token it appends.  One block of 1024 threads per row; the bookkeeping is greedy_select_k's (generate.hip).
#include "common.h"
#include "kernels.h"
#include "penalty.h"

namespace {
using namespace uvx;

constexpr int NT = 1024, NW = NT / 64;

__global__ void seen_mark_k(const int64_t* __restrict__ ids, long long stride, int B, int n, int V, uint32_t* __restrict__ seen, int words) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * n) return;
  const long long b = i / n, j = i % n;
  const int64_t id = ids[b * stride + j];
  if (id < 0 || id >= V) return;                  // outside the vocabulary: no bit, nothing dereferenced
  atomicOr(&seen[b * words + (id >> 5)], 1u << (id & 31));
}

// (value, index) pairs: the larger value wins, the lower index among equal values
__device__ __forceinline__ void take(float& best, int& idx, float o, int oi) {
  if (o > best || (o == best && oi < idx)) { best = o; idx = oi; }
}

template <typename T>
__global__ void __launch_bounds__(NT) greedy_select_penalized_k(const T* __restrict__ logits, int V, float penalty, uint32_t* seen_all, int words,
                                                                float* __restrict__ scores_out, const int64_t* __restrict__ eos_ids, int n_eos,
                                                                int64_t pad, int32_t* __restrict__ unfinished, int64_t* __restrict__ next_tokens,
                                                                int64_t* __restrict__ sequences, long long stride, long long col,
                                                                const int32_t* __restrict__ pos0, int32_t* __restrict__ pos, int step,
                                                                int32_t* __restrict__ counter) {
  __shared__ float bv[NW];
  __shared__ int bi[NW];
  const int b = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t* seen = seen_all + (long long)b * words;
  float* so = scores_out ? scores_out + (long long)b * V : nullptr;
  float best = -__builtin_huge_valf();
  int idx = 0x7fffffff;
  // ascending index within a thread: strict > keeps the lowest index; NaN never compares greater
  for_row_penalized<T>(logits + (long long)b * V, V, seen, penalty, [&](float s, int c) {
    if (so) so[c] = s;
    if (s > best) { best = s; idx = c; }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) take(best, idx, __shfl_xor(best, o, 64), __shfl_xor(idx, o, 64));
  if (lane == 0) { bv[wv] = best; bi[wv] = idx; }
  __syncthreads();                                // every thread's bitmap reads lie before this barrier
  if (threadIdx.x != 0) return;
  for (int i = 1; i < NW; ++i) take(best, idx, bv[i], bi[i]);
  const int token = idx == 0x7fffffff ? 0 : idx;  // nothing above -inf: index 0, like uvx_argmax
  // ---- the bookkeeping of greedy_select_k (generate.hip), verbatim ----
  if (b == 0) counter[(step & 1) ^ 1] = 0;
  const bool live = unfinished[b] != 0;
  const int64_t tok = live ? (int64_t)token : pad;
  next_tokens[b] = tok;
  sequences[(long long)b * stride + col] = tok;
  bool still = live;
  for (int e = 0; e < n_eos; ++e) still = still && tok != eos_ids[e];
  unfinished[b] = still ? 1 : 0;
  if (pos) pos[b] = pos0[b] + step;
  if (still) atomicAdd(&counter[step & 1], 1);
  // the token WRITTEN joins the row (HF's input_ids hold the pads of a finished row too); a pad outside the vocabulary (-1) has no bit.
  // Only this block touches the row's words, and all its reads are done: a plain read-modify-write.
  if (tok >= 0 && tok < V) seen[tok >> 5] |= 1u << (tok & 31);
}

}  // namespace

extern "C" int32_t uvx_seen_mark(void* stream, const int64_t* ids, int64_t stride, int32_t B, int32_t n, int32_t V, uint32_t* seen, int32_t words) {
  UVX_CHECK(seen && (ids || B == 0 || n == 0), UVX_ERR_INVALID, "seen_mark: null argument");
  UVX_CHECK(B >= 0 && n >= 0 && V > 0 && V < (1 << 23) && words >= (V + 31) / 32 && stride >= 0, UVX_ERR_SHAPE,
            "seen_mark: B=%d n=%d V=%d words=%d stride=%lld", B, n, V, words, (long long)stride);
  if (B == 0 || n == 0) return UVX_OK;
  hipLaunchKernelGGL(seen_mark_k, dim3(cdiv((long long)B * n, 256)), dim3(256), 0, (hipStream_t)stream, ids, (long long)stride, B, n, V, seen, words);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}

extern "C" int32_t uvx_greedy_select_penalized(void* stream, int32_t logits_dtype, const void* logits, int32_t B, int32_t V, float penalty, uint32_t* seen,
                                               int32_t words, float* scores_out, const int64_t* eos_ids, int32_t n_eos, int64_t pad,
                                               int32_t* unfinished, int64_t* next_tokens, int64_t* sequences, int64_t stride, int64_t col,
                                               const int32_t* positions0, int32_t* positions, int32_t step, int32_t* counter) {
  // (null pointers first: a caller that passes zero words everywhere leaves the float argument's register undefined)
  UVX_CHECK(logits && seen && unfinished && next_tokens && sequences && counter && (n_eos == 0 || eos_ids) && (!positions || positions0), UVX_ERR_INVALID,
            "greedy_select_penalized: null argument");
  UVX_CHECK(logits_dtype == DT_BF16 || logits_dtype == DT_F32, UVX_ERR_INVALID, "greedy_select_penalized: logits_dtype=%d", logits_dtype);
  UVX_CHECK(B >= 0 && V > 0 && V < (1 << 23) && words >= (V + 31) / 32 && col >= 0 && col < stride && n_eos >= 0 && step >= 0, UVX_ERR_SHAPE,
            "greedy_select_penalized: B=%d V=%d words=%d col=%lld stride=%lld", B, V, words, (long long)col, (long long)stride);
  UVX_CHECK(penalty > 0.f && penalty <= 3.4028234663852886e38f, UVX_ERR_INVALID, "greedy_select_penalized: penalty=%g has to be positive and finite",
            (double)penalty);
  if (B == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (logits_dtype == DT_BF16)
    hipLaunchKernelGGL(greedy_select_penalized_k<bf16_t>, dim3(B), dim3(NT), 0, st, (const bf16_t*)logits, V, penalty, seen, words, scores_out, eos_ids, n_eos,
                       pad, unfinished, next_tokens, sequences, (long long)stride, (long long)col, positions0, positions, step, counter);
  else
    hipLaunchKernelGGL(greedy_select_penalized_k<float>, dim3(B), dim3(NT), 0, st, (const float*)logits, V, penalty, seen, words, scores_out, eos_ids, n_eos,
                       pad, unfinished, next_tokens, sequences, (long long)stride, (long long)col, positions0, positions, step, counter);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}
