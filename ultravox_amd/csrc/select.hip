// Token selection for generate() in one launch per token: uvx_argmax, uvx_greedy_select, uvx_seen_mark + uvx_greedy_select_penalized,
// uvx_sample_select, uvx_sample_select_penalized.
//
// Reference: [3P] GenerationMixin._sample as the reference's inference path reaches it (ultravox_model.py:422-426 -> language_model.generate;
// the pipeline calls it with repetition_penalty = 1.1 and, given a temperature, do_sample = True: ultravox_pipeline.py:97-121).  Processors
// come before warpers, so the penalty acts on the raw f32 logit and the temperature on the penalised score.
//
// The four selectors are the corners of a 2 x 2 table, and select_k is that table:
//   reader   how a row is read     PlainRow (sample.h): as it lies      PenalizedRow (penalty.h): through the penalty over the `seen` bitmap
//   chooser  how the token is got  argmax_row (select.h)                 sample_row (sample.h): warpers and the draw
// followed by the loop's bookkeeping (select_bookkeeping), which exists once.  One block of 1024 threads per row, no second launch.
// The chooser, the bookkeeping and the argument checks live in select.h: select_banned.hip reads its rows through a ban bitmap (ban.h) and uses
// the same ones.
#include "select.h"

namespace {
using namespace uvx;
using namespace uvx::sampler;

__global__ void seen_mark_k(const int64_t* __restrict__ ids, long long stride, int B, int n, int V, uint32_t* __restrict__ seen, int words) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)B * n) return;
  const long long b = i / n, j = i % n;
  const int64_t id = ids[b * stride + j];
  if (id < 0 || id >= V) return;                  // outside the vocabulary: no bit, nothing dereferenced
  atomicOr(&seen[b * words + (id >> 5)], 1u << (id & 31));
}

template <typename T>
__global__ void __launch_bounds__(NT) argmax_k(const T* __restrict__ logits, int64_t* __restrict__ out, int V) {
  const int idx = argmax_row(PlainRow<T>{logits + (long long)blockIdx.x * V}, V, nullptr);
  if (threadIdx.x == 0) out[blockIdx.x] = idx;
}

// Pick = ArgmaxArgs or SampleArgs.  The greedy instantiations carry none of the sampler's LDS.
template <typename T, bool PENALIZED, typename Pick>
__global__ void __launch_bounds__(NT) select_k(const T* __restrict__ logits, int V, Penalty p, Pick pick, Book k) {
  const int b = blockIdx.x;
  const T* r = logits + (long long)b * V;
  uint32_t* seen = PENALIZED ? p.seen + (long long)b * p.words : nullptr;
  const auto rd = [&] {
    if constexpr (PENALIZED) return PenalizedRow<T>{r, seen, p.penalty};
    else return PlainRow<T>{r};
  }();
  int token;
  if constexpr (std::is_same<Pick, SampleArgs>::value) {
    __shared__ Lds s;
    token = sample_row(rd, V, pick, b, s);
    if constexpr (PENALIZED) __syncthreads();     // every thread's bitmap reads - the probs_out pass and the draw's tail included - lie before this barrier
  } else {
    float* so = nullptr;                          // (known at compile time where the entry point has none: uvx_greedy_select)
    if constexpr (PENALIZED) so = pick.scores_out ? pick.scores_out + (long long)b * V : nullptr;
    token = argmax_row(rd, V, so);                // (its own barrier does the same)
  }
  if (threadIdx.x != 0) return;
  const int64_t tok = select_bookkeeping(b, token, k);
  // the token WRITTEN joins the row (HF's input_ids hold the pads of a finished row too); a pad outside the vocabulary (-1) has no bit.
  // Only this block touches the row's words, and all its reads are done: a plain read-modify-write.
  if constexpr (PENALIZED)
    if (tok >= 0 && tok < V) seen[tok >> 5] |= 1u << (tok & 31);
}

template <bool PENALIZED, typename Pick>
int launch_select(void* stream, int dtype, const void* logits, int B, int V, const Penalty& p, const Pick& pick, const Book& k) {
  if (B == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DT_BF16) hipLaunchKernelGGL((select_k<bf16_t, PENALIZED, Pick>), dim3(B), dim3(NT), 0, st, (const bf16_t*)logits, V, p, pick, k);
  else hipLaunchKernelGGL((select_k<float, PENALIZED, Pick>), dim3(B), dim3(NT), 0, st, (const float*)logits, V, p, pick, k);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}

}  // namespace

extern "C" int32_t uvx_argmax(void* stream, int32_t dtype, const void* logits, int32_t rows, int32_t V, int64_t* out) {
  UVX_CHECK(logits && out, UVX_ERR_INVALID, "argmax: null argument");
  if (rows == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == DT_BF16) hipLaunchKernelGGL(argmax_k<bf16_t>, dim3(rows), dim3(NT), 0, st, (const bf16_t*)logits, out, V);
  else hipLaunchKernelGGL(argmax_k<float>, dim3(rows), dim3(NT), 0, st, (const float*)logits, out, V);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}

extern "C" int32_t uvx_greedy_select(void* stream, int32_t dtype, const void* logits, int32_t B, int32_t V, UVX_BOOK_PARAMS) {
  const Book k = UVX_BOOK;
  if (const int rc = check_select("greedy_select", dtype, logits, B, V, nullptr, nullptr, k)) return rc;
  return launch_select<false>(stream, dtype, logits, B, V, Penalty{}, ArgmaxArgs{nullptr}, k);
}

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
                                               int32_t words, float* scores_out, UVX_BOOK_PARAMS) {
  const Book k = UVX_BOOK;
  const Penalty p{penalty, seen, words};
  if (const int rc = check_select("greedy_select_penalized", logits_dtype, logits, B, V, &p, nullptr, k)) return rc;
  return launch_select<true>(stream, logits_dtype, logits, B, V, p, ArgmaxArgs{scores_out}, k);
}

extern "C" int32_t uvx_sample_select(void* stream, int32_t logits_dtype, const void* logits, int32_t B, int32_t V, float temperature, int32_t top_k,
                                     float top_p, float min_p, int32_t min_keep, uint64_t seed, uint64_t offset, const float* uniforms,
                                     float* probs_out, UVX_BOOK_PARAMS) {
  const Book k = UVX_BOOK;
  const SampleArgs a{temperature, top_p, min_p, top_k, min_keep, seed, offset, uniforms, probs_out};
  if (const int rc = check_select("sample_select", logits_dtype, logits, B, V, nullptr, &a, k)) return rc;
  return launch_select<false>(stream, logits_dtype, logits, B, V, Penalty{}, a, k);
}

extern "C" int32_t uvx_sample_select_penalized(void* stream, int32_t logits_dtype, const void* logits, int32_t B, int32_t V, float penalty, uint32_t* seen,
                                               int32_t words, float temperature, int32_t top_k, float top_p, float min_p, int32_t min_keep, uint64_t seed,
                                               uint64_t offset, const float* uniforms, float* probs_out, UVX_BOOK_PARAMS) {
  const Book k = UVX_BOOK;
  const Penalty p{penalty, seen, words};
  const SampleArgs a{temperature, top_p, min_p, top_k, min_keep, seed, offset, uniforms, probs_out};
  if (const int rc = check_select("sample_select_penalized", logits_dtype, logits, B, V, &p, &a, k)) return rc;
  return launch_select<true>(stream, logits_dtype, logits, B, V, p, a, k);
}

#undef UVX_BOOK_PARAMS
#undef UVX_BOOK
