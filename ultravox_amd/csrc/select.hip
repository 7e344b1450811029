// Token selection for generate() in one launch per token: uvx_argmax, uvx_greedy_select, uvx_seen_mark + uvx_greedy_select_penalized,
// uvx_sample_select, uvx_sample_select_penalized.
//
// Reference: [3P] GenerationMixin._sample as the reference's inference path reaches it (ultravox_model.py:422-426 -> language_model.generate;
// the pipeline calls it with repetition_penalty = 1.1 and, given a temperature, do_sample = True: ultravox_pipeline.py:97-121).  Processors
// come before warpers, so the penalty acts on the raw f32 logit and the temperature on the penalised score.
//
// The four selectors are the corners of a 2 x 2 table, and select_k is that table:
//   reader   how a row is read     PlainRow (sample.h): as it lies      PenalizedRow (penalty.h): through the penalty over the `seen` bitmap
//   chooser  how the token is got  argmax_row (below)                   sample_row (sample.h): warpers and the draw
// followed by the loop's bookkeeping (select_bookkeeping), which exists once.  One block of 1024 threads per row, no second launch.
#include <type_traits>
#include "penalty.h"
#include "sample.h"

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

// (value, index) pairs: the larger value wins, the lower index among equal values
__device__ __forceinline__ void take(float& best, int& idx, float o, int oi) {
  if (o > best || (o == best && oi < idx)) { best = o; idx = oi; }
}

// argmax of one row by the whole block (NT threads), valid in thread 0; scores_out (or null) receives the row's scores as read.
// Every thread's reads of the row lie before the function's one barrier.
template <typename R>
__device__ __forceinline__ int argmax_row(const R& rd, int V, float* __restrict__ scores_out) {
  __shared__ float bv[NW];
  __shared__ int bi[NW];
  float best = -__builtin_huge_valf();
  int idx = 0x7fffffff;
  // ascending index within a thread: strict > keeps the lowest index; NaN never compares greater
  walk_row(rd, V, [&](float s, int c) {
    if (scores_out) scores_out[c] = s;
    if (s > best) { best = s; idx = c; }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) take(best, idx, __shfl_xor(best, o, 64), __shfl_xor(idx, o, 64));
  if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < NW; ++i) take(best, idx, bv[i], bi[i]);
  return idx == 0x7fffffff ? 0 : idx;             // nothing above -inf: index 0, like torch.argmax
}

template <typename T>
__global__ void __launch_bounds__(NT) argmax_k(const T* __restrict__ logits, int64_t* __restrict__ out, int V) {
  const int idx = argmax_row(PlainRow<T>{logits + (long long)blockIdx.x * V}, V, nullptr);
  if (threadIdx.x == 0) out[blockIdx.x] = idx;
}

// The per-token state of a generate() loop, as every select entry point takes it (include/uvx.h, uvx_greedy_select)
struct Book {
  const int64_t* eos_ids;
  int n_eos;
  int64_t pad;
  int32_t* unfinished;
  int64_t *next_tokens, *sequences;
  long long stride, col;
  const int32_t* pos0;
  int32_t* pos;
  int step;
  int32_t* counter;
};

// The per-token bookkeeping of the loop in the same launch as the choice, instead of eight small torch kernels, by ONE thread of row b's
// block: the next token is the one chosen while the sequence is unfinished, pad_token_id afterwards; it is appended to the sequences buffer; a
// sequence is finished once it has produced an EOS id; the next decode step's RoPE position is written; the number of still unfinished rows
// goes to counter[step & 1] (block 0 zeroes the other slot for the next launch: launches of one loop are stream-ordered).  -> the token written
__device__ __forceinline__ int64_t select_bookkeeping(int b, int token, const Book& k) {
  if (b == 0) k.counter[(k.step & 1) ^ 1] = 0;
  const bool live = k.unfinished[b] != 0;
  const int64_t tok = live ? (int64_t)token : k.pad;
  k.next_tokens[b] = tok;
  k.sequences[(long long)b * k.stride + k.col] = tok;
  bool still = live;
  const int64_t* __restrict__ eos_ids = k.eos_ids;
  for (int e = 0; e < k.n_eos; ++e) still = still && tok != eos_ids[e];
  k.unfinished[b] = still ? 1 : 0;
  if (k.pos) k.pos[b] = k.pos0[b] + k.step;
  if (still) atomicAdd(&k.counter[k.step & 1], 1);
  return tok;
}

struct Penalty {
  float penalty;
  uint32_t* seen;       // [B][words]
  int words;
};
struct ArgmaxArgs { float* scores_out; };

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

// The argument checks of the four select entry points under the entry point's short name; p / a: null where it takes no penalty / does not
// sample.  uvx_greedy_select alone (neither) takes any dtype code as f32 and any V.
int check_select(const char* name, int dtype, const void* logits, int B, int V, const Penalty* p, const SampleArgs* a, const Book& k) {
  // (null pointers first: a caller that passes zero words everywhere leaves the float arguments' registers undefined)
  UVX_CHECK(logits && (!p || p->seen) && k.unfinished && k.next_tokens && k.sequences && k.counter && (k.n_eos == 0 || k.eos_ids) && (!k.pos || k.pos0),
            UVX_ERR_INVALID, "%s: null argument", name);
  const bool plain_greedy = !p && !a;
  UVX_CHECK(plain_greedy || dtype == DT_BF16 || dtype == DT_F32, UVX_ERR_INVALID, "%s: logits_dtype=%d", name, dtype);
  const bool shape = B >= 0 && V > 0 && (plain_greedy || V < (1 << 23)) && k.n_eos >= 0 && k.step >= 0 && k.col >= 0 && k.col < k.stride;
  if (p) {
    UVX_CHECK(shape && p->words >= (V + 31) / 32, UVX_ERR_SHAPE, "%s: B=%d V=%d words=%d col=%lld stride=%lld", name, B, V, p->words, k.col, k.stride);
    UVX_CHECK(p->penalty > 0.f && p->penalty <= 3.4028234663852886e38f, UVX_ERR_INVALID, "%s: penalty=%g has to be positive and finite", name,
              (double)p->penalty);
  } else {
    UVX_CHECK(shape, UVX_ERR_SHAPE, "%s: B=%d V=%d col=%lld stride=%lld", name, B, V, k.col, k.stride);
  }
  if (a)
    UVX_CHECK(a->temperature > 0.f && a->top_k >= 0 && a->top_p > 0.f && a->top_p <= 1.f && a->min_p >= 0.f && a->min_p <= 1.f && a->min_keep >= 1,
              UVX_ERR_INVALID, "%s: temperature=%g top_k=%d top_p=%g min_p=%g min_keep=%d", name, (double)a->temperature, a->top_k, (double)a->top_p,
              (double)a->min_p, a->min_keep);
  return UVX_OK;
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

// the bookkeeping tail of the four select entry points (include/uvx.h), and the Book made of it
#define UVX_BOOK_PARAMS                                                                                                                       \
  const int64_t *eos_ids, int32_t n_eos, int64_t pad, int32_t *unfinished, int64_t *next_tokens, int64_t *sequences, int64_t stride, int64_t col, \
      const int32_t *positions0, int32_t *positions, int32_t step, int32_t *counter
#define UVX_BOOK \
  Book { eos_ids, n_eos, pad, unfinished, next_tokens, sequences, (long long)stride, (long long)col, positions0, positions, step, counter }

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
