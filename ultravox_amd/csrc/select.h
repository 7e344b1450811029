// What the token selectors of select.hip and select_banned.hip share: the argmax chooser, the loop's per-token bookkeeping, the argument checks
// and the bookkeeping tail of their entry points.  Everything lies in an anonymous namespace: each translation unit has its own copy.
#pragma once
#include <type_traits>
#include "penalty.h"
#include "sample.h"

namespace {
using namespace uvx;
using namespace uvx::sampler;

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

}  // namespace

// the bookkeeping tail of the select entry points (include/uvx.h), and the Book made of it
#define UVX_BOOK_PARAMS                                                                                                                       \
  const int64_t *eos_ids, int32_t n_eos, int64_t pad, int32_t *unfinished, int64_t *next_tokens, int64_t *sequences, int64_t stride, int64_t col, \
      const int32_t *positions0, int32_t *positions, int32_t step, int32_t *counter
#define UVX_BOOK \
  Book { eos_ids, n_eos, pad, unfinished, next_tokens, sequences, (long long)stride, (long long)col, positions0, positions, step, counter }
