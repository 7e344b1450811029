// HF's token-ban score processors for a device-side token selector: a per-row ban bitmap that the row's block rebuilds every step (ban_build),
// and a row reader over it (BannedRow) that wraps PlainRow (sample.h) or PenalizedRow (penalty.h).  select_banned.hip uses both.
//
// Reference: [3P] NoRepeatNGramLogitsProcessor, NoBadWordsLogitsProcessor, MinLengthLogitsProcessor, MinNewTokensLengthLogitsProcessor,
// ForcedEOSTokenLogitsProcessor, SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor in the order HF's _get_logits_processor lists
// them (the reference forwards every generate keyword to HF: ultravox_model.py:422-426).  All of them set ids to -inf and the forced step sets
// the rest to 0: no arithmetic, so the scores are HF's bit for bit.
//
// Bitmap: uint32 [B][words], words >= ceil(V / 32), the layout of penalty.h's `seen`, in global memory (2^23 ids are 1 MB per row).
// Every id is compared by value wherever it stands and becomes a bit position only inside [0, V); sequence positions stay in [0, L); an entry
// of the bad-word table is read only if its offsets lie inside the token array.
#pragma once
#include "common.h"
#include "penalty.h"
#include "sample.h"

namespace uvx {

__device__ __forceinline__ void ban_set(uint32_t* ban, int V, int64_t id) {
  if (id >= 0 && id < V) atomicOr(&ban[id >> 5], 1u << (id & 31));
}

__device__ __forceinline__ bool ban_listed(const int64_t* __restrict__ ids, int n, int64_t id) {
  for (int i = 0; i < n; ++i)
    if (ids[i] == id) return true;
  return false;
}

// Row b's words of the bitmap for this step, by the row's whole block (sampler::NT threads); seq: the row's ids, L of them.  Two barriers: fill,
// mark.  Every thread's first read of the bitmap has to lie behind the call.
__device__ __forceinline__ void ban_build(uint32_t* ban, int V, const uvx_ban_rules_t& r, uint32_t flags, const int64_t* __restrict__ seq, long long L) {
  const int tid = threadIdx.x, NT = sampler::NT;
  const bool forced = flags & UVX_BAN_FORCED;
  const bool begin = (flags & UVX_BAN_BEGIN) && r.n_begin > 0;
  const int nw = (V + 31) >> 5;
  for (int w = tid; w < nw; w += NT) ban[w] = forced ? 0xffffffffu : 0u;
  __syncthreads();
  if (forced) {
    // everything but the forced ids; the suppress lists act after HF's fill, so a forced id among them stays banned (no bit is both set and cleared)
    for (int i = tid; i < r.n_forced; i += NT) {
      const int64_t id = r.forced_ids[i];
      if (id < 0 || id >= V || ban_listed(r.suppress_ids, r.n_suppress, id) || (begin && ban_listed(r.begin_ids, r.n_begin, id))) continue;
      atomicAnd(&ban[id >> 5], ~(1u << (id & 31)));
    }
  } else {
    const long long n = r.ngram;
    if (n > 0 && L >= n) {
      // window j = ids [j, j + n): its first n - 1 against the row's last n - 1 (at L - n + 1); j + n - 1 <= L - 1
      const long long tail = L - n + 1;
      for (long long j = tid; j <= L - n; j += NT) {
        bool same = true;
        for (long long i = 0; i < n - 1 && same; ++i) same = seq[j + i] == seq[tail + i];
        if (same) ban_set(ban, V, seq[j + n - 1]);
      }
    }
    for (int e = tid; e < r.n_bad; e += NT) {
      const long long o0 = r.bad_offsets[e], o1 = r.bad_offsets[e + 1], len = o1 - o0;
      if (o0 < 0 || len < 1 || o1 > r.n_bad_tokens || len > L) continue;      // malformed, or longer than the context (HF skips those)
      bool same = true;
      for (long long i = 0; i < len - 1 && same; ++i) same = seq[L - (len - 1) + i] == r.bad_tokens[o0 + i];
      if (same) ban_set(ban, V, r.bad_tokens[o1 - 1]);
    }
    if (flags & UVX_BAN_MIN)
      for (int i = tid; i < r.n_min; i += NT) ban_set(ban, V, r.min_ids[i]);
  }
  for (int i = tid; i < r.n_suppress; i += NT) ban_set(ban, V, r.suppress_ids[i]);
  if (begin)
    for (int i = tid; i < r.n_begin; i += NT) ban_set(ban, V, r.begin_ids[i]);
  __syncthreads();
}

// A row behind the bans: the inner reader's score, -inf where the element's bit is set, and on a forced step 0 for the others.  ld8 wants c a
// multiple of 8, as PenalizedRow: the eight flags are one byte of one word, and a zero byte costs nothing.
template <typename R>
struct BannedRow {
  R in;
  const uint32_t* ban;        // the row's words (written by this block before its first read: no __restrict__)
  bool forced;
  __device__ __forceinline__ bool vec(int V) const { return in.vec(V); }
  __device__ __forceinline__ void ld8(long long c, float* v) const {
    in.ld8(c, v);
    const uint32_t flags = (ban[c >> 5] >> (c & 31)) & 0xffu;
    if (forced) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (flags >> e) & 1u ? -__builtin_huge_valf() : 0.0f;
    } else if (flags) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if ((flags >> e) & 1u) v[e] = -__builtin_huge_valf();
    }
  }
  __device__ __forceinline__ float ld(long long c) const {
    const float s = in.ld(c);
    if (seen_bit(ban, (int)c)) return -__builtin_huge_valf();
    return forced ? 0.0f : s;
  }
};

}  // namespace uvx
