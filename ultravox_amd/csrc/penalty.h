// The repetition penalty on a logits row, as a row reader over a "seen" bitmap: what a device-side token selector needs of
// [3P] RepetitionPenaltyLogitsProcessor.  The penalised selectors of select.hip read their rows through PenalizedRow.
//
// Bitmap: uint32 [B][words], words >= ceil(V / 32); bit (id & 31) of word (id >> 5) of row b = "id occurred in row b" (prompt, padding and
// generated tokens alike: HF penalises every id of input_ids).  2^23 vocabulary entries are 1 MB per row, so the bitmap is read from global
// memory (it stays in L2), never staged in LDS.
#pragma once
#include "common.h"

namespace uvx {

// HF as it is written: torch.where(score < 0, score * penalty, score / penalty) - ONE correctly rounded f32 operation either way (the build has
// no fast-math flag; a multiplication by 1 / penalty differs in the last bit on about a tenth of the elements).  NaN and -0 take the division.
__device__ __forceinline__ float penalize(float s, float penalty) { return s < 0.f ? s * penalty : s / penalty; }

__device__ __forceinline__ bool seen_bit(const uint32_t* seen, int id) { return (seen[id >> 5] >> (id & 31)) & 1u; }

// One row behind the penalty, element by element and eight at a time: a reader for walk_row and the sampler's body (sample.h).
// ld8 wants c a multiple of 8 - the eight flags are then one byte of one bitmap word, and a zero byte skips the penalty work.
template <typename T>
struct PenalizedRow {
  const T* __restrict__ r;
  const uint32_t* seen;       // the row's words; the selector sets a bit in them once all its reads are done, so no __restrict__
  float penalty;
  __device__ __forceinline__ bool vec(int V) const { return V % 8 == 0 && (reinterpret_cast<uintptr_t>(r) & 15) == 0; }
  __device__ __forceinline__ void ld8(long long c, float* v) const {
    ::ld8<T>(r + c, v);
    const uint32_t flags = (seen[c >> 5] >> (c & 31)) & 0xffu;
    if (flags) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if ((flags >> e) & 1u) v[e] = penalize(v[e], penalty);
    }
  }
  __device__ __forceinline__ float ld(long long c) const {
    const float s = ldf<T>(r + c);
    return seen_bit(seen, (int)c) ? penalize(s, penalty) : s;
  }
};

}  // namespace uvx
