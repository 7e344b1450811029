// The body of the device sampler, templated on how a logits row is read, and the one walk over a row that every chooser of select.hip uses:
// select.hip reads the row as it lies (PlainRow below: uvx_sample_select) or through the repetition penalty (PenalizedRow of penalty.h:
// uvx_sample_select_penalized).
//
// Reference: [3P] GenerationMixin._sample with do_sample = True, as the reference's inference path reaches it (LocalInference._generate
// sets do_sample whenever temperature > 0): TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper ->
// softmax -> multinomial, then the pad / EOS / position bookkeeping of the loop.  One block of 1024 threads per row.
//
// Every warper keeps "the tokens whose value is at least some threshold", so the block works on order-preserving 32-bit keys of the f32
// values x_v = score / temperature and finds each threshold EXACTLY by a radix select (11 + 11 + 10 bits, most significant first):
//   top-k         the largest key T with  count{key >= T} >= k                       (ties with the k-th value stay, as `x < kth` in torch)
//   top-p         the largest key T with  mass{key >= T}  >= top_p * total mass      (= drop v when C(x_v) <= 1 - top_p, C the ascending
//                                                                                      cumulative probability; equal values stay or go as a group)
//   min-p         x_v >= x_max + log(min_p)
//   min_keep      the min_keep-th largest key bounds the top-p and min-p thresholds from above
// Masses are exp(x - x_max) in fixed point, summed as integers (64 bits at 2^-(62 - ceil(log2 V)) in the top-p histogram, which LDS atomics fill;
// 128 bits at 2^-100 in the draw): the histogram, the block scans and the draw's running sum are then exact and independent of the order of the
// additions - the same inputs, seed and offset give the same token on every run.
// The draw walks the kept masses in index order (each wave owns a contiguous slice of the row): token = lowest v with cum_v > u * total.
//
// A row reader R gives the f32 score of an element before the temperature:
//   bool  vec(int V)              the row takes 16-byte loads (V % 8 == 0 and an aligned start)
//   void  ld8(long long c, float* v)      the scores of elements [c, c + 8), c a multiple of 8; only where vec(V) holds
//   float ld(long long c)         the score of element c
// Every pass over the row goes through it - the threshold passes, the draw's lane sums, its element-by-element tail and the probs_out pass -
// so all of them see the same scores.
#pragma once
#include "common.h"
#include "kernels.h"

namespace uvx {
namespace sampler {

constexpr int NT = 1024, NW = NT / 64, BINS = 2048;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

// order-preserving key of an f32 (NaN and -0 are canonicalised by the caller)
__device__ __forceinline__ uint32_t key_of(float x) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float canon(float v) {
  if (!(v == v)) v = -__builtin_huge_valf();      // NaN never wins
  return v == 0.f ? 0.f : v;                      // -0 and +0 compare equal: one key
}

struct Row {
  float temperature;      // a division per element, as TemperatureLogitsWarper does
  bool scale;
  __device__ __forceinline__ float x(float score) const { return canon(scale ? score / temperature : score); }
};

// the row as it lies
template <typename T>
struct PlainRow {
  const T* __restrict__ r;
  __device__ __forceinline__ bool vec(int V) const { return V % 8 == 0 && (reinterpret_cast<uintptr_t>(r) & 15) == 0; }
  __device__ __forceinline__ void ld8(long long c, float* v) const { ::ld8<T>(r + c, v); }
  __device__ __forceinline__ float ld(long long c) const { return ldf<T>(r + c); }
};

// f(score_v, v) for every element of the row as the reader gives it, 16-byte loads where the row allows them (a 128256-wide row took 190 us
// with 256 threads and 2-byte loads).  Every thread visits its elements in ascending index order.
template <typename R, typename F>
__device__ __forceinline__ void walk_row(const R& rd, int V, F f) {
  const int V8 = rd.vec(V) ? V : 0;
  for (int c = threadIdx.x * 8; c < V8; c += NT * 8) {
    float v[8];
    rd.ld8(c, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) f(v[e], c + e);
  }
  for (int c = V8 + threadIdx.x; c < V; c += NT) f(rd.ld(c), c);
}

// f(x_v, v): the sampler's view of the same walk
template <typename R, typename F>
__device__ __forceinline__ void for_row(const R& rd, int V, const Row& row, F f) {
  walk_row(rd, V, [&](float score, int c) { f(row.x(score), c); });
}

__device__ __forceinline__ u64 shfl_up_(u64 v, int o) { return __shfl_up(v, o, 64); }
__device__ __forceinline__ u128 shfl_up_(u128 v, int o) {
  return ((u128)__shfl_up((u64)(v >> 64), o, 64) << 64) | __shfl_up((u64)v, o, 64);
}
__device__ __forceinline__ u128 shfl128(u128 v, int l) { return ((u128)__shfl((u64)(v >> 64), l, 64) << 64) | __shfl((u64)v, l, 64); }
template <typename U>
__device__ __forceinline__ U wave_incl_scan(U v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const U t = shfl_up_(v, o);
    if (lane >= o) v += t;
  }
  return v;
}

struct Lds {
  u64 hist[BINS];
  u64 wsum[NW];
  u128 wsum128[NW];
  float red[NW];
  uint32_t sel_bin;
  u64 sel_rest;
  int token;
};

// exp(x - x_max) in 2^-fix_log2 fixed point for the top-p histogram: 64-bit LDS atomics, so the scale leaves room for V terms of at most 1
__device__ __forceinline__ u64 mass_of(float x, float xmax, float fix) { return (u64)(expf(x - xmax) * fix); }
// ... and in 2^-100 fixed point for the draw (an f32 taken apart: mantissa shifted by its exponent): every probability expf can return above
// 2^-100 of the top token's takes part with all its bits; below 2^23 tokens of at most 2^100 each the sum stays under 2^124
__device__ __forceinline__ u128 mass128(float x, float xmax) {
  const uint32_t bits = __builtin_bit_cast(uint32_t, expf(x - xmax));
  const int e = (bits >> 23) & 255;
  const uint32_t m = (bits & 0x7fffffu) | (e ? 0x800000u : 0u);
  const int sh = max(e, 1) - 50;                   // value = m * 2^(e - 150), times 2^100
  return sh >= 0 ? (u128)m << sh : (u128)(m >> min(-sh, 31));
}

// The largest key T with  sum of w(x_v) over {key_v >= T, key_v >= floor_key}  >= target   (1 <= target <= the sum over everything).
// w: 64-bit integer weight of a value.  frac >= 0: the target is that share of the sum over everything, which the first histogram gives.
template <typename R, typename W>
__device__ uint32_t radix_select(const R& rd, int V, const Row& row, uint32_t floor_key, u64 target, double frac, W w, Lds& s) {
  uint32_t prefix = 0, mask = 0;
  for (int pass = 0; pass < 3; ++pass) {
    const int sh = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const uint32_t dmask = pass == 2 ? 1023u : 2047u;
    __syncthreads();
    for (int i = threadIdx.x; i < BINS; i += NT) s.hist[i] = 0;
    __syncthreads();
    for_row(rd, V, row, [&](float x, int) {
      const uint32_t k = key_of(x);
      if (k < floor_key || (k & mask) != prefix || x == -__builtin_huge_valf()) return;
      const u64 wv = w(x);
      if (wv) atomicAdd(&s.hist[(k >> sh) & dmask], wv);
    });
    __syncthreads();
    // bins in descending key order: thread t owns reversed bins 2t, 2t + 1
    const u64 a = s.hist[BINS - 1 - 2 * threadIdx.x], b = s.hist[BINS - 2 - 2 * threadIdx.x];
    const u64 incl = wave_incl_scan(a + b);
    if ((threadIdx.x & 63) == 63) s.wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    u64 base = 0, all = 0;
    for (int i = 0; i < NW; ++i) {
      if (i < (int)(threadIdx.x >> 6)) base += s.wsum[i];
      all += s.wsum[i];
    }
    if (pass == 0 && frac >= 0.0) target = (u64)(frac * (double)all);
    if (target > all) target = all;              // (a count beyond the finite entries; rounding of frac * all)
    if (target < 1) target = 1;
    const u64 ex = base + incl - (a + b);          // weight of all bins above this thread's pair
    if (ex < target && target <= ex + a + b) {     // exactly one thread (weights are non-negative, the pair is not empty)
      const bool first = target <= ex + a;
      s.sel_bin = BINS - 1 - 2 * threadIdx.x - (first ? 0 : 1);
      s.sel_rest = target - ex - (first ? 0 : a);
    }
    if (all == 0 && threadIdx.x == 0) { s.sel_bin = 0; s.sel_rest = 1; }     // nothing finite: the lowest key
    __syncthreads();
    prefix |= s.sel_bin << sh;
    mask |= dmask << sh;
    target = s.sel_rest;
  }
  return prefix;
}

// Philox4x32-10, first output word
__device__ __forceinline__ uint32_t philox_w0(u64 seed, u64 offset, uint32_t b) {
  uint32_t c0 = (uint32_t)offset, c1 = (uint32_t)(offset >> 32), c2 = b, c3 = 0;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int i = 0; i < 10; ++i) {
    const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}

struct SampleArgs {
  float temperature, top_p, min_p;
  int top_k, min_keep;
  u64 seed, offset;
  const float* uniforms;
  float* probs_out;
};

// The warpers and the draw on row b, read through rd: -> the token, the same value in every thread of the block (no thread leaves early).
// The row's last read lies before the return.
template <typename R>
__device__ __forceinline__ int sample_row(const R& rd, int V, const SampleArgs& a, int b, Lds& s) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* po = a.probs_out ? a.probs_out + (long long)b * V : nullptr;
  const Row row{a.temperature, a.temperature != 1.0f};
  const float NEG = -__builtin_huge_valf();

  float m = NEG;
  for_row(rd, V, row, [&](float x, int) { m = fmaxf(m, x); });
  const float xmax = block_max(m, s.red);
  int token = 0;
  if (xmax == NEG) {                    // nothing above -inf: index 0, like uvx_argmax; no probability anywhere
    if (po) for (int c = threadIdx.x; c < V; c += NT) po[c] = 0.f;
  } else {
    const uint32_t kmax = key_of(xmax);
    auto one = [](float) -> u64 { return 1; };
    const float fix = __builtin_ldexpf(1.f, 62 - (V > 1 ? 32 - __clz(V - 1) : 0));      // V terms of at most 2^(62 - ceil(log2 V)) stay below 2^62
    auto mass = [xmax, fix](float x) -> u64 { return mass_of(x, xmax, fix); };
    uint32_t T_k = 0;                   // top-k: everything below is gone for the later steps
    if (a.top_k > 0) {
      const int k = min(max(a.top_k, a.min_keep), V);
      T_k = k == 1 ? kmax : radix_select(rd, V, row, 0, (u64)k, -1.0, one, s);
    }
    uint32_t T_keep = kmax;             // the min_keep largest are never dropped by top-p / min-p
    if (a.min_keep > 1 && (a.top_p < 1.0f || a.min_p > 0.f)) T_keep = radix_select(rd, V, row, 0, (u64)min(a.min_keep, V), -1.0, one, s);
    uint32_t thr = T_k;
    if (a.top_p < 1.0f) {
      const uint32_t T_p = radix_select(rd, V, row, T_k, 0, (double)a.top_p, mass, s);
      thr = max(thr, min(T_p, T_keep));
    }
    if (a.min_p > 0.f) {
      const uint32_t T_m = key_of(canon(xmax + logf(a.min_p)));
      thr = max(thr, min(T_m, T_keep));
    }
    // ---- the draw: kept masses in index order; wave w owns [w * seg, (w + 1) * seg), 512 elements per step, 8 per lane ----
    const bool vec = rd.vec(V);
    const int seg = ((V + NW - 1) / NW + 7) & ~7;
    const long long s0 = (long long)wv * seg, s1 = min((long long)V, s0 + seg);
    auto kept_mass = [&](float x) -> u128 { return (x != NEG && key_of(x) >= thr) ? mass128(x, xmax) : (u128)0; };
    auto lane_masses = [&](long long c) -> u128 {      // the sum of the kept masses of elements [c, c + 8) below s1 (c is a multiple of 8)
      float v[8];
      if (vec && c + 8 <= s1) rd.ld8(c, v);
      else
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = c + e < s1 ? rd.ld(c + e) : NEG;
      u128 t = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) t += kept_mass(c + e < s1 ? row.x(v[e]) : NEG);
      return t;
    };
    u128 mine = 0;
    for (long long c = s0 + lane * 8; c < s1; c += 512) mine += lane_masses(c);
    mine = wave_incl_scan(mine);
    __syncthreads();
    if (lane == 63) s.wsum128[wv] = mine;
    if (threadIdx.x == 0) s.token = 0;
    __syncthreads();
    u128 before = 0, total = 0;
    for (int i = 0; i < NW; ++i) {
      if (i < wv) before += s.wsum128[i];
      total += s.wsum128[i];
    }
    const float u = a.uniforms ? a.uniforms[b] : (float)(philox_w0(a.seed, a.offset, (uint32_t)b) >> 8) * 5.9604644775390625e-08f;
    // target = floor(u * total) with u = mu * 2^(eu - 150) taken apart (total's low 24 bits, 2^-76 of the top token's mass, do not take part)
    const uint32_t ub = __builtin_bit_cast(uint32_t, u);
    const int eu = max((int)((ub >> 23) & 255), 1);
    const uint32_t mu = (ub & 0x7fffffu) | ((ub >> 23) & 255 ? 0x800000u : 0u);
    u128 target = !(u > 0.f) ? (u128)0 : eu > 126 ? total : ((total >> 24) * mu) >> (126 - eu);
    if (target >= total) target = total - 1;          // u = 1 - 2^-24 (or a uniform >= 1) must not run off the end: the last kept token
                                                      // (total >= 2^100: x_max is kept)
    if (before <= target && target < before + s.wsum128[wv]) {     // exactly one wave holds the crossing
      u128 run = before;
      for (long long c0 = s0; c0 < s1; c0 += 512) {
        const long long c = c0 + lane * 8;
        const u128 t = c < s1 ? lane_masses(c) : (u128)0;
        const u128 incl = wave_incl_scan(t);
        const u128 step_total = shfl128(incl, 63);
        if (run + step_total > target) {
          const u64 hit = __ballot(run + incl > target);
          if (lane == __ffsll((long long)hit) - 1) {
            u128 cum = run + incl - t;                  // the first of the lane's 8 elements at which the running sum passes the target
            long long v = c;
#pragma unroll 1
            for (; v < min(c + 7, s1 - 1); ++v) {
              cum += kept_mass(row.x(rd.ld(v)));
              if (cum > target) break;
            }
            s.token = (int)v;
          }
          break;
        }
        run += step_total;
      }
    }
    __syncthreads();
    token = min(max(s.token, 0), V - 1);
    if (po) {
      const float tf = (float)(((double)(u64)(total >> 64) * 18446744073709551616.0 + (double)(u64)total) * 7.888609052210118e-31);      // * 2^-100
      for_row(rd, V, row, [&](float x, int c) { po[c] = (x != NEG && key_of(x) >= thr) ? expf(x - xmax) / tf : 0.f; });
    }
  }
  return token;
}

}  // namespace sampler
}  // namespace uvx
