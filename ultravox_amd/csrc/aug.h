// Constants and shared pieces of the audio augmentation kernels (aug.hip: gain, IIR filter, noise statistics and mix; aug_fft.hip: the
// coloured-noise spectrum and its inverse transform).  The definitions are the comments of uvx_aug_gain, uvx_aug_iir and uvx_aug_noise in
// include/uvx.h.
//
// The transform of the coloured noise.  A row of n samples has M = max(2, 2^ceil(log2 n)) and needs the first n samples of a real inverse DFT
// of length M.  It is computed as a packed real transform: one complex inverse FFT of length N = M / 2 whose output element p is
// (noise[2p], noise[2p + 1]).  The passes, each over every row of the launch that needs it (a row's N follows from its own n; its blocks leave
// the passes it does not need at their first instruction):
//   1. noise_spec_k      draws the Hermitian half spectrum, shapes it, and folds it into the N complex inputs (one launch).
//   2. fft_pass_k        one radix-2 decimation-in-frequency pass in global memory per launch, half-spans N / 2, N / 4, ... down to LDS_SPAN:
//                        log2(N) - LDS_LOG2 launches for the longest row, none for N <= LDS_SPAN.
//   3. fft_lds_k         the remaining log2(min(N, LDS_SPAN)) stages of each contiguous run of min(N, LDS_SPAN) elements, in LDS (one launch).
// The passes work in place and leave output p at the bit-reversed position; the statistics and mix kernels read it from there.
// LDS span: LDS_SPAN = 4096 complex f32 = 32 KiB per block of 256 threads, so the largest M that needs no global pass is 2 * LDS_SPAN = 8192.
// Nothing here is tuned beyond that: twiddles come from sincospif per butterfly, the LDS stages are not padded against bank conflicts and the
// global passes are radix 2.
#pragma once
#include <stdint.h>

#include "common.h"

namespace uvx {
namespace aug {

constexpr int THREADS = 256;       // every kernel but the filter
constexpr int TILE = 4096;         // outputs of one row that one block of an element-wise launch (gain, mix) writes
constexpr int CHUNK = 16384;       // samples of one row that one block reduces to one (S2x, S2n) pair: uvx_wave_norm's chunk and order
constexpr int BLOCK = 256;         // outputs of one row that one thread of the filter produces after its warm-up
constexpr int IIR_THREADS = 64;    // threads of a filter block
constexpr int MAX_ORDER = 16;      // the filter's largest order
constexpr int LDS_LOG2 = 12;
constexpr int LDS_SPAN = 4096;     // complex elements of the transform that one block holds in LDS (= 1 << LDS_LOG2)
constexpr int MAX_LOG2_M = 21;     // coloured noise: max_n <= 2^21

__device__ __forceinline__ float pcm_f32(const float* p) { return *p; }
__device__ __forceinline__ float pcm_f32(const int16_t* p) { return (float)*p * 0x1p-15f; }      // exact in f32
__device__ __forceinline__ int clamp_n(int n, int max_n) { return n < 0 ? 0 : (n > max_n ? max_n : n); }

// log2 of M = max(2, smallest power of two >= n), for n >= 1
__host__ __device__ __forceinline__ int log2_m(int n) {
  int l = 1;
  while (l < 31 && (1ll << l) < (long long)n) ++l;
  return l;
}

// Philox4x32-10 (the constants of sample.h), all four output words
__device__ __forceinline__ void philox4(uint64_t seed, uint64_t offset, uint32_t c2, uint32_t c3, uint32_t* w) {
  uint32_t c0 = (uint32_t)offset, c1 = (uint32_t)(offset >> 32);
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c0; w[1] = c1; w[2] = c2; w[3] = c3;
}

// normals 4q + 2 * pair and 4q + 2 * pair + 1 of row b: Box-Muller on (w0, w1) for pair 0, (w2, w3) for pair 1
__device__ __forceinline__ float2 normal_pair(uint64_t seed, uint64_t offset, uint32_t b, uint32_t q, int pair) {
  uint32_t w[4];
  philox4(seed, offset, q, b, w);
  const uint32_t wa = pair ? w[2] : w[0], wb = pair ? w[3] : w[1];
  const float u = ((float)(wa >> 9) + 0.5f) * 0x1p-23f;      // 24 significant bits, never 0 or 1
  const float v = (float)(wb >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u));
  float s, c;
  sincospif(2.0f * v, &s, &c);
  return make_float2(r * c, r * s);
}

// where the noise of a row comes from: element i of the row, as f32
struct WhiteSrc {      // normal i, drawn where it is used
  uint64_t seed, offset;
  uint32_t b;
  __device__ __forceinline__ float operator()(int i) const {
    const float2 g = normal_pair(seed, offset, b, (uint32_t)i >> 2, (i >> 1) & 1);
    return (i & 1) ? g.y : g.x;
  }
};
struct TransformSrc {      // the packed transform's output: (noise[2p], noise[2p + 1]) lies at the bit-reversed position of p among N = 2^log_n
  const float2* z;
  int log_n;
  __device__ __forceinline__ float operator()(int i) const {
    const uint32_t p = (uint32_t)i >> 1;
    const float2 v = z[log_n ? (__brev(p) >> (32 - log_n)) : 0u];
    return (i & 1) ? v.y : v.x;
  }
};

// aug_fft.hip: fills row b of z (N complex elements from z + b * z_stride, N = M / 2 of the row's own n) with the coloured noise of the row
// in the layout TransformSrc reads.  colour in 1 .. 4, max_n in [1, 2^MAX_LOG2_M], B >= 1.
int noise_transform(hipStream_t st, const int32_t* n, int B, int max_n, int colour, uint64_t seed, uint64_t offset, float2* z, long long z_stride);

}  // namespace aug
}  // namespace uvx
