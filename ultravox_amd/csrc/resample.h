// Index arithmetic of the polyphase resampler (resample.hip; the definition is uvx_resample_poly's comment in include/uvx.h).
//
// Everything is 64-bit: k * down and i * up pass 2^31 for a 44.1 kHz clip of about five minutes.  The functions are host + device and depend
// on nothing else, so a plain C++ program can include this file and check them against exact integers (tests/test_resample_cpu.py).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UVX_RS_HD __host__ __device__ inline
#else
#define UVX_RS_HD inline
#endif

namespace uvx {
namespace resample {

constexpr int TILE = 256;            // consecutive outputs of one row per block, one per thread
constexpr int MAX_RATIO = 1024;      // up and down are each at most this: the tap table (20 * max(up, down) + 1 floats) stays within 80 KB + 4 B
constexpr int XCHUNK = 16384;        // input samples staged per pass (64 KB of f32); a longer span takes several passes

// n_out = ceil(n * up / down)
UVX_RS_HD int64_t n_out(int64_t n, int64_t up, int64_t down) { return (n * up + down - 1) / down; }

// first input of output k: the smallest i >= 0 with k * down - i * up <= half
UVX_RS_HD int64_t first_i(int64_t k, int64_t up, int64_t down, int64_t half) {
  const int64_t a = k * down - half;
  return a <= 0 ? 0 : (a + up - 1) / up;
}

// last input of output k: the largest i < n with i * up - k * down <= half (k * down + half >= 0 always)
UVX_RS_HD int64_t last_i(int64_t k, int64_t up, int64_t down, int64_t half, int64_t n) {
  const int64_t i = (k * down + half) / up;
  return i < n - 1 ? i : n - 1;
}

// index into the tap table of input i's weight in output k: half + (k * down - i * up), in [0, 2 * half] for first_i <= i <= last_i
UVX_RS_HD int64_t tap_index(int64_t k, int64_t i, int64_t up, int64_t down, int64_t half) { return half + k * down - i * up; }

}  // namespace resample
}  // namespace uvx
