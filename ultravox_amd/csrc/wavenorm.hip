// Zero-mean / unit-variance normalisation of a ragged batch of raw-waveform clips, padded into the [B, L] batch the wav2vec2 tower reads:
// uvx_wave_norm (the definition is its comment in include/uvx.h; the constants are wavenorm.h's).
//
// Two launches.  wave_stats_k: one block per CHUNK samples of one row, counted from the row's own start.  Thread t adds samples t, t + 256, ...
// of the chunk in float64 (x * x is exact there), then the 256 partial pairs are folded by a halving tree in LDS and (S1, S2) of the chunk goes
// to the workspace.  wave_apply_k: one block per TILE outputs of one row.  Every thread adds the row's pairs in ascending chunk order (the
// same addresses for the whole block), forms mean and rstd, and the block writes its tile: (x - mean) * rstd below n, padding_value from n
// to out_width.  No atomics, and no order that depends on anything but the row's samples and n: a row's bits are the same wherever it stands
// in whatever batch.  The float64 arithmetic is compiled as written (contraction is off in this file).
//
// Loads from global memory are per element (coalesced across the block): a row may start at any element offset, so an int16 row is only
// 2-byte aligned.  The work is launch latency and HBM traffic (30 s at 16 kHz: 480 000 samples read twice, 1.9 MB written); nobody has
// measured a need for more, so nothing here is tuned beyond coalesced access.
#include <cmath>

#include "common.h"
#include "wavenorm.h"

#pragma clang fp contract(off)

namespace {
using namespace uvx::wavenorm;

__device__ __forceinline__ float pcm_f32(const float* p) { return *p; }
__device__ __forceinline__ float pcm_f32(const int16_t* p) { return (float)*p * 0x1p-15f; }      // exact in f32

__device__ __forceinline__ int clamp_n(int n, int max_n) { return n < 0 ? 0 : (n > max_n ? max_n : n); }

template <typename T>
__global__ void __launch_bounds__(THREADS) wave_stats_k(const T* __restrict__ pcm, const int64_t* __restrict__ row_offset,
                                                        const int32_t* __restrict__ n_in, int max_n, int n_chunks, double2* __restrict__ ws) {
  __shared__ double2 part[THREADS];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int n = clamp_n(n_in[b], max_n);
  const int c0 = blockIdx.x * CHUNK;                  // blockIdx.x < n_chunks = ceil(max_n / CHUNK): below 2^31
  if (c0 >= n) return;                                // not a chunk of this row (the same for the whole block); its pair is never read
  const int c1 = n - c0 < CHUNK ? n : c0 + CHUNK;
  const T* x = pcm + row_offset[b];
  double s1 = 0.0, s2 = 0.0;
  for (int i = c0 + tid; i < c1; i += THREADS) {
    const double v = (double)pcm_f32(x + i);
    s1 += v;
    s2 += v * v;
  }
  part[tid] = make_double2(s1, s2);
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      part[tid].x += part[tid + s].x;
      part[tid].y += part[tid + s].y;
    }
    __syncthreads();
  }
  if (tid == 0) ws[(long long)b * n_chunks + blockIdx.x] = part[0];
}

template <typename T>
__global__ void __launch_bounds__(THREADS) wave_apply_k(const T* __restrict__ pcm, const int64_t* __restrict__ row_offset,
                                                        const int32_t* __restrict__ n_in, int max_n, int n_chunks, const double2* __restrict__ ws,
                                                        int normalize, float padding_value, float* __restrict__ out, long long out_stride,
                                                        int out_width) {
  const int tid = threadIdx.x, b = blockIdx.y;
  const int n = clamp_n(n_in[b], max_n);              // <= max_n <= out_width
  const long long k0 = (long long)blockIdx.x * TILE;
  const long long k1 = k0 + TILE < out_width ? k0 + TILE : out_width;
  float* orow = out + (long long)b * out_stride;
  double mean = 0.0, rstd = 1.0;
  if (normalize && k0 < n) {                          // (a tile of padding only needs neither)
    const double2* p = ws + (long long)b * n_chunks;
    const int nc = (n + CHUNK - 1) / CHUNK;
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < nc; ++c) {
      s1 += p[c].x;
      s2 += p[c].y;
    }
    mean = s1 / (double)n;
    const double var = s2 / (double)n - mean * mean;
    rstd = 1.0 / sqrt((var > 0.0 ? var : 0.0) + EPS);
  }
  const T* x = pcm + row_offset[b];
  for (long long k = k0 + tid; k < k1; k += THREADS) {
    float y = padding_value;
    if (k < n) {
      const float v = pcm_f32(x + k);
      y = normalize ? (float)(((double)v - mean) * rstd) : v;
    }
    orow[k] = y;
  }
}

template <typename T>
int launch(hipStream_t st, const void* pcm, const int64_t* row_offset, const int32_t* n_in, int B, int max_n, int normalize, float padding_value,
           float* out, long long out_stride, int out_width, void* workspace) {
  const int n_chunks = cdiv(max_n, CHUNK);
  if (normalize && n_chunks > 0) {
    hipLaunchKernelGGL(wave_stats_k<T>, dim3(n_chunks, B), dim3(THREADS), 0, st, (const T*)pcm, row_offset, n_in, max_n, n_chunks,
                       (double2*)workspace);
    UVX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(wave_apply_k<T>, dim3(cdiv(out_width, TILE), B), dim3(THREADS), 0, st, (const T*)pcm, row_offset, n_in, max_n, n_chunks,
                     (const double2*)workspace, normalize, padding_value, out, out_stride, out_width);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}

}  // namespace

extern "C" size_t uvx_wave_norm_ws_bytes(int32_t B, int32_t max_n) {
  if (B <= 0 || max_n <= 0) return 0;
  return (size_t)B * (size_t)cdiv(max_n, CHUNK) * sizeof(double2);
}

extern "C" int32_t uvx_wave_norm(void* stream, int32_t pcm_format, const void* pcm, const int64_t* row_offset, const int32_t* n, int32_t B,
                                 int32_t max_n, int32_t normalize, float padding_value, float* out, int64_t out_stride, int32_t out_width,
                                 void* workspace, size_t ws_bytes) {
  UVX_CHECK(pcm && row_offset && n && out, UVX_ERR_INVALID, "wave_norm: null argument");
  UVX_CHECK(pcm_format == 0 || pcm_format == 1, UVX_ERR_INVALID, "wave_norm: pcm_format=%d (0: f32, 1: int16)", pcm_format);
  UVX_CHECK(B >= 0 && B <= 65535 && max_n >= 0 && out_stride >= out_width, UVX_ERR_INVALID,
            "wave_norm: B=%d (at most 65535) max_n=%d out_width=%d out_stride=%lld", B, max_n, out_width, (long long)out_stride);
  UVX_CHECK(out_width >= max_n, UVX_ERR_INVALID, "wave_norm: out_width=%d is below the %d samples of a row of max_n=%d", out_width, max_n, max_n);
  UVX_CHECK(std::isfinite(padding_value), UVX_ERR_INVALID, "wave_norm: padding_value=%f is not finite", (double)padding_value);
  const size_t need = normalize ? uvx_wave_norm_ws_bytes(B, max_n) : 0;
  UVX_CHECK(need == 0 || (workspace && ws_bytes >= need), UVX_ERR_INVALID, "wave_norm: workspace=%p of %zu bytes, but B=%d rows of max_n=%d need %zu",
            workspace, ws_bytes, B, max_n, need);
  if (B == 0 || out_width == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
  return pcm_format == 1 ? launch<int16_t>(st, pcm, row_offset, n, B, max_n, normalize, padding_value, out, (long long)out_stride, out_width, workspace)
                         : launch<float>(st, pcm, row_offset, n, B, max_n, normalize, padding_value, out, (long long)out_stride, out_width, workspace);
}
