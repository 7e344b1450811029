// Audio augmentation of a ragged batch of clips on the input layout of uvx_resample_poly / uvx_wave_norm: uvx_aug_gain, uvx_aug_iir and
// uvx_aug_noise (the definitions are their comments in include/uvx.h; the constants and the transform's pass structure are aug.h's).
//
// gain_k: one block per TILE outputs of one row, one multiply and a clamp per element.
// iir_k: one THREAD per BLOCK outputs of one row.  It runs scipy.signal.lfilter's transposed direct form II in float64 from zero state at sample
// max(0, j * BLOCK - warm) and stores from j * BLOCK on; the order is a template argument, so the state lives in registers.  A thread reads
// and writes its own run of the row (neighbouring lanes are BLOCK elements apart); nobody has measured whether staging through LDS pays.
// noise_stats_k / noise_mix_k: uvx_wave_norm's two launches with (S2x, S2n) in the place of (S1, S2), the noise read through a source
// (aug.h: white normals drawn where they are used, or the transform's output).  No atomics; the float64 arithmetic is compiled as written
// (contraction is off in this file).  Loads are per element: a row may start at any element offset.
#include <cmath>

#include "aug.h"

#pragma clang fp contract(off)

namespace {
using namespace uvx::aug;

template <typename T>
__global__ void __launch_bounds__(THREADS) gain_k(const T* __restrict__ pcm, const int64_t* __restrict__ row_offset, const int32_t* __restrict__ n_in,
                                                  int max_n, const float* __restrict__ gain, float* __restrict__ out, long long out_stride,
                                                  int out_width) {
  const int b = blockIdx.y;
  const int n = clamp_n(n_in[b], max_n);
  const long long k0 = (long long)blockIdx.x * TILE;
  const long long k1 = k0 + TILE < out_width ? k0 + TILE : out_width;
  const T* x = pcm + row_offset[b];
  const float g = gain[b];
  float* orow = out + (long long)b * out_stride;
  for (long long k = k0 + threadIdx.x; k < k1; k += THREADS) orow[k] = k < n ? fminf(fmaxf(pcm_f32(x + k) * g, -1.0f), 1.0f) : 0.0f;
}

template <typename T, int ORD>
__global__ void __launch_bounds__(IIR_THREADS) iir_k(const T* __restrict__ pcm, const int64_t* __restrict__ row_offset, const int32_t* __restrict__ n_in,
                                                     int max_n, const double* __restrict__ bc, const double* __restrict__ ac, int warm,
                                                     float* __restrict__ out, long long out_stride, int out_width) {
  const int b = blockIdx.y;
  const int n = clamp_n(n_in[b], max_n);
  const long long k0 = ((long long)blockIdx.x * IIR_THREADS + threadIdx.x) * BLOCK;
  if (k0 >= out_width) return;
  const long long k1 = k0 + BLOCK < out_width ? k0 + BLOCK : out_width;
  float* orow = out + (long long)b * out_stride;
  if (k0 < n) {
    double cb[ORD + 1], ca[ORD + 1], z[ORD];
#pragma unroll
    for (int q = 0; q <= ORD; ++q) {
      cb[q] = bc[q];
      ca[q] = ac[q];
    }
#pragma unroll
    for (int q = 0; q < ORD; ++q) z[q] = 0.0;
    const T* x = pcm + row_offset[b];
    const long long e = k1 < n ? k1 : n;
    for (long long i = k0 > warm ? k0 - warm : 0; i < e; ++i) {
      const double xv = (double)pcm_f32(x + i);
      const double y = z[0] + cb[0] * xv;
#pragma unroll
      for (int q = 0; q < ORD - 1; ++q) z[q] = z[q + 1] + cb[q + 1] * xv - ca[q + 1] * y;
      z[ORD - 1] = cb[ORD] * xv - ca[ORD] * y;
      if (i >= k0) orow[i] = (float)y;
    }
  }
  for (long long i = k0 > n ? k0 : n; i < k1; ++i) orow[i] = 0.0f;
}

template <typename T, typename Src>
__device__ __forceinline__ void stats_body(const T* x, int n, const Src& src, double2* chunk_pair) {
  __shared__ double2 part[THREADS];
  const int tid = threadIdx.x;
  const int c0 = blockIdx.x * CHUNK;
  const int c1 = n - c0 < CHUNK ? n : c0 + CHUNK;
  double s2x = 0.0, s2n = 0.0;
  for (int i = c0 + tid; i < c1; i += THREADS) {
    const double v = (double)pcm_f32(x + i), w = (double)src(i);
    s2x += v * v;
    s2n += w * w;
  }
  part[tid] = make_double2(s2x, s2n);
  __syncthreads();
  for (int s = THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      part[tid].x += part[tid + s].x;
      part[tid].y += part[tid + s].y;
    }
    __syncthreads();
  }
  if (tid == 0) *chunk_pair = part[0];
}

template <typename T, typename Src>
__device__ __forceinline__ void mix_body(const T* x, int n, const Src& src, const double2* pairs, double ratio, float* orow, int out_width) {
  const long long k0 = (long long)blockIdx.x * TILE;
  const long long k1 = k0 + TILE < out_width ? k0 + TILE : out_width;
  double scale = 0.0;
  bool mix = false;
  if (k0 < n) {
    const int nc = (n + CHUNK - 1) / CHUNK;
    double s2x = 0.0, s2n = 0.0;
    for (int c = 0; c < nc; ++c) {
      s2x += pairs[c].x;
      s2n += pairs[c].y;
    }
    mix = s2x != 0.0 && s2n != 0.0;
    if (mix) scale = sqrt((s2x / (double)n) * ratio / (s2n / (double)n));
  }
  for (long long k = k0 + threadIdx.x; k < k1; k += THREADS) {
    float y = 0.0f;
    if (k < n) {
      const float v = pcm_f32(x + k);
      y = mix ? (float)((double)v + (double)src((int)k) * scale) : v;
    }
    orow[k] = y;
  }
}

// colour 0: white normals; otherwise the transform's rows at z
template <typename T>
__global__ void __launch_bounds__(THREADS) noise_stats_k(const T* __restrict__ pcm, const int64_t* __restrict__ row_offset,
                                                         const int32_t* __restrict__ n_in, int max_n, int n_chunks, int coloured, uint64_t seed,
                                                         uint64_t offset, const float2* __restrict__ z, long long z_stride, double2* __restrict__ ws) {
  const int b = blockIdx.y;
  const int n = clamp_n(n_in[b], max_n);
  if (blockIdx.x * CHUNK >= n) return;                // not a chunk of this row (the same for the whole block); its pair is never read
  const T* x = pcm + row_offset[b];
  double2* pair = ws + (long long)b * n_chunks + blockIdx.x;
  if (coloured) stats_body(x, n, TransformSrc{z + (long long)b * z_stride, log2_m(n) - 1}, pair);
  else stats_body(x, n, WhiteSrc{seed, offset, (uint32_t)b}, pair);
}

template <typename T>
__global__ void __launch_bounds__(THREADS) noise_mix_k(const T* __restrict__ pcm, const int64_t* __restrict__ row_offset,
                                                       const int32_t* __restrict__ n_in, int max_n, int n_chunks, int coloured, uint64_t seed,
                                                       uint64_t offset, const float2* __restrict__ z, long long z_stride, const double2* __restrict__ ws,
                                                       const double* __restrict__ noise_ratio, float* __restrict__ out, long long out_stride,
                                                       int out_width) {
  const int b = blockIdx.y;
  const int n = clamp_n(n_in[b], max_n);              // <= max_n <= out_width
  const T* x = pcm + row_offset[b];
  const double2* pairs = ws + (long long)b * n_chunks;
  float* orow = out + (long long)b * out_stride;
  const double ratio = noise_ratio[b];
  if (coloured) mix_body(x, n, TransformSrc{z + (long long)b * z_stride, n > 0 ? log2_m(n) - 1 : 0}, pairs, ratio, orow, out_width);
  else mix_body(x, n, WhiteSrc{seed, offset, (uint32_t)b}, pairs, ratio, orow, out_width);
}

template <typename T>
int launch_gain(hipStream_t st, const void* pcm, const int64_t* row_offset, const int32_t* n, int B, int max_n, const float* gain, float* out,
                long long out_stride, int out_width) {
  hipLaunchKernelGGL(gain_k<T>, dim3(cdiv(out_width, TILE), B), dim3(THREADS), 0, st, (const T*)pcm, row_offset, n, max_n, gain, out, out_stride,
                     out_width);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}

template <typename T, int ORD>
int launch_iir_ord(hipStream_t st, const void* pcm, const int64_t* row_offset, const int32_t* n, int B, int max_n, const double* bc, const double* ac,
                   int warm, float* out, long long out_stride, int out_width) {
  hipLaunchKernelGGL((iir_k<T, ORD>), dim3(cdiv(out_width, (long long)BLOCK * IIR_THREADS), B), dim3(IIR_THREADS), 0, st, (const T*)pcm, row_offset, n,
                     max_n, bc, ac, warm, out, out_stride, out_width);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}

template <typename T>
int launch_iir(hipStream_t st, int order, const void* pcm, const int64_t* row_offset, const int32_t* n, int B, int max_n, const double* bc,
               const double* ac, int warm, float* out, long long out_stride, int out_width) {
  switch (order) {
#define UVX_IIR_CASE(O) \
  case O: return launch_iir_ord<T, O>(st, pcm, row_offset, n, B, max_n, bc, ac, warm, out, out_stride, out_width);
    UVX_IIR_CASE(1) UVX_IIR_CASE(2) UVX_IIR_CASE(3) UVX_IIR_CASE(4) UVX_IIR_CASE(5) UVX_IIR_CASE(6) UVX_IIR_CASE(7) UVX_IIR_CASE(8)
    UVX_IIR_CASE(9) UVX_IIR_CASE(10) UVX_IIR_CASE(11) UVX_IIR_CASE(12) UVX_IIR_CASE(13) UVX_IIR_CASE(14) UVX_IIR_CASE(15) UVX_IIR_CASE(16)
#undef UVX_IIR_CASE
  }
  return UVX_ERR_INVALID;
}

size_t transform_elems(int max_n) { return max_n > 0 ? (size_t)1 << (log2_m(max_n) - 1) : 0; }      // N of the longest row

template <typename T>
int launch_noise(hipStream_t st, const void* pcm, const int64_t* row_offset, const int32_t* n, int B, int max_n, int colour, const double* noise_ratio,
                 uint64_t seed, uint64_t offset, float* out, long long out_stride, int out_width, void* workspace) {
  const int n_chunks = cdiv(max_n, CHUNK);
  double2* pairs = (double2*)workspace;
  float2* z = (float2*)(pairs + (size_t)B * n_chunks);
  const long long z_stride = (long long)transform_elems(max_n);
  if (n_chunks > 0) {
    if (colour) {
      const int rc = noise_transform(st, n, B, max_n, colour, seed, offset, z, z_stride);
      if (rc != UVX_OK) return rc;
    }
    hipLaunchKernelGGL(noise_stats_k<T>, dim3(n_chunks, B), dim3(THREADS), 0, st, (const T*)pcm, row_offset, n, max_n, n_chunks, colour, seed, offset,
                       (const float2*)z, z_stride, pairs);
    UVX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(noise_mix_k<T>, dim3(cdiv(out_width, TILE), B), dim3(THREADS), 0, st, (const T*)pcm, row_offset, n, max_n, n_chunks, colour, seed,
                     offset, (const float2*)z, z_stride, (const double2*)pairs, noise_ratio, out, out_stride, out_width);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}

// the checks the three entries share; `what` names the entry in the message
int check_layout(const char* what, int32_t pcm_format, const void* pcm, const int64_t* row_offset, const int32_t* n, int32_t B, int32_t max_n,
                 const float* out, int64_t out_stride, int32_t out_width) {
  UVX_CHECK(pcm && row_offset && n && out, UVX_ERR_INVALID, "%s: null argument", what);
  UVX_CHECK(pcm_format == 0 || pcm_format == 1, UVX_ERR_INVALID, "%s: pcm_format=%d (0: f32, 1: int16)", what, pcm_format);
  UVX_CHECK(B >= 0 && B <= 65535 && max_n >= 0 && out_stride >= out_width, UVX_ERR_INVALID,
            "%s: B=%d (at most 65535) max_n=%d out_width=%d out_stride=%lld", what, B, max_n, out_width, (long long)out_stride);
  UVX_CHECK(out_width >= max_n, UVX_ERR_INVALID, "%s: out_width=%d is below the %d samples of a row of max_n=%d", what, out_width, max_n, max_n);
  return UVX_OK;
}

}  // namespace

extern "C" int32_t uvx_aug_gain(void* stream, int32_t pcm_format, const void* pcm, const int64_t* row_offset, const int32_t* n, int32_t B,
                                int32_t max_n, const float* gain, float* out, int64_t out_stride, int32_t out_width) {
  const int rc = check_layout("aug_gain", pcm_format, pcm, row_offset, n, B, max_n, out, out_stride, out_width);
  if (rc != UVX_OK) return rc;
  UVX_CHECK(gain, UVX_ERR_INVALID, "aug_gain: null gain");
  if (B == 0 || out_width == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
  return pcm_format == 1 ? launch_gain<int16_t>(st, pcm, row_offset, n, B, max_n, gain, out, (long long)out_stride, out_width)
                         : launch_gain<float>(st, pcm, row_offset, n, B, max_n, gain, out, (long long)out_stride, out_width);
}

extern "C" int32_t uvx_aug_iir(void* stream, int32_t pcm_format, const void* pcm, const int64_t* row_offset, const int32_t* n, int32_t B,
                               int32_t max_n, const double* b, const double* a, int32_t order, int32_t warm, float* out, int64_t out_stride,
                               int32_t out_width) {
  const int rc = check_layout("aug_iir", pcm_format, pcm, row_offset, n, B, max_n, out, out_stride, out_width);
  if (rc != UVX_OK) return rc;
  UVX_CHECK(b && a, UVX_ERR_INVALID, "aug_iir: null coefficients");
  UVX_CHECK(order >= 1 && order <= MAX_ORDER, UVX_ERR_INVALID, "aug_iir: order=%d (1 to %d)", order, MAX_ORDER);
  UVX_CHECK(warm >= 0, UVX_ERR_INVALID, "aug_iir: warm=%d is negative", warm);
  if (B == 0 || out_width == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
  return pcm_format == 1 ? launch_iir<int16_t>(st, order, pcm, row_offset, n, B, max_n, b, a, warm, out, (long long)out_stride, out_width)
                         : launch_iir<float>(st, order, pcm, row_offset, n, B, max_n, b, a, warm, out, (long long)out_stride, out_width);
}

extern "C" size_t uvx_aug_noise_ws_bytes(int32_t B, int32_t max_n, int32_t colour) {
  if (B <= 0 || max_n <= 0) return 0;
  return (size_t)B * ((size_t)cdiv(max_n, CHUNK) * sizeof(double2) + (colour ? transform_elems(max_n) * sizeof(float2) : 0));
}

extern "C" int32_t uvx_aug_noise(void* stream, int32_t pcm_format, const void* pcm, const int64_t* row_offset, const int32_t* n, int32_t B,
                                 int32_t max_n, int32_t colour, const double* noise_ratio, uint64_t seed, uint64_t offset, float* out,
                                 int64_t out_stride, int32_t out_width, void* workspace, size_t ws_bytes) {
  const int rc = check_layout("aug_noise", pcm_format, pcm, row_offset, n, B, max_n, out, out_stride, out_width);
  if (rc != UVX_OK) return rc;
  UVX_CHECK(noise_ratio, UVX_ERR_INVALID, "aug_noise: null noise_ratio");
  UVX_CHECK(colour >= 0 && colour <= 4, UVX_ERR_INVALID, "aug_noise: colour=%d (0 white, 1 pink, 2 brown, 3 blue, 4 violet)", colour);
  UVX_CHECK(colour == 0 || max_n <= (1 << MAX_LOG2_M), UVX_ERR_UNSUPPORTED,
            "aug_noise: coloured noise is built for max_n <= %d (2^%d), but max_n=%d; white noise has no limit", 1 << MAX_LOG2_M, MAX_LOG2_M, max_n);
  const size_t need = uvx_aug_noise_ws_bytes(B, max_n, colour);
  UVX_CHECK(need == 0 || (workspace && ws_bytes >= need), UVX_ERR_INVALID,
            "aug_noise: workspace=%p of %zu bytes, but B=%d rows of max_n=%d in colour %d need %zu", workspace, ws_bytes, B, max_n, colour, need);
  if (B == 0 || out_width == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
  return pcm_format == 1 ? launch_noise<int16_t>(st, pcm, row_offset, n, B, max_n, colour, noise_ratio, seed, offset, out, (long long)out_stride,
                                                 out_width, workspace)
                         : launch_noise<float>(st, pcm, row_offset, n, B, max_n, colour, noise_ratio, seed, offset, out, (long long)out_stride,
                                               out_width, workspace);
}
