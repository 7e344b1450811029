// Polyphase resampling of a ragged batch of PCM clips to the model's rate in one launch: uvx_resample_poly (the definition is its comment in
// include/uvx.h; the index arithmetic is resample.h's).
//
// One block owns TILE consecutive outputs of one row, one output per thread.  The whole tap table (at most 80 KB + 4 B) and the input span of
// the tile go to LDS, int16 converted to f32 on the way; a span longer than XCHUNK samples (only ratios far beyond audio rates need that:
// 192 kHz stages 3 312) is walked in passes of XCHUNK.  Every output adds its terms in ascending input index with one fmaf each, whatever the
// pass boundaries, the tile, the row or the batch are: a row's bits depend on its samples, the taps and (up, down) alone.
//
// Loads from global memory are per element (coalesced across the block): a row may start at any element offset, so an int16 row is only
// 2-byte aligned.  LDS reads: lane j reads x at a stride of down / up elements (3 at 48 kHz: conflict-free; 6 at 96 kHz: two-way) and the taps
// at its own phase (one address for the whole wave when up == 1).  The kernel is launch-latency work (30 s at 48 kHz: 29 M multiply-adds,
// 2.9 MB read), so neither is tuned further.
#include "common.h"
#include "resample.h"

namespace {
using namespace uvx::resample;

__device__ __forceinline__ float pcm_f32(const float* p) { return *p; }
__device__ __forceinline__ float pcm_f32(const int16_t* p) { return (float)*p * 0x1p-15f; }      // exact in f32

template <typename T>
__global__ void __launch_bounds__(TILE) resample_poly_k(const T* __restrict__ pcm, const int64_t* __restrict__ row_offset,
                                                        const int32_t* __restrict__ n_in, int max_n_in, int up, int down,
                                                        const float* __restrict__ taps, int half, float* __restrict__ out, long long out_stride,
                                                        int out_width) {
  extern __shared__ float lds[];
  float* hs = lds;                          // taps [2 * half + 1]
  float* xs = lds + (2 * half + 1);         // inputs of the current pass
  const int tid = threadIdx.x, b = blockIdx.y;
  const int64_t k0 = (int64_t)blockIdx.x * TILE, k = k0 + tid;
  int n = n_in[b];
  n = n < 0 ? 0 : (n > max_n_in ? max_n_in : n);      // the host sized out_width for max_n_in
  int64_t nout = n_out(n, up, down);
  if (nout > out_width) nout = out_width;
  float* orow = out + (long long)b * out_stride;
  if (k0 >= nout) {                                    // a tile of padding only (the same for the whole block)
    if (k < out_width) orow[k] = 0.f;
    return;
  }
  for (int t = tid; t <= 2 * half; t += TILE) hs[t] = taps[t];
  const T* x = pcm + row_offset[b];
  const int64_t k_last = (k0 + TILE < nout ? k0 + TILE : nout) - 1;
  const int64_t i_lo = first_i(k0, up, down, half), i_hi = last_i(k_last, up, down, half, n);
  const bool live = k < nout;
  const int64_t my_first = live ? first_i(k, up, down, half) : 1, my_last = live ? last_i(k, up, down, half, n) : 0;
  float acc = 0.f;
  for (int64_t c = i_lo; c <= i_hi; c += XCHUNK) {
    const int cn = (int)(i_hi - c + 1 < XCHUNK ? i_hi - c + 1 : XCHUNK);
    __syncthreads();                                   // the pass before has been read
    for (int j = tid; j < cn; j += TILE) xs[j] = pcm_f32(x + (c + j));
    __syncthreads();                                   // (the first pass: the taps as well)
    const int64_t lo = my_first > c ? my_first : c, hi = my_last < c + cn - 1 ? my_last : c + cn - 1;
    if (lo <= hi) {
      int t = (int)tap_index(k, lo, up, down, half);
      const int j0 = (int)(lo - c), cnt = (int)(hi - lo + 1);
      for (int j = 0; j < cnt; ++j, t -= up) acc = fmaf(xs[j0 + j], hs[t], acc);
    }
  }
  if (k < out_width) orow[k] = live ? acc : 0.f;
}

template <typename T>
int launch(hipStream_t st, const void* pcm, const int64_t* row_offset, const int32_t* n_in, int B, int max_n_in, int up, int down, const float* taps,
           int half, float* out, long long out_stride, int out_width) {
  const long long span = ((long long)(TILE - 1) * down + 2LL * half) / up + 2;      // >= any tile's input span (resample.h)
  const size_t smem = ((size_t)(2 * half + 1) + (size_t)(span < XCHUNK ? span : XCHUNK)) * sizeof(float);
  if (smem > 64 * 1024) {
    static PerDeviceOnce attr_set;
    UVX_SET_ATTR_ONCE(attr_set, resample_poly_k<T>, 160 * 1024);
  }
  hipLaunchKernelGGL(resample_poly_k<T>, dim3(cdiv(out_width, TILE), B), dim3(TILE), smem, st, (const T*)pcm, row_offset, n_in, max_n_in, up, down,
                     taps, half, out, out_stride, out_width);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}

}  // namespace

extern "C" int32_t uvx_resample_poly(void* stream, int32_t pcm_format, const void* pcm, const int64_t* row_offset, const int32_t* n_in, int32_t B,
                                     int32_t max_n_in, int32_t up, int32_t down, const float* taps, int32_t half_len, float* out,
                                     int64_t out_stride, int32_t out_width) {
  UVX_CHECK(pcm && row_offset && n_in && taps && out, UVX_ERR_INVALID, "resample_poly: null argument");
  UVX_CHECK(pcm_format == 0 || pcm_format == 1, UVX_ERR_INVALID, "resample_poly: pcm_format=%d (0: f32, 1: int16)", pcm_format);
  UVX_CHECK(up >= 1 && down >= 1 && half_len >= 1, UVX_ERR_INVALID, "resample_poly: up=%d down=%d half_len=%d must each be at least 1", up, down,
            half_len);
  UVX_CHECK(B >= 0 && B <= 65535 && max_n_in >= 0 && out_width >= 0 && out_stride >= out_width, UVX_ERR_INVALID,
            "resample_poly: B=%d (at most 65535) max_n_in=%d out_width=%d out_stride=%lld", B, max_n_in, out_width, (long long)out_stride);
  UVX_CHECK(up <= MAX_RATIO && down <= MAX_RATIO && half_len <= 10 * MAX_RATIO, UVX_ERR_UNSUPPORTED,
            "resample_poly: up=%d down=%d half_len=%d: the kernel is built for up and down of at most %d each and half_len of at most %d", up, down,
            half_len, MAX_RATIO, 10 * MAX_RATIO);
  UVX_CHECK(n_out(max_n_in, up, down) <= out_width, UVX_ERR_INVALID, "resample_poly: out_width=%d is below the %lld outputs of a row of max_n_in=%d",
            out_width, (long long)n_out(max_n_in, up, down), max_n_in);
  if (B == 0 || out_width == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
  return pcm_format == 1 ? launch<int16_t>(st, pcm, row_offset, n_in, B, max_n_in, up, down, taps, half_len, out, (long long)out_stride, out_width)
                         : launch<float>(st, pcm, row_offset, n_in, B, max_n_in, up, down, taps, half_len, out, (long long)out_stride, out_width);
}
