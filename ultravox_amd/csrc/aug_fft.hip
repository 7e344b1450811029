// The coloured noise of uvx_aug_noise before the mix: the shaped random half spectrum of every row and its real inverse DFT, in f32.  The pass
// structure, the LDS span and the layout of the result are aug.h's header comment; the definition is uvx_aug_noise's comment in include/uvx.h.
//
// Packing.  With X_k (k = 0 .. N, N = M / 2; X_0 and X_N real) the shaped half spectrum including the inverse transform's 1 / M,
//   noise[2p] + i noise[2p + 1] = sum over k < N of C_k e^(+2 pi i k p / N),    C_k = (X_k + conj X_(N-k)) + i (X_k - conj X_(N-k)) e^(+i pi k / N),
// and C_(N-k) = conj(E_k) + i conj(O_k) for the same two terms E_k, O_k: one thread forms C_k and C_(N-k) from X_k and X_(N-k).
#include "aug.h"

namespace {
using namespace uvx::aug;

__device__ __forceinline__ float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// X_k of row b: (g_2k + i g_(2k+1)) * sqrt(M / 2) * factor(f_k) / M, real with sqrt(M) at k = 0 and k = N
__device__ __forceinline__ float2 shaped_bin(uint64_t seed, uint64_t offset, uint32_t b, int k, int N, int colour) {
  float2 g = normal_pair(seed, offset, b, (uint32_t)k >> 1, k & 1);      // normals 2k, 2k + 1
  const float M = (float)N * 2.0f, kk = (float)(k > 0 ? k : 1);          // f_k = kk / M, f_0 := f_1; both exact in f32
  const float factor = colour == 1 ? sqrtf(M / kk) : colour == 2 ? M / kk : colour == 3 ? sqrtf(kk / M) : kk / M;
  const bool real = k == 0 || k == N;
  const float amp = factor * (sqrtf(real ? M : M * 0.5f) / M);
  return make_float2(g.x * amp, real ? 0.0f : g.y * amp);
}

__global__ void __launch_bounds__(THREADS) noise_spec_k(const int32_t* __restrict__ n_in, int max_n, int colour, uint64_t seed, uint64_t offset,
                                                        float2* __restrict__ z, long long z_stride) {
  const int b = blockIdx.y;
  const int n = clamp_n(n_in[b], max_n);
  if (n == 0) return;
  const int N = 1 << (log2_m(n) - 1);
  const int k = blockIdx.x * THREADS + threadIdx.x;
  if (k > N / 2) return;
  float2* row = z + (long long)b * z_stride;
  const float2 xk = shaped_bin(seed, offset, b, k, N, colour), xp = shaped_bin(seed, offset, b, N - k, N, colour);
  if (k == 0) {
    row[0] = make_float2(xk.x + xp.x, xk.x - xp.x);
    return;
  }
  const float2 E = make_float2(xk.x + xp.x, xk.y - xp.y), D = make_float2(xk.x - xp.x, xk.y + xp.y);
  float s, c;
  sincospif((float)k / (float)N, &s, &c);
  const float2 O = cmul(D, make_float2(c, s));
  row[k] = make_float2(E.x - O.y, E.y + O.x);
  row[N - k] = make_float2(E.x + O.y, O.x - E.y);      // (k = N / 2 writes the same value twice)
}

// one decimation-in-frequency pass of half-span h = LDS_SPAN << (s - 1) over the rows that have at least s global passes
__global__ void __launch_bounds__(THREADS) fft_pass_k(const int32_t* __restrict__ n_in, int max_n, float2* __restrict__ z, long long z_stride, int s) {
  const int b = blockIdx.y;
  const int n = clamp_n(n_in[b], max_n);
  if (n == 0) return;
  const int log_n = log2_m(n) - 1;
  if (log_n - LDS_LOG2 < s) return;
  const int t = blockIdx.x * THREADS + threadIdx.x;      // butterfly of the row: below 2^(MAX_LOG2_M - 2)
  if (t >= (1 << log_n) / 2) return;
  const int h = LDS_SPAN << (s - 1);
  const int j = t & (h - 1), i0 = ((t - j) << 1) + j, i1 = i0 + h;
  float2* row = z + (long long)b * z_stride;
  const float2 a = row[i0], c = row[i1];
  float sn, cs;
  sincospif((float)j / (float)h, &sn, &cs);
  row[i0] = make_float2(a.x + c.x, a.y + c.y);
  row[i1] = cmul(make_float2(a.x - c.x, a.y - c.y), make_float2(cs, sn));
}

// the stages of half-span below LDS_SPAN: each run of L = min(N, LDS_SPAN) elements is a transform of its own
__global__ void __launch_bounds__(THREADS) fft_lds_k(const int32_t* __restrict__ n_in, int max_n, float2* __restrict__ z, long long z_stride) {
  __shared__ float2 sm[LDS_SPAN];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = clamp_n(n_in[b], max_n);
  if (n == 0) return;
  const int N = 1 << (log2_m(n) - 1);
  const int L = N < LDS_SPAN ? N : LDS_SPAN;
  const long long base = (long long)blockIdx.x * L;
  if (base >= N) return;                                  // (the same for the whole block)
  float2* row = z + (long long)b * z_stride + base;
  for (int i = tid; i < L; i += THREADS) sm[i] = row[i];
  __syncthreads();
  for (int h = L >> 1; h >= 1; h >>= 1) {
    for (int t = tid; t < L / 2; t += THREADS) {
      const int j = t & (h - 1), i0 = ((t - j) << 1) + j, i1 = i0 + h;
      const float2 a = sm[i0], c = sm[i1];
      float sn, cs;
      sincospif((float)j / (float)h, &sn, &cs);
      sm[i0] = make_float2(a.x + c.x, a.y + c.y);
      sm[i1] = cmul(make_float2(a.x - c.x, a.y - c.y), make_float2(cs, sn));
    }
    __syncthreads();
  }
  for (int i = tid; i < L; i += THREADS) row[i] = sm[i];
}

}  // namespace

namespace uvx {
namespace aug {

int noise_transform(hipStream_t st, const int32_t* n, int B, int max_n, int colour, uint64_t seed, uint64_t offset, float2* z, long long z_stride) {
  const int log_n = log2_m(max_n) - 1;      // of the longest row a launch may hold
  const int N = 1 << log_n;
  hipLaunchKernelGGL(noise_spec_k, dim3(cdiv(N / 2 + 1, THREADS), B), dim3(THREADS), 0, st, n, max_n, colour, seed, offset, z, z_stride);
  UVX_LAUNCH_CHECK();
  for (int s = log_n - LDS_LOG2; s >= 1; --s) {
    hipLaunchKernelGGL(fft_pass_k, dim3(N / 2 / THREADS, B), dim3(THREADS), 0, st, n, max_n, z, z_stride, s);
    UVX_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(fft_lds_k, dim3(N > LDS_SPAN ? N / LDS_SPAN : 1, B), dim3(THREADS), 0, st, n, max_n, z, z_stride);
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}

}  // namespace aug
}  // namespace uvx
