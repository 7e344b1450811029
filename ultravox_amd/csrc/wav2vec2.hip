// Alt audio tower (BASELINE.json config 5): [3P] transformers Wav2Vec2Model.forward behind the C ABI - the AutoModel branch
// of UltravoxModel._create_audio_tower (ultravox_model.py:460-467, :476-485) for facebook/wav2vec2-large-960h-style towers
// (GroupNorm after the first conv layer, bias-free convs, post-LN encoder) and the layer-norm (-lv60) family.  Frozen tower: forward only; under
// apply_lora (audio_model_lora_config.r > 0): uvx_wav2vec2_fwd_train / uvx_wav2vec2_bwd at the end of this file.
//
//   input_values [B, L]  (zero-mean / unit-variance waveform; the `input_values` fallback of ultravox_processing.py:308)
//   -> 7 x Conv1d(+GELU): layer 0 (1 -> C, k 10, s 5) as im2col + GEMM, then GroupNorm(C groups) over time + GELU;
//      layers 1..6 (C -> C, k 3/2, s 2) as GEMMs on a STRIDED VIEW of the time-major activations: output frame t reads the
//      contiguous K = k C run starting at row s t (row stride s C) - no im2col copy for the 146 GFLOP/clip conv stack
//   -> LayerNorm(C) -> Linear(C -> d)
//   -> + GELU(grouped Conv1d(d, d, k 128, pad 64, groups 16))  [weight norm folded at pack time]: per group a GEMM over the
//      contiguous K = 128 x d/G run of a zero-padded per-group copy of the hidden states
//   -> LayerNorm -> layers x { x = LN(x + attn(x));  x = LN(x + fc2(gelu(fc1(x)))) }   -> last_hidden_state [B, T, d]
//
// Rounding points are torch's module-by-module bf16 rounding (conv / norm / activation / linear / residual outputs).
#include "host_util.h"
#include "enc_stack.h"
#include "../../include/uvx.h"

namespace {

using namespace uvx;

constexpr int K0P = 64;     // the first conv's kernel (10 taps) zero padded to one GEMM K-tile
constexpr int GN_ROWS = 512;  // time rows per GroupNorm partial block
constexpr size_t WS_TAIL = 256;  // what uvx_wav2vec2_ws_bytes / _train_ws_bytes report past the last buffer; the entry points ask for all of it

// out[(b T0 + t), k] = round(in[b, s t + k]) for k < k0, 0 for k0 <= k < 64
template <typename T, typename TIN>
__global__ void w2v_im2col0_k(const TIN* __restrict__ in, T* __restrict__ out, long long rows, int T0, int L, int k0, int s0) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // one thread per (row, 8-column group)
  if (i >= rows * (K0P / 8)) return;
  const long long row = i / (K0P / 8);
  const int c0 = (int)(i % (K0P / 8)) * 8;
  const int b = (int)(row / T0), t = (int)(row % T0);
  const TIN* src = in + (long long)b * L + (long long)t * s0;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = c0 + j;
    v[j] = k < k0 ? (float)src[k] : 0.f;
    if (sizeof(TIN) == 2) v[j] = k < k0 ? bf2f(((const bf16_t*)src)[k]) : 0.f;
  }
  st8<T>(out + row * K0P + c0, v);
}

// GroupNorm(num_groups = C): per (clip, channel) statistics over the T0 frames of a time-major [B, T0, C] tensor.
// pass 1: each block takes GN_ROWS rows for all channels and leaves the chunk's (mean, sum of squared deviations from it); pass 2: merges the chunks
// in double.  A chunk is walked twice: a plain sum gives its rough mean, then the sums run over the deviations from that.  E[x^2] - mean^2 over
// plain sums loses the variance of a channel whose offset is many times its spread over time (a conv bias of 10 .. 30 spreads, 1799 rows, f32: rstd
// off by 6e-5 .. 1e-4); deviations from the chunk's first row would lose it the same way where that row is an outlier.
// Block = (C / 8, ny): thread (tx, ty) walks rows r0 + ty, r0 + ty + ny, .. of 8 channels; the ny partial sums of a channel meet in LDS (red: ny C
// floats) and are added in the order of ty by every thread alike.
template <typename T>
__global__ void w2v_gn_partial_k(const T* __restrict__ x, float* __restrict__ part, int T0, int C, int nchunk) {
  extern __shared__ float red[];
  const int b = blockIdx.y, ch = blockIdx.x, ty = threadIdx.y, ny = blockDim.y;
  const int c = threadIdx.x * 8;
  const int r0 = ch * GN_ROWS, r1 = min(T0, r0 + GN_ROWS);
  const T* p0 = x + ((long long)b * T0 + r0 + ty) * C + c;
  const float inv_n = 1.f / (float)(r1 - r0);
  float m[8], s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { m[j] = 0.f; s[j] = 0.f; q[j] = 0.f; }
  const T* p = p0;
  for (int r = r0 + ty; r < r1; r += ny, p += (long long)ny * C) {
    float v[8];
    ld8<T>(p, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] += v[j];
  }
  auto block_sum = [&](float* a) {      // a[j] <- the sum over ty of a[j], the same bits in every thread of the channel
#pragma unroll
    for (int j = 0; j < 8; ++j) red[ty * C + c + j] = a[j];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float t = 0.f;
      for (int y = 0; y < ny; ++y) t += red[y * C + c + j];
      a[j] = t;
    }
    __syncthreads();
  };
  block_sum(m);
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j] *= inv_n;
  p = p0;
  for (int r = r0 + ty; r < r1; r += ny, p += (long long)ny * C) {
    float v[8];
    ld8<T>(p, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float dv = v[j] - m[j];
      s[j] += dv; q[j] += dv * dv;
    }
  }
  block_sum(s);
  block_sum(q);
  if (ty != 0) return;
  float* o = part + (((long long)b * nchunk + ch) * C + c) * 2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    o[2 * j] = m[j] + s[j] * inv_n;
    o[2 * j + 1] = fmaxf(q[j] - s[j] * s[j] * inv_n, 0.f);
  }
}
// rows of a chunk that one block walks side by side: as many as 1024 threads allow, 8 at the most
inline int gn_lanes(int C) {
  const int n = 1024 / (C / 8);
  return n < 1 ? 1 : n > 8 ? 8 : n;
}
__global__ void w2v_gn_final_k(const float* __restrict__ part, float* __restrict__ stat, int T0, int C, int nchunk, float eps) {
  const int b = blockIdx.y, c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  double n = 0., mean = 0., m2 = 0.;
  for (int ch = 0; ch < nchunk; ++ch) {      // the pairwise update of (count, mean, sum of squared deviations)
    const float* p = part + (((long long)b * nchunk + ch) * C + c) * 2;
    const double nb = min(GN_ROWS, T0 - ch * GN_ROWS), delta = (double)p[0] - mean, nt = n + nb;
    mean += delta * nb / nt;
    m2 += (double)p[1] + delta * delta * n * nb / nt;
    n = nt;
  }
  const double var = m2 / T0;   // biased variance, as torch.nn.GroupNorm
  stat[((long long)b * C + c) * 2] = (float)mean;
  stat[((long long)b * C + c) * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
}
// x = round(gelu(round((x - mean) rstd gamma + beta)))  in place
template <typename T>
__global__ void w2v_gn_gelu_k(T* __restrict__ x, const float* __restrict__ stat, const T* __restrict__ gamma,
                              const T* __restrict__ beta, long long n8, int T0, int C) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const int cv = C / 8;
  const int c = (int)(i % cv) * 8;
  const int b = (int)(i / cv / T0);
  float v[8], g[8], be[8];
  ld8<T>(x + i * 8, v);
  ld8<T>(gamma + c, g);
  ld8<T>(beta + c, be);
  const float* st = stat + ((long long)b * C + c) * 2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float y = rnd<T>((v[j] - st[2 * j]) * st[2 * j + 1] * g[j] + be[j]);
    v[j] = sizeof(T) == 2 ? gelu_fast(y) : gelu_erf(y);
  }
  st8<T>(x + i * 8, v);
}

// xg[b][g][r][c] = h[b, r - K/2, g dg + c] for K/2 <= r < K/2 + T, else 0;  r in [0, T + K)
template <typename T>
__global__ void w2v_pos_pack_k(const T* __restrict__ h, T* __restrict__ xg, long long n8, int Tn, int d, int G, int K) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const int dg = d / G, cv = dg / 8, R = Tn + K;
  const int c = (int)(i % cv) * 8;
  long long rest = i / cv;
  const int r = (int)(rest % R); rest /= R;
  const int g = (int)(rest % G);
  const int b = (int)(rest / G);
  float v[8];
  const int t = r - K / 2;
  if (t >= 0 && t < Tn) ld8<T>(h + ((long long)b * Tn + t) * d + g * dg + c, v);
  else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
  }
  st8<T>(xg + i * 8, v);
}
// h = round(h + round(gelu(round(acc + bias))))   (conv output, activation and residual add each rounded once)
template <typename T>
__global__ void w2v_pos_finish_k(T* __restrict__ h, const float* __restrict__ acc, const T* __restrict__ bias, long long n8, int d) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n8) return;
  const int c = (int)(i % (d / 8)) * 8;
  float x[8], a[8], bv[8];
  ld8<T>(h + i * 8, x);
  ld8<float>(acc + i * 8, a);
  ld8<T>(bias + c, bv);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float y = rnd<T>(a[j] + bv[j]);
    x[j] += rnd<T>(sizeof(T) == 2 ? gelu_fast(y) : gelu_erf(y));
  }
  st8<T>(h + i * 8, x);
}

inline unsigned g1(long long n, int b) { return (unsigned)((n + b - 1) / b); }

struct W2vWs {
  int T[9];          // frames after conv layer i
  int Tn, nchunk;
  void *im2col, *bufA, *bufB, *xg;
  float *part, *stat, *acc;
  EncStackWs t;      // the shared layer stack's buffers (enc_stack.h); t.x = the hidden states the stem leaves
};

int frames(const uvx_w2v_config_t& c, int L, int* T) {
  int n = L;
  for (int i = 0; i < c.n_conv; ++i) {
    if (n < c.conv_kernel[i]) return -1;
    n = (n - c.conv_kernel[i]) / c.conv_stride[i] + 1;
    T[i] = n;
  }
  return n;
}

// what this tower asks of the shared stack: either layer form, no mask, the attention adapters only, one launch per adapter product and GELU pass
EncStackDesc stack_desc(const uvx_w2v_config_t& c, int B, int Tn, bool train) {
  EncStackDesc D = {};
  D.dtype = c.dtype; D.d = c.d; D.heads = c.heads; D.ffn = c.ffn; D.layers = c.layers; D.ln_eps = c.ln_eps;
  D.B = B; D.T = Tn; D.Tp = rup(Tn, 64);
  D.train = train; D.post_ln = !c.stable_ln; D.key_padding = false;
  return D;
}
W2vWs carve(Arena& a, const uvx_w2v_config_t& c, int B, int L, bool train = false) {
  W2vWs w = {};
  w.Tn = frames(c, L, w.T);
  if (w.Tn <= 0) return w;
  const size_t es = esz(c.dtype);
  const int C = c.conv_dim, d = c.d;
  w.nchunk = (w.T[0] + GN_ROWS - 1) / GN_ROWS;
  w.im2col = a.take((size_t)B * w.T[0] * K0P * es);
  w.bufA = a.take((size_t)B * w.T[0] * C * es);
  w.bufB = a.take((size_t)B * (c.n_conv > 1 ? w.T[1] : 1) * C * es);
  w.part = (float*)a.take(sizeof(float) * (size_t)B * w.nchunk * C * 2);
  w.stat = (float*)a.take(sizeof(float) * (size_t)B * C * 2);
  w.xg = a.take((size_t)B * c.pos_groups * (w.Tn + c.pos_k) * (d / c.pos_groups) * es);
  w.acc = (float*)a.take(sizeof(float) * (size_t)B * w.Tn * d);
  w.t = enc_stack_carve(a, stack_desc(c, B, w.Tn, train));
  return w;
}

int check(const uvx_w2v_config_t* c) {
  UVX_CHECK(c != nullptr, UVX_ERR_INVALID, "wav2vec2: null config");
  UVX_CHECK(c->dtype == DT_BF16 || c->dtype == DT_F32, UVX_ERR_INVALID, "wav2vec2: bad dtype %d", c->dtype);
  UVX_CHECK(c->n_conv >= 2 && c->n_conv <= 8, UVX_ERR_SHAPE, "wav2vec2: %d conv layers (2..8)", c->n_conv);
  UVX_CHECK(c->conv_dim % 64 == 0 && c->conv_dim <= 8192, UVX_ERR_SHAPE, "wav2vec2: conv_dim %d must be a multiple of 64", c->conv_dim);
  UVX_CHECK(c->conv_kernel[0] <= K0P, UVX_ERR_SHAPE, "wav2vec2: first conv kernel %d > %d", c->conv_kernel[0], K0P);
  UVX_CHECK(!c->feat_norm_layer || c->conv_dim % 8 == 0, UVX_ERR_SHAPE, "wav2vec2: conv_dim %d", c->conv_dim);
  UVX_CHECK(c->d % c->heads == 0 && c->d % c->pos_groups == 0 && (c->d / c->pos_groups) % 8 == 0 &&
                (c->pos_k * (c->d / c->pos_groups)) % 64 == 0,
            UVX_ERR_SHAPE, "wav2vec2: hidden %d / heads %d / positional-conv groups %d, kernel %d unsupported", c->d, c->heads,
            c->pos_groups, c->pos_k);
  return UVX_OK;
}

// only the attention projections' adapters are built for this tower (EncStackDesc::mlp_adapters = false): forward and backward both refuse the rest
int refuse_mlp_adapters(const uvx_encoder_lora_t* lora, int layers) {
  for (int l = 0; l < layers; ++l)
    UVX_CHECK(!lora->layers[l].g.a && !lora->layers[l].u.a && !lora->layers[l].d.a, UVX_ERR_UNSUPPORTED,
              "wav2vec2 LoRA: layer %d has a feed-forward adapter (the attention projections q / k / v / out_proj are built for this tower)", l);
  return UVX_OK;
}

}  // namespace

extern "C" int32_t uvx_wav2vec2_frames(const uvx_w2v_config_t* cfg, int32_t L) {
  if (!cfg) return -1;
  int T[9];
  return frames(*cfg, L, T);
}

extern "C" size_t uvx_wav2vec2_ws_bytes(const uvx_w2v_config_t* cfg, int32_t B, int32_t L) {
  if (!cfg) return 0;
  Arena a(nullptr, 0);
  carve(a, *cfg, B, L);
  return a.off + WS_TAIL;
}

// lora != NULL: the LoRA-training forward (apply_lora on the AutoModel tower, ultravox_model.py:460-467, 690-709) - adapters on the attention
// projections and a per-layer stash for uvx_wav2vec2_bwd; the feature encoder, projection and positional conv have no adapter and stay forward-only
static int w2v_forward(void* stream, const uvx_w2v_config_t* cfg, const uvx_w2v_weights_t* w, const uvx_encoder_lora_t* lora, const void* input_values,
                       int32_t values_is_f32, int32_t B, int32_t L, void* out, void* workspace, size_t ws_bytes) {
  RC(check(cfg));
  UVX_CHECK(w && w->layers && input_values && out && workspace, UVX_ERR_INVALID, "wav2vec2_fwd: null argument");
  const uvx_w2v_config_t& c = *cfg;
  hipStream_t st = (hipStream_t)stream;
  const bool train = lora != nullptr;
  if (train) RC(lora_check(lora, c.layers, nullptr, "wav2vec2 LoRA"));
  if (train) RC(refuse_mlp_adapters(lora, c.layers));
  for (int i = 0; i < c.n_conv; ++i) {
    UVX_CHECK(!c.conv_bias || w->conv_b[i], UVX_ERR_INVALID, "wav2vec2_fwd: conv_bias is set but conv layer %d has no bias", i);
    UVX_CHECK(!c.feat_norm_layer || (w->conv_ln_w[i] && w->conv_ln_b[i]), UVX_ERR_INVALID, "wav2vec2_fwd: conv layer %d has no layer norm", i);
  }
  UVX_CHECK(c.feat_norm_layer || (w->gn_w && w->gn_b), UVX_ERR_INVALID, "wav2vec2_fwd: the first conv layer's GroupNorm weights are missing");
  if (B == 0) return UVX_OK;
  Arena a(workspace, ws_bytes);
  W2vWs s = carve(a, c, B, L, train);
  UVX_CHECK(s.Tn > 0, UVX_ERR_SHAPE, "wav2vec2_fwd: %d samples are shorter than the conv stack's receptive field", L);
  UVX_CHECK(ws_bytes >= a.off + WS_TAIL, UVX_ERR_WORKSPACE, "wav2vec2_fwd: workspace %zu < %zu bytes", ws_bytes, a.off + WS_TAIL);
  const int dt = c.dtype, C = c.conv_dim, d = c.d, M = B * s.Tn, Tn = s.Tn;
  const EncStackDesc D = stack_desc(c, B, Tn, train);
  UVX_CHECK(dt == DT_BF16 || values_is_f32, UVX_ERR_INVALID, "wav2vec2_fwd: f32 mode needs f32 input_values");

  // ---- feature encoder ----
  {
    const long long rows = (long long)B * s.T[0], n = rows * (K0P / 8);
    if (dt == DT_BF16) {
      if (values_is_f32) hipLaunchKernelGGL((w2v_im2col0_k<bf16_t, float>), dim3(g1(n, 256)), dim3(256), 0, st, (const float*)input_values, (bf16_t*)s.im2col, rows, s.T[0], L, c.conv_kernel[0], c.conv_stride[0]);
      else hipLaunchKernelGGL((w2v_im2col0_k<bf16_t, bf16_t>), dim3(g1(n, 256)), dim3(256), 0, st, (const bf16_t*)input_values, (bf16_t*)s.im2col, rows, s.T[0], L, c.conv_kernel[0], c.conv_stride[0]);
    } else {
      hipLaunchKernelGGL((w2v_im2col0_k<float, float>), dim3(g1(n, 256)), dim3(256), 0, st, (const float*)input_values, (float*)s.im2col, rows, s.T[0], L, c.conv_kernel[0], c.conv_stride[0]);
    }
    UVX_LAUNCH_CHECK();
    {
      GemmDesc g0 = lin(s.im2col, w->conv0_w, s.bufA, (int)rows, C, K0P);
      g0.bias = c.conv_bias ? w->conv_b[0] : nullptr;
      RC(gemm(st, dt, g0));
    }
    const dim3 gp(s.nchunk, B);
    const long long n8 = rows * C / 8;
    if (c.feat_norm_layer) {      // Wav2Vec2LayerNormConvLayer: conv -> LayerNorm over the channels -> GELU, each a rounded tensor
      RC(layernorm_fwd(st, dt, s.bufA, w->conv_ln_w[0], w->conv_ln_b[0], s.bufA, (int)rows, C, 1e-5f));
      RC(gelu_fwd(st, dt, s.bufA, s.bufA, rows * C));
    } else if (dt == DT_BF16) {      // GroupNorm over time (per clip and channel) + GELU
      hipLaunchKernelGGL(w2v_gn_partial_k<bf16_t>, gp, dim3(C / 8, gn_lanes(C)), sizeof(float) * gn_lanes(C) * C, st, (const bf16_t*)s.bufA, s.part, s.T[0], C, s.nchunk);
      hipLaunchKernelGGL(w2v_gn_final_k, dim3(g1(C, 128), B), dim3(128), 0, st, s.part, s.stat, s.T[0], C, s.nchunk, 1e-5f);
      hipLaunchKernelGGL(w2v_gn_gelu_k<bf16_t>, dim3(g1(n8, 256)), dim3(256), 0, st, (bf16_t*)s.bufA, s.stat, (const bf16_t*)w->gn_w, (const bf16_t*)w->gn_b, n8, s.T[0], C);
    } else {
      hipLaunchKernelGGL(w2v_gn_partial_k<float>, gp, dim3(C / 8, gn_lanes(C)), sizeof(float) * gn_lanes(C) * C, st, (const float*)s.bufA, s.part, s.T[0], C, s.nchunk);
      hipLaunchKernelGGL(w2v_gn_final_k, dim3(g1(C, 128), B), dim3(128), 0, st, s.part, s.stat, s.T[0], C, s.nchunk, 1e-5f);
      hipLaunchKernelGGL(w2v_gn_gelu_k<float>, dim3(g1(n8, 256)), dim3(256), 0, st, (float*)s.bufA, s.stat, (const float*)w->gn_w, (const float*)w->gn_b, n8, s.T[0], C);
    }
    UVX_LAUNCH_CHECK();
  }
  void* cur = s.bufA;
  void* nxt = s.bufB;
  for (int i = 1; i < c.n_conv; ++i) {   // Conv1d(C, C, k, s) + GELU on the strided view (no bias: conv_bias = False)
    UVX_CHECK(w->conv_w[i] != nullptr, UVX_ERR_INVALID, "wav2vec2_fwd: conv layer %d has no weights", i);
    const int k = c.conv_kernel[i], sd = c.conv_stride[i];
    GemmDesc g = lin(cur, w->conv_w[i], nxt, s.T[i], C, k * C);
    g.lda = sd * C; g.act = c.feat_norm_layer ? 0 : 1; g.batch = B;
    g.sA = (long long)s.T[i - 1] * C; g.sC = (long long)s.T[i] * C;
    g.bias = c.conv_bias ? w->conv_b[i] : nullptr;
    RC(gemm(st, dt, g));
    if (c.feat_norm_layer) {
      RC(layernorm_fwd(st, dt, nxt, w->conv_ln_w[i], w->conv_ln_b[i], nxt, B * s.T[i], C, 1e-5f));
      RC(gelu_fwd(st, dt, nxt, nxt, (long long)B * s.T[i] * C));
    }
    void* t = cur; cur = nxt; nxt = t;
  }
  // ---- feature projection: LayerNorm(C) -> Linear(C, d) ----
  RC(layernorm_fwd(st, dt, cur, w->fp_ln_w, w->fp_ln_b, nxt, M, C, c.ln_eps));
  {
    GemmDesc g = lin(nxt, w->fp_w, s.t.x, M, d, C);
    g.bias = w->fp_b;
    RC(gemm(st, dt, g));
  }
  // ---- positional conv embedding (grouped, k = pos_k, "same" padding, last frame dropped for even k) ----
  {
    const int G = c.pos_groups, dg = d / G, K = c.pos_k, R = Tn + K;
    const long long n8 = (long long)B * G * R * dg / 8;
    if (dt == DT_BF16) hipLaunchKernelGGL(w2v_pos_pack_k<bf16_t>, dim3(g1(n8, 256)), dim3(256), 0, st, (const bf16_t*)s.t.x, (bf16_t*)s.xg, n8, Tn, d, G, K);
    else hipLaunchKernelGGL(w2v_pos_pack_k<float>, dim3(g1(n8, 256)), dim3(256), 0, st, (const float*)s.t.x, (float*)s.xg, n8, Tn, d, G, K);
    UVX_LAUNCH_CHECK();
    for (int b = 0; b < B; ++b) {   // one batched GEMM per clip: batch = groups (their weights differ, the clip's do not)
      GemmDesc g = lin(at(s.xg, (size_t)b * G * R * dg, dt), w->pos_w, s.acc + (size_t)b * Tn * d, Tn, dg, K * dg);
      g.lda = dg; g.ldc = d; g.out_f32 = 1; g.batch = G;
      g.sA = (long long)R * dg; g.sB = (long long)dg * K * dg; g.sC = dg;
      RC(gemm(st, dt, g));
    }
    const long long m8 = (long long)M * d / 8;
    if (dt == DT_BF16) hipLaunchKernelGGL(w2v_pos_finish_k<bf16_t>, dim3(g1(m8, 256)), dim3(256), 0, st, (bf16_t*)s.t.x, s.acc, (const bf16_t*)w->pos_b, m8, d);
    else hipLaunchKernelGGL(w2v_pos_finish_k<float>, dim3(g1(m8, 256)), dim3(256), 0, st, (float*)s.t.x, s.acc, (const float*)w->pos_b, m8, d);
    UVX_LAUNCH_CHECK();
  }
  if (c.stable_ln) {
    // ---- encoder, do_stable_layer_norm = True ([3P] Wav2Vec2EncoderStableLayerNorm / ...EncoderLayerStableLayerNorm): pre-LN layers,
    //      encoder.layer_norm after the last one.  Training: the residual stream starts in layer 0's stash and ends in s.t.x (kept for the backward) ----
    void* h = s.t.x;
    if (train && c.layers > 0) {
      h = enc_stack_layer(s.t, 0).x_in;
      UVX_HIP(hipMemcpyAsync(h, s.t.x, (size_t)M * d * esz(dt), hipMemcpyDeviceToDevice, st));
    }
    RC(enc_stack_fwd_pre_ln(st, D, s.t, w->layers, lora, h));
    return layernorm_fwd(st, dt, h, w->ln_w, w->ln_b, out, M, d, c.ln_eps);
  }
  // ---- encoder (post-LN, do_stable_layer_norm = False): encoder.layer_norm in front of the layers; the last layer writes `out` ----
  void* x = train && c.layers > 0 ? enc_stack_layer(s.t, 0).x_in : s.t.n;
  RC(layernorm_fwd(st, dt, s.t.x, w->ln_w, w->ln_b, x, M, d, c.ln_eps));
  if (c.layers == 0) UVX_HIP(hipMemcpyAsync(out, x, (size_t)M * d * esz(dt), hipMemcpyDeviceToDevice, st));
  return enc_stack_fwd_post_ln(st, D, s.t, w->layers, lora, x, out);
}

extern "C" int32_t uvx_wav2vec2_fwd(void* stream, const uvx_w2v_config_t* cfg, const uvx_w2v_weights_t* w, const void* input_values,
                                    int32_t values_is_f32, int32_t B, int32_t L, void* out, void* workspace, size_t ws_bytes) {
  return w2v_forward(stream, cfg, w, nullptr, input_values, values_is_f32, B, L, out, workspace, ws_bytes);
}

extern "C" size_t uvx_wav2vec2_train_ws_bytes(const uvx_w2v_config_t* cfg, int32_t B, int32_t L) {
  if (!cfg) return 0;
  Arena a(nullptr, 0);
  carve(a, *cfg, B, L, true);
  return a.off + WS_TAIL;
}

extern "C" int32_t uvx_wav2vec2_fwd_train(void* stream, const uvx_w2v_config_t* cfg, const uvx_w2v_weights_t* w, const uvx_encoder_lora_t* lora,
                                          const void* input_values, int32_t values_is_f32, int32_t B, int32_t L, void* out, void* workspace,
                                          size_t ws_bytes) {
  UVX_CHECK(lora != nullptr, UVX_ERR_INVALID, "wav2vec2_fwd_train: null LoRA descriptor");
  return w2v_forward(stream, cfg, w, lora, input_values, values_is_f32, B, L, out, workspace, ws_bytes);
}

// Backward of the LoRA-adapted wav2vec2 encoder: d last_hidden_state [B, frames, d] -> the adapters' gradients in every layer (everything else is
// frozen: apply_lora, ultravox_model.py:690-709).  Walks the stash of uvx_wav2vec2_fwd_train; nothing below layer 0's q|k|v input is trainable, so the
// walk stops there (no gradient for the positional conv / feature projection / feature encoder).
extern "C" int32_t uvx_wav2vec2_bwd(void* stream, const uvx_w2v_config_t* cfg, const uvx_w2v_weights_t* w, const uvx_encoder_lora_t* lora,
                                    const void* d_out, int32_t B, int32_t L, const uvx_encoder_lora_grads_t* grads, void* workspace, size_t ws_bytes) {
  RC(check(cfg));
  UVX_CHECK(w && w->layers && lora && d_out && grads && grads->layers && workspace, UVX_ERR_INVALID, "wav2vec2_bwd: null argument");
  const uvx_w2v_config_t& c = *cfg;
  RC(lora_check(lora, c.layers, grads, "wav2vec2_bwd"));
  RC(refuse_mlp_adapters(lora, c.layers));
  hipStream_t st = (hipStream_t)stream;
  if (B == 0 || c.layers == 0) return UVX_OK;
  Arena a(workspace, ws_bytes);
  W2vWs s = carve(a, c, B, L, true);
  UVX_CHECK(s.Tn > 0, UVX_ERR_SHAPE, "wav2vec2_bwd: %d samples are shorter than the conv stack's receptive field", L);
  UVX_CHECK(ws_bytes >= a.off + WS_TAIL, UVX_ERR_WORKSPACE, "wav2vec2_bwd: workspace %zu < %zu bytes", ws_bytes, a.off + WS_TAIL);
  EncStackDesc D = stack_desc(c, B, s.Tn, true);
  D.who = "wav2vec2_bwd";
  if (c.stable_ln) {
    // out = encoder.layer_norm(h_final); h_final = s.t.x (left there by the forward)
    RC(layernorm_bwd(st, c.dtype, d_out, s.t.x, w->ln_w, nullptr, s.t.dx, D.M(), c.d, c.ln_eps));
    return enc_stack_bwd_pre_ln(st, D, s.t, w->layers, lora, grads);
  }
  return enc_stack_bwd_post_ln(st, D, s.t, w->layers, lora, grads, d_out);
}
