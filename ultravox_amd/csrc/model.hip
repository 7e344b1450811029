// Host-side orchestration of the hot path behind the C ABI (include/uvx.h): which kernels run, in
// what order, on which slices of the caller's workspace.  No device allocation, no synchronisation.
// Here: log-mel, the Whisper tower, the projector, embedding merge, the optimizer step.  The language model: llm_stack.hip, generate.hip.
#include <algorithm>
#include "host_util.h"
#include "enc_stack.h"
#include "llm_rules.h"
#include "../../include/uvx.h"

namespace {

using namespace uvx;

__global__ void enc_kvlen_k(const int64_t* __restrict__ audio_lens, int32_t* __restrict__ kv_len, int B, int Te) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  // _get_feat_extract_output_lengths: (len - 1) // 2 + 1   (python floor division)
  const long long l = audio_lens[b];
  long long o = (l - 1 >= 0 ? (l - 1) / 2 : -((2 - l) / 2)) + 1;
  kv_len[b] = (int32_t)(o < 0 ? 0 : (o > Te ? Te : o));
}

// ------------------------------------------------------------------ encoder
// the conv stem's buffers in front of the shared layer stack's (enc_stack.h)
struct EncWs {
  void *im2col, *c1;
  int Kp1;
  EncStackWs t;
};
// what the Whisper tower asks of the shared stack: pre-LN layers, key padding and the latency mask, every launch form built so far
EncStackDesc enc_desc(const uvx_config_t& c, int B, int F, bool train) {
  EncStackDesc D = {};
  D.dtype = c.dtype; D.d = c.enc_d; D.heads = c.enc_heads; D.ffn = c.enc_ffn; D.layers = c.enc_layers; D.ln_eps = c.ln_eps;
  D.B = B; D.T = (F - 1) / 2 + 1; D.Tp = rup(D.T, 64);
  D.train = train; D.post_ln = false; D.key_padding = true; D.block = c.enc_block;
  // one or two clips (generate() at B = 1, 2): 1500 / 3000 rows are 48 ... 144 of the 128- / 256-wide tiles on 256 CUs
  D.splitk = !train && c.dtype == DT_BF16 && D.M() > 64 && D.M() <= 3072;
  D.pair_qk = true; D.fuse_gelu = c.dtype == DT_BF16 && opt(UVX_OPT_TOWER_GELU_SEPARATE) != 1; D.mlp_adapters = true;
  return D;
}
EncWs enc_carve(Arena& a, const uvx_config_t& c, const EncStackDesc& D, int F) {
  EncWs w = {};
  const size_t es = esz(c.dtype);
  w.Kp1 = rup(3 * c.n_mels, 64);
  w.im2col = a.take((size_t)D.B * F * w.Kp1 * es);
  w.c1 = a.take((size_t)D.B * (F + 2) * c.enc_d * es);
  w.t = enc_stack_carve(a, D);
  return w;
}

// ------------------------------------------------------------------ projector
struct ProjWs {
  void *stacked, *xn, *h1, *a, *an, *ypre;                                        // forward stash
  void *dy2, *dyT, *anT, *w2T, *d_an, *d_a, *d_h1, *dh1T, *xnT, *w1T, *d_xn;      // backward temps
  float* dwp;                                                                     // per-block partials of the RMSNorm weight gradients (fixed-order sum)
  int J, R, Rp, C8, H, Hh, D;
};
ProjWs proj_carve(Arena& a, const uvx_config_t& c, int B, int Te) {
  ProjWs w;
  const size_t es = esz(c.dtype);
  w.J = (Te + c.stack_factor - 1) / c.stack_factor;
  w.R = B * w.J;
  w.Rp = rup(w.R, 64);
  w.C8 = c.enc_d * c.stack_factor;
  w.H = c.proj_hidden;
  w.Hh = c.proj_act == UVX_PROJ_SWIGLU ? c.proj_hidden / 2 : c.proj_hidden;     // SwiGLU halves the width, a plain activation keeps it
  w.D = c.llm_d;
  w.stacked = a.take((size_t)w.R * w.C8 * es);
  w.xn = a.take((size_t)w.R * w.C8 * es);
  w.h1 = a.take((size_t)w.R * w.H * es);
  w.a = a.take((size_t)w.R * w.Hh * es);
  w.an = c.proj_ln_mid ? a.take((size_t)w.R * w.Hh * es) : w.a;
  w.ypre = c.proj_ln_mid ? nullptr : a.take((size_t)w.R * w.D * es);
  w.dy2 = c.proj_ln_mid ? nullptr : a.take((size_t)w.R * w.D * es);
  w.dyT = a.take((size_t)w.D * w.Rp * es);
  w.anT = a.take((size_t)w.Hh * w.Rp * es);
  w.w2T = a.take((size_t)w.Hh * w.D * es);
  w.d_an = a.take((size_t)w.R * w.Hh * es);
  w.d_a = c.proj_ln_mid ? a.take((size_t)w.R * w.Hh * es) : w.d_an;
  w.d_h1 = a.take((size_t)w.R * w.H * es);
  w.dh1T = a.take((size_t)w.H * w.Rp * es);
  w.xnT = a.take((size_t)w.C8 * w.Rp * es);
  w.w1T = a.take((size_t)w.C8 * w.H * es);
  w.d_xn = a.take((size_t)w.R * w.C8 * es);
  w.dwp = (float*)a.take(sizeof(float) * (size_t)rmsnorm_bwd_dw_scratch_floats(w.R, std::max(std::max(w.C8, w.D), w.Hh)));
  return w;
}

}  // namespace

// =====================================================================================
extern "C" int32_t uvx_logmel(void* stream, const float* pcm, const float* window, const float* tw_cos,
                              const float* tw_sin, const float* mel_fb, float* out, float* scratch, int32_t B, int32_t L,
                              int32_t n_mels, int32_t F_stride) {
  return uvx::logmel((hipStream_t)stream, pcm, window, tw_cos, tw_sin, mel_fb, out, scratch, B, L, n_mels, F_stride);
}

extern "C" size_t uvx_encoder_ws_bytes(const uvx_config_t* cfg, int32_t B, int32_t F) {
  if (!cfg) return 0;
  Arena a(nullptr, 0);
  enc_carve(a, *cfg, enc_desc(*cfg, B, F, false), F);
  return a.off + 256;
}

static int enc_forward(hipStream_t st, const uvx_config_t& c, const uvx_encoder_weights_t* w, const uvx_encoder_lora_t* lora,
                       const void* mel, int mel_is_f32, const int64_t* audio_lens, int B, int F, void* out, void* workspace,
                       size_t ws_bytes) {
  const bool train = lora != nullptr;
  // ultravox_model.py:874-878: the mel length may not exceed max_source_positions * conv strides
  UVX_CHECK(F <= c.enc_max_pos * 2, UVX_ERR_SHAPE,
            "Whisper expects the mel input features to be of length %d or less, but found %d", c.enc_max_pos * 2, F);
  UVX_CHECK(c.enc_d % c.enc_heads == 0, UVX_ERR_SHAPE, "encoder: d=%d not divisible by heads=%d", c.enc_d, c.enc_heads);
  UVX_CHECK(c.enc_block == 0 || (c.enc_max_pos * 2) % c.enc_block == 0, UVX_ERR_SHAPE,
            "audio_latency_block_size %d must divide %d evenly.", c.enc_block, c.enc_max_pos * 2);
  if (train) RC(lora_check(lora, c.enc_layers, nullptr, "encoder LoRA"));
  for (int l = 0; train && l < c.enc_layers; ++l)
    UVX_CHECK(!lora->layers[l].u.a, UVX_ERR_INVALID, "encoder LoRA: layer %d has an up_proj adapter (the Whisper MLP is fc1 / fc2: g / d)", l);
  if (B == 0 || F == 0) return UVX_OK;
  Arena a(workspace, ws_bytes);
  EncStackDesc D = enc_desc(c, B, F, train);
  const EncWs s = enc_carve(a, c, D, F);
  UVX_CHECK(a.fits(), UVX_ERR_WORKSPACE, "encoder_fwd: workspace %zu < %zu bytes", ws_bytes, a.off);
  const int dt = c.dtype, d = c.enc_d, Te = D.T, M = D.M();
  const size_t es = esz(dt);

  // conv1 + GELU (ultravox_model.py:893) as im2col + GEMM, written time-major into a buffer with one
  // zero frame before and after each clip so that conv2 (k3, s2, p1) reads 3 consecutive frames as ONE
  // contiguous K = 3d row: A row t = frames 2t-1..2t+1, row stride 2d.
  RC(im2col_conv1(st, dt, mel, mel_is_f32, s.im2col, B, c.n_mels, F, F, s.Kp1));
  RC(fill_zero(st, s.c1, (long long)B * (F + 2) * d * es));
  {
    GemmDesc g = lin(s.im2col, w->conv1_w, at(s.c1, d, dt), F, d, s.Kp1);
    g.bias = w->conv1_b; g.act = 1; g.batch = B;
    g.sA = (long long)F * s.Kp1; g.sC = (long long)(F + 2) * d;
    RC(gemm(st, dt, g));
  }
  void* x = train ? enc_stack_layer(s.t, 0).x_in : s.t.x;   // the running hidden state (training: lives in the layer stashes)
  {  // conv2 + GELU (:894), permute (:896), + embed_positions[:Te] (:897-899)
    GemmDesc g = lin(s.c1, w->conv2_w, x, Te, d, 3 * d);
    g.lda = 2 * d; g.bias = w->conv2_b; g.act = 1; g.batch = B;
    g.sA = (long long)(F + 2) * d; g.sC = (long long)Te * d;
    g.residual = w->pos; g.ldr = d; g.sR = 0;
    g.splitk_ws = s.t.sk; g.splitk_ws_bytes = s.t.sk_bytes;
    RC(gemm(st, dt, g));
  }
  // key padding mask from audio_len (:915-926)
  if (audio_lens) {
    hipLaunchKernelGGL(enc_kvlen_k, dim3(cdiv(B, 64)), dim3(64), 0, st, audio_lens, s.t.kvlen, B, Te);
    UVX_LAUNCH_CHECK();
    D.kv_len = s.t.kvlen;
  }
  RC(enc_stack_fwd_pre_ln(st, D, s.t, w->layers, lora, x));
  RC(layernorm_fwd(st, dt, x, w->lnf_w, w->lnf_b, out, M, d, c.ln_eps));  // :980
  return UVX_OK;
}

extern "C" int32_t uvx_encoder_fwd(void* stream, const uvx_config_t* cfg, const uvx_encoder_weights_t* w, const void* mel,
                                   int32_t mel_is_f32, const int64_t* audio_lens, int32_t B, int32_t F, void* out,
                                   void* workspace, size_t ws_bytes) {
  RC(check_cfg(cfg));
  UVX_CHECK(w && mel && out && workspace, UVX_ERR_INVALID, "encoder_fwd: null argument");
  return enc_forward((hipStream_t)stream, *cfg, w, nullptr, mel, mel_is_f32, audio_lens, B, F, out, workspace, ws_bytes);
}

extern "C" size_t uvx_encoder_train_ws_bytes(const uvx_config_t* cfg, int32_t B, int32_t F) {
  if (!cfg) return 0;
  Arena a(nullptr, 0);
  enc_carve(a, *cfg, enc_desc(*cfg, B, F, true), F);
  return a.off + 256;
}

extern "C" int32_t uvx_encoder_fwd_train(void* stream, const uvx_config_t* cfg, const uvx_encoder_weights_t* w,
                                         const uvx_encoder_lora_t* lora, const void* mel, int32_t mel_is_f32,
                                         const int64_t* audio_lens, int32_t B, int32_t F, void* out, void* workspace,
                                         size_t ws_bytes) {
  RC(check_cfg(cfg));
  UVX_CHECK(w && lora && mel && out && workspace, UVX_ERR_INVALID, "encoder_fwd_train: null argument");
  return enc_forward((hipStream_t)stream, *cfg, w, lora, mel, mel_is_f32, audio_lens, B, F, out, workspace, ws_bytes);
}

// Backward of the LoRA-adapted encoder: d out [B, Te, d] -> gradients of lora_A / lora_B of q_proj and k_proj in every
// layer (everything else is frozen: apply_lora, ultravox_model.py:690-709).  Walks the stash of uvx_encoder_fwd_train.
extern "C" int32_t uvx_encoder_bwd(void* stream, const uvx_config_t* cfg, const uvx_encoder_weights_t* w,
                                   const uvx_encoder_lora_t* lora, const void* d_out, const int64_t* audio_lens, int32_t B,
                                   int32_t F, const uvx_encoder_lora_grads_t* grads, void* workspace, size_t ws_bytes) {
  RC(check_cfg(cfg));
  UVX_CHECK(w && lora && d_out && grads && grads->layers && workspace, UVX_ERR_INVALID, "encoder_bwd: null argument");
  const uvx_config_t& c = *cfg;
  RC(lora_check(lora, c.enc_layers, grads, "encoder_bwd"));
  hipStream_t st = (hipStream_t)stream;
  if (B == 0 || F == 0) return UVX_OK;
  Arena a(workspace, ws_bytes);
  EncStackDesc D = enc_desc(c, B, F, true);
  D.who = "encoder_bwd";
  const EncWs s = enc_carve(a, c, D, F);
  UVX_CHECK(a.fits(), UVX_ERR_WORKSPACE, "encoder_bwd: workspace %zu < %zu bytes", ws_bytes, a.off);
  D.kv_len = audio_lens ? s.t.kvlen : nullptr;          // written by the forward pass (same audio_lens)
  // ln_post backward: out = LN(x_final); x_final is the running state after the last layer (s.t.x)
  RC(layernorm_bwd(st, c.dtype, d_out, s.t.x, w->lnf_w, nullptr, s.t.dx, D.M(), c.enc_d, c.ln_eps));
  return enc_stack_bwd_pre_ln(st, D, s.t, w->layers, lora, grads);
}

// =====================================================================================
extern "C" size_t uvx_projector_ws_bytes(const uvx_config_t* cfg, int32_t B, int32_t Te) {
  if (!cfg) return 0;
  Arena a(nullptr, 0);
  proj_carve(a, *cfg, B, Te);
  return a.off + 256;
}

extern "C" int32_t uvx_projector_fwd(void* stream, const uvx_config_t* cfg, const uvx_projector_weights_t* w,
                                     const void* enc_out, int32_t B, int32_t Te, void* out, void* workspace,
                                     size_t ws_bytes) {
  RC(check_cfg(cfg));
  UVX_CHECK(w && enc_out && out && workspace, UVX_ERR_INVALID, "projector_fwd: null argument");
  const uvx_config_t& c = *cfg;
  UVX_CHECK(c.proj_hidden % 16 == 0, UVX_ERR_SHAPE, "projector hidden %d must be a multiple of 16", c.proj_hidden);
  UVX_CHECK(c.proj_ln_mid ? (w->ln_mid != nullptr) : (w->ln_post != nullptr), UVX_ERR_INVALID,
            "projector: ln_%s weight missing", c.proj_ln_mid ? "mid" : "post");
  hipStream_t st = (hipStream_t)stream;
  if (B == 0 || Te == 0) return UVX_OK;
  Arena a(workspace, ws_bytes);
  ProjWs s = proj_carve(a, c, B, Te);
  UVX_CHECK(a.fits(), UVX_ERR_WORKSPACE, "projector_fwd: workspace %zu < %zu bytes", ws_bytes, a.off);
  const int dt = c.dtype;
  // _pad_and_stack + ln_pre (:790-791)
  RC(stack_rmsnorm_fwd(st, dt, enc_out, w->ln_pre, s.xn, s.stacked, B, Te, c.enc_d, c.stack_factor, c.proj_eps));
  // a few clips (generate(): 188 rows per 30 s): the two linears are 2 x 16 tiles - split-K (gemm.hip) with the backward's W1^T buffer,
  // idle during any forward, as the scratch for the partial tiles.  Larger batches (training at C2: 1504 rows) keep the plain path.
  auto psk = [&](GemmDesc g) {
    if (dt == DT_BF16 && s.R > 64 && s.R <= 1024) { g.splitk_ws = s.w1T; g.splitk_ws_bytes = (size_t)s.C8 * s.H * esz(dt); }
    return g;
  };
  RC(gemm(st, dt, psk(lin(s.xn, w->w1, s.h1, s.R, s.H, s.C8))));            // linear_1 (:793)
  UVX_CHECK(c.proj_act >= UVX_PROJ_SWIGLU && c.proj_act <= UVX_PROJ_RELU, UVX_ERR_INVALID, "projector: unknown proj_act %d", c.proj_act);
  if (c.proj_act == UVX_PROJ_SWIGLU) RC(swiglu_fwd(st, dt, s.h1, s.a, s.R, s.Hh, /*gate_first=*/0));           // SwiGLU (:739-742, :795)
  else RC(act_fwd(st, dt, s.h1, s.a, (long long)s.R * s.H, c.proj_act - 1));                                   // ACT2FN[projector_act] (:754, :795)
  if (c.proj_ln_mid) {
    RC(rmsnorm_fwd(st, dt, s.a, w->ln_mid, s.an, nullptr, s.R, s.Hh, c.proj_eps));  // ln_mid (:796)
    RC(gemm(st, dt, psk(lin(s.an, w->w2, out, s.R, s.D, s.Hh))));                   // linear_2 (:798)
  } else {
    RC(gemm(st, dt, psk(lin(s.a, w->w2, s.ypre, s.R, s.D, s.Hh))));
    RC(rmsnorm_fwd(st, dt, s.ypre, w->ln_post, out, nullptr, s.R, s.D, c.proj_eps));  // ln_post (:799)
  }
  return UVX_OK;
}

extern "C" int32_t uvx_projector_bwd(void* stream, const uvx_config_t* cfg, const uvx_projector_weights_t* w,
                                     const void* dout, int32_t B, int32_t Te, const uvx_projector_grads_t* gr,
                                     void* d_enc_out, void* workspace, size_t ws_bytes) {
  RC(check_cfg(cfg));
  UVX_CHECK(w && dout && gr && workspace, UVX_ERR_INVALID, "projector_bwd: null argument");
  const uvx_config_t& c = *cfg;
  hipStream_t st = (hipStream_t)stream;
  if (B == 0 || Te == 0) return UVX_OK;
  Arena a(workspace, ws_bytes);
  ProjWs s = proj_carve(a, c, B, Te);
  UVX_CHECK(a.fits(), UVX_ERR_WORKSPACE, "projector_bwd: workspace %zu < %zu bytes", ws_bytes, a.off);
  const int dt = c.dtype;
  const void* dy = dout;
  RC(fill_zero(st, gr->ln_pre, sizeof(float) * s.C8));
  if (c.proj_ln_mid) RC(fill_zero(st, gr->ln_mid, sizeof(float) * s.Hh));
  else {
    RC(fill_zero(st, gr->ln_post, sizeof(float) * s.D));
    RC(rmsnorm_bwd(st, dt, dout, s.ypre, w->ln_post, nullptr, s.dy2, gr->ln_post, s.R, s.D, c.proj_eps, 0, nullptr, s.dwp));
    dy = s.dy2;
  }
  // linear_2: dW2[D, Hh] = dy^T . an ; d_an = dy . W2
  RC(transpose2d(st, dt, dy, s.dyT, s.R, s.D, s.D, s.Rp, 1, 0, 0));
  RC(transpose2d(st, dt, s.an, s.anT, s.R, s.Hh, s.Hh, s.Rp, 1, 0, 0));
  {
    GemmDesc g = lin(s.dyT, s.anT, gr->w2, s.D, s.Hh, s.Rp);
    g.out_f32 = 1;
    RC(gemm(st, dt, g));
  }
  RC(transpose2d(st, dt, w->w2, s.w2T, s.D, s.Hh, s.Hh, s.D, 1, 0, 0));
  RC(gemm(st, dt, lin(dy, s.w2T, s.d_an, s.R, s.Hh, s.D)));
  if (c.proj_ln_mid)
    RC(rmsnorm_bwd(st, dt, s.d_an, s.a, w->ln_mid, nullptr, s.d_a, gr->ln_mid, s.R, s.Hh, c.proj_eps, 0, nullptr, s.dwp));
  if (c.proj_act == UVX_PROJ_SWIGLU) RC(swiglu_bwd(st, dt, s.d_a, s.h1, s.d_h1, s.R, s.Hh, 0));
  else RC(act_bwd(st, dt, s.d_a, s.h1, s.d_h1, (long long)s.R * s.H, c.proj_act - 1));
  // linear_1: dW1[H, C8] = d_h1^T . xn ; d_xn = d_h1 . W1 (only needed for the ln_pre weight gradient)
  RC(transpose2d(st, dt, s.d_h1, s.dh1T, s.R, s.H, s.H, s.Rp, 1, 0, 0));
  RC(transpose2d(st, dt, s.xn, s.xnT, s.R, s.C8, s.C8, s.Rp, 1, 0, 0));
  {
    GemmDesc g = lin(s.dh1T, s.xnT, gr->w1, s.H, s.C8, s.Rp);
    g.out_f32 = 1;
    RC(gemm(st, dt, g));
  }
  RC(transpose2d(st, dt, w->w1, s.w1T, s.H, s.C8, s.C8, s.H, 1, 0, 0));
  RC(gemm(st, dt, lin(s.d_h1, s.w1T, s.d_xn, s.R, s.C8, s.H)));
  if (!d_enc_out) {
    RC(rmsnorm_bwd(st, dt, s.d_xn, s.stacked, w->ln_pre, nullptr, nullptr, gr->ln_pre, s.R, s.C8, c.proj_eps, 0, nullptr, s.dwp));
    return UVX_OK;
  }
  // the encoder trains too (LoRA): d stacked [R, S*C] in place of d_xn, then un-stack: clip b's frames are the first
  // Te * C elements of its J * S * C block (the padded tail frames get no gradient consumer)
  RC(rmsnorm_bwd(st, dt, s.d_xn, s.stacked, w->ln_pre, nullptr, s.d_xn, gr->ln_pre, s.R, s.C8, c.proj_eps, 0, nullptr, s.dwp));
  const size_t es = esz(dt);
  UVX_HIP(hipMemcpy2DAsync(d_enc_out, (size_t)Te * c.enc_d * es, s.d_xn, (size_t)s.J * s.C8 * es, (size_t)Te * c.enc_d * es, B,
                           hipMemcpyDeviceToDevice, st));
  return UVX_OK;
}

// =====================================================================================
extern "C" int32_t uvx_embed_merge(void* stream, const uvx_config_t* cfg, const void* embed_table, const int64_t* input_ids,
                                   const void* audio_embeds, const int64_t* audio_batch_size,
                                   const int64_t* audio_token_start_idx, const int32_t* audio_token_len, int32_t B,
                                   int32_t T, int32_t n_items, int32_t Na, void* inputs_embeds, int32_t* scratch) {
  RC(check_cfg(cfg));
  UVX_CHECK(inputs_embeds && scratch, UVX_ERR_INVALID, "embed_merge: null argument");
  hipStream_t st = (hipStream_t)stream;
  const uvx_config_t& c = *cfg;
  if (input_ids) RC(embed_gather(st, c.dtype, embed_table, input_ids, inputs_embeds, B * T, c.llm_d, c.vocab));
  // Gemma-3: the embedding MODULE scales its rows ([3P] Gemma3TextScaledWordEmbedding: lookup * sqrt(hidden) in the table's dtype);
  // the audio rows merged over them below are not scaled
  if (input_ids && c.llm_flavor == UVX_LLM_GEMMA3) RC(scale_inplace(st, c.dtype, inputs_embeds, (long long)B * T * c.llm_d, gemma_normalizer(c)));
  int32_t* owner = scratch;
  int32_t* item_batch = scratch + (size_t)B * T;
  if (n_items > 0) {
    UVX_CHECK(audio_embeds && audio_batch_size && audio_token_start_idx && audio_token_len, UVX_ERR_INVALID,
              "inputs_embeds/audio_values/audio_token_start_idx/audio_token_len/audio_lens/audio_batch_size must be provided.");
  }
  RC(merge_owner(st, owner, item_batch, audio_batch_size, audio_token_start_idx, audio_token_len, B, n_items, T, Na));
  RC(merge_audio(st, c.dtype, inputs_embeds, audio_embeds, nullptr, owner, item_batch, audio_token_start_idx,
                 audio_token_len, n_items, T, c.llm_d, Na, 0));
  return UVX_OK;
}

extern "C" int32_t uvx_merge_embeds_bwd(void* stream, const uvx_config_t* cfg, const void* d_inputs_embeds,
                                        const int64_t* audio_token_start_idx, const int32_t* audio_token_len, int32_t B,
                                        int32_t T, int32_t n_items, int32_t Na, void* d_audio_embeds,
                                        const int32_t* scratch) {
  RC(check_cfg(cfg));
  hipStream_t st = (hipStream_t)stream;
  const int32_t* owner = scratch;
  const int32_t* item_batch = scratch + (size_t)B * T;
  return merge_audio(st, cfg->dtype, const_cast<void*>(d_inputs_embeds), nullptr, d_audio_embeds, owner, item_batch,
                     audio_token_start_idx, audio_token_len, n_items, T, cfg->llm_d, Na, 1);
}

// =====================================================================================
extern "C" int32_t uvx_adamw_clip_step(void* stream, int32_t state_dtype, void* param, float* master, const float* grad,
                                       void* m, void* v, int64_t n, float max_norm, float lr, float beta1, float beta2,
                                       float eps, float weight_decay, int32_t step, float* scratch) {
  hipStream_t st = (hipStream_t)stream;
  UVX_CHECK(param && grad && m && v && scratch, UVX_ERR_INVALID, "adamw: null argument");
  RC(uvx::grad_sq_norm(st, grad, n, scratch + 1, scratch));
  return uvx::adamw_clip_step(st, state_dtype, param, master, grad, m, v, n, scratch, max_norm, lr, beta1, beta2, eps,
                              weight_decay, step);
}
