// The transformer stack both audio towers end in (Whisper: model.hip; wav2vec2: wav2vec2.hip): per layer LayerNorm, q|k|v projection with
// attention adapters, attention, out_proj + residual, fc1, GELU, fc2 + residual - inference, the LoRA-training forward that stashes per-layer
// activations, and the backward that walks the stash.  Each tower keeps its stem, its argument checks and its final LayerNorm; what differs
// between them inside the stack is spelled out in EncStackDesc.
#pragma once
#include "host_util.h"

namespace uvx {

struct EncStackDesc {
  int dtype, d, heads, ffn, layers;
  float ln_eps;
  int B, T, Tp;                      // clips, frames per clip, frames rounded up to 64
  bool train;                        // the LoRA-training layout: per-layer stashes and the backward's buffers
  bool post_ln;                      // x = LN(x + branch(x)) (wav2vec2 960h) instead of x += branch(LN(x)) (Whisper, wav2vec2 stable_ln)
  bool key_padding;                  // carve kv_len [B] (Whisper: the caller fills it from audio_lens)
  const int32_t* kv_len = nullptr;   // attention's valid keys per clip, or null = all T (Whisper only)
  int block = 0;                     // attention's latency block size, 0 = none (Whisper only)
  bool splitk = false;               // lend the layer GEMMs a split-K scratch (Whisper inference at one or two clips)
  bool pair_qk = false;              // q and k adapters both present: lora_transpose2 / down2 / up2 / wgrad_batch, one launch per pair (Whisper)
  bool fuse_gelu = false;            // training: GELU in the fc1 / fc2-dgrad GEMM epilogue (act 2 / 3: bf16, option 21 != 1, no fc1 / fc2 adapter) (Whisper)
  bool mlp_adapters = false;         // fc1 / fc2 adapters run (else ignored: the tower refuses them); carves t3 / u3 / lbT and a wgrad scratch as wide as ffn (Whisper)
  const char* who = "";              // the backward entry point's name, for its error messages
  int M() const { return B * T; }
};

// per-layer stash of the LoRA-training forward.  x_in = the layer's input (pre-LN: the residual stream; post-LN: the normalised x), x_mid = x_in +
// attention branch, y2 = LN1(x_mid) + feed-forward branch (post-LN only: the input of final_layer_norm), pre = fc1's pre-activation
struct EncLayerStash {
  void *x_in, *qkv, *o, *x_mid, *y2, *pre;
  float* lse;
  void *t, *bqT, *bkT;     // t = [lora_A_q(n) | lora_A_k(n)] [M, 128] (columns 0..r-1 and 64..64+r-1); lora_B^T [r, d] of q / k: every rank-r product reads rows
  void *t2, *bvT, *boT;    // v_proj / out_proj adapters (ABI 17): t2 = [lora_A_v(n) | lora_A_o(attention output)] [M, 128]
  void* t3;                // fc1 / fc2 adapters (ABI 18): [lora_A_fc1(n2) | lora_A_fc2(gelu(fc1))] [M, 128]
};
struct EncStackWs {
  void *x, *n, *qkv, *vt, *o, *f;
  int32_t* kvlen;
  void* sk; size_t sk_bytes;    // split-K scratch of the layer GEMMs (gemm.hip "Split-K"), else null
  // training only
  size_t slot_bytes; EncLayerStash ls0;      // layer 0's stash; layer l's starts slot_bytes * l later
  void *dx, *d_n, *d_o, *d_f, *d_qkv, *qT, *kT, *doT;
  void *u, *u2;       // u = [dq . B_q | dk . B_k], u2 = [d v . B_v | d x_mid . B_o]  [M, 128] each
  void *u3, *lbT;     // u3 = [d pre . B_fc1 | d x_out . B_fc2] [M, 128]; lbT: one MLP adapter's lora_B^T [r, max(d, ffn)] (transposed again in the backward)
  float *delta, *wg;  // wg: lora_wgrad scratch of wg_floats floats
  long long wg_floats;
};
// carves the stack's part of a tower's workspace for the configuration D describes; buffers only one configuration needs exist only for it
EncStackWs enc_stack_carve(Arena& a, const EncStackDesc& D);
EncLayerStash enc_stack_layer(const EncStackWs& w, int l);

// Forward walks over all layers.  Pre-LN: h is the residual stream on entry (inference: updated in place; training: layer 0's stash x_in)
// and where the last layer left it on return.  Post-LN: x = encoder.layer_norm(embeddings) (training: layer 0's stash x_in, else w.n); the
// last layer's final_layer_norm writes `out`.
int enc_stack_fwd_pre_ln(hipStream_t st, const EncStackDesc& D, const EncStackWs& w, const uvx_enc_layer_t* layers, const uvx_encoder_lora_t* lora, void*& h);
int enc_stack_fwd_post_ln(hipStream_t st, const EncStackDesc& D, const EncStackWs& w, const uvx_enc_layer_t* layers, const uvx_encoder_lora_t* lora, void* x,
                          void* out);
// Backward walks over the stash.  Pre-LN: w.dx holds the gradient of the last layer's output.  Post-LN: d_out is the gradient of the last layer's
// final_layer_norm output.  Nothing below layer 0 is trainable, so both stop at its q|k|v input.
int enc_stack_bwd_pre_ln(hipStream_t st, const EncStackDesc& D, const EncStackWs& w, const uvx_enc_layer_t* layers, const uvx_encoder_lora_t* lora,
                         const uvx_encoder_lora_grads_t* grads);
int enc_stack_bwd_post_ln(hipStream_t st, const EncStackDesc& D, const EncStackWs& w, const uvx_enc_layer_t* layers, const uvx_encoder_lora_t* lora,
                          const uvx_encoder_lora_grads_t* grads, const void* d_out);

}  // namespace uvx
