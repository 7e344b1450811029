// The per-layer rules of the language model that training (llm_stack.hip) and inference (generate.hip: prefill, chunked prefill, decode) must
// agree on - each written once: attention scale, a layer's rotary table and sliding window, the attention descriptor over a fused q|k|v buffer,
// the Gemma-3 weight check, the embedding scale.  A copy that drifts makes the two paths disagree for Gemma-3 or Mistral only.
#pragma once
#include <math.h>
#include <algorithm>
#include "host_util.h"

namespace uvx {

// [3P] transformers 4.51.3 GemmaModel.forward: normalizer = torch.tensor(hidden_size ** 0.5, dtype=hidden_states.dtype) -
// the square root is ROUNDED to the model dtype before it multiplies (55.5 for hidden_size 3072 in bf16)
inline float gemma_normalizer(const uvx_config_t& c) {
  const float n = sqrtf((float)c.llm_d);
  return c.dtype == DT_BF16 ? bf2f(f2bf(n)) : n;
}
// the merged inputs_embeds enter the stack: copied to `dst`, Gemma (4.51.3: inside the model) scales them
inline int embed_in(hipStream_t st, const uvx_config_t& c, void* dst, const void* inputs_embeds, long long rows) {
  UVX_HIP(hipMemcpyAsync(dst, inputs_embeds, (size_t)rows * c.llm_d * esz(c.dtype), hipMemcpyDeviceToDevice, st));
  return c.llm_flavor == UVX_LLM_GEMMA ? scale_inplace(st, c.dtype, dst, rows * c.llm_d, gemma_normalizer(c)) : UVX_OK;
}

inline float attn_scale_of(const uvx_config_t& c) { return c.llm_attn_scale > 0.f ? c.llm_attn_scale : 1.0f / sqrtf((float)c.llm_head_dim); }
// a sliding-window layer (Gemma-3's local layers, every Mistral layer)
inline bool layer_is_local(const uvx_llm_weights_t* w, int l) { return w->layer_local && w->layer_local[l]; }
// (Gemma-3: the sliding-window layers rotate with their own table)
inline const float* rope_of(const uvx_config_t& c, const uvx_llm_weights_t* w, int l) {
  return c.llm_flavor == UVX_LLM_GEMMA3 && layer_is_local(w, l) ? w->rope_cos_sin_local : w->rope_cos_sin;
}
// AttnDesc::window of layer l over a key range of length T: a sequence LONGER than the window (up to the window it is plain causal attention)
inline int window_of(const uvx_config_t& c, const uvx_llm_weights_t* w, int l, int T) {
  return c.llm_window > 0 && T > c.llm_window && layer_is_local(w, l) ? c.llm_window : 0;
}
// Decode has no AttnDesc: its one query is the newest of cur_len + 1 cache slots, and the slots of a sequence are contiguous, so the same window
// is a clamp of the first visible slot rather than a mask width
inline int decode_first_slot(const uvx_config_t& c, const uvx_llm_weights_t* w, int l, int cur_len) {
  return c.llm_window > 0 && layer_is_local(w, l) ? std::max(0, cur_len + 1 - c.llm_window) : 0;
}
// causal GQA attention over a fused q|k|v buffer [B * T, QKV] with output rows of OD; the caller sets what differs: vt, o, lse, kv_start,
// kv_len, q_begin, window, block
inline AttnDesc causal_gqa_desc(const uvx_config_t& c, const void* qkv, int B, int T, int Tp, int QKV, int OD) {
  AttnDesc ad;
  const int Hq = c.llm_heads, Hkv = c.llm_kv_heads, dh = c.llm_head_dim;
  ad.q = qkv; ad.k = at(qkv, (size_t)Hq * dh, c.dtype); ad.v = at(qkv, (size_t)(Hq + Hkv) * dh, c.dtype);
  ad.B = B; ad.T = T; ad.Tp = Tp; ad.Hq = Hq; ad.Hkv = Hkv; ad.D = dh;
  ad.ldq = ad.ldk = ad.ldv = QKV; ad.ldo = OD; ad.causal = 1;
  ad.scale = attn_scale_of(c);
  return ad;
}
// Gemma-3: post norms present and a local rotary table where layers are flagged
inline int gemma3_check(const uvx_config_t& c, const uvx_llm_weights_t* w) {
  if (c.llm_flavor != UVX_LLM_GEMMA3) return UVX_OK;
  bool any_local = false;
  for (int l = 0; l < c.llm_layers; ++l) {
    UVX_CHECK(w->layers[l].ln1_post && w->layers[l].ln2_post, UVX_ERR_INVALID, "llm: Gemma-3 layer %d has no post norms", l);
    any_local = any_local || layer_is_local(w, l);
  }
  UVX_CHECK(!any_local || w->rope_cos_sin_local, UVX_ERR_INVALID, "llm: Gemma-3 sliding-window layers need rope_cos_sin_local");
  return UVX_OK;
}

}  // namespace uvx
