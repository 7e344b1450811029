// The language model's training stack (llm_stack.hip): the forward that stashes per-layer activations, the activation-gradient backward that
// walks the stash, and the uvx_llm_* entry points in front of them.  This header holds what the two walks share: the call descriptor and the
// ONE description of the workspace - every buffer is declared once, with its size and how a batch slice moves it; the carve (with its
// dry-run size), the per-layer offset and the batch-slice view below all come from that declaration.
#pragma once
#include <algorithm>
#include "host_util.h"

namespace uvx {

// One call of llm_forward / llm_backward: what every entry point passes, then the modes (all off by default).
struct LlmCallDesc {
  hipStream_t st = nullptr;
  const uvx_config_t* cfg = nullptr;
  const uvx_llm_weights_t* w = nullptr;
  int B = 0, T = 0;
  void* workspace = nullptr;
  size_t ws_bytes = 0;
  const void* inputs_embeds = nullptr;         // forward: [B, T, D]
  const int64_t* attention_mask = nullptr;     // forward: [B, T] or null = every key valid (the key ranges stay in the workspace for the backward)
  void* d_inputs_embeds = nullptr;             // backward: [B, T, D]
  const int64_t* labels = nullptr;   // forward: the CE loss is computed (needs `loss`); backward: d logits = d CE, else the workspace already holds d logits (KL)
  float* loss = nullptr;             // forward: the loss output
  void* logits = nullptr;            // forward: the caller's full logits [B, T, vocab]
  int save_for_bwd = 0;              // forward: a stash slot per layer and the backward's buffers (else two alternating slots)
  const int32_t* rows = nullptr;     // forward (uvx_llm_fwd_rows): the LM head is evaluated only for the listed positions (device list, ascending,
  int n_rows = 0;                    //   host-known length); the compact logits stay in the workspace with the list, like the supervised-row CE path,
  void* logits_rows = nullptr;       //   and are copied here if given
  const uvx_encoder_lora_t* lora = nullptr;             // LLM LoRA: the adapters run (forward and backward)
  const uvx_encoder_lora_grads_t* lgrads = nullptr;     // backward under LoRA: where the adapter gradients go
  bool top_rows = false;             // the training pair (uvx_llm_fwd_train / _bwd_train): the last layer's row-wise half on the supervised rows only
  bool compact_in_place = false;     // backward: the workspace holds d loss / d logits for the compact rows of its row list (uvx_llm_kl_loss_rows)
  int first_pos = 0;                 // backward: the caller needs no gradient below this position of any sequence
  float grad_scale = 1.0f;           // backward: scales d CE
};

struct LlmLayerStash {
  void *x_in, *qkv, *o, *x_mid, *gu;
  float* lse;
  void *t, *bqT, *bkT;   // LLM LoRA (text_model_lora_config): [lora_A_q(n) | lora_A_k(n)] [M, 128]; lora_B^T of q / k
  void *t2, *bvT, *boT;  // v_proj / o_proj adapters (ABI 17): [lora_A_v(n) | lora_A_o(attention output)] [M, 128]; lora_B^T of v / o
  void *t3, *t4;         // MLP adapters (ABI 18): t3 = [lora_A_gate(n2) | lora_A_up(n2)], t4 = [lora_A_down(act) | -]  [M, 128] each
  void* qk_raw;          // Qwen3 / Gemma-3 (llm_qk_norm): the q | k projections before q_norm / k_norm [M, (Hq + Hkv) * dh]
  void *o_pre, *m_pre;   // Gemma-3: o_proj / down_proj outputs BEFORE their post norms [M, D] (the post norms' backward needs them)
};
struct LlmWs {
  LlmLayerStash ls0;     // layer-0 slot; slot i starts slot_bytes * i later
  size_t slot_bytes;
  void *x_final, *hn, *n, *act, *vt, *logits;
  float* ce_scratch;
  int32_t* sup;          // supervised-row compaction list (sup_rows), count at [M]
  int32_t* sup_c;        // the same rows' indices among the row-compacted gradients (llm_backward, first_pos > 0)
  int32_t *kvs, *kvl;
  // backward (save only)
  void *dx, *d_hn, *d_act, *d_gu, *d_n, *d_o, *d_qkv, *qT, *kT, *doT;
  float* delta;
  float* dkv_part;
  void *lu, *lu2; // LoRA backward: u = [dq . B_q | dk . B_k] [M, 128]; lu2 = [dv . B_v | d (o_proj output) . B_o]
  void *lu3, *lu4, *lbT;   // MLP adapters: lu3 = [d gate . B_g | d up . B_u], lu4 = [d (down output) . B_d | -]; lbT = one adapter's lora_B^T [r, max(D, I)]
  float* lwg;    // lora_wgrad scratch
  void *wt[2], *head_t;   // llm_wt_stream: two alternating sets of one layer's transposed weights, and lm_head^T
  const uvx_config_t* c;
  int M, T, Tp, QKV, OD, save;   // rows (of this view), sequence length, T rounded up to 64, q|k|v and attention-output widths
};

// elements of one layer's four transposed matrices (wqkv_t | wo_t | wgu_t | wd_t, in this order)
inline size_t layer_wt_elems(const uvx_config_t& c) {
  const size_t QKV = (size_t)(c.llm_heads + 2 * c.llm_kv_heads) * c.llm_head_dim, OD = (size_t)c.llm_heads * c.llm_head_dim;
  return (QKV + OD + 3 * (size_t)c.llm_inter) * c.llm_d;
}
// lora_wgrad scratch of the LLM's adapters: the widest adapted linear (hidden, heads * head_dim or the MLP width)
inline long long llm_wg_floats(const uvx_config_t& c, int M) {
  return lora_wgrad_scratch_floats(M, std::max(std::max(c.llm_d, c.llm_heads * c.llm_head_dim), c.llm_inter), 64);
}

// How a buffer is laid out over the batch, i.e. what a batch slice [b0, b0 + nb) does to its pointer: PER_ROW = `bytes` per row of [B * T],
// PER_SEQ = `bytes` per sequence, WHOLE = `bytes` in all, not batch-indexed (a slice sees the same buffer).
enum LlmSpan { PER_ROW, PER_SEQ, WHOLE };

// THE list of a layer slot's buffers, in carve order: f(field, span, bytes).  A buffer only some configurations need has 0 bytes elsewhere.
template <class F>
void llm_stash_fields(LlmLayerStash& s, const LlmWs& w, F&& f) {
  const uvx_config_t& c = *w.c;
  const size_t es = esz(c.dtype), D = c.llm_d, OD = (size_t)c.llm_heads * c.llm_head_dim, KD = (size_t)c.llm_kv_heads * c.llm_head_dim;
  const bool g3 = c.llm_flavor == UVX_LLM_GEMMA3;
  f(s.x_in, PER_ROW, D * es);  f(s.qkv, PER_ROW, (OD + 2 * KD) * es);
  f(s.o, PER_ROW, OD * es);    f(s.x_mid, PER_ROW, D * es);
  f(s.gu, PER_ROW, 2 * (size_t)c.llm_inter * es);  f(s.lse, PER_SEQ, sizeof(float) * c.llm_heads * w.T);
  f(s.t, PER_ROW, 128 * es);
  f(s.bqT, WHOLE, 64 * OD * es);  f(s.bkT, WHOLE, 64 * KD * es);
  f(s.t2, PER_ROW, 128 * es);
  f(s.bvT, WHOLE, 64 * KD * es);  f(s.boT, WHOLE, 64 * D * es);
  f(s.t3, PER_ROW, 128 * es);  f(s.t4, PER_ROW, 128 * es);
  f(s.qk_raw, PER_ROW, c.llm_qk_norm ? (OD + KD) * es : 0);
  f(s.o_pre, PER_ROW, g3 ? D * es : 0);  f(s.m_pre, PER_ROW, g3 ? D * es : 0);
}
// THE list of the call-wide buffers behind the layer slots, in carve order (w.c and the dimensions are set)
template <class F>
void llm_ws_fields(LlmWs& w, F&& f) {
  const uvx_config_t& c = *w.c;
  const size_t es = esz(c.dtype), D = c.llm_d, I = c.llm_inter, M = w.M, KD = (size_t)c.llm_kv_heads * c.llm_head_dim;
  f(w.x_final, PER_ROW, D * es);  f(w.hn, PER_ROW, D * es);  f(w.n, PER_ROW, D * es);
  f(w.act, PER_ROW, I * es);  f(w.vt, PER_SEQ, KD * w.Tp * es);
  f(w.logits, PER_ROW, (size_t)c.vocab * es);
  f(w.lbT, WHOLE, 64 * std::max(D, I) * es);  f(w.ce_scratch, WHOLE, sizeof(float) * (2 + M));
  f(w.sup, WHOLE, sizeof(int32_t) * (M + 1));  f(w.sup_c, WHOLE, sizeof(int32_t) * (M + 1));
  f(w.kvs, PER_SEQ, sizeof(int32_t));  f(w.kvl, PER_SEQ, sizeof(int32_t));
  if (!w.save) return;
  f(w.dx, PER_ROW, D * es);  f(w.d_hn, PER_ROW, D * es);
  f(w.d_act, PER_ROW, I * es);  f(w.d_gu, PER_ROW, 2 * I * es);
  f(w.d_n, PER_ROW, D * es);  f(w.d_o, PER_ROW, w.OD * es);  f(w.d_qkv, PER_ROW, w.QKV * es);
  f(w.qT, PER_SEQ, (size_t)w.OD * w.Tp * es);  f(w.kT, PER_SEQ, KD * w.Tp * es);  f(w.doT, PER_SEQ, (size_t)w.OD * w.Tp * es);
  f(w.delta, PER_SEQ, sizeof(float) * c.llm_heads * w.T);  f(w.dkv_part, PER_ROW, sizeof(float) * 2 * w.OD);
  f(w.lu, PER_ROW, 128 * es);  f(w.lu2, PER_ROW, 128 * es);  f(w.lu3, PER_ROW, 128 * es);  f(w.lu4, PER_ROW, 128 * es);
  f(w.lwg, WHOLE, sizeof(float) * (size_t)llm_wg_floats(c, w.M));
  f(w.wt[0], WHOLE, c.llm_wt_stream ? layer_wt_elems(c) * es : 0);  f(w.wt[1], WHOLE, c.llm_wt_stream ? layer_wt_elems(c) * es : 0);
  f(w.head_t, WHOLE, c.llm_wt_stream ? (size_t)c.vocab * D * es : 0);
}

template <class P> void set_ptr(P*& p, void* to) { p = (P*)to; }

// carves the workspace of a [B, T] call (a.base == NULL: measures only); save: a slot per layer and the backward's buffers, else two slots.
// The record keeps a pointer to `c`.
inline LlmWs llm_carve(Arena& a, const uvx_config_t& c, int B, int T, int save) {
  LlmWs w = {};
  w.c = &c; w.M = B * T; w.T = T; w.Tp = rup(T, 64); w.save = save;
  w.QKV = (c.llm_heads + 2 * c.llm_kv_heads) * c.llm_head_dim;
  w.OD = c.llm_heads * c.llm_head_dim;
  const size_t rows = (size_t)B * T;
  auto take = [&](auto& p, LlmSpan span, size_t bytes) { set_ptr(p, a.take(bytes * (span == PER_ROW ? rows : span == PER_SEQ ? (size_t)B : 1))); };
  // layer slots: `n_slots` identical records laid out back to back
  const int n_slots = save ? c.llm_layers : 2;
  const size_t start = a.off = (a.off + 255) & ~(size_t)255;
  llm_stash_fields(w.ls0, w, take);
  a.off = (a.off + 255) & ~(size_t)255;
  w.slot_bytes = a.off - start;
  a.off = start + w.slot_bytes * n_slots;
  llm_ws_fields(w, take);
  return w;
}
// stash record of slot `slot` (layer l's is slot l when saving, slot l & 1 otherwise)
inline LlmLayerStash llm_layer(const LlmWs& w, int slot) {
  LlmLayerStash s = w.ls0;
  llm_stash_fields(s, w, [&](auto& p, LlmSpan, size_t) { set_ptr(p, (char*)p + w.slot_bytes * slot); });
  return s;
}
// batch slice [b0, b0 + nb) of a carved workspace: the same record with every batch-indexed pointer advanced
inline LlmWs llm_view(const LlmWs& w, int b0, int nb) {
  LlmWs v = w;
  if (b0 == 0 && nb * w.T == w.M) return v;
  v.M = nb * w.T;
  const size_t r0 = (size_t)b0 * w.T;
  auto slice = [&](auto& p, LlmSpan span, size_t bytes) {
    if (span != WHOLE) set_ptr(p, (char*)p + bytes * (span == PER_ROW ? r0 : (size_t)b0));
  };
  llm_stash_fields(v.ls0, v, slice);
  llm_ws_fields(v, slice);
  return v;
}

}  // namespace uvx
