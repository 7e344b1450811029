// The encoder-layer stack shared by the Whisper and wav2vec2 towers (enc_stack.h): workspace carve, the four branch functions (attention and
// feed-forward, forward and backward) and the pre-LN / post-LN walks built on them.  Host orchestration only.
#include <algorithm>
#include "enc_stack.h"

namespace uvx {

EncStackWs enc_stack_carve(Arena& a, const EncStackDesc& D) {
  EncStackWs w = {};
  const size_t es = esz(D.dtype), M = (size_t)D.M(), d = D.d;
  const size_t ht = (size_t)D.B * D.heads * (D.d / D.heads) * D.Tp * es;      // one [B, heads, head_dim, Tp] transposed copy
  w.x = a.take(M * d * es);
  w.n = a.take(M * d * es);
  w.qkv = a.take(M * 3 * d * es);
  w.vt = a.take(ht);
  w.o = a.take(M * d * es);
  w.f = a.take(M * D.ffn * es);
  if (D.key_padding) w.kvlen = (int32_t*)a.take(sizeof(int32_t) * D.B);
  w.sk_bytes = D.splitk ? gemm_splitk_ws_bytes(D.M(), D.ffn) : 0;
  w.sk = w.sk_bytes ? a.take(w.sk_bytes) : nullptr;
  if (!D.train) return w;
  // layer slots: `layers` identical records laid out back to back
  const size_t start = (a.off + 255) & ~(size_t)255;
  a.off = start;
  EncLayerStash& s = w.ls0;
  s.x_in = a.take(M * d * es); s.qkv = a.take(M * 3 * d * es); s.o = a.take(M * d * es); s.x_mid = a.take(M * d * es);
  if (D.post_ln) s.y2 = a.take(M * d * es);
  s.pre = a.take(M * D.ffn * es);
  s.lse = (float*)a.take(sizeof(float) * (size_t)D.B * D.heads * D.T);
  s.t = a.take(M * 128 * es); s.bqT = a.take(64 * d * es); s.bkT = a.take(64 * d * es);
  s.t2 = a.take(M * 128 * es); s.bvT = a.take(64 * d * es); s.boT = a.take(64 * d * es);
  if (D.mlp_adapters) s.t3 = a.take(M * 128 * es);
  a.off = (a.off + 255) & ~(size_t)255;
  w.slot_bytes = a.off - start;
  a.off = start + w.slot_bytes * D.layers;
  w.dx = a.take(M * d * es); w.d_n = a.take(M * d * es); w.d_o = a.take(M * d * es);
  w.d_f = a.take(M * D.ffn * es); w.d_qkv = a.take(M * 3 * d * es);
  w.qT = a.take(ht); w.kT = a.take(ht); w.doT = a.take(ht);
  w.u = a.take(M * 128 * es); w.u2 = a.take(M * 128 * es);
  const int wide = D.mlp_adapters ? std::max(D.d, D.ffn) : D.d;      // the widest adapted linear
  if (D.mlp_adapters) { w.u3 = a.take(M * 128 * es); w.lbT = a.take((size_t)64 * wide * es); }
  w.delta = (float*)a.take(sizeof(float) * (size_t)D.B * D.heads * D.T);
  w.wg_floats = lora_wgrad_scratch_floats(D.M(), wide, 64);
  w.wg = (float*)a.take(sizeof(float) * (size_t)w.wg_floats);
  return w;
}

EncLayerStash enc_stack_layer(const EncStackWs& w, int l) {
  EncLayerStash s = w.ls0;
  const size_t off = w.slot_bytes * l;
  void** ps[] = {&s.x_in, &s.qkv, &s.o, &s.x_mid, &s.y2, &s.pre, (void**)&s.lse, &s.t, &s.bqT, &s.bkT, &s.t2, &s.bvT, &s.boT, &s.t3};
  for (void** q : ps) if (*q) *q = (char*)*q + off;
  return s;
}

namespace {

// what every branch function takes: one call's stream, descriptor, carved workspace, weights and adapters
struct Ctx {
  hipStream_t st;
  const EncStackDesc& D;
  const EncStackWs& w;
  const uvx_enc_layer_t* layers;
  const uvx_encoder_lora_t* lora;
  const uvx_encoder_lora_grads_t* grads;
  float qscale() const { return 1.0f / sqrtf((float)(D.d / D.heads)); }
  GemmDesc sk(GemmDesc g) const { g.splitk_ws = w.sk; g.splitk_ws_bytes = w.sk_bytes; return g; }      // lends the split-K scratch (null: never split)
};

int ln_fwd(const Ctx& c, const void* x, const void* lw, const void* lb, void* y) {
  return probe_skip(128) ? UVX_OK : layernorm_fwd(c.st, c.D.dtype, x, lw, lb, y, c.D.M(), c.D.d, c.D.ln_eps);
}
int ln_bwd(const Ctx& c, const void* dy, const void* x, const void* lw, const void* add, void* dx) {
  return layernorm_bwd(c.st, c.D.dtype, dy, x, lw, add, dx, c.D.M(), c.D.d, c.D.ln_eps);
}

AttnDesc attn_desc(const Ctx& c, const void* qkv, void* o, float* lse) {
  const EncStackDesc& D = c.D;
  const int d = D.d, dt = D.dtype;
  AttnDesc ad;
  ad.q = qkv; ad.k = at(qkv, d, dt); ad.v = at(qkv, 2 * d, dt); ad.vt = c.w.vt; ad.o = o; ad.lse = lse;
  ad.kv_len = D.kv_len; ad.B = D.B; ad.T = D.T; ad.Tp = D.Tp; ad.Hq = D.heads; ad.Hkv = D.heads; ad.D = d / D.heads;
  ad.ldq = ad.ldk = ad.ldv = 3 * d; ad.ldo = d; ad.causal = 0; ad.block = D.block;
  ad.scale = 1.0f;  // q_proj (weight and bias) is pre-scaled by head_dim^-0.5 at pack time (exact for a power of two)
  return ad;
}

// attention branch: q|k|v projection of `in` (+ adapters), attention, out_proj + residual `res` (+ adapter) -> `dst`
int attn_fwd(const Ctx& c, int l, const void* in, const void* res, void* dst) {
  const EncStackDesc& D = c.D;
  const EncStackWs& w = c.w;
  const uvx_enc_layer_t& L = c.layers[l];
  hipStream_t st = c.st;
  const int dt = D.dtype, d = D.d, M = D.M(), dh = d / D.heads;
  const EncLayerStash S = D.train ? enc_stack_layer(w, l) : EncLayerStash{};
  void* qkv = D.train ? S.qkv : w.qkv;
  void* o = D.train ? S.o : w.o;
  {
    GemmDesc g = lin(in, L.wqkv, qkv, M, 3 * d, d);
    g.bias = L.bqkv;
    RC(gemm(st, dt, c.sk(g)));
  }
  if (D.train) {
    // peft LoRA: result += lora_B(lora_A(x)) * scaling (and q carries the head_dim^-0.5 folded into wqkv at pack time).  Rank-r products on
    // the VALU (lora.hip): HBM-bound, no padding to an MFMA tile.
    // (Round 6, tried and removed: the two up-projections as terms of the q|k|v GEMM's whole-line epilogue - and of its dgrad's - instead
    //  of read-modify-write passes over qkv / d n.  Bit-identical, 96 launches fewer per step and 0.25 ms per step SLOWER: the terms'
    //  loads sit in an epilogue nothing overlaps, and their registers cost the 256-row tile its spill-free budget - profiles/r06_flavours.txt.)
    const uvx_enc_lora_layer_t& R = c.lora->layers[l];
    const int r = c.lora->r;
    const float sc = c.lora->scaling, qs = c.qscale();
    if (D.pair_qk && R.q.a && R.k.a) {      // the default target_modules: the pair in one launch each
      RC(lora_transpose2(st, dt, R.q.b, S.bqT, d, R.k.b, S.bkT, d, r));
      RC(lora_down2(st, dt, in, in, d, R.q.a, R.k.a, S.t, at(S.t, 64, dt), 128, M, d, r, 1.0f, 1.0f));
      RC(lora_up2(st, dt, S.t, at(S.t, 64, dt), 128, S.bqT, S.bkT, qkv, at(qkv, d, dt), 3 * d, M, d, d, r, sc * qs, sc));
    } else {
      if (R.q.a) RC(lora_apply(st, dt, in, d, R.q, S.bqT, S.t, qkv, 3 * d, M, d, d, r, sc * qs));
      if (R.k.a) RC(lora_apply(st, dt, in, d, R.k, S.bkT, at(S.t, 64, dt), at(qkv, d, dt), 3 * d, M, d, d, r, sc));
    }
    // v_proj (target_modules beyond the default; ABI 17): the same product into the v columns
    if (R.v.a) RC(lora_apply(st, dt, in, d, R.v, S.bvT, S.t2, at(qkv, 2 * d, dt), 3 * d, M, d, d, r, sc));
  }
  if (attention_needs_transposed_copies(dt)) RC(heads_transpose(st, dt, at(qkv, 2 * d, dt), w.vt, D.B, D.T, D.Tp, D.heads, dh, 3 * d));
  if (!probe_skip(64)) RC(attention_fwd(st, dt, attn_desc(c, qkv, o, D.train ? S.lse : nullptr)));
  {
    GemmDesc g = lin(o, L.wo, dst, M, d, d);
    g.bias = L.bo; g.residual = res; g.ldr = d;
    RC(gemm(st, dt, c.sk(g)));
  }
  // out_proj adapter: dst += lora_B(lora_A(attention output)) * scaling
  if (D.train && c.lora->layers[l].o.a)
    RC(lora_apply(st, dt, o, d, c.lora->layers[l].o, S.boT, at(S.t2, 64, dt), dst, d, M, d, d, c.lora->r, c.lora->scaling));
  return UVX_OK;
}

// feed-forward branch: fc1 + GELU (training: the pre-activation is kept for the GELU backward), fc2 + residual `res` -> `dst`
int ffn_fwd(const Ctx& c, int l, const void* in, const void* res, void* dst) {
  const EncStackDesc& D = c.D;
  const EncStackWs& w = c.w;
  const uvx_enc_layer_t& L = c.layers[l];
  hipStream_t st = c.st;
  const int dt = D.dtype, d = D.d, M = D.M(), ffn = D.ffn;
  const EncLayerStash S = D.train ? enc_stack_layer(w, l) : EncLayerStash{};
  GemmDesc g1 = lin(in, L.fc1_w, D.train ? S.pre : w.f, M, ffn, d);
  g1.bias = L.fc1_b;
  if (D.train) {
    // fuse_gelu: the GELU runs in the GEMM's epilogue, which writes the pre-activation AND the activation (act 2; otherwise the separate
    // gelu_fwd pass - bit-identical)
    const uvx_lora_proj_t& A1 = c.lora->layers[l].g;      // fc1 adapter (ABI 18): joins the pre-activation, so the GELU runs after it
    const bool a1 = D.mlp_adapters && A1.a;
    const bool fused = D.fuse_gelu && !a1;
    if (fused) { g1.act = 2; g1.C2 = w.f; g1.ldc2 = ffn; }
    RC(gemm(st, dt, g1));
    if (a1) RC(lora_apply(st, dt, in, d, A1, w.lbT, S.t3, S.pre, ffn, M, d, ffn, c.lora->r, c.lora->scaling));
    if (!fused) RC(gelu_fwd(st, dt, S.pre, w.f, (long long)M * ffn));
  } else {
    g1.act = 1;
    RC(gemm(st, dt, c.sk(g1)));
  }
  GemmDesc g2 = lin(w.f, L.fc2_w, dst, M, d, ffn);
  g2.bias = L.fc2_b; g2.residual = res; g2.ldr = d;
  RC(gemm(st, dt, c.sk(g2)));
  if (D.train && D.mlp_adapters && c.lora->layers[l].d.a)      // fc2 adapter
    RC(lora_apply(st, dt, w.f, ffn, c.lora->layers[l].d, w.lbT, at(S.t3, 64, dt), dst, d, M, ffn, d, c.lora->r, c.lora->scaling));
  return UVX_OK;
}

// Gradient `dy` [M, d] of the attention branch's output -> the adapters' gradients; unless `last`, d (branch input) in w.d_n = d qkv . Wqkv +
// u . [A_q ; A_k (; A_v)] (+ `add`: the residual path's gradient, folded into the dgrad's epilogue).  The branch input is LayerNorm(S.x_in; lw,
// lb), recomputed into w.n when an adapter needs it (pre-LN), or S.x_in itself (lw == NULL: post-LN).
int attn_bwd(const Ctx& c, int l, const void* dy, const void* add, bool last, const void* lw, const void* lb) {
  const EncStackDesc& D = c.D;
  const EncStackWs& w = c.w;
  const uvx_enc_layer_t& L = c.layers[l];
  hipStream_t st = c.st;
  const int dt = D.dtype, d = D.d, M = D.M(), dh = d / D.heads, r = c.lora->r;
  const float sc = c.lora->scaling, qs = c.qscale();
  const EncLayerStash S = enc_stack_layer(w, l);
  const uvx_enc_lora_layer_t& R = c.lora->layers[l];
  const uvx_enc_lora_layer_grads_t& G = c.grads->layers[l];
  RC(gemm(st, dt, lin(dy, L.wo_t, w.d_o, M, d, d)));
  if (R.o.a) {   // out_proj adapter: its gradients, and d o += (dy . B_o * scaling) . A_o
    RC(lora_apply_bwd(st, dt, S.o, d, dy, d, S.boT, at(S.t2, 64, dt), at(w.u2, 64, dt), G.o, M, d, d, r, sc, w.wg, w.wg_floats));
    RC(lora_up(st, dt, at(w.u2, 64, dt), 128, R.o.a, 1, w.d_o, d, M, d, r, 1.0f, 1));
  }
  if (attention_needs_transposed_copies(dt)) {
    RC(heads_transpose(st, dt, S.qkv, w.qT, D.B, D.T, D.Tp, D.heads, dh, 3 * d));
    RC(heads_transpose(st, dt, at(S.qkv, d, dt), w.kT, D.B, D.T, D.Tp, D.heads, dh, 3 * d));
    RC(heads_transpose(st, dt, w.d_o, w.doT, D.B, D.T, D.Tp, D.heads, dh, d));
  }
  AttnBwdDesc bd;
  bd.f = attn_desc(c, S.qkv, S.o, S.lse);      // (kv_len: written by the forward pass, same audio_lens)
  bd.f.vt = nullptr;
  bd.dout = w.d_o; bd.qt = w.qT; bd.kt = w.kT; bd.dot = w.doT; bd.delta = w.delta; bd.dkv_part = nullptr;
  bd.dq = w.d_qkv; bd.dk = at(w.d_qkv, d, dt); bd.dv = at(w.d_qkv, 2 * d, dt);
  bd.lddq = bd.lddk = bd.lddv = 3 * d;
  RC(attention_bwd(st, dt, bd));
  // ---- LoRA gradients of q_proj / k_proj / v_proj (rank-r products on the VALU, lora.hip) ----
  const void* in = S.x_in;
  if (lw && (R.q.a || R.k.a || R.v.a)) {      // the normalised input is recomputed (not stashed)
    RC(ln_fwd(c, S.x_in, lw, lb, w.n));
    in = w.n;
  }
  const bool qk_pair = D.pair_qk && R.q.a && R.k.a;
  if (qk_pair) {
    // u = [dq . B_q * (scaling * qscale) | dk . B_k * scaling]  [M, 128] (columns 0..r-1 and 64..64+r-1)
    RC(lora_down2(st, dt, w.d_qkv, at(w.d_qkv, d, dt), 3 * d, S.bqT, S.bkT, w.u, at(w.u, 64, dt), 128, M, d, r, sc * qs, sc));
    // d lora_A [r, d] = u^T . n;  d lora_B [d, r] = scale * dq^T . t
    const LoraWgradItem items[4] = {{in, d, w.u, 128, G.q.a, d, 0, 1.0f}, {in, d, at(w.u, 64, dt), 128, G.k.a, d, 0, 1.0f},
                                    {w.d_qkv, 3 * d, S.t, 128, G.q.b, d, 1, sc * qs},
                                    {at(w.d_qkv, d, dt), 3 * d, at(S.t, 64, dt), 128, G.k.b, d, 1, sc}};
    RC(lora_wgrad_batch(st, dt, items, 4, M, r, w.wg, w.wg_floats));      // (one reduce launch for the four)
  } else {
    if (R.q.a) RC(lora_apply_bwd(st, dt, in, d, w.d_qkv, 3 * d, S.bqT, S.t, w.u, G.q, M, d, d, r, sc * qs, w.wg, w.wg_floats));
    if (R.k.a) RC(lora_apply_bwd(st, dt, in, d, at(w.d_qkv, d, dt), 3 * d, S.bkT, at(S.t, 64, dt), at(w.u, 64, dt), G.k, M, d, d, r, sc, w.wg, w.wg_floats));
  }
  if (R.v.a) RC(lora_apply_bwd(st, dt, in, d, at(w.d_qkv, 2 * d, dt), 3 * d, S.bvT, S.t2, w.u2, G.v, M, d, d, r, sc, w.wg, w.wg_floats));
  if (last) return UVX_OK;      // nothing below the first layer is trainable (frozen stem): its input gradient has no consumer
  {
    GemmDesc g = lin(w.d_qkv, L.wqkv_t, w.d_n, M, d, 3 * d);
    g.residual = add; g.ldr = d;
    RC(gemm(st, dt, g));
  }
  if (qk_pair) {
    RC(lora_up2(st, dt, w.u, at(w.u, 64, dt), 128, R.q.a, R.k.a, w.d_n, w.d_n, d, M, d, d, r, 1.0f, 1.0f));      // (same rows: one pass, q term then k term)
  } else {
    if (R.q.a) RC(lora_up(st, dt, w.u, 128, R.q.a, 1, w.d_n, d, M, d, r, 1.0f, 1));
    if (R.k.a) RC(lora_up(st, dt, at(w.u, 64, dt), 128, R.k.a, 1, w.d_n, d, M, d, r, 1.0f, 1));
  }
  if (R.v.a) RC(lora_up(st, dt, w.u2, 128, R.v.a, 1, w.d_n, d, M, d, r, 1.0f, 1));
  return UVX_OK;
}

// Gradient `dy` of the feed-forward branch's output -> w.d_n = (dy . W_fc2 * gelu'(pre)) . W_fc1 (+ `add`), and the fc1 / fc2 adapters'
// gradients.  The branch input is LayerNorm(S.x_mid; lw, lb), recomputed into w.n when the fc1 adapter needs it.
int ffn_bwd(const Ctx& c, int l, const void* dy, const void* add, const void* lw, const void* lb) {
  const EncStackDesc& D = c.D;
  const EncStackWs& w = c.w;
  const uvx_enc_layer_t& L = c.layers[l];
  hipStream_t st = c.st;
  const int dt = D.dtype, d = D.d, M = D.M(), ffn = D.ffn, r = c.lora->r;
  const EncLayerStash S = enc_stack_layer(w, l);
  const uvx_enc_lora_layer_t& R = c.lora->layers[l];
  const uvx_enc_lora_layer_grads_t& G = c.grads->layers[l];
  // d f = (dy . W_fc2) * gelu'(pre): fuse_gelu - in the dgrad GEMM's epilogue (act 3; otherwise the separate gelu_bwd pass, bit-identical)
  GemmDesc g2 = lin(dy, L.fc2_t, w.d_f, M, ffn, d);
  const bool a1 = D.mlp_adapters && R.g.a, a2 = D.mlp_adapters && R.d.a;      // the fc1 / fc2 adapters, where the tower builds them
  const bool fused = D.fuse_gelu && !a2;
  if (fused) { g2.act = 3; g2.C2 = S.pre; g2.ldc2 = ffn; }
  RC(gemm(st, dt, g2));
  if (a2) {      // fc2 adapter: its input gelu(pre) is recomputed; d f += (dy . B * scaling) . A BEFORE the GELU backward
    RC(gelu_fwd(st, dt, S.pre, w.f, (long long)M * ffn));
    RC(lora_transpose(st, dt, R.d.b, w.lbT, d, r));
    RC(lora_apply_bwd(st, dt, w.f, ffn, dy, d, w.lbT, at(S.t3, 64, dt), at(w.u3, 64, dt), G.d, M, ffn, d, r, c.lora->scaling, w.wg, w.wg_floats));
    RC(lora_up(st, dt, at(w.u3, 64, dt), 128, R.d.a, 1, w.d_f, ffn, M, ffn, r, 1.0f, 1));
  }
  if (!fused) RC(gelu_bwd(st, dt, w.d_f, S.pre, w.d_f, (long long)M * ffn));
  GemmDesc g1 = lin(w.d_f, L.fc1_t, w.d_n, M, d, ffn);
  g1.residual = add; g1.ldr = d;
  RC(gemm(st, dt, g1));
  if (a1) {      // fc1 adapter: its input is recomputed; d (branch input) += (d pre . B * scaling) . A
    RC(ln_fwd(c, S.x_mid, lw, lb, w.n));
    RC(lora_transpose(st, dt, R.g.b, w.lbT, ffn, r));
    RC(lora_apply_bwd(st, dt, w.n, d, w.d_f, ffn, w.lbT, S.t3, w.u3, G.g, M, d, ffn, r, c.lora->scaling, w.wg, w.wg_floats));
    RC(lora_up(st, dt, w.u3, 128, R.g.a, 1, w.d_n, d, M, d, r, 1.0f, 1));
  }
  return UVX_OK;
}

int check_transposed(const EncStackDesc& D, const uvx_enc_layer_t& L, int l) {
  UVX_CHECK(L.wqkv_t && L.wo_t && L.fc1_t && L.fc2_t, UVX_ERR_INVALID, "%s: layer %d lacks transposed weights", D.who, l);
  return UVX_OK;
}

}  // namespace

// per layer: h = h + attention(LN1(h));  h = h + feed_forward(LN2(h)).  Inference updates the residual stream in place; training keeps it in the
// layer stashes (x_in -> x_mid -> the next layer's x_in; the last layer's output in w.x, kept for the backward).
int enc_stack_fwd_pre_ln(hipStream_t st, const EncStackDesc& D, const EncStackWs& w, const uvx_enc_layer_t* layers, const uvx_encoder_lora_t* lora, void*& h) {
  const Ctx c = {st, D, w, layers, lora, nullptr};
  for (int l = 0; l < D.layers; ++l) {
    const uvx_enc_layer_t& L = layers[l];
    void* h_mid = D.train ? enc_stack_layer(w, l).x_mid : h;
    void* h_next = !D.train ? h : (l + 1 < D.layers ? enc_stack_layer(w, l + 1).x_in : w.x);
    RC(ln_fwd(c, h, L.ln1_w, L.ln1_b, w.n));
    RC(attn_fwd(c, l, w.n, h, h_mid));
    RC(ln_fwd(c, h_mid, L.ln2_w, L.ln2_b, w.n));
    RC(ffn_fwd(c, l, w.n, h_mid, h_next));
    h = h_next;
  }
  return UVX_OK;
}

// per layer: x = LN1(x + attention(x));  x = LN2(x + feed_forward(x)).  Inference: x alternates between its buffer and w.x; training: x_in /
// x_mid / y2 of the layer stashes, x1 = LN1(x_mid) in w.n.
int enc_stack_fwd_post_ln(hipStream_t st, const EncStackDesc& D, const EncStackWs& w, const uvx_enc_layer_t* layers, const uvx_encoder_lora_t* lora, void* x,
                          void* out) {
  const Ctx c = {st, D, w, layers, lora, nullptr};
  for (int l = 0; l < D.layers; ++l) {
    const uvx_enc_layer_t& L = layers[l];
    const EncLayerStash S = D.train ? enc_stack_layer(w, l) : EncLayerStash{};
    void* mid = D.train ? S.x_mid : w.x;
    void* x1 = D.train ? w.n : x;
    void* y2 = D.train ? S.y2 : w.x;
    RC(attn_fwd(c, l, x, x, mid));
    RC(ln_fwd(c, mid, L.ln1_w, L.ln1_b, x1));       // layers.N.layer_norm
    RC(ffn_fwd(c, l, x1, x1, y2));
    void* dst = l + 1 == D.layers ? out : (D.train ? enc_stack_layer(w, l + 1).x_in : x);
    RC(ln_fwd(c, y2, L.ln2_w, L.ln2_b, dst));       // layers.N.final_layer_norm
    x = dst;
  }
  return UVX_OK;
}

int enc_stack_bwd_pre_ln(hipStream_t st, const EncStackDesc& D, const EncStackWs& w, const uvx_enc_layer_t* layers, const uvx_encoder_lora_t* lora,
                         const uvx_encoder_lora_grads_t* grads) {
  const Ctx c = {st, D, w, layers, lora, grads};
  for (int l = D.layers - 1; l >= 0; --l) {
    const uvx_enc_layer_t& L = layers[l];
    RC(check_transposed(D, L, l));
    const EncLayerStash S = enc_stack_layer(w, l);
    RC(ffn_bwd(c, l, w.dx, nullptr, L.ln2_w, L.ln2_b));                          // d n2 in w.d_n
    RC(ln_bwd(c, w.d_n, S.x_mid, L.ln2_w, w.dx, w.dx));                          // d x_mid = d x_out + LN2'(d n2)
    RC(attn_bwd(c, l, w.dx, nullptr, l == 0, L.ln1_w, L.ln1_b));                 // d n1 in w.d_n
    if (l > 0) RC(ln_bwd(c, w.d_n, S.x_in, L.ln1_w, w.dx, w.dx));                // d x_in = d x_mid + LN1'(d n1)
  }
  return UVX_OK;
}

// the layer's output = final_layer_norm(y2), y2 = x1 + ffn(x1), x1 = layer_norm(x_mid), x_mid = x_in + attention(x_in)
int enc_stack_bwd_post_ln(hipStream_t st, const EncStackDesc& D, const EncStackWs& w, const uvx_enc_layer_t* layers, const uvx_encoder_lora_t* lora,
                          const uvx_encoder_lora_grads_t* grads, const void* d_out) {
  const Ctx c = {st, D, w, layers, lora, grads};
  const void* dx = d_out;
  for (int l = D.layers - 1; l >= 0; --l) {
    const uvx_enc_layer_t& L = layers[l];
    RC(check_transposed(D, L, l));
    const EncLayerStash S = enc_stack_layer(w, l);
    RC(ln_bwd(c, dx, S.y2, L.ln2_w, nullptr, w.dx));                             // d y2 in w.dx
    RC(ffn_bwd(c, l, w.dx, w.dx, L.ln1_w, L.ln1_b));                             // d x1 = d y2 + ffn'(d y2) in w.d_n
    RC(ln_bwd(c, w.d_n, S.x_mid, L.ln1_w, nullptr, w.dx));                       // d x_mid in w.dx
    RC(attn_bwd(c, l, w.dx, w.dx, l == 0, nullptr, nullptr));                    // d x_in = d x_mid + attention'(d x_mid) in w.d_n
    dx = w.d_n;
  }
  return UVX_OK;
}

}  // namespace uvx
