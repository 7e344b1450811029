// The language model's training stack behind the C ABI (include/uvx.h, uvx_llm_*): which kernels run, in what order, on which slices of the
// caller's workspace (llm_stack.h).  No device allocation, no synchronisation.
#include <mutex>
#include <unordered_map>
#include "llm_stack.h"
#include "llm_rules.h"
#include "../../include/uvx.h"

namespace {

using namespace uvx;

__global__ void mask_range_k(const int64_t* __restrict__ mask, int32_t* __restrict__ kv_start, int32_t* __restrict__ kv_len,
                             int T) {
  __shared__ int lo, hi;
  if (threadIdx.x == 0) { lo = T; hi = 0; }
  __syncthreads();
  const int64_t* m = mask + (long long)blockIdx.x * T;
  int l = T, h = 0;
  for (int t = threadIdx.x; t < T; t += blockDim.x)
    if (m[t] != 0) { l = min(l, t); h = max(h, t + 1); }
  atomicMin(&lo, l);
  atomicMax(&hi, h);
  __syncthreads();
  if (threadIdx.x == 0) { kv_start[blockIdx.x] = lo < hi ? lo : 0; kv_len[blockIdx.x] = hi; }
}

__global__ void full_range_k(int32_t* __restrict__ kv_start, int32_t* __restrict__ kv_len, int B, int T) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) { kv_start[b] = 0; kv_len[b] = T; }
}

__global__ void set_i32_k(int32_t* p, int32_t v) { *p = v; }

// What uvx_llm_fwd_train left in a workspace (host-side note keyed by the workspace address): whether the last layer's stash is
// row-compacted.  uvx_llm_bwd_train re-derives that from tuning option 3; if the option changed in between it would misread the
// stash silently - now it is an error.
std::mutex g_pair_mu;
std::unordered_map<const void*, bool> g_pair_compact;
void note_pair(const void* ws, bool compact) { std::lock_guard<std::mutex> l(g_pair_mu); g_pair_compact[ws] = compact; }
int check_pair(const void* ws, bool compact) {
  std::lock_guard<std::mutex> l(g_pair_mu);
  auto it = g_pair_compact.find(ws);
  UVX_CHECK(it == g_pair_compact.end() || it->second == compact, UVX_ERR_INVALID,
            "llm_bwd_train: the forward pass left a %s last-layer stash in this workspace, the backward expects %s (uvx_set_option(3, ..) "
            "changed between uvx_llm_fwd_train and uvx_llm_bwd_train)", it->second ? "row-compacted" : "full-row", compact ? "row-compacted" : "full-row");
  return UVX_OK;
}

// Multi-stream schedule (tuning option 11 = number of chains, default 1 = one chain on the caller's stream): the batch is cut into slices whose layer chains are
// independent (frozen LLM: no weight gradient couples them); they run on the caller's stream and on side streams.  Every kernel
// of a chain depends on its predecessor, so on ONE stream the tail of each GEMM (a partly filled last round of tiles: 1120
// tiles = 4.4 rounds of 256 CUs at N = 28672, 560 = 2.2 at N = 14336) and every HBM-bound elementwise kernel leave CUs
// idle; with two chains in flight the other half's kernel takes those CUs.  Same kernels on the same rows: results are
// bit-identical to the one-stream schedule.  Fork / join by events (legal under stream capture as well).
struct Fork {
  hipStream_t side[3] = {nullptr, nullptr, nullptr};
  hipEvent_t e_fork = nullptr, e_join[3] = {nullptr, nullptr, nullptr};
  bool ok = false;
};
Fork* fork_for_device() {
  static Fork forks[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  Fork& f = forks[dev];
  // One set of side streams / events per DEVICE, created once (under a lock: two host threads may make their first call together).
  // The set is shared by every call on the device: calls that use it must be issued from one stream at a time (the trainer's
  // usage); a partly failed creation is torn down so that a retry starts clean.
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (!f.ok) {
    bool good = hipEventCreateWithFlags(&f.e_fork, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; i < 3 && good; ++i)
      good = hipStreamCreateWithFlags(&f.side[i], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&f.e_join[i], hipEventDisableTiming) == hipSuccess;
    if (!good) {
      if (f.e_fork) (void)hipEventDestroy(f.e_fork);
      for (int i = 0; i < 3; ++i) {
        if (f.side[i]) (void)hipStreamDestroy(f.side[i]);
        if (f.e_join[i]) (void)hipEventDestroy(f.e_join[i]);
      }
      f = Fork{};
      return nullptr;
    }
    f.ok = true;
  }
  return &f;
}
// llm_wt_stream: the side stream that transposes layer l - 1's weights while layer l is differentiated, and its events
struct WtStream {
  hipStream_t side = nullptr;
  hipEvent_t e_start = nullptr, e_head = nullptr, e_ready[2] = {nullptr, nullptr}, e_free[2] = {nullptr, nullptr};
  bool ok = false;
};
WtStream* wt_stream_for_device() {
  static WtStream all[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return nullptr;
  WtStream& f = all[dev];
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (!f.ok) {
    hipEvent_t* ev[6] = {&f.e_start, &f.e_head, &f.e_ready[0], &f.e_ready[1], &f.e_free[0], &f.e_free[1]};
    bool good = true;
    for (hipEvent_t* e : ev) good = good && hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess;
    good = good && hipStreamCreateWithFlags(&f.side, hipStreamNonBlocking) == hipSuccess;
    if (!good) {      // tear down what exists: a retry starts clean
      for (hipEvent_t* e : ev)
        if (*e) (void)hipEventDestroy(*e);
      if (f.side) (void)hipStreamDestroy(f.side);
      f = WtStream{};
      return nullptr;
    }
    f.ok = true;
  }
  return &f;
}
// The chains of one call: batch slices [b0[i], b0[i + 1]) with their workspace views and streams (chain 0 = the caller's).
// Option 11 = number of chains (2 by default, up to 4; 0 / 1 = one chain); a chain needs at least one sequence.
// `allowed`: bf16, and neither LoRA nor llm_wt_stream - the adapters' rank-r products (one wgrad scratch, one lora_B^T buffer, gradients summed
// over the whole batch) and the weight-transpose stream's waits are written for a single chain.
struct Chains {
  int n = 1;
  int b0[5] = {0, 0, 0, 0, 0};
  LlmWs v[4];
  hipStream_t st[4];
  Fork* fk = nullptr;
  int B(int h) const { return b0[h + 1] - b0[h]; }
};
Chains make_chains(hipStream_t st, const LlmWs& s, int B, bool allowed) {
  Chains ch;
  int want = opt(UVX_OPT_LLM_CHAINS) < 2 ? 1 : (opt(UVX_OPT_LLM_CHAINS) > 4 ? 4 : opt(UVX_OPT_LLM_CHAINS));
  if (want > B) want = B;
  ch.fk = (allowed && want >= 2) ? fork_for_device() : nullptr;
  ch.n = ch.fk ? want : 1;
  for (int i = 0; i <= ch.n; ++i) ch.b0[i] = (int)(((long long)B * i + ch.n - 1) / ch.n);   // sizes differ by at most one, larger first
  for (int i = 0; i < ch.n; ++i) {
    ch.v[i] = ch.n == 1 ? s : llm_view(s, ch.b0[i], ch.B(i));
    ch.st[i] = i == 0 ? st : ch.fk->side[i - 1];
  }
  return ch;
}
int chains_fork(const Chains& ch) {
  if (ch.n < 2) return UVX_OK;
  UVX_HIP(hipEventRecord(ch.fk->e_fork, ch.st[0]));
  for (int i = 1; i < ch.n; ++i) UVX_HIP(hipStreamWaitEvent(ch.st[i], ch.fk->e_fork, 0));
  return UVX_OK;
}
int chains_join(const Chains& ch) {
  for (int i = 1; i < ch.n; ++i) {
    UVX_HIP(hipEventRecord(ch.fk->e_join[i - 1], ch.st[i]));
    UVX_HIP(hipStreamWaitEvent(ch.st[0], ch.fk->e_join[i - 1], 0));
  }
  return UVX_OK;
}

// The dgrad of a frozen linear y = x . W^T (W [N_out, N_in]):  d x [M, N_in] = d y [M, N_out] . W.  With the transposed copy Wt [N_in, N_out]
// it is the NT problem lin(d y, Wt, ..); without one (Wt == NULL; bf16, round 6) the NN form reads W as it lies (GemmDesc::b_kn: B [K, N],
// row stride N) - bit-identical, and the copy (16 GB of them for Llama-3-8B) need not exist.
GemmDesc lin_dgrad(const void* dY, const void* Wt, const void* W, void* dX, int M, int N_in, int N_out) {
  GemmDesc g = lin(dY, Wt ? Wt : W, dX, M, N_in, N_out);
  if (!Wt) { g.b_kn = 1; g.ldb = N_in; }
  return g;
}

int llm_check(const uvx_config_t& c, const uvx_llm_weights_t* w, int T) {
  UVX_CHECK(c.llm_heads % c.llm_kv_heads == 0, UVX_ERR_SHAPE, "llm: heads %d not a multiple of kv heads %d", c.llm_heads, c.llm_kv_heads);
  UVX_CHECK(c.llm_inter % 16 == 0, UVX_ERR_SHAPE, "llm: intermediate size %d must be a multiple of 16", c.llm_inter);
  UVX_CHECK(w->rope_len >= T, UVX_ERR_SHAPE, "llm: rope table (%d) shorter than sequence (%d)", w->rope_len, T);
  if (c.llm_qk_norm)
    for (int l = 0; l < c.llm_layers; ++l)
      UVX_CHECK(w->layers[l].q_norm && w->layers[l].k_norm, UVX_ERR_INVALID, "llm: llm_qk_norm is set but layer %d has no q_norm / k_norm", l);
  return gemma3_check(c, w);
}

struct LayerT { const void *wqkv_t, *wo_t, *wgu_t, *wd_t; };

// One call's walk over the layers: the call, its carved workspace, and every derived decision - each made once, here.
struct LlmWalk {
  const LlmCallDesc& d;
  const uvx_config_t& c;
  const uvx_llm_weights_t* w;
  const uvx_encoder_lora_t* lora;
  const LlmWs s;        // the whole batch's workspace (the branch functions get a chain's view of it)
  const int dt, D, I, T, Hq, Hkv, dh;
  const int fl;         // 0 Llama, 1 Gemma, 2 Gemma-3 (norm flavour - any non-zero value is Gemma's -, GLU activation, embedding scale)
  const bool g3;
  const bool save;      // a stash slot per layer (else two alternating ones)
  // top: only some rows' logits leave the call or are differentiated - the supervised rows of the training pair (top_rows), or a caller-supplied
  // row list (uvx_llm_fwd_rows: teacher; student with uvx_llm_bwd_rows).  In the LAST layer nothing downstream of its attention mixes positions any
  // more - o_proj, the MLP and the final norm are row-wise - so their results are needed (and have a gradient) on those rows alone.
  // tc: that half then runs on the compacted rows (device-side list, no host sync; GEMMs clamp to the device count).  Same loss, same gradients.
  // (tuning option 3 off, or Gemma-3's post norms: the plain full-row path, in both calls of the pair)
  const bool top, tc;
  const bool rope_fused;   // the bf16 attention backward writes dq / dk RoPE-inverted (epilogue of the dQ kernel, GQA group reduction): no separate pass
  const bool wts;          // backward: transposed weights made on the fly (include/uvx.h llm_wt_stream)
  WtStream* wt = nullptr;
  // first_pos (uvx_llm_bwd_train_from): the caller needs no gradient below that position of any sequence - the text prefix before the first audio
  // token: under the causal mask a position only feeds later ones, so nothing the adapter training updates is reachable from it.  Below the
  // row-compacted last layer every gradient tensor then holds the positions >= rs.skip only (sequence b at row b * rs.tc): the dgrad GEMMs, the SwiGLU
  // and norm backward run on B * rs.tc rows and read the stash through the map (kernels.h RowSkip), the fused attention backward takes the
  // compacted d o / d q|k|v (AttnBwdDesc::d_first; it still needs every key for d q).  Same arithmetic per remaining row: the audio rows of
  // d_inputs_embeds are bit-identical; its rows below rs.skip are zeros.  Conditions: the training step's entry points, the bf16 attention kernels on
  // natural-layout operands, one chain, no per-row stash reader outside the kernels that take the map (the LLM adapters' products do not).
  RowSkip rs;

  LlmWalk(const LlmCallDesc& d_, const LlmWs& s_, bool save_)
      : d(d_), c(*d_.cfg), w(d_.w), lora(d_.lora), s(s_), dt(c.dtype), D(c.llm_d), I(c.llm_inter), T(d_.T), Hq(c.llm_heads), Hkv(c.llm_kv_heads),
        dh(c.llm_head_dim), fl(c.llm_flavor), g3(fl == UVX_LLM_GEMMA3), save(save_),
        top(d_.top_rows || ((d_.rows || d_.compact_in_place) && !d_.lora)), tc(top && opt(UVX_OPT_LOSS_HEAD_SUPERVISED_ROWS) && !g3),
        rope_fused(attention_bwd_fuses_rope(dt) && opt(UVX_OPT_ATTN_BWD_ROPE_FUSED)), wts(c.llm_wt_stream != 0) {
    const int s16 = d.first_pos / 16 * 16;
    if (s16 > 0 && s16 < T && (d.top_rows || d.compact_in_place) && !lora && opt(UVX_OPT_LLM_CHAINS) < 2 && opt(UVX_OPT_ATTN_BWD_ROPE_FUSED) &&
        attention_bwd_takes_d_first(dt, causal_gqa_desc(c, s.ls0.qkv, d.B, T, s.Tp, s.QKV, s.OD))) { rs.skip = s16; rs.tc = T - s16; }      // (option 14: RoPE inverted inside the attention backward, by position - rope_k would take the row index)
  }
  int slot_of(int l) const { return save ? l : (l & 1); }
  int rows_bwd(const LlmWs& v) const { return rs.skip ? v.M / T * rs.tc : v.M; }
  long long lwg_floats() const { return llm_wg_floats(c, s.M); }
  bool ad_in(int l) const { return lora && (lora->layers[l].g.a || lora->layers[l].u.a); }
  bool ad_out(int l) const { return lora && lora->layers[l].d.a; }

  // ------------------------------------------------------------------ forward
  // first half of a layer, rows of the view v (a batch slice): norm, q|k|v projection, RoPE, V^T, causal GQA flash attention
  int layer_attn(hipStream_t sx, const LlmWs& v, int Bv, int l) const {
    const uvx_llm_layer_t& L = w->layers[l];
    LlmLayerStash cur = llm_layer(v, slot_of(l));
    const int Mv = v.M;
    // (probe bit 256: the kernel runs but writes elsewhere - the GEMM then reads a buffer nobody has just written)
    if (!probe_skip(16)) RC(rmsnorm_fwd(sx, dt, cur.x_in, L.ln1, probe_skip(256) && save ? v.d_n : v.n, nullptr, Mv, D, c.rms_eps, fl));
    {
      GemmDesc g = lin(v.n, L.wqkv, cur.qkv, Mv, s.QKV, D);
      g.bias = L.bqkv;     // Qwen2: q / k / v projection biases (null otherwise)
      RC(gemm(sx, dt, g));
    }
    if (lora) {   // peft LoRA on q_proj / k_proj (/ v_proj) (text_model_lora_config): added to the projections, before q_norm / RoPE
      const uvx_enc_lora_layer_t& R = lora->layers[l];
      const int r = lora->r, qc = Hq * dh, kc = Hkv * dh;
      if (R.q.a && R.k.a) {
        RC(lora_transpose2(sx, dt, R.q.b, cur.bqT, qc, R.k.b, cur.bkT, kc, r));
        RC(lora_down(sx, dt, v.n, D, R.q.a, 0, cur.t, 128, Mv, D, r, 1.0f));
        RC(lora_down(sx, dt, v.n, D, R.k.a, 0, at(cur.t, 64, dt), 128, Mv, D, r, 1.0f));
        RC(lora_up(sx, dt, cur.t, 128, cur.bqT, 1, cur.qkv, s.QKV, Mv, qc, r, lora->scaling, 1));
        RC(lora_up(sx, dt, at(cur.t, 64, dt), 128, cur.bkT, 1, at(cur.qkv, (size_t)qc, dt), s.QKV, Mv, kc, r, lora->scaling, 1));
      } else {
        if (R.q.a) RC(lora_apply(sx, dt, v.n, D, R.q, cur.bqT, cur.t, cur.qkv, s.QKV, Mv, D, qc, r, lora->scaling));
        if (R.k.a) RC(lora_apply(sx, dt, v.n, D, R.k, cur.bkT, at(cur.t, 64, dt), at(cur.qkv, (size_t)qc, dt), s.QKV, Mv, D, kc, r, lora->scaling));
      }
      if (R.v.a) RC(lora_apply(sx, dt, v.n, D, R.v, cur.bvT, cur.t2, at(cur.qkv, (size_t)(qc + kc), dt), s.QKV, Mv, D, kc, r, lora->scaling));
    }
    const float* rope = rope_of(c, w, l);
    if (c.llm_qk_norm)   // Qwen3 / Gemma-3: q_norm / k_norm per head, then RoPE - one pass; the raw rows stay for the backward
      RC(qk_norm_rope(sx, dt, cur.qkv, L.q_norm, L.k_norm, save ? cur.qk_raw : nullptr, rope, nullptr, Mv, T, Hq, Hkv,
                      dh, s.QKV, c.rms_eps, g3 ? 1 : 0));
    else if (!probe_skip(32)) RC(rope_inplace(sx, dt, cur.qkv, rope, nullptr, Mv, T, Hq + Hkv, dh, s.QKV, 0));
    if (attention_needs_transposed_copies(dt)) RC(heads_transpose(sx, dt, at(cur.qkv, (size_t)(Hq + Hkv) * dh, dt), v.vt, Bv, T, s.Tp, Hkv, dh, s.QKV));
    AttnDesc ad = causal_gqa_desc(c, cur.qkv, Bv, T, s.Tp, s.QKV, s.OD);
    ad.vt = v.vt; ad.o = cur.o; ad.lse = cur.lse; ad.kv_start = v.kvs; ad.kv_len = v.kvl;
    ad.window = window_of(c, w, l, T);
    return probe_skip(2) ? UVX_OK : attention_fwd(sx, dt, ad);
  }
  // MLP adapters (ABI 18).  gate_proj / up_proj: result += lora_B(lora_A(n2)) * scaling on the gate / up half of the interleaved gate|up tensor -
  // the rank-r kernels work on contiguous columns, so the term is formed in v.act (free until the GLU writes it) and added half by half
  int mlp_in_adapters(hipStream_t sx, const LlmWs& v, const LlmLayerStash& cur, int l) const {
    const uvx_enc_lora_layer_t& R = lora->layers[l];
    const int r = lora->r;
    for (int which = 0; which < 2; ++which) {
      const uvx_lora_proj_t& P = which ? R.u : R.g;
      if (!P.a) continue;
      void* t = at(cur.t3, 64 * which, dt);
      RC(lora_transpose(sx, dt, P.b, v.lbT, I, r));
      RC(lora_down(sx, dt, v.n, D, P.a, 0, t, 128, v.M, D, r, 1.0f));
      RC(lora_up(sx, dt, t, 128, v.lbT, 1, v.act, I, v.M, I, r, lora->scaling, 0));
      RC(gu_half(sx, dt, cur.gu, v.act, v.M, I, which, 1));
    }
    return UVX_OK;
  }
  // second half: o_proj + residual, norm, gate|up (+ SwiGLU), down + residual.  compact (last layer when tc, whole batch only): on the listed
  // rows gathered into the idle backward scratch.
  int layer_mlp(hipStream_t sx, const LlmWs& v, int l, bool compact) const {
    const uvx_llm_layer_t& L = w->layers[l];
    const bool last = l + 1 == c.llm_layers;
    LlmLayerStash cur = llm_layer(v, slot_of(l));
    void* x_out = last ? v.x_final : llm_layer(v, slot_of(l + 1)).x_in;
    const int Mv = v.M;
    const int32_t* mdev = compact ? v.sup + Mv : nullptr;
    if (g3) {
      // Gemma3DecoderLayer: x_mid = x_in + post_attention_norm(o_proj(o));  x_out = x_mid + post_feedforward_norm(mlp(pre_feedforward_norm(x_mid)))
      // (the branch outputs before their post norms stay in the stash for the backward: o_pre, m_pre)
      RC(gemm(sx, dt, lin(cur.o, L.wo, cur.o_pre, Mv, D, s.OD)));
      if (lora && lora->layers[l].o.a)      // o_proj adapter: joins the branch before its post norm
        RC(lora_apply(sx, dt, cur.o, s.OD, lora->layers[l].o, cur.boT, at(cur.t2, 64, dt), cur.o_pre, D, Mv, s.OD, D, lora->r, lora->scaling));
      RC(rmsnorm_fwd(sx, dt, cur.o_pre, L.ln1_post, cur.x_mid, nullptr, Mv, D, c.rms_eps, fl, nullptr, cur.x_in));
      RC(rmsnorm_fwd(sx, dt, cur.x_mid, L.ln2, v.n, nullptr, Mv, D, c.rms_eps, fl));
      RC(gemm(sx, dt, lin(v.n, L.wgu, cur.gu, Mv, 2 * I, D)));
      if (ad_in(l)) RC(mlp_in_adapters(sx, v, cur, l));
      RC(swiglu_fwd(sx, dt, cur.gu, v.act, Mv, I, /*layout=*/2, /*act=*/c.llm_act));
      RC(gemm(sx, dt, lin(v.act, L.wd, cur.m_pre, Mv, D, I)));
      if (ad_out(l))      // down_proj adapter: joins the branch before its post norm
        RC(lora_apply(sx, dt, v.act, I, lora->layers[l].d, v.lbT, cur.t4, cur.m_pre, D, Mv, I, D, lora->r, lora->scaling));
      return rmsnorm_fwd(sx, dt, cur.m_pre, L.ln2_post, x_out, nullptr, Mv, D, c.rms_eps, fl, nullptr, cur.x_mid);
    }
    // gather targets of the compact last layer: the idle backward scratch, or - a forward without stash (the KL teacher) - the other
    // layer slot's o / x_in, dead since the previous layer finished
    void* g_o = save ? v.d_o : llm_layer(v, slot_of(l) ^ 1).o;
    void* g_x = save ? v.dx : llm_layer(v, slot_of(l) ^ 1).x_in;
    if (compact) {   // gather the listed rows of the attention output and of the residual stream
      if (d.rows) {    // (uvx_llm_fwd_rows: the caller's list)
        UVX_HIP(hipMemcpyAsync(v.sup, d.rows, sizeof(int32_t) * d.n_rows, hipMemcpyDeviceToDevice, sx));
        hipLaunchKernelGGL(set_i32_k, dim3(1), dim3(1), 0, sx, v.sup + Mv, d.n_rows);
        UVX_LAUNCH_CHECK();
      } else {
        RC(sup_rows(sx, d.labels, v.sup, d.B, T, c.vocab));
      }
      RC(gather_rows(sx, dt, cur.o, v.sup, Mv, g_o, s.OD));
      RC(gather_rows(sx, dt, cur.x_in, v.sup, Mv, g_x, D));
    }
    {
      GemmDesc g = lin(compact ? g_o : cur.o, L.wo, cur.x_mid, Mv, D, s.OD);
      g.residual = compact ? g_x : cur.x_in; g.ldr = D; g.m_dev = mdev;
      RC(gemm(sx, dt, g));
    }
    if (lora && lora->layers[l].o.a)        // o_proj adapter (never on the compact path: top is false under LoRA)
      RC(lora_apply(sx, dt, cur.o, s.OD, lora->layers[l].o, cur.boT, at(cur.t2, 64, dt), cur.x_mid, D, Mv, s.OD, D, lora->r, lora->scaling));
    if (!probe_skip(16)) RC(rmsnorm_fwd(sx, dt, cur.x_mid, L.ln2, probe_skip(256) && save ? v.d_n : v.n, nullptr, Mv, D, c.rms_eps, fl, mdev));
    {  // gate|up projection; wgu rows are packed as alternating 16-row gate / up blocks (weights.py)
      GemmDesc g = lin(v.n, L.wgu, cur.gu, Mv, 2 * I, D);
      const bool fused = dt == DT_BF16 && fl == UVX_LLM_LLAMA && !ad_in(l);   // SwiGLU fused into the epilogue (GeGLU, or adapters on gate / up: separate kernel)
      if (fused) { g.C2 = v.act; g.ldc2 = I; g.swiglu = 1; }
      g.m_dev = mdev;
      RC(gemm(sx, dt, g));
      if (ad_in(l)) RC(mlp_in_adapters(sx, v, cur, l));
      if (!fused) RC(swiglu_fwd(sx, dt, cur.gu, v.act, Mv, I, /*layout=*/2, /*act=*/c.llm_act, mdev));
    }
    {
      GemmDesc g = lin(v.act, L.wd, x_out, Mv, D, I);
      g.residual = cur.x_mid; g.ldr = D; g.m_dev = mdev;
      RC(gemm(sx, dt, g));
    }
    if (ad_out(l))      // down_proj adapter (never on the compact path: top is false under LoRA)
      RC(lora_apply(sx, dt, v.act, I, lora->layers[l].d, v.lbT, cur.t4, x_out, D, Mv, I, D, lora->r, lora->scaling));
    return UVX_OK;
  }
  // final norm's output s.hn (tc: the listed rows only, in list order) -> LM head, loss
  int head_fwd() const {
    const hipStream_t st = d.st;
    const int M = s.M;
    const size_t es = esz(dt);
    if (d.rows) {
      if (!tc) {       // (compact last layer: the list is in place and s.hn holds its rows, in list order)
        if (d.n_rows > 0) UVX_HIP(hipMemcpyAsync(s.sup, d.rows, sizeof(int32_t) * d.n_rows, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(set_i32_k, dim3(1), dim3(1), 0, st, s.sup + M, d.n_rows);
        UVX_LAUNCH_CHECK();
      }
      if (d.n_rows == 0) return UVX_OK;
      if (!tc) RC(gather_rows(st, dt, s.hn, s.sup, M, s.n, D));
      RC(gemm(st, dt, lin(tc ? s.hn : s.n, w->lm_head, s.logits, d.n_rows, c.vocab, D)));
      if (d.logits_rows) UVX_HIP(hipMemcpyAsync(d.logits_rows, s.logits, (size_t)d.n_rows * c.vocab * es, hipMemcpyDeviceToDevice, st));
      return UVX_OK;
    }
    if (d.labels && dt == DT_BF16 && opt(UVX_OPT_LOSS_HEAD_SUPERVISED_ROWS)) {
      // Loss path on the SUPERVISED rows only (positions whose next token carries a label): every other row of the
      // logits has zero weight in ForCausalLMLoss and a zero gradient, so the head GEMM, the CE and (uvx_llm_bwd) the
      // head dgrad run on the compacted rows - identical loss and gradients, ~T / n_supervised less head work.  The
      // row list is built on the device (no host sync): GEMMs are launched for M rows and clamp to the device count.
      if (d.logits) RC(gemm(st, dt, lin(s.hn, w->lm_head, d.logits, M, c.vocab, D)));   // the caller's full logits, if asked
      if (!tc) {   // (top_rows: the last layer already left s.hn compact, in the order of the row list)
        RC(sup_rows(st, d.labels, s.sup, d.B, T, c.vocab));
        RC(gather_rows(st, dt, s.hn, s.sup, M, s.n, D));
      }
      GemmDesc g = lin(tc ? s.hn : s.n, w->lm_head, s.logits, M, c.vocab, D);
      g.m_dev = s.sup + M;
      RC(gemm(st, dt, g));
      return ce_loss_fwd_bwd(st, dt, s.logits, d.labels, d.loss, s.ce_scratch, nullptr, d.B, T, c.vocab, c.vocab, 1.0f, s.sup);
    }
    RC(gemm(st, dt, lin(s.hn, w->lm_head, s.logits, M, c.vocab, D)));
    if (d.logits) UVX_HIP(hipMemcpyAsync(d.logits, s.logits, (size_t)M * c.vocab * es, hipMemcpyDeviceToDevice, st));
    if (d.labels) RC(ce_loss_fwd_bwd(st, dt, s.logits, d.labels, d.loss, s.ce_scratch, nullptr, d.B, T, c.vocab, c.vocab, 1.0f));
    return UVX_OK;
  }

  // ------------------------------------------------------------------ backward
  // llm_wt_stream: a side stream transposes lm_head and then, one layer ahead of the layer being differentiated, each layer's
  // four matrices into the alternating buffers s.wt[l & 1]; e_ready[b] = buffer b holds its layer, e_free[b] = the caller's stream
  // is done with buffer b.  (One chain only: the chains' side streams would each need the same waits.)
  // (neither resident copies nor the stream, bf16: the transposed pointers stay NULL and lin_dgrad takes the NN form on the forward weights)
  LayerT layer_t(int l) const {
    const uvx_llm_layer_t& L = w->layers[l];
    if (!wts) return LayerT{L.wqkv_t, L.wo_t, L.wgu_t, L.wd_t};
    const size_t es = esz(dt), nq = (size_t)s.QKV * D, no = (size_t)s.OD * D, ng = (size_t)2 * I * D;
    char* b = (char*)s.wt[l & 1];
    return LayerT{b, b + nq * es, b + (nq + no) * es, b + (nq + no + ng) * es};
  }
  int issue_layer_t(int l) const {      // on the side stream: W^T of layer l into its buffer
    const uvx_llm_layer_t& L = w->layers[l];
    const LayerT t = layer_t(l);
    UVX_HIP(hipStreamWaitEvent(wt->side, wt->e_free[l & 1], 0));
    RC(transpose2d_streaming(wt->side, dt, L.wqkv, const_cast<void*>(t.wqkv_t), s.QKV, D, D, s.QKV));
    RC(transpose2d_streaming(wt->side, dt, L.wo, const_cast<void*>(t.wo_t), D, s.OD, s.OD, D));
    RC(transpose2d_streaming(wt->side, dt, L.wgu, const_cast<void*>(t.wgu_t), 2 * I, D, D, 2 * I));
    RC(transpose2d_streaming(wt->side, dt, L.wd, const_cast<void*>(t.wd_t), D, I, I, D));
    UVX_HIP(hipEventRecord(wt->e_ready[l & 1], wt->side));
    return UVX_OK;
  }
  // d logits (in place over the saved logits), then the frozen head: d_hn = dlogits . W_head
  // (labels == NULL: uvx_llm_kl_loss already replaced the saved logits by their gradient)
  int head_bwd(const void* head_t) const {
    const hipStream_t st = d.st;
    const int M = s.M;
    if (d.compact_in_place || (d.labels && dt == DT_BF16 && opt(UVX_OPT_LOSS_HEAD_SUPERVISED_ROWS))) {
      // compact supervised rows (see head_fwd): d logits in place, head dgrad on those rows, scattered back
      if (!d.compact_in_place)
        RC(ce_loss_fwd_bwd(st, dt, s.logits, d.labels, nullptr, s.ce_scratch, s.logits, d.B, T, c.vocab, c.vocab, d.grad_scale, s.sup));
      UVX_HIP(hipMemsetAsync(s.d_hn, 0, (size_t)M * D * esz(dt), st));
      // d_hn[rows] = d logits_c . W_head: few rows x D outputs over K = vocab -> split K for parallelism on the first
      // `cap` compact rows (f32 partials in the not-yet-used d_gu scratch, summed in a fixed order), plain GEMM beyond
      const int nkt = c.vocab / 64;
      const int cap = M < 512 ? M : 512;
      const size_t room = (size_t)M * 2 * I * esz(dt) / ((size_t)cap * D * sizeof(float));
      int nsplit = 1;
      for (int k = 2; k <= 24 && (size_t)k <= room; ++k)
        if (c.vocab % 64 == 0 && nkt % k == 0 && nkt / k >= 16) nsplit = k;
      if (nsplit > 1) {
        float* partial = (float*)s.d_gu;
        const int Kc = c.vocab / nsplit;
        GemmDesc g = lin(s.logits, head_t, partial, cap, D, Kc);
        g.lda = c.vocab; g.ldb = c.vocab; g.batch = nsplit; g.sA = Kc; g.sB = Kc; g.sC = (long long)cap * D; g.out_f32 = 1;
        g.m_dev = s.sup + M;
        RC(gemm(st, dt, g));
        RC(splitk_reduce_scatter(st, dt, partial, nsplit, cap, s.sup, M, s.d_hn, D));
      }
      const int first = nsplit > 1 ? cap : 0;
      if (M > first) {
        GemmDesc g = lin(at(s.logits, (size_t)first * c.vocab, dt), head_t, s.d_n, M - first, D, c.vocab);
        g.m_dev = s.sup + M; g.m_dev_off = first;
        RC(gemm(st, dt, g));
        RC(scatter_rows(st, dt, s.d_n, s.sup, M, s.d_hn, D, first));
      }
      return UVX_OK;
    }
    if (d.labels) RC(ce_loss_fwd_bwd(st, dt, s.logits, d.labels, nullptr, s.ce_scratch, s.logits, d.B, T, c.vocab, c.vocab, d.grad_scale));
    return gemm(st, dt, lin(s.logits, head_t, s.d_hn, M, D, c.vocab));
  }
  // MLP adapters, backward.  down_proj: dy = the gradient of the down projection's output; its input act = GLU(gate|up) is recomputed into v.act;
  // d act += u . A_d BEFORE the GLU backward.
  int mlp_out_adapter_bwd(hipStream_t sx, const LlmWs& v, const LlmLayerStash& cur, int l, const void* dy) const {
    const uvx_lora_proj_t& P = lora->layers[l].d;
    const int r = lora->r;
    RC(swiglu_fwd(sx, dt, cur.gu, v.act, v.M, I, /*layout=*/2, /*act=*/c.llm_act));
    RC(lora_transpose(sx, dt, P.b, v.lbT, D, r));
    RC(lora_apply_bwd(sx, dt, v.act, I, dy, D, v.lbT, cur.t4, v.lu4, d.lgrads->layers[l].d, v.M, I, D, r, lora->scaling, v.lwg, lwg_floats()));
    return lora_up(sx, dt, v.lu4, 128, P.a, 1, v.d_act, I, v.M, I, r, 1.0f, 1);
  }
  // gate_proj / up_proj: dy = the gate / up half of d gate|up, extracted into v.d_act (free once the GLU backward has consumed it); their input
  // n2 = norm(x_mid) is recomputed into v.n; d n2 += u . A after the dgrad GEMM has written v.d_n
  int mlp_in_adapters_bwd(hipStream_t sx, const LlmWs& v, const LlmLayerStash& cur, int l, const void* ln2) const {
    const uvx_enc_lora_layer_t& R = lora->layers[l];
    const int r = lora->r;
    RC(rmsnorm_fwd(sx, dt, cur.x_mid, ln2, v.n, nullptr, v.M, D, c.rms_eps, fl));
    for (int which = 0; which < 2; ++which) {
      const uvx_lora_proj_t& P = which ? R.u : R.g;
      if (!P.a) continue;
      void* u = at(v.lu3, 64 * which, dt);
      RC(gu_half(sx, dt, v.d_gu, v.d_act, v.M, I, which, 0));
      RC(lora_transpose(sx, dt, P.b, v.lbT, I, r));
      RC(lora_apply_bwd(sx, dt, v.n, D, v.d_act, I, v.lbT, at(cur.t3, 64 * which, dt), u, which ? d.lgrads->layers[l].u : d.lgrads->layers[l].g, v.M, D, I, r,
                        lora->scaling, v.lwg, lwg_floats()));
      RC(lora_up(sx, dt, u, 128, P.a, 1, v.d_n, D, v.M, D, r, 1.0f, 1));
    }
    return UVX_OK;
  }
  // MLP half of a layer's backward on the rows of the view v: v.dx (gradient of the layer's output) -> v.dx (gradient of
  // x_mid: residual + norm branch).  compact: the listed rows of the last layer (whole batch, device-side count).
  int layer_mlp_bwd(hipStream_t sx, const LlmWs& v, int l, bool compact) const {
    const uvx_llm_layer_t& L = w->layers[l];
    const LayerT Lt = layer_t(l);
    LlmLayerStash cur = llm_layer(v, l);
    const int Mv = compact ? v.M : rows_bwd(v);      // (rs: the gradient tensors hold the positions >= rs.skip only; the stash is read through the map)
    const RowSkip map = compact ? RowSkip() : rs;
    const int32_t* mdev = compact ? v.sup + v.M : nullptr;
    if (g3) {
      // x_out = x_mid + post_ffw_norm(m_pre): d m_pre = norm'(dx) -> d act -> d gate|up -> d n2; d x_mid = dx + pre_ffw_norm'(d n2)
      RC(rmsnorm_bwd(sx, dt, v.dx, cur.m_pre, L.ln2_post, nullptr, v.d_n, nullptr, Mv, D, c.rms_eps, fl, nullptr, nullptr, map));
      RC(gemm(sx, dt, lin_dgrad(v.d_n, Lt.wd_t, L.wd, v.d_act, Mv, I, D)));
      if (ad_out(l)) RC(mlp_out_adapter_bwd(sx, v, cur, l, v.d_n));      // (d m_pre: behind the post norm)
      RC(swiglu_bwd(sx, dt, v.d_act, cur.gu, v.d_gu, Mv, I, /*layout=*/2, /*act=*/c.llm_act, nullptr, map));
      RC(gemm(sx, dt, lin_dgrad(v.d_gu, Lt.wgu_t, L.wgu, v.d_n, Mv, D, 2 * I)));
      if (ad_in(l)) RC(mlp_in_adapters_bwd(sx, v, cur, l, L.ln2));
      return rmsnorm_bwd(sx, dt, v.d_n, cur.x_mid, L.ln2, v.dx, v.dx, nullptr, Mv, D, c.rms_eps, fl, nullptr, nullptr, map);
    }
    if (dt == DT_BF16 && opt(UVX_OPT_SWIGLU_BWD_IN_DGRAD) && fl == UVX_LLM_LLAMA && !ad_out(l) && !map.skip) {   // d act = dx . W_down^T with the SwiGLU backward fused into the epilogue: writes d gate|up directly
      GemmDesc g = lin_dgrad(v.dx, Lt.wd_t, L.wd, v.d_gu, Mv, I, D);
      g.ldc = 2 * I; g.C2 = cur.gu; g.ldc2 = 2 * I; g.swiglu = 2; g.m_dev = mdev;
      RC(gemm(sx, dt, g));
    } else {
      GemmDesc g = lin_dgrad(v.dx, Lt.wd_t, L.wd, v.d_act, Mv, I, D);
      g.m_dev = mdev;
      RC(gemm(sx, dt, g));
      if (ad_out(l)) RC(mlp_out_adapter_bwd(sx, v, cur, l, v.dx));
      if (!probe_skip(4)) RC(swiglu_bwd(sx, dt, v.d_act, cur.gu, v.d_gu, Mv, I, /*layout=*/2, /*act=*/c.llm_act, mdev, map));
    }
    {
      GemmDesc g = lin_dgrad(v.d_gu, Lt.wgu_t, L.wgu, v.d_n, Mv, D, 2 * I);
      g.m_dev = mdev;
      RC(gemm(sx, dt, g));
    }
    if (ad_in(l)) RC(mlp_in_adapters_bwd(sx, v, cur, l, L.ln2));
    return probe_skip(8) ? UVX_OK : rmsnorm_bwd(sx, dt, v.d_n, cur.x_mid, L.ln2, v.dx, v.dx, nullptr, Mv, D, c.rms_eps, fl, mdev, nullptr, map);
  }
  // attention half: v.dx (gradient of x_mid) -> dx_out (gradient of the layer's input).  d_o_ready: v.d_o and the residual
  // gradient `resid` were already produced for the whole batch (compact last layer), else d_o = dx . W_o^T here.
  // (dx_full: dx_out keeps every row - layer 0 writes the caller's d_inputs_embeds through the map)
  int layer_attn_bwd(hipStream_t sx, const LlmWs& v, int Bv, int l, bool d_o_ready, const void* resid, void* dx_out, bool dx_full) const {
    const uvx_llm_layer_t& L = w->layers[l];
    const LayerT Lt = layer_t(l);
    LlmLayerStash cur = llm_layer(v, l);
    const int Mv = rows_bwd(v);
    if (g3) {      // x_mid = x_in + post_attention_norm(o_pre): d o_pre = norm'(d x_mid), then the o_proj dgrad
      RC(rmsnorm_bwd(sx, dt, v.dx, cur.o_pre, L.ln1_post, nullptr, v.d_n, nullptr, Mv, D, c.rms_eps, fl, nullptr, nullptr, rs));
      RC(gemm(sx, dt, lin_dgrad(v.d_n, Lt.wo_t, L.wo, v.d_o, Mv, s.OD, D)));
    } else if (!d_o_ready) RC(gemm(sx, dt, lin_dgrad(v.dx, Lt.wo_t, L.wo, v.d_o, Mv, s.OD, D)));
    if (lora && lora->layers[l].o.a) {   // o_proj adapter: its gradients from d (o_proj output) - Gemma-3: behind the post norm -, and d o += u . A_o
      const void* d_y = g3 ? v.d_n : v.dx;
      RC(lora_apply_bwd(sx, dt, cur.o, s.OD, d_y, D, cur.boT, at(cur.t2, 64, dt), at(v.lu2, 64, dt), d.lgrads->layers[l].o, Mv, s.OD, D, lora->r, lora->scaling,
                        v.lwg, lwg_floats()));
      RC(lora_up(sx, dt, at(v.lu2, 64, dt), 128, lora->layers[l].o.a, 1, v.d_o, s.OD, Mv, s.OD, lora->r, 1.0f, 1));
    }
    if (attention_needs_transposed_copies(dt)) RC(heads_transpose(sx, dt, cur.qkv, v.qT, Bv, T, s.Tp, Hq, dh, s.QKV));
    if (attention_needs_transposed_copies(dt)) RC(heads_transpose(sx, dt, at(cur.qkv, (size_t)Hq * dh, dt), v.kT, Bv, T, s.Tp, Hkv, dh, s.QKV));
    if (attention_needs_transposed_copies(dt)) RC(heads_transpose(sx, dt, v.d_o, v.doT, Bv, T, s.Tp, Hq, dh, s.OD));
    AttnBwdDesc bd;
    bd.f = causal_gqa_desc(c, cur.qkv, Bv, T, s.Tp, s.QKV, s.OD);
    bd.f.o = cur.o; bd.f.lse = cur.lse;
    bd.f.kv_start = v.kvs; bd.f.kv_len = v.kvl;  // written by the forward pass
    bd.f.window = window_of(c, w, l, T);
    bd.dout = v.d_o; bd.qt = v.qT; bd.kt = v.kT; bd.dot = v.doT; bd.delta = v.delta; bd.dkv_part = v.dkv_part;
    bd.dq = v.d_qkv; bd.dk = at(v.d_qkv, (size_t)Hq * dh, dt); bd.dv = at(v.d_qkv, (size_t)(Hq + Hkv) * dh, dt);
    bd.lddq = bd.lddk = bd.lddv = s.QKV;
    bd.d_first = rs.skip;
    const float* rope = rope_of(c, w, l);
    if (rope_fused) bd.rope_cos_sin = rope;
    if (!probe_skip(1)) RC(attention_bwd(sx, dt, bd));
    if (!rope_fused) RC(rope_inplace(sx, dt, v.d_qkv, rope, nullptr, Mv, T, Hq + Hkv, dh, s.QKV, 1));
    if (c.llm_qk_norm) RC(qk_norm_bwd(sx, dt, v.d_qkv, cur.qk_raw, L.q_norm, L.k_norm, Mv, Hq, Hkv, dh, s.QKV, c.rms_eps, g3 ? 1 : 0, rs));
    RC(gemm(sx, dt, lin_dgrad(v.d_qkv, Lt.wqkv_t, L.wqkv, v.d_n, Mv, D, s.QKV)));
    if (lora) {   // LoRA gradients of q_proj / k_proj (/ v_proj) and their contribution to d n1 (rank-r products, lora.hip)
      const uvx_enc_lora_layer_t& R = lora->layers[l];
      const uvx_enc_lora_layer_grads_t& G = d.lgrads->layers[l];
      const int r = lora->r, qc = Hq * dh, kc = Hkv * dh;
      void* dk = at(v.d_qkv, (size_t)qc, dt);
      void* dv = at(v.d_qkv, (size_t)(qc + kc), dt);
      if (R.q.a || R.k.a || R.v.a) RC(rmsnorm_fwd(sx, dt, cur.x_in, L.ln1, v.n, nullptr, Mv, D, c.rms_eps, fl));        // n1 recomputed
      if (R.q.a && R.k.a) {
        RC(lora_down(sx, dt, v.d_qkv, s.QKV, cur.bqT, 0, v.lu, 128, Mv, qc, r, lora->scaling));
        RC(lora_down(sx, dt, dk, s.QKV, cur.bkT, 0, at(v.lu, 64, dt), 128, Mv, kc, r, lora->scaling));
        const LoraWgradItem items[4] = {{v.n, D, v.lu, 128, G.q.a, D, 0, 1.0f}, {v.n, D, at(v.lu, 64, dt), 128, G.k.a, D, 0, 1.0f},
                                        {v.d_qkv, s.QKV, cur.t, 128, G.q.b, qc, 1, lora->scaling}, {dk, s.QKV, at(cur.t, 64, dt), 128, G.k.b, kc, 1, lora->scaling}};
        RC(lora_wgrad_batch(sx, dt, items, 4, Mv, r, v.lwg, lwg_floats()));
      } else {
        if (R.q.a) RC(lora_apply_bwd(sx, dt, v.n, D, v.d_qkv, s.QKV, cur.bqT, cur.t, v.lu, G.q, Mv, D, qc, r, lora->scaling, v.lwg, lwg_floats()));
        if (R.k.a) RC(lora_apply_bwd(sx, dt, v.n, D, dk, s.QKV, cur.bkT, at(cur.t, 64, dt), at(v.lu, 64, dt), G.k, Mv, D, kc, r, lora->scaling, v.lwg, lwg_floats()));
      }
      if (R.v.a) RC(lora_apply_bwd(sx, dt, v.n, D, dv, s.QKV, cur.bvT, cur.t2, v.lu2, G.v, Mv, D, kc, r, lora->scaling, v.lwg, lwg_floats()));
      if (R.q.a) RC(lora_up(sx, dt, v.lu, 128, R.q.a, 1, v.d_n, D, Mv, D, r, 1.0f, 1));
      if (R.k.a) RC(lora_up(sx, dt, at(v.lu, 64, dt), 128, R.k.a, 1, v.d_n, D, Mv, D, r, 1.0f, 1));
      if (R.v.a) RC(lora_up(sx, dt, v.lu2, 128, R.v.a, 1, v.d_n, D, Mv, D, r, 1.0f, 1));
    }
    return probe_skip(8) ? UVX_OK : rmsnorm_bwd(sx, dt, v.d_n, cur.x_in, L.ln1, resid, dx_out, nullptr, Mv, D, c.rms_eps, fl, nullptr, nullptr, rs, dx_full && rs.skip);
  }
};

int llm_forward(const LlmCallDesc& d) {
  RC(check_cfg(d.cfg));
  UVX_CHECK(d.w && d.inputs_embeds && d.workspace, UVX_ERR_INVALID, "llm_fwd: null argument");
  UVX_CHECK(!d.labels || d.loss, UVX_ERR_INVALID, "llm_fwd: labels given but no loss output");
  const uvx_config_t& c = *d.cfg;
  const int B = d.B, T = d.T, M = B * T, dt = c.dtype, D = c.llm_d;
  RC(llm_check(c, d.w, T));
  if (B == 0 || T == 0) return UVX_OK;
  // what the modes need of each other
  UVX_CHECK(!d.top_rows || (d.labels && d.loss && dt == DT_BF16 && d.save_for_bwd && !d.logits && !d.rows), UVX_ERR_INVALID,
            "llm_fwd_train: labels and a loss output are required, bf16 only");
  UVX_CHECK(!d.rows || dt == DT_BF16, UVX_ERR_UNSUPPORTED, "llm_fwd_rows: bf16 only");
  UVX_CHECK(!d.rows || (d.n_rows >= 0 && d.n_rows <= M), UVX_ERR_SHAPE, "llm_fwd_rows: %d rows of %d", d.n_rows, M);
  Arena a(d.workspace, d.ws_bytes);
  const LlmWalk k(d, llm_carve(a, c, B, T, d.save_for_bwd), d.save_for_bwd != 0);
  UVX_CHECK(a.fits(), UVX_ERR_WORKSPACE, "llm_fwd: workspace %zu < %zu bytes", d.ws_bytes, a.off);
  const LlmWs& s = k.s;
  const hipStream_t st = d.st;
  // valid-key range per sequence (kept in the workspace for the backward pass)
  if (d.attention_mask) hipLaunchKernelGGL(mask_range_k, dim3(B), dim3(256), 0, st, d.attention_mask, s.kvs, s.kvl, T);
  else hipLaunchKernelGGL(full_range_k, dim3(cdiv(B, 64)), dim3(64), 0, st, s.kvs, s.kvl, B, T);
  UVX_LAUNCH_CHECK();
  if (k.top && d.save_for_bwd) note_pair(d.workspace, k.tc);
  RC(embed_in(st, c, llm_layer(s, 0).x_in, d.inputs_embeds, M));
  // schedule: one chain on the caller's stream, or (option 11) the batch slices on several streams - see Fork above.  The
  // chains advance in lockstep (same kernel at the same time): a staggered start was measured 3.3 ms per step slower
  // (profiles/r03_two_stream_stagger_and_tiles_ab.txt).
  const Chains ch = make_chains(st, s, B, dt == DT_BF16 && !d.lora);
  RC(chains_fork(ch));
  int rc = UVX_OK;
  for (int l = 0; l < c.llm_layers && rc == UVX_OK; ++l) {
    const bool compact = k.tc && l + 1 == c.llm_layers;      // the last layer's second half follows the join, on the whole batch's listed rows
    for (int h = 0; h < ch.n && rc == UVX_OK; ++h) {
      rc = k.layer_attn(ch.st[h], ch.v[h], ch.B(h), l);
      if (rc == UVX_OK && !compact) rc = k.layer_mlp(ch.st[h], ch.v[h], l, false);
    }
  }
  RC(chains_join(ch));   // (also after an error above: the side streams must not be left forked)
  RC(rc);
  if (k.tc) RC(k.layer_mlp(st, s, c.llm_layers - 1, true));
  RC(rmsnorm_fwd(st, dt, s.x_final, d.w->norm, s.hn, nullptr, M, D, c.rms_eps, k.fl, k.tc ? s.sup + M : nullptr));   // (compact last layer: its rows only)
  return k.head_fwd();
}

int llm_backward(const LlmCallDesc& d) {
  RC(check_cfg(d.cfg));
  UVX_CHECK(d.w && d.d_inputs_embeds && d.workspace, UVX_ERR_INVALID, "llm_bwd: null argument");
  UVX_CHECK(d.first_pos >= 0 && d.first_pos <= d.T, UVX_ERR_INVALID, "llm_bwd: first_pos %d outside [0, T = %d]", d.first_pos, d.T);
  const uvx_config_t& c = *d.cfg;
  const uvx_llm_weights_t* w = d.w;
  const int B = d.B, T = d.T, M = B * T, dt = c.dtype, D = c.llm_d, last = c.llm_layers - 1;
  RC(llm_check(c, w, T));
  UVX_CHECK(c.llm_wt_stream || w->lm_head_t != nullptr, UVX_ERR_INVALID, "llm_bwd: transposed weights (lm_head_t, *_t) are required (or llm_wt_stream)");
  if (B == 0 || T == 0) return UVX_OK;
  // what the modes need of each other
  UVX_CHECK(!d.top_rows || (!d.compact_in_place && d.labels && dt == DT_BF16), UVX_ERR_INVALID, "llm_bwd_train: labels are required, bf16 only");
  UVX_CHECK(!d.compact_in_place || dt == DT_BF16, UVX_ERR_UNSUPPORTED, "llm_bwd_rows: bf16 only");
  for (int l = 0; l < c.llm_layers; ++l) {
    const uvx_llm_layer_t& L = w->layers[l];
    UVX_CHECK(c.llm_wt_stream || dt == DT_BF16 || (L.wd_t && L.wgu_t && L.wo_t && L.wqkv_t), UVX_ERR_INVALID,
              "llm_bwd: layer %d lacks transposed weights (f32: the NN form of the dgrads exists on the bf16 path only)", l);
  }
  Arena a(d.workspace, d.ws_bytes);
  LlmWalk k(d, llm_carve(a, c, B, T, 1), true);
  UVX_CHECK(a.fits(), UVX_ERR_WORKSPACE, "llm_bwd: workspace %zu < %zu bytes", d.ws_bytes, a.off);
  const LlmWs& s = k.s;
  const RowSkip& rs = k.rs;
  const hipStream_t st = d.st;
  const size_t es = esz(dt);
  // (after uvx_llm_fwd_train / uvx_llm_fwd_rows: the compact last-layer stash they noted must be the one this call expects)
  if (k.top) RC(check_pair(d.workspace, k.tc));

  const void* head_t = w->lm_head_t;
  WtStream* wt = nullptr;
  if (k.wts) {      // see layer_t
    wt = k.wt = wt_stream_for_device();
    UVX_CHECK(wt != nullptr, UVX_ERR_RUNTIME, "llm_bwd: could not create the weight-transpose stream");
    UVX_HIP(hipEventRecord(wt->e_start, st));                 // everything issued before (an earlier backward's reads of the buffers)
    UVX_HIP(hipStreamWaitEvent(wt->side, wt->e_start, 0));
    RC(transpose2d_streaming(wt->side, dt, w->lm_head, s.head_t, c.vocab, D, D, c.vocab));
    UVX_HIP(hipEventRecord(wt->e_head, wt->side));
    RC(k.issue_layer_t(last));
    UVX_HIP(hipStreamWaitEvent(st, wt->e_head, 0));
    head_t = s.head_t;
  }
  RC(k.head_bwd(head_t));
  // the final norm.  tc: the last layer's stash (x_final, x_mid, gate|up) holds the listed rows only; its MLP / o_proj gradients run on those
  // rows and are scattered back before the attention backward
  const int32_t* mdev_top = k.tc ? s.sup + M : nullptr;
  if (rs.skip) UVX_HIP(hipMemsetAsync(d.d_inputs_embeds, 0, (size_t)M * D * es, st));      // (layer 0 writes the rows >= rs.skip of every sequence)
  if (k.tc) {
    RC(gather_rows(st, dt, s.d_hn, s.sup, M, s.d_n, D));                 // d_hn was scattered to full rows: back to compact
    RC(rmsnorm_bwd(st, dt, s.d_n, s.x_final, w->norm, nullptr, s.dx, nullptr, M, D, c.rms_eps, k.fl, mdev_top));
  } else if (rs.skip) {      // (no compact last layer - Gemma-3, option 3 = 0: the final norm's backward on every row, then the kept rows to the front)
    RC(rmsnorm_bwd(st, dt, s.d_hn, s.x_final, w->norm, nullptr, s.d_n, nullptr, M, D, c.rms_eps, k.fl));
    RC(take_rows_from(st, dt, s.d_n, s.dx, B * rs.tc, D, rs));
  } else {
    RC(rmsnorm_bwd(st, dt, s.d_hn, s.x_final, w->norm, nullptr, s.dx, nullptr, M, D, c.rms_eps, k.fl));
  }
  if (k.wts) UVX_HIP(hipStreamWaitEvent(st, wt->e_ready[last & 1], 0));
  if (k.tc) {   // last layer: MLP and o_proj gradients on the compact rows (whole batch, this stream), then d o and the
                // residual-stream gradient go back to their full rows for the attention backward
    RC(k.layer_mlp_bwd(st, s, last, true));
    GemmDesc g = lin_dgrad(s.dx, k.layer_t(last).wo_t, w->layers[last].wo, s.doT, M, s.OD, D);     // doT ([B, Hq, Tp, dh] >= M * OD) is free until the transpose
    g.m_dev = mdev_top;
    RC(gemm(st, dt, g));
    const int32_t* rows_to = s.sup;
    if (rs.skip) {      // the listed rows' places among the row-compacted gradients
      RC(compact_row_list(st, s.sup, s.sup_c, M, T, rs.skip));
      rows_to = s.sup_c;
    }
    UVX_HIP(hipMemsetAsync(s.d_o, 0, (size_t)M * s.OD * es, st));
    RC(scatter_rows(st, dt, s.doT, rows_to, M, s.d_o, s.OD));
    UVX_HIP(hipMemsetAsync(s.d_hn, 0, (size_t)M * D * es, st));
    RC(scatter_rows(st, dt, s.dx, rows_to, M, s.d_hn, D));
  }
  // schedule: one chain on the caller's stream, or (option 11) the batch slices on several streams - see Fork above
  const Chains ch = make_chains(st, s, B, dt == DT_BF16 && !d.lora && !k.wts);
  RC(chains_fork(ch));
  int rc = UVX_OK;
  for (int l = last; l >= 0 && rc == UVX_OK; --l) {
    const bool compact = k.tc && l == last;
    if (k.wts) {      // this layer's W^T must have landed; the next one's is started now, into the buffer layer l + 1 has released
      if (l != last && hipStreamWaitEvent(st, wt->e_ready[l & 1], 0) != hipSuccess) rc = UVX_ERR_RUNTIME;
      if (l > 0 && rc == UVX_OK) rc = k.issue_layer_t(l - 1);
    }
    for (int h = 0; h < ch.n && rc == UVX_OK; ++h) {
      const LlmWs& v = ch.v[h];
      if (!compact) rc = k.layer_mlp_bwd(ch.st[h], v, l, false);
      void* dx_out = l == 0 ? (void*)((char*)d.d_inputs_embeds + (size_t)ch.b0[h] * T * D * es) : v.dx;
      if (rc == UVX_OK) rc = k.layer_attn_bwd(ch.st[h], v, ch.B(h), l, compact, compact ? v.d_hn : v.dx, dx_out, l == 0);
    }
    if (k.wts && hipEventRecord(wt->e_free[l & 1], st) != hipSuccess && rc == UVX_OK) rc = UVX_ERR_RUNTIME;
  }
  RC(chains_join(ch));   // (also after an error above: the side streams must not be left forked)
  RC(rc);
  if (k.fl == UVX_LLM_GEMMA) RC(scale_inplace(st, dt, d.d_inputs_embeds, (long long)M * D, gemma_normalizer(c)));   // d (x * normalizer)
  return UVX_OK;
}

// the part of a call descriptor every entry point fills
LlmCallDesc llm_call(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, int32_t B, int32_t T, void* workspace, size_t ws_bytes) {
  LlmCallDesc d;
  d.st = (hipStream_t)stream; d.cfg = cfg; d.w = w; d.B = B; d.T = T; d.workspace = workspace; d.ws_bytes = ws_bytes;
  return d;
}

}  // namespace

// =====================================================================================
extern "C" size_t uvx_llm_ws_bytes(const uvx_config_t* cfg, int32_t B, int32_t T, int32_t save_for_bwd) {
  if (!cfg) return 0;
  Arena a(nullptr, 0);
  llm_carve(a, *cfg, B, T, save_for_bwd);
  return a.off + 256;
}

extern "C" int32_t uvx_llm_fwd(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, const void* inputs_embeds,
                               const int64_t* attention_mask, const int64_t* labels, int32_t B, int32_t T, void* logits,
                               float* loss, int32_t save_for_bwd, void* workspace, size_t ws_bytes) {
  LlmCallDesc d = llm_call(stream, cfg, w, B, T, workspace, ws_bytes);
  d.inputs_embeds = inputs_embeds; d.attention_mask = attention_mask;
  d.labels = labels; d.loss = loss; d.logits = logits; d.save_for_bwd = save_for_bwd;
  return llm_forward(d);
}

extern "C" int32_t uvx_llm_fwd_rows(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, const void* inputs_embeds,
                                    const int64_t* attention_mask, int32_t B, int32_t T, const int32_t* rows, int32_t n_rows,
                                    void* logits_rows, int32_t save_for_bwd, void* workspace, size_t ws_bytes) {
  UVX_CHECK(rows != nullptr, UVX_ERR_INVALID, "llm_fwd_rows: null row list");
  LlmCallDesc d = llm_call(stream, cfg, w, B, T, workspace, ws_bytes);
  d.inputs_embeds = inputs_embeds; d.attention_mask = attention_mask;
  d.rows = rows; d.n_rows = n_rows; d.logits_rows = logits_rows; d.save_for_bwd = save_for_bwd;
  return llm_forward(d);
}

// KL loss on the compact student rows left by uvx_llm_fwd_rows(save_for_bwd = 1): pair [2][n_rows] = index into the teacher's
// compact rows (or -1), weights alike; d loss / d logits replaces the compact logits in place.
extern "C" int32_t uvx_llm_kl_loss_rows(void* stream, const uvx_config_t* cfg, const void* teacher_logits_rows,
                                        const int32_t* pair, const float* pair_w, int32_t B, int32_t T, int32_t n_rows,
                                        float temperature, float grad_scale, float* loss, void* workspace, size_t ws_bytes) {
  RC(check_cfg(cfg));
  UVX_CHECK(teacher_logits_rows && pair && pair_w && loss && workspace, UVX_ERR_INVALID, "llm_kl_loss_rows: null argument");
  const uvx_config_t& c = *cfg;
  if (B == 0 || T == 0) return UVX_OK;
  Arena a(workspace, ws_bytes);
  LlmWs s = llm_carve(a, c, B, T, 1);
  UVX_CHECK(a.fits(), UVX_ERR_WORKSPACE, "llm_kl_loss_rows: workspace %zu < %zu bytes", ws_bytes, a.off);
  UVX_CHECK(n_rows > 0 && n_rows <= s.M, UVX_ERR_SHAPE, "llm_kl_loss_rows: %d rows of %d", n_rows, s.M);
  return kl_loss_fwd_bwd((hipStream_t)stream, c.dtype, s.logits, teacher_logits_rows, pair, pair_w, loss, s.ce_scratch + 2,
                         s.logits, (long long)n_rows, c.vocab, c.vocab, c.vocab, temperature, grad_scale);
}

extern "C" int32_t uvx_llm_kl_loss(void* stream, const uvx_config_t* cfg, const void* teacher_logits, int64_t teacher_rows,
                                   const int32_t* pair_row, const float* pair_w, int32_t B, int32_t T, float temperature,
                                   float grad_scale, float* loss, void* workspace, size_t ws_bytes) {
  RC(check_cfg(cfg));
  UVX_CHECK(teacher_logits && pair_row && pair_w && loss && workspace, UVX_ERR_INVALID, "llm_kl_loss: null argument");
  UVX_CHECK(teacher_rows > 0, UVX_ERR_SHAPE, "llm_kl_loss: no teacher rows");
  const uvx_config_t& c = *cfg;
  if (B == 0 || T == 0) return UVX_OK;
  Arena a(workspace, ws_bytes);
  LlmWs s = llm_carve(a, c, B, T, 1);
  UVX_CHECK(a.fits(), UVX_ERR_WORKSPACE, "llm_kl_loss: workspace %zu < %zu bytes", ws_bytes, a.off);
  // student logits were left in the workspace by uvx_llm_fwd(save_for_bwd = 1); their gradient replaces them
  return kl_loss_fwd_bwd((hipStream_t)stream, c.dtype, s.logits, teacher_logits, pair_row, pair_w, loss, s.ce_scratch + 2,
                         s.logits, (long long)s.M, c.vocab, c.vocab, c.vocab, temperature, grad_scale);
}

extern "C" int32_t uvx_llm_bwd(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, const int64_t* labels,
                               int32_t B, int32_t T, float grad_scale, void* d_inputs_embeds, void* workspace,
                               size_t ws_bytes) {
  LlmCallDesc d = llm_call(stream, cfg, w, B, T, workspace, ws_bytes);
  d.labels = labels; d.grad_scale = grad_scale; d.d_inputs_embeds = d_inputs_embeds;
  return llm_backward(d);
}

// The adapter-training step's own pair (include/uvx.h): identical loss and gradients to uvx_llm_fwd(save_for_bwd = 1, logits =
// NULL) + uvx_llm_bwd, with the last layer's o_proj / MLP / final norm and their gradients on the supervised rows only.
extern "C" int32_t uvx_llm_fwd_train(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, const void* inputs_embeds,
                                     const int64_t* attention_mask, const int64_t* labels, int32_t B, int32_t T, float* loss,
                                     void* workspace, size_t ws_bytes) {
  LlmCallDesc d = llm_call(stream, cfg, w, B, T, workspace, ws_bytes);
  d.inputs_embeds = inputs_embeds; d.attention_mask = attention_mask;
  d.labels = labels; d.loss = loss; d.save_for_bwd = 1; d.top_rows = true;
  return llm_forward(d);
}
// ... when the caller needs no gradient below position first_pos of any sequence (include/uvx.h)
extern "C" int32_t uvx_llm_bwd_train_from(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, const int64_t* labels,
                                          int32_t B, int32_t T, int32_t first_pos, float grad_scale, void* d_inputs_embeds, void* workspace,
                                          size_t ws_bytes) {
  LlmCallDesc d = llm_call(stream, cfg, w, B, T, workspace, ws_bytes);
  d.labels = labels; d.grad_scale = grad_scale; d.d_inputs_embeds = d_inputs_embeds;
  d.top_rows = true; d.first_pos = first_pos;
  return llm_backward(d);
}
extern "C" int32_t uvx_llm_bwd_train(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, const int64_t* labels,
                                     int32_t B, int32_t T, float grad_scale, void* d_inputs_embeds, void* workspace,
                                     size_t ws_bytes) {
  return uvx_llm_bwd_train_from(stream, cfg, w, labels, B, T, 0, grad_scale, d_inputs_embeds, workspace, ws_bytes);
}

// LLM under LoRA training (text_model_lora_config.r > 0, apply_lora on the language model, ultravox_model.py:500-526):
// the forward adds the adapters to q_proj / k_proj, the backward also returns their gradients.
extern "C" int32_t uvx_llm_fwd_lora(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, const uvx_encoder_lora_t* lora,
                                    const void* inputs_embeds, const int64_t* attention_mask, const int64_t* labels, int32_t B,
                                    int32_t T, void* logits, float* loss, int32_t save_for_bwd, void* workspace, size_t ws_bytes) {
  RC(check_cfg(cfg));
  RC(lora_check(lora, cfg->llm_layers, nullptr, "llm_fwd_lora"));
  LlmCallDesc d = llm_call(stream, cfg, w, B, T, workspace, ws_bytes);
  d.inputs_embeds = inputs_embeds; d.attention_mask = attention_mask;
  d.labels = labels; d.loss = loss; d.logits = logits; d.save_for_bwd = save_for_bwd; d.lora = lora;
  return llm_forward(d);
}
extern "C" int32_t uvx_llm_bwd_lora(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, const uvx_encoder_lora_t* lora,
                                    const int64_t* labels, int32_t B, int32_t T, float grad_scale, void* d_inputs_embeds,
                                    const uvx_encoder_lora_grads_t* grads, void* workspace, size_t ws_bytes) {
  RC(check_cfg(cfg));
  UVX_CHECK(grads && grads->layers, UVX_ERR_INVALID, "llm_bwd_lora: bad LoRA descriptor");
  RC(lora_check(lora, cfg->llm_layers, grads, "llm_bwd_lora"));
  LlmCallDesc d = llm_call(stream, cfg, w, B, T, workspace, ws_bytes);
  d.labels = labels; d.grad_scale = grad_scale; d.d_inputs_embeds = d_inputs_embeds;
  d.lora = lora; d.lgrads = grads;
  return llm_backward(d);
}

extern "C" int32_t uvx_llm_bwd_rows_from(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, int32_t B, int32_t T, int32_t first_pos,
                                         void* d_inputs_embeds, void* workspace, size_t ws_bytes) {
  LlmCallDesc d = llm_call(stream, cfg, w, B, T, workspace, ws_bytes);
  d.d_inputs_embeds = d_inputs_embeds; d.compact_in_place = true; d.first_pos = first_pos;
  return llm_backward(d);
}
extern "C" int32_t uvx_llm_bwd_rows(void* stream, const uvx_config_t* cfg, const uvx_llm_weights_t* w, int32_t B, int32_t T,
                                    void* d_inputs_embeds, void* workspace, size_t ws_bytes) {
  return uvx_llm_bwd_rows_from(stream, cfg, w, B, T, 0, d_inputs_embeds, workspace, ws_bytes);
}
