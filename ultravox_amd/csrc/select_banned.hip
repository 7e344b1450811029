// Token selection behind HF's token-ban score processors, still one launch per token: uvx_greedy_select_banned, uvx_sample_select_banned.
//
// Reference: [3P] GenerationMixin._sample with a LogitsProcessorList in front of the argmax / the warpers, as the reference's inference path
// reaches it (ultravox_model.py:422-426 forwards every generate keyword to language_model.generate).
//
// banned_select_k is select.hip's 2 x 2 table once more with every reader wrapped in BannedRow (ban.h): the row's block first rebuilds the
// row's ban bitmap from the sequence so far (ban_build), then argmax_row / sample_row read the row through it, unchanged, and the loop's
// bookkeeping follows (select.h).  A translation unit of its own: select.hip's set of kernels stays what it was.
#include "ban.h"
#include "select.h"

namespace {

struct Ban {
  uvx_ban_rules_t rules;
  uint32_t flags;
  uint32_t* ban;        // [B][words]
  int words;
};

template <typename T, bool PENALIZED, typename Pick>
__global__ void __launch_bounds__(NT) banned_select_k(const T* __restrict__ logits, int V, Penalty p, Ban bn, Pick pick, Book k) {
  const int b = blockIdx.x;
  const T* r = logits + (long long)b * V;
  uint32_t* seen = PENALIZED ? p.seen + (long long)b * p.words : nullptr;
  uint32_t* ban = bn.ban + (long long)b * bn.words;
  ban_build(ban, V, bn.rules, bn.flags, k.sequences + (long long)b * k.stride, k.col);      // (ends in a barrier: marking before reading)
  const bool forced = bn.flags & UVX_BAN_FORCED;
  const auto rd = [&] {
    if constexpr (PENALIZED) return BannedRow<PenalizedRow<T>>{{r, seen, p.penalty}, ban, forced};
    else return BannedRow<PlainRow<T>>{{r}, ban, forced};
  }();
  int token;
  if constexpr (std::is_same<Pick, SampleArgs>::value) {
    __shared__ Lds s;
    token = sample_row(rd, V, pick, b, s);
    if constexpr (PENALIZED) __syncthreads();     // every thread's reads of `seen` lie before this barrier
  } else {
    token = argmax_row(rd, V, pick.scores_out ? pick.scores_out + (long long)b * V : nullptr);      // (its own barrier does the same)
  }
  if (threadIdx.x != 0) return;
  const int64_t tok = select_bookkeeping(b, token, k);
  // the token WRITTEN joins the row's `seen` words, as in select_k
  if constexpr (PENALIZED)
    if (tok >= 0 && tok < V) seen[tok >> 5] |= 1u << (tok & 31);
}

// after check_select: the rule struct and the flag word
int check_ban(const char* name, const uvx_ban_rules_t& r, uint32_t flags) {
  UVX_CHECK(r.ngram >= 0 && r.n_bad >= 0 && r.n_bad_tokens >= 0 && r.n_min >= 0 && r.n_forced >= 0 && r.n_suppress >= 0 && r.n_begin >= 0,
            UVX_ERR_INVALID, "%s: rules: ngram=%d n_bad=%d n_bad_tokens=%d n_min=%d n_forced=%d n_suppress=%d n_begin=%d have to be non-negative", name,
            r.ngram, r.n_bad, r.n_bad_tokens, r.n_min, r.n_forced, r.n_suppress, r.n_begin);
  UVX_CHECK((r.n_bad == 0 || (r.bad_offsets && (r.bad_tokens || r.n_bad_tokens == 0))) && (r.n_min == 0 || r.min_ids) && (r.n_forced == 0 || r.forced_ids) &&
                (r.n_suppress == 0 || r.suppress_ids) && (r.n_begin == 0 || r.begin_ids),
            UVX_ERR_INVALID, "%s: rules: a null list with a count above 0", name);
  UVX_CHECK((flags & ~(UVX_BAN_MIN | UVX_BAN_FORCED | UVX_BAN_BEGIN)) == 0, UVX_ERR_INVALID, "%s: flags=0x%x", name, flags);
  return UVX_OK;
}

template <typename Pick>
int launch_banned(void* stream, int dtype, const void* logits, int B, int V, const Penalty& p, const Ban& bn, const Pick& pick, const Book& k) {
  if (B == 0) return UVX_OK;
  hipStream_t st = (hipStream_t)stream;
#define UVX_BANNED(T, PEN) hipLaunchKernelGGL((banned_select_k<T, PEN, Pick>), dim3(B), dim3(NT), 0, st, (const T*)logits, V, p, bn, pick, k)
  if (dtype == DT_BF16) {
    if (p.seen) UVX_BANNED(bf16_t, true);
    else UVX_BANNED(bf16_t, false);
  } else {
    if (p.seen) UVX_BANNED(float, true);
    else UVX_BANNED(float, false);
  }
#undef UVX_BANNED
  UVX_LAUNCH_CHECK();
  return UVX_OK;
}

// the checks of both entry points in their order: null pointers, shape, values
template <typename Pick>
int select_banned(const char* name, void* stream, int dtype, const void* logits, int B, int V, float penalty, uint32_t* seen, int words, const SampleArgs* a,
                  const Pick& pick, const uvx_ban_rules_t* rules, uint32_t flags, uint32_t* ban, int ban_words, const Book& k) {
  UVX_CHECK(rules && ban, UVX_ERR_INVALID, "%s: null argument", name);
  const Penalty p{penalty, seen, words};
  // check_select sees the smaller of the two bitmaps' widths (every shape error before any value error), and without a penalty a penalty of 1
  // over the ban buffer: it then tests the dtype and V < 2^23 as for a penalised call
  const Penalty checked{seen ? penalty : 1.0f, seen ? seen : ban, seen && words < ban_words ? words : ban_words};
  if (const int rc = check_select(name, dtype, logits, B, V, &checked, a, k)) return rc;
  if (const int rc = check_ban(name, *rules, flags)) return rc;
  return launch_banned(stream, dtype, logits, B, V, p, Ban{*rules, flags, ban, ban_words}, pick, k);
}

}  // namespace

extern "C" int32_t uvx_greedy_select_banned(void* stream, int32_t logits_dtype, const void* logits, int32_t B, int32_t V, float penalty, uint32_t* seen,
                                            int32_t words, float* scores_out, const uvx_ban_rules_t* rules, uint32_t flags, uint32_t* ban,
                                            int32_t ban_words, UVX_BOOK_PARAMS) {
  return select_banned("greedy_select_banned", stream, logits_dtype, logits, B, V, penalty, seen, words, nullptr, ArgmaxArgs{scores_out}, rules, flags, ban,
                       ban_words, UVX_BOOK);
}

extern "C" int32_t uvx_sample_select_banned(void* stream, int32_t logits_dtype, const void* logits, int32_t B, int32_t V, float penalty, uint32_t* seen,
                                            int32_t words, float temperature, int32_t top_k, float top_p, float min_p, int32_t min_keep, uint64_t seed,
                                            uint64_t offset, const float* uniforms, float* probs_out, const uvx_ban_rules_t* rules, uint32_t flags,
                                            uint32_t* ban, int32_t ban_words, UVX_BOOK_PARAMS) {
  const SampleArgs a{temperature, top_p, min_p, top_k, min_keep, seed, offset, uniforms, probs_out};
  return select_banned("sample_select_banned", stream, logits_dtype, logits, B, V, penalty, seen, words, &a, a, rules, flags, ban, ban_words, UVX_BOOK);
}

#undef UVX_BOOK_PARAMS
#undef UVX_BOOK
