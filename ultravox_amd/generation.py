"""Score processors, warpers and stopping criteria of `generate(**kwargs)`.

The reference hands every keyword of `UltravoxModel.generate` to [3P] HF `GenerationMixin.generate` (ultravox_model.py:398-426), which turns the
generation-config fields into a LogitsProcessorList applied to the f32 scores of the last position before the argmax / the multinomial draw
(transformers/generation/utils.py `_get_logits_processor`; logits_process.py).  This module restates the processors the decode loop of
`ultravox_amd/model.py` applies on its one `[B, V]` row per step - host-side policy on device tensors, not a kernel.  Each function cites the HF class it
restates; tests/test_generate_host_cpu.py pins every one of them against that class on random inputs, and the whole loop against HF `generate`
through the oracle.

Order (HF's): repetition_penalty, no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens, forced_eos_token_id, suppress_tokens,
begin_suppress_tokens, then the caller's own `logits_processor` callables; sampling adds temperature -> top_k -> top_p -> min_p (model.py `_sample`).
Keywords of HF's generation config that would change the tokens and are NOT built raise instead of being ignored.

The repetition penalty and the seven token-ban processors also exist as kernels (uvx_greedy_select_penalized / uvx_greedy_select_banned and their
sampling twins, include/uvx.h): where every active processor is one of those, model.py's device loop takes them and `ScoreProcessors` only hands it
the rule lists (`device_rules`) and the per-step flags (`step_flags`); the restatements below stay the host loop's and the beam search's.
"""
from typing import Callable, List, Optional, Sequence

import torch

NEG_INF = float("-inf")

# generation-config fields HF would act on and this loop does not implement: refused by name (a warning would return other tokens than the reference)
UNBUILT = ("max_length", "max_time", "stop_strings", "penalty_alpha", "dola_layers", "typical_p", "epsilon_cutoff", "eta_cutoff", "diversity_penalty",
           "encoder_repetition_penalty", "encoder_no_repeat_ngram_size", "force_words_ids", "constraints", "renormalize_logits", "forced_bos_token_id",
           "remove_invalid_values", "exponential_decay_length_penalty", "sequence_bias", "token_healing", "guidance_scale", "watermarking_config",
           "num_beam_groups", "prefix_allowed_tokens_fn", "assistant_model", "prompt_lookup_num_tokens", "cache_implementation", "generation_config",
           "negative_prompt_ids", "temperature_last", "top_h")
# fields that only select what is reported / how HF manages its own cache: no effect on the tokens
HARMLESS = ("use_cache", "output_attentions", "output_hidden_states", "synced_gpus", "return_legacy_cache", "use_model_defaults", "tokenizer",
            "bos_token_id", "decoder_start_token_id", "trust_remote_code", "custom_generate")
HANDLED = ("no_repeat_ngram_size", "bad_words_ids", "min_length", "min_new_tokens", "forced_eos_token_id", "suppress_tokens", "begin_suppress_tokens",
           "logits_processor", "stopping_criteria", "min_p")


def repetition_penalty_(scores: torch.Tensor, seen_ids: torch.Tensor, penalty: float) -> torch.Tensor:
    """[3P] RepetitionPenaltyLogitsProcessor: every id already in the sequence - prompt, padding and generated tokens alike - has its score divided by
    the penalty if positive, multiplied if negative.  scores f32 [B, V] (modified in place), seen_ids int64 [B, n]."""
    s = torch.gather(scores, 1, seen_ids)
    s = torch.where(s < 0, s * penalty, s / penalty)
    return scores.scatter_(1, seen_ids, s)


def no_repeat_ngram_(scores: torch.Tensor, ids: torch.Tensor, n: int) -> torch.Tensor:
    """[3P] NoRepeatNGramLogitsProcessor: a token that would complete an n-gram already present in the row (prompt included) gets -inf.  For the last
    n - 1 tokens `p` of a row, every position j with ids[j : j + n - 1] == p bans ids[j + n - 1]."""
    B, L = ids.shape
    if n <= 0 or L < n:                           # (no complete n-gram in the row yet)
        return scores
    if n == 1:                                   # every token already present is banned
        return scores.scatter_(1, ids, NEG_INF)
    win = ids.unfold(1, n, 1)                     # [B, L - n + 1, n]: all n-grams of the row
    match = (win[:, :, : n - 1] == ids[:, None, L - (n - 1):]).all(-1)      # n-grams whose first n - 1 tokens are the current suffix
    banned = win[:, :, n - 1]
    rows, cols = torch.nonzero(match, as_tuple=True)
    scores[rows, banned[rows, cols]] = NEG_INF
    return scores


def bad_words_(scores: torch.Tensor, ids: torch.Tensor, bad_words_ids: Sequence[Sequence[int]], eos_ids: Sequence[int]) -> torch.Tensor:
    """[3P] NoBadWordsLogitsProcessor (a SequenceBiasLogitsProcessor with -inf): a one-token entry is always banned; the last token of a longer entry is
    banned in the rows whose tail equals the entry's prefix.  Entries equal to a lone EOS id are dropped, as HF does."""
    words = [list(map(int, w)) for w in bad_words_ids if not (len(w) == 1 and int(w[0]) in set(map(int, eos_ids)))]
    L = ids.shape[1]
    for w in words:
        if len(w) == 1:
            scores[:, w[0]] = NEG_INF
        elif len(w) <= L:                           # (HF skips an entry longer than the context)
            prefix = torch.tensor(w[:-1], device=ids.device, dtype=ids.dtype)
            hit = (ids[:, L - len(prefix):] == prefix).all(-1)
            scores[hit, w[-1]] = NEG_INF
    return scores


def suppress_(scores: torch.Tensor, token_ids: Sequence[int]) -> torch.Tensor:
    """[3P] MinLength / MinNewTokensLength / SuppressTokens (the same mask: the listed ids to -inf)."""
    if len(token_ids):
        scores[:, torch.as_tensor(list(map(int, token_ids)), device=scores.device, dtype=torch.int64)] = NEG_INF
    return scores


def force_(scores: torch.Tensor, token_ids: Sequence[int]) -> torch.Tensor:
    """[3P] ForcedEOSTokenLogitsProcessor at the last position: everything to -inf, the forced ids to 0."""
    scores.fill_(NEG_INF)
    scores[:, torch.as_tensor(list(map(int, token_ids)), device=scores.device, dtype=torch.int64)] = 0.0
    return scores


def min_p_(x: torch.Tensor, min_p: float, min_tokens_to_keep: int = 1) -> torch.Tensor:
    """[3P] MinPLogitsWarper: tokens whose probability is below min_p x the row's top probability are removed (at least min_tokens_to_keep stay)."""
    probs = torch.softmax(x, dim=-1)
    remove = probs < min_p * probs.amax(dim=-1, keepdim=True)
    order = torch.argsort(x, dim=-1, descending=True)
    keep_top = torch.zeros_like(remove).scatter_(1, order[:, :min_tokens_to_keep], True)
    return x.masked_fill(remove & ~keep_top, NEG_INF)


class PhiloxGenerator:
    """The random stream of the device sampler (uvx_sample_select, include/uvx.h): a host object holding the Philox4x32-10 key (`seed`) and the
    counter's low 64 bits (`offset`).  Decode step s of a generate() call draws row b's uniform from counter (offset + s, b); the call then
    advances the offset by the steps it ran, so consecutive calls never reuse a counter and a (seed, offset) pair replays a call.
    penalty_on_device=True additionally lets generate() take a `repetition_penalty` that is the only score processor onto the device
    (uvx_seen_mark + uvx_sample_select_penalized); without the flag that combination is refused.  processors_on_device=True implies it and also
    takes the token-ban processors (no_repeat_ngram_size, bad_words_ids, min_length, min_new_tokens, forced_eos_token_id, suppress_tokens,
    begin_suppress_tokens, alone or next to the penalty) onto the device (uvx_sample_select_banned); without that flag they are refused, and a
    caller's own `logits_processor` is refused either way."""
    MASK = (1 << 64) - 1

    def __init__(self, seed: int = 0, penalty_on_device: bool = False, processors_on_device: bool = False):
        self.processors_on_device = bool(processors_on_device)
        self.penalty_on_device = bool(penalty_on_device) or self.processors_on_device
        self.manual_seed(seed)

    def manual_seed(self, seed: int) -> "PhiloxGenerator":
        self.seed, self.offset = int(seed) & self.MASK, 0
        return self

    def advance(self, n: int) -> "PhiloxGenerator":
        if n < 0:
            raise ValueError(f"PhiloxGenerator.advance: n has to be non-negative, but is {n}")
        self.offset = (self.offset + int(n)) & self.MASK
        return self


def _ids(v) -> List[int]:
    if v is None:
        return []
    if isinstance(v, torch.Tensor):
        return [int(t) for t in v.reshape(-1).tolist()]
    return [int(t) for t in v] if isinstance(v, (list, tuple)) else [int(v)]


def check_kwargs(kwargs: dict, known: Sequence[str]) -> List[str]:
    """Sort generate()'s extra keywords: the unbuilt ones raise, the harmless ones are returned for a warning, unknown names raise like HF's
    `_validate_model_kwargs` ("The following `model_kwargs` are not used by the model")."""
    extra = set(kwargs) - set(known) - set(HANDLED)
    refused = sorted(k for k in extra if k in UNBUILT and kwargs[k] is not None)
    if refused:
        raise NotImplementedError(f"generate(): {refused} are not built (HF `generate` would act on them; ignoring them would return other tokens than "
                                  "the reference)")
    unknown = sorted(k for k in extra if k not in UNBUILT and k not in HARMLESS)
    if unknown:
        raise ValueError(f"The following `model_kwargs` are not used by the model: {unknown} (note: typos in the generate arguments will also show up in "
                         "this list)")
    return sorted(k for k in extra if k in HARMLESS)


class ScoreProcessors:
    """The processor list of one generate() call.  __call__(ids [B, L] incl. the prompt, scores f32 [B, V]) -> scores, applied before argmax / sampling."""

    def __init__(self, kwargs: dict, prompt_len: int, max_new_tokens: int, eos_ids: Sequence[int], repetition_penalty: Optional[float] = None):
        g = kwargs.get
        self.rep = repetition_penalty
        self.ngram = int(g("no_repeat_ngram_size") or 0)
        self.bad_words = g("bad_words_ids") or []
        for w in self.bad_words:
            if not isinstance(w, (list, tuple)) or not len(w) or any((not isinstance(t, int)) or t < 0 for t in w):
                raise ValueError(f"`bad_words_ids` has to be a list of non-empty lists of positive integers, but is {self.bad_words}.")
        self.eos = list(map(int, eos_ids))
        self.min_length = int(g("min_length") or 0)
        self.min_new = int(g("min_new_tokens") or 0)
        self.forced_eos = _ids(g("forced_eos_token_id"))
        self.suppress = _ids(g("suppress_tokens"))
        self.begin_suppress = _ids(g("begin_suppress_tokens"))
        self.user: List[Callable] = list(g("logits_processor") or [])
        self.prompt_len, self.max_len = int(prompt_len), int(prompt_len) + int(max_new_tokens)
        if self.ngram < 0:
            raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {self.ngram}")

    @property
    def active(self) -> bool:
        return bool(self.rep is not None or self.ngram or self.bad_words or self.min_length > 0 or self.min_new > 0 or self.forced_eos or self.suppress
                    or self.begin_suppress or self.user)

    @property
    def only_repetition_penalty(self) -> bool:
        """The repetition penalty is the one active processor: what uvx_greedy_select_penalized and uvx_sample_select_penalized do on the device."""
        return bool(self.rep is not None and not (self.ngram or self.bad_words or self.min_length > 0 or self.min_new > 0 or self.forced_eos
                                                  or self.suppress or self.begin_suppress or self.user))

    # ---- the same rule set for the banned selectors (uvx_greedy_select_banned / uvx_sample_select_banned, include/uvx.h) ----
    @property
    def bans(self) -> bool:
        """One of the seven token-ban processors is active."""
        return bool(self.ngram or self.bad_words or self.min_length > 0 or self.min_new > 0 or self.forced_eos or self.suppress or self.begin_suppress)

    def _kept_bad_words(self) -> List[List[int]]:
        eos = set(self.eos)
        return [list(map(int, w)) for w in self.bad_words if not (len(w) == 1 and int(w[0]) in eos)]      # (as bad_words_ drops them)

    def on_device(self, vocab: int) -> bool:
        """Every active processor is one the banned selectors express: a ban rule is active, no caller `logits_processor`, and every listed id lies
        in [0, vocab) (torch indexes with the others - wrapping or raising; that stays the host loop's business)."""
        listed = [t for w in self._kept_bad_words() for t in w] + self.forced_eos + self.suppress + self.begin_suppress
        return bool(self.bans and not self.user and all(0 <= t < vocab for t in listed))

    def device_rules(self, device) -> dict:
        """The rule lists uploaded once per generate() call: the fields of uvx_ban_rules_t, the pointers as tensors (None for an empty list)."""
        def ids(v, dtype=torch.int64):
            return torch.tensor(v, device=device, dtype=dtype) if len(v) else None
        words = self._kept_bad_words()
        offsets = [0]
        for w in words:
            offsets.append(offsets[-1] + len(w))
        min_ids = [e for e in self.eos if e >= 0] if (self.min_length > 0 or self.min_new > 0) else []
        return dict(bad_tokens=ids([t for w in words for t in w]), bad_offsets=ids(offsets, torch.int32) if words else None, min_ids=ids(min_ids),
                    forced_ids=ids(self.forced_eos), suppress_ids=ids(self.suppress), begin_ids=ids(self.begin_suppress), ngram=self.ngram,
                    n_bad=len(words), n_bad_tokens=offsets[-1], n_min=len(min_ids), n_forced=len(self.forced_eos), n_suppress=len(self.suppress),
                    n_begin=len(self.begin_suppress))

    def step_flags(self, L: int) -> int:
        """The step-dependent conditions of __call__ for a row of length L (the same for every row): UVX_BAN_MIN | UVX_BAN_FORCED | UVX_BAN_BEGIN."""
        short = (self.min_length > 0 and L < self.min_length) or (self.min_new > 0 and L - self.prompt_len < self.min_new)
        return ((1 if short and any(e >= 0 for e in self.eos) else 0) | (2 if self.forced_eos and L == self.max_len - 1 else 0)
                | (4 if self.begin_suppress and L == self.prompt_len else 0))

    def __call__(self, ids: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
        L = ids.shape[1]
        if self.rep is not None:
            scores = repetition_penalty_(scores, ids, self.rep)
        if self.ngram:
            scores = no_repeat_ngram_(scores, ids, self.ngram)
        if self.bad_words:
            scores = bad_words_(scores, ids, self.bad_words, self.eos)
        if self.min_length > 0 and L < self.min_length and any(e >= 0 for e in self.eos):          # MinLengthLogitsProcessor: the WHOLE row's length
            scores = suppress_(scores, [e for e in self.eos if e >= 0])
        if self.min_new > 0 and L - self.prompt_len < self.min_new and any(e >= 0 for e in self.eos):   # MinNewTokensLengthLogitsProcessor
            scores = suppress_(scores, [e for e in self.eos if e >= 0])
        if self.forced_eos and L == self.max_len - 1:
            scores = force_(scores, self.forced_eos)
        if self.suppress:
            scores = suppress_(scores, self.suppress)
        if self.begin_suppress and L == self.prompt_len:
            scores = suppress_(scores, self.begin_suppress)
        for f in self.user:
            scores = f(ids, scores)
        return scores


def stopped(criteria, ids: torch.Tensor, scores: torch.Tensor) -> torch.Tensor:
    """[3P] StoppingCriteriaList.__call__: the OR of the caller's criteria, each (input_ids, scores) -> bool [B] (a plain bool stops every row)."""
    done = torch.zeros(ids.shape[0], dtype=torch.bool, device=ids.device)
    for c in criteria or ():
        r = c(ids, scores)
        done = done | (r.to(ids.device).bool() if isinstance(r, torch.Tensor) else torch.full_like(done, bool(r)))
    return done
