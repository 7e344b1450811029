"""Reference for the token-ban score processors of the banned selectors (uvx_greedy_select_banned / uvx_sample_select_banned, include/uvx.h); no
GPU needed here.

`Rules` is the rule set of one generate() call; `banned(row_ids, rules, L, prompt_len, max_len)` restates HF's seven processors on ONE row in numpy as
a bool mask over the vocabulary plus the forced flag; `apply` turns it into the f32 scores (-inf where banned, on a forced step 0.0 elsewhere).
tests/test_banned_select_cpu.py pins this against transformers' own processors assembled in HF's order, bit for bit;
tests/test_banned_select_gpu.py holds the kernels to it without a tolerance.  Ids outside [0, V) - which HF's processors index with and raise on -
are compared by value and never banned, as the C header states."""
from dataclasses import dataclass, field
from typing import List, Sequence

import numpy as np

BAN_MIN, BAN_FORCED, BAN_BEGIN = 1, 2, 4


@dataclass
class Rules:
    V: int
    ngram: int = 0
    bad_words: List[Sequence[int]] = field(default_factory=list)
    eos: Sequence[int] = ()
    min_length: int = 0
    min_new: int = 0
    forced: Sequence[int] = ()
    suppress: Sequence[int] = ()
    begin: Sequence[int] = ()

    def kept_bad_words(self):
        """HF drops the entries that are a lone EOS id."""
        return [list(map(int, w)) for w in self.bad_words if not (len(w) == 1 and int(w[0]) in set(map(int, self.eos)))]

    def min_ids(self):
        return [int(e) for e in self.eos if e >= 0] if (self.min_length > 0 or self.min_new > 0) else []

    def flags(self, L, prompt_len, max_len):
        short = (self.min_length > 0 and L < self.min_length) or (self.min_new > 0 and L - prompt_len < self.min_new)
        return ((BAN_MIN if short and self.min_ids() else 0) | (BAN_FORCED if len(self.forced) and L == max_len - 1 else 0)
                | (BAN_BEGIN if len(self.begin) and L == prompt_len else 0))


def _mark(mask, ids):
    for t in ids:
        if 0 <= int(t) < len(mask):
            mask[int(t)] = True


def banned_by_flags(ids, V, ngram, bad_words, min_ids, forced, suppress, begin, flags):
    """bool [V]: the C entry point's own terms - the lists of uvx_ban_rules_t (bad_words as a list of id lists) and the step's flag word."""
    ids = [int(t) for t in ids]
    L = len(ids)
    mask = np.zeros(V, dtype=bool)
    n = int(ngram)
    if n > 0 and L >= n:
        tail = ids[L - (n - 1):] if n > 1 else []
        _mark(mask, [ids[j + n - 1] for j in range(L - n + 1) if ids[j:j + n - 1] == tail])
    for w in bad_words:
        w = [int(t) for t in w]
        if len(w) == 1 or (1 < len(w) <= L and ids[L - (len(w) - 1):] == w[:-1]):
            _mark(mask, w[-1:])
    if flags & BAN_MIN:
        _mark(mask, min_ids)
    if flags & BAN_FORCED:              # HF's fill_(-inf) voids what came before
        mask[:] = True
        for t in forced:
            if 0 <= int(t) < V:
                mask[int(t)] = False
    _mark(mask, suppress)
    if flags & BAN_BEGIN:
        _mark(mask, begin)
    return mask


def banned(row_ids, rules: Rules, L: int, prompt_len: int, max_len: int):
    """-> (bool [V]: the ids banned at this step, forced: the step is the forced one).  The row is row_ids[:L]."""
    ids = np.asarray(row_ids).reshape(-1)[:L]
    assert len(ids) == L
    fl = rules.flags(L, prompt_len, max_len)
    mask = banned_by_flags(ids, rules.V, rules.ngram, rules.kept_bad_words(), rules.min_ids(), rules.forced, rules.suppress, rules.begin, fl)
    return mask, bool(fl & BAN_FORCED)


def apply(scores, mask, forced):
    """f32 [V]: the scores behind the bans."""
    s = np.zeros(len(mask), dtype=np.float32) if forced else np.array(scores, dtype=np.float32)
    s[mask] = -np.inf
    return s


def mask_of(bitmap_row, V):
    """bool [V] from one row of the kernel's ban bitmap (bits at or past V ignored)."""
    bits = np.unpackbits(np.ascontiguousarray(bitmap_row, dtype="<u4").view(np.uint8), bitorder="little")
    return bits[:V].astype(bool)


@dataclass
class Case:
    name: str
    rows: np.ndarray        # int64 [3, L]: the rows so far
    rules: Rules
    prompt_len: int
    max_len: int
    hf: bool = True         # transformers' processors take these inputs (they raise on ids outside the vocabulary)

    @property
    def L(self):
        return self.rows.shape[1]


def edge_cases(V: int) -> List[Case]:
    """The rule edges the kernel tests and the pin against transformers share, on three rows: row 0 = a b c ... a b (a tail that matches at j = 0),
    row 1 = one id repeated (every window matches, the last one included), row 2 = random ids."""
    g = np.random.default_rng(V)
    a, b, c, d, e = 0, V - 1, V // 2, V // 3, (2 * V) // 3
    L0 = 12
    base = g.integers(0, V, size=(3, L0)).astype(np.int64)
    base[0, :3], base[0, -2:] = [a, b, c], [a, b]
    base[1] = d
    far = 10 ** 6          # prompt_len / max_len that switch the step rules off
    out = []

    def add(name, rules, rows=base, prompt_len=0, max_len=far, hf=True):
        out.append(Case(name, np.ascontiguousarray(rows), rules, prompt_len, max_len, hf))
    R = lambda **kw: Rules(V, **kw)
    for n in (1, 2, 3):
        for L in (n - 2, n - 1, n):
            if L >= 0:
                add(f"ngram n={n} L={L}", R(ngram=n), base[:, L0 - L:] if L else base[:, :0])
        add(f"ngram n={n} L={L0}", R(ngram=n))
    for bad in (-1, V, V + 40):
        rows = base.copy()
        rows[0, 2] = bad                   # the id the match at j = 0 bans
        add(f"ngram bans id {bad}", R(ngram=3), rows, hf=False)
    rows = base.copy()
    rows[0, 0] = rows[0, -2] = V + 40      # an id outside the vocabulary inside the matching prefix: compared by value
    add("ngram prefix holds an outside id", R(ngram=3), rows, hf=False)
    add("ngram larger than int16 and the row", R(ngram=70000))
    add("bad words: one token", R(bad_words=[[c]]))
    add("bad words: a tail in row 0 only", R(bad_words=[[a, b, e]]))
    add("bad words: longer than the context", R(bad_words=[list(base[0]) + [e]]))
    add("bad words: as long as the context", R(bad_words=[list(base[0, 1:]) + [e]]))
    add("bad words: two entries ban one id", R(bad_words=[[e], [a, b, e], [b, e]]))
    add("bad words: a lone EOS entry is dropped", R(bad_words=[[c], [e]], eos=[c]))
    add("bad words: last token outside", R(bad_words=[[a, b, V + 5], [V], [d, e]]), hf=False)
    add("min_new_tokens on", R(eos=[c, -1], min_new=2), prompt_len=L0 - 1)
    add("min_new_tokens off", R(eos=[c, -1], min_new=2), prompt_len=L0 - 2)
    add("min_length on", R(eos=[c, e], min_length=L0 + 1), prompt_len=3)
    add("min_length off", R(eos=[c, e], min_length=L0), prompt_len=3)
    add("begin on", R(begin=[d, a]), prompt_len=L0)
    add("begin off", R(begin=[d, a]), prompt_len=L0 - 1)
    add("suppress", R(suppress=[a, b, c, 31 % V, 32 % V, 33 % V]))
    add("forced: one id", R(forced=[c]), max_len=L0 + 1)
    add("forced: two ids", R(forced=[c, e]), max_len=L0 + 1)
    add("forced: not yet", R(forced=[c, e], suppress=[a]), max_len=L0 + 2)
    add("forced: one of two also suppressed", R(forced=[c, e], suppress=[c]), max_len=L0 + 1)
    add("forced: every forced id suppressed", R(forced=[c], suppress=[a, c]), max_len=L0 + 1)
    add("forced: a forced id begin-suppressed", R(forced=[c, e], begin=[e]), prompt_len=L0, max_len=L0 + 1)
    add("forced: an id outside", R(forced=[c, V + 3, -2]), max_len=L0 + 1, hf=False)
    add("forced voids the other rules", R(ngram=2, bad_words=[[d], [a, b, e]], eos=[b], min_new=50, forced=[e], suppress=[a]), max_len=L0 + 1)
    add("everything", R(ngram=2, bad_words=[[d], [a, b, e]], eos=[b], min_new=50, min_length=40, forced=[e], suppress=[a], begin=[c]), prompt_len=L0)
    return out


def hf_processors(rules: Rules, prompt_len: int, max_len: int, penalty=None):
    """transformers' own processors for the rule set, in the order of GenerationMixin._get_logits_processor."""
    from transformers.generation import logits_process as LP
    eos = [int(e) for e in rules.eos]
    out = LP.LogitsProcessorList()
    if penalty is not None:
        out.append(LP.RepetitionPenaltyLogitsProcessor(penalty))
    if rules.ngram:
        out.append(LP.NoRepeatNGramLogitsProcessor(rules.ngram))
    if rules.bad_words:
        out.append(LP.NoBadWordsLogitsProcessor([list(w) for w in rules.bad_words], eos_token_id=eos))
    if rules.min_length > 0 and any(e >= 0 for e in eos):
        out.append(LP.MinLengthLogitsProcessor(rules.min_length, [e for e in eos if e >= 0], device="cpu"))
    if rules.min_new > 0 and any(e >= 0 for e in eos):
        out.append(LP.MinNewTokensLengthLogitsProcessor(prompt_len, rules.min_new, [e for e in eos if e >= 0], device="cpu"))
    if len(rules.forced):
        out.append(LP.ForcedEOSTokenLogitsProcessor(max_len, list(rules.forced), device="cpu"))
    if len(rules.suppress):
        out.append(LP.SuppressTokensLogitsProcessor(list(rules.suppress), device="cpu"))
    if len(rules.begin):
        out.append(LP.SuppressTokensAtBeginLogitsProcessor(list(rules.begin), prompt_len, device="cpu"))
    return out
