"""Reference for greedy decoding under a repetition penalty (uvx_seen_mark / uvx_greedy_select_penalized, include/uvx.h); no GPU needed here.

numpy f32, HF's RepetitionPenaltyLogitsProcessor as it is written: np.where(s < 0, s * p, s / p) with p an f32, on the distinct in-range ids of a
row; the token is np.argmax (first maximum) with NaN mapped to -inf.  tests/test_penalized_select_cpu.py pins this against transformers' processor
bit for bit; tests/test_penalized_select_gpu.py holds the kernels to it without a tolerance."""
import numpy as np


def words_of(V):
    return (int(V) + 31) // 32


def in_range(ids, V):
    """The distinct ids of one row that lie in [0, V), ascending."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    return np.unique(ids[(ids >= 0) & (ids < V)])


def bitmap(rows_of_ids, V, words=None):
    """uint32 [B, words]: bit (id & 31) of word (id >> 5) of row b is set for every in-range id of rows_of_ids[b]."""
    words = words_of(V) if words is None else words
    out = np.zeros((len(rows_of_ids), words), dtype=np.uint32)
    for b, ids in enumerate(rows_of_ids):
        ids = in_range(ids, V)
        np.bitwise_or.at(out[b], ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return out


def ids_of(bitmap_row, V=None):
    """The ids whose bits are set in one bitmap row, ascending (all words; bits at or past V included unless V is given)."""
    bits = np.unpackbits(np.ascontiguousarray(bitmap_row, dtype="<u4").view(np.uint8), bitorder="little")
    ids = np.flatnonzero(bits)
    return ids if V is None else ids[ids < V]


def penalized(row, ids, penalty):
    """f32 [V]: the row with the scores of the distinct in-range `ids` penalised."""
    s = np.array(row, dtype=np.float32)
    ids = in_range(ids, s.shape[0])
    p = np.float32(penalty)
    with np.errstate(all="ignore"):
        v = s[ids]
        s[ids] = np.where(v < 0, v * p, v / p)
    return s


def argmax(scores):
    """First maximum; NaN never wins; index 0 if nothing is above -inf."""
    s = np.where(np.isnan(scores), -np.inf, scores)
    return int(np.argmax(s))


def same_bits(a, b):
    """Bitwise equality of two f32 arrays, NaN positions compared as positions."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def greedy_loop(row, penalty, steps, ids=()):
    """`steps` consecutive selections on the same f32 logits row, every selected token joining the seen ids -> the tokens."""
    ids, toks = list(ids), []
    for _ in range(steps):
        toks.append(argmax(penalized(row, ids, penalty)))
        ids.append(toks[-1])
    return toks
