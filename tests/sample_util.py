"""Reference, random numbers and acceptance rules for the device sampler (uvx_sample_select, include/uvx.h); no GPU needed here.

* `RowRef`: a float64 restatement of the kernel's steps 1-5 on ONE row.  It takes the f32-rounded x = logit / temperature the kernel takes (the
  division is one correctly rounded f32 operation on both sides) and does everything after it in float64.
* `philox4x32_10` / `philox_uniform`: numpy Philox4x32-10 and the kernel's uniform u = (w0 >> 8) * 2^-24.
* `bound(n)`, `token_ok`: the tolerances of tests/test_sample_gpu.py.

Tolerance.  bound(n) = (n + 96) * 2^-24, relative: an f32 sum of n non-negative terms in any order is off by at most n * 2^-24 of its value; the
exponent's argument x - x_max, at most 88 in size, carries one f32 rounding (88 * 2^-24, relative after exp); expf adds a few ulp.  (The kernel
sums in integer fixed point and does better; the bound does not rely on that.)

Margins.  Whether a token survives top-p is the comparison of a sum of probabilities with a share of the total.  HF and `RowRef` write it as
C(x_v) <= (1 - top_p) * total with C the ascending cumulative sum; it is the same statement as S(x_v) >= top_p * total with S(x_v) = total - C(x_v)
the mass strictly above x_v, and a rounding error of a sum of non-negative terms is relative to THAT sum.  `RowRef` evaluates both forms in float64,
asserts that they agree, and reports as its margin the smallest relative distance |S - top_p * total| / max(S, top_p * total) over the row's values
(for top_p = 1e-6 the form with C would measure 1e-6 against C = total, which no summation gets wrong: S is an empty sum there).  For min-p the
comparison is x_v against x_max + log(min_p); the margin is their distance, which is the relative distance of p_v and min_p * p_max.  The GPU
tests require every margin to exceed 2 * bound(n) on the reference before they look at the kernel.
"""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def bound(n: int) -> float:
    return (n + 96) * 2.0 ** -24


def x_of(logits, temperature: float) -> np.ndarray:
    """f32 x as the kernel forms it: float(logit) / temperature, skipped at temperature 1."""
    x = np.asarray(logits, dtype=np.float32)
    return x if temperature == 1.0 else (x / np.float32(temperature)).astype(np.float32)


class RowRef:
    """Steps 2-5 on one f32 row x (after the temperature), float64.  The sort is done once; `warp` may be called for many settings."""

    def __init__(self, x: np.ndarray):
        assert x.dtype == np.float32 and x.ndim == 1
        self.x = x.astype(np.float64)
        self.V = len(x)
        self.vals, self.inv = np.unique(self.x, return_inverse=True)       # ascending distinct values; equal values act as a group
        self.desc = np.sort(self.x)[::-1]

    def warp(self, top_k=0, top_p=1.0, min_p=0.0, min_keep=1):
        """-> dict(kept bool [V], probs f64 [V], margins: [(margin, n)] for every boundary met, n the tokens alive when it was applied)."""
        x, V = self.x, self.V
        top_p, min_p = float(np.float32(top_p)), float(np.float32(min_p))          # the C ABI takes them as f32
        alive = x > -np.inf
        margins = []
        if not alive.any():
            return dict(kept=alive, probs=np.zeros(V), margins=margins)
        xmax = x.max()
        if top_k > 0:
            k = min(max(top_k, min_keep), V)
            alive &= x >= self.desc[k - 1]                      # ties with the k-th value stay
        protect = x >= self.desc[min(min_keep, V) - 1]          # the min_keep largest (and what is tied with them)
        if top_p < 1.0:
            e = np.where(alive, np.exp(x - xmax), 0.0)
            per_val = np.bincount(self.inv, weights=e, minlength=len(self.vals))
            C = np.cumsum(per_val)                              # C(t) = mass of {x_v <= t}
            total = C[-1]
            # S(t) = mass strictly above t, summed from the top so that it is accurate where it is small
            S = np.concatenate([np.cumsum(per_val[::-1])[::-1][1:], [0.0]])
            drop_val = C <= (1.0 - top_p) * total
            live_val = per_val > 0
            assert np.array_equal(drop_val[live_val], (S >= top_p * total)[live_val]), "the two forms of the top-p test disagree on the reference"
            rel = np.abs(S - top_p * total) / np.maximum(S, top_p * total)
            unprot = live_val & (self.vals < self.desc[min(min_keep, V) - 1])       # a protected value's decision is not the sum's
            if unprot.any():
                margins.append((float(rel[unprot].min()), int(alive.sum())))
            alive &= ~(drop_val[self.inv] & ~protect)
        if min_p > 0.0:
            thr = xmax + math.log(min_p)
            cand = alive & ~protect
            if cand.any():
                margins.append((float(np.abs(x[cand] - thr).min()), int(alive.sum())))
            alive &= ~((x < thr) & ~protect)
        e = np.where(alive, np.exp(x - xmax), 0.0)
        return dict(kept=alive, probs=e / e.sum(), margins=margins)


def margins_ok(ref: dict) -> bool:
    """The precondition of the kept-set tests: every boundary of the reference is further away than twice the bound."""
    return all(m > 2.0 * bound(n) for m, n in ref["margins"])


def token_ok(tok: int, u: float, ref: dict) -> bool:
    """The draw's acceptance: the token is kept and CDF[t - 1] - tol <= u * total <= CDF[t] + tol with the kept probabilities cumulated in index
    order (total = 1 here: `probs` is normalised) and tol = bound(n_kept) relative to the larger of the two numbers compared."""
    kept, p = ref["kept"], ref["probs"]
    if not kept.any():
        return tok == 0
    if not (0 <= tok < len(p)) or not kept[tok]:
        return False
    cdf = np.cumsum(p)
    b = bound(int(kept.sum()))
    lo = cdf[tok - 1] if tok > 0 else 0.0
    return lo - b * max(lo, u) <= u <= cdf[tok] + b * max(cdf[tok], u)


def philox4x32_10(key, counter) -> np.ndarray:
    """numpy Philox4x32-10.  key: uint32 [..., 2], counter: uint32 [..., 4] -> uint32 [..., 4]."""
    k = np.asarray(key, dtype=np.uint64).copy()
    c = np.asarray(counter, dtype=np.uint64).copy()
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[..., 0], np.uint64(M1) * c[..., 2]
        c = np.stack([(p1 >> np.uint64(32)) ^ c[..., 1] ^ k[..., 0], p1 & mask, (p0 >> np.uint64(32)) ^ c[..., 3] ^ k[..., 1], p0 & mask], axis=-1)
        k = np.stack([(k[..., 0] + np.uint64(W0)) & mask, (k[..., 1] + np.uint64(W1)) & mask], axis=-1)
    return c.astype(np.uint32)


def philox_python(key, counter):
    """The same in plain Python integers (a second restatement to hold the numpy one against)."""
    k0, k1 = key
    c0, c1, c2, c3 = counter
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_uniform(seed: int, offset: int, B: int) -> np.ndarray:
    """The kernel's uniforms of one launch, f64 [B]: key (seed_lo, seed_hi), counter (offset_lo, offset_hi, b, 0), u = (w0 >> 8) * 2^-24."""
    key = np.array([[seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF]] * B, dtype=np.uint32)
    ctr = np.array([[offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF, b, 0] for b in range(B)], dtype=np.uint32)
    return (philox4x32_10(key, ctr)[:, 0] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def chi2_quantile(df: int, alpha: float) -> float:
    """Upper alpha quantile of chi-square(df): scipy if it is there, else Wilson-Hilferty."""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(alpha, df))
    except ImportError:
        from statistics import NormalDist
        z = NormalDist().inv_cdf(1.0 - alpha)
        return df * (1.0 - 2.0 / (9.0 * df) + z * math.sqrt(2.0 / (9.0 * df))) ** 3


def peaked_rows(V: int, B: int, seed: int) -> np.ndarray:
    """f32 [B, V] test logits: a flat tail N(0, 0.5) under a head of up to 12 tokens at random columns, the top one near 16 and each next one
    0.5 - 0.9 below the last.  The head holds ~99 % of the mass, so the top-p and min-p boundaries fall between head tokens, where neighbouring
    cumulative sums differ by tens of per cent - far more than 2 * bound(V) even at V = 131077 (a smooth row of that width has neighbours a few
    1e-5 apart and cannot meet the margin)."""
    g = np.random.default_rng(seed)
    rows = (g.standard_normal((B, V)) * 0.5).astype(np.float32)
    H = min(12, V)
    for b in range(B):
        cols = g.choice(V, size=H, replace=False)
        rows[b, cols] = (16.0 + g.uniform(-0.5, 0.5) - np.concatenate([[0.0], np.cumsum(g.uniform(0.5, 0.9, size=H - 1))])).astype(np.float32)
    return rows
