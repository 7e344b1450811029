"""Shared float64 oracle of the polyphase resampler's tests (test_resample_cpu.py, test_resample_gpu.py): the definition in uvx_resample_poly's
comment (include/uvx.h) evaluated in float64 on the f32 inputs and the f32 taps, and the per-output error bar of an f32 dot product.

    y[k]   = sum over i in [0, n) with |k * down - i * up| <= half  of  x[i] * hf[half + k * down - i * up]
    bar[k] = (T_k + 2) * 2^-24 * sum_i |x[i]| * |hf[...]|  +  2^-126          T_k = the number of terms of output k

The bar is the standard bound of an f32 dot product of T_k terms in any order, with or without FMA (each product and each addition rounds with
relative error at most 2^-24; the +2 absorbs the second-order terms; 2^-126 covers results in the subnormal range).  It is derived, not
measured: a strictly sequential FMA-free f32 emulation stayed below 0.17 of it over eleven rate / length cases.

Nothing here calls the code under test; indices are Python / numpy int64 throughout.
"""
import math

import numpy as np

# up / down of 48, 44.1, 8, 24, 11.025, 96 and 32 kHz against 16 kHz
RATIOS = [(1, 3), (160, 441), (2, 1), (2, 3), (640, 441), (1, 6), (1, 2)]


def ratio(rate, target=16000):
    g = math.gcd(target, rate)
    return target // g, rate // g


def n_out(n, up, down):
    return -(-n * up // down)


def design_taps_f64(up, down):
    """The filter of the definition, numpy only (a restatement independent of ops.design_resample_taps) -> (float64 taps, half)."""
    m = max(up, down)
    half = 10 * m
    t = np.arange(-half, half + 1, dtype=np.float64)
    w = np.sinc(t / m) / m * np.kaiser(2 * half + 1, 5.0)
    return up * w / w.sum(), half


def taps_f32(up, down):
    h, half = design_taps_f64(up, down)
    return h.astype(np.float32), half


def oracle_at(ks, n, up, down, hf, half, x_at):
    """Outputs `ks` (any int64 array) of a clip of n samples whose sample i is x_at(i) (vectorised over an int64 array of valid indices).
    -> (y float64 [len(ks)], bar float64 [len(ks)])"""
    ks = np.asarray(ks, dtype=np.int64)
    hf64 = np.asarray(hf, dtype=np.float64)
    a = ks * down - half
    first = np.where(a <= 0, 0, -(-a // up))                      # ceil for a > 0
    width = 2 * half // up + 1                                    # no output has more terms
    i = first[:, None] + np.arange(width, dtype=np.int64)[None, :]
    t = ks[:, None] * down - i * up
    valid = (i < n) & (np.abs(t) <= half)
    xv = np.where(valid, x_at(np.where(valid, i, 0)).astype(np.float64), 0.0)
    hv = np.where(valid, hf64[np.where(valid, t + half, 0)], 0.0)
    y = (xv * hv).sum(axis=1)
    terms = valid.sum(axis=1)
    bar = (terms + 2) * 2.0 ** -24 * (np.abs(xv) * np.abs(hv)).sum(axis=1) + 2.0 ** -126
    return y, bar


def oracle(x, up, down, hf=None, half=None):
    """Every output of the clip x (f32, or float64 for the comparison with scipy; int16 callers pass x * 2^-15) -> (y, bar), float64 [n_out]."""
    if hf is None:
        hf, half = taps_f32(up, down)
    x = np.asarray(x)
    ks = np.arange(n_out(len(x), up, down), dtype=np.int64)
    return oracle_at(ks, len(x), up, down, hf, half, lambda i: x[i])


def counter_pcm(i):
    """The counter-based int16 pattern of the long-clip test: sample i from its index alone (numpy int64 here; the test builds the same values
    on the device with torch)."""
    i = np.asarray(i, dtype=np.int64)
    return (((i * 2654435761) >> 7) & 0xFFFF) - 32768
