"""Shared float64 yardstick of the raw-waveform normaliser's tests (test_wavenorm_cpu.py, test_wavenorm_gpu.py): the definition in uvx_wave_norm's
comment (include/uvx.h) evaluated beyond float64 on the f32 inputs, and a per-element error bar for an implementation that accumulates the two
sums in float64 and rounds once to f32.

    mean = sum x / n (the sum by math.fsum: correctly rounded),  var = sum (x - mean)^2 / n  (two passes, in numpy's extended precision),
    rstd = 1 / sqrt(var + 1e-7),  y = (x - mean) * rstd,  A = mean |x|,  E2 = mean x^2,  gamma = (n + 4) * 2^-53

    bar_i = |y_i| * (2^-24 + 1.5 * gamma * E2 / (var + 1e-7) + 2^-50)  +  rstd * gamma * A  +  2^-149

Derivation.  2^-24 |y_i| is the one correctly rounded double -> float conversion of the result.  gamma bounds the relative error of a float64 sum
of n terms added in ANY order (n - 1 additions, each relative 2^-53; the + 4 absorbs the divisions by n, the product mean * mean, the
subtraction and second-order terms), so the computed mean is within gamma * A of the exact one, and S2 / n - mean^2 is within
gamma * E2 + 2 * gamma * A * |mean| <= 3 * gamma * E2 of the exact variance (A^2 <= E2, |mean| <= A).  rstd = (var + 1e-7)^-1/2 moves by half of
the relative change of var + 1e-7: 1.5 * gamma * E2 / (var + 1e-7), which scales y_i; the mean's error shifts every output by at most
rstd * gamma * A.  2^-50 covers the float64 divide, square root and multiply, and x_i - mean (one rounding each); 2^-149 a result in the subnormal
range.  Nothing in the bar is fitted to the code under test.  With n < 10^5, gamma stays below 2^-36, so an implementation with f32 accumulators
(or numpy's own f32 mean / var) exceeds the bar wherever more than one sample differs; keep test lengths there.

Nothing here imports the package.
"""
import math
from fractions import Fraction

import numpy as np

EPS = 1e-7          # the float64 constant of zero_mean_unit_var_norm


def as_f32(x):
    """What a sample counts as: int16 is x * 2^-15 (exact in f32), f32 is itself."""
    x = np.asarray(x)
    return x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x.astype(np.float32)


def stats(x):
    """-> (mean, var) in numpy's extended precision (longdouble) and A = mean |x|, E2 = mean x^2 in float64, of the f32 clip x."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    x64 = x.astype(np.float64)
    mean = np.longdouble(math.fsum(x64)) / np.longdouble(n)
    d = x64.astype(np.longdouble) - mean
    var = (d * d).sum() / np.longdouble(n)
    return mean, var, math.fsum(np.abs(x64)) / n, math.fsum(x64 * x64) / n      # x * x is exact in float64


def oracle(x):
    """Every output of the f32 clip x (int16 callers pass as_f32(x)) -> (y, bar), float64 [n]."""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    mean, var, A, E2 = stats(x)
    rstd = np.longdouble(1) / np.sqrt(var + np.longdouble(EPS))
    y = ((x.astype(np.longdouble) - mean) * rstd).astype(np.float64)
    gamma = (n + 4) * 2.0 ** -53
    bar = np.abs(y) * (2.0 ** -24 + 1.5 * gamma * E2 / float(var + np.longdouble(EPS)) + 2.0 ** -50) + float(rstd) * gamma * A + 2.0 ** -149
    return y, bar


def exact(x):
    """The definition in rational arithmetic (mean and var exactly; rstd from a 60-digit square root) -> y as float64 [n]; for short clips."""
    from decimal import Decimal, getcontext
    getcontext().prec = 60
    fx = [Fraction(float(v)) for v in np.asarray(x, dtype=np.float32)]
    n = len(fx)
    mean = sum(fx) / n
    var = sum((v - mean) ** 2 for v in fx) / n + Fraction(EPS)
    rstd = 1 / (Decimal(var.numerator) / Decimal(var.denominator)).sqrt()
    return np.array([float(Decimal((v - mean).numerator) / Decimal((v - mean).denominator) * rstd) for v in fx])


def host_f32(x):
    """The host path of frontend.Wav2Vec2FeatureExtractor restated: numpy's float32 mean and variance."""
    x = np.asarray(x, dtype=np.float32)
    return (x - x.mean()) / np.sqrt(x.var() + 1e-7)


def named_cases(rng):
    """The clips the issue names, as (name, clip) with int16 or f32 dtype."""
    return [("dc_offset", (0.5 + 0.01 * rng.standard_normal(5000)).astype(np.float32)),
            ("quiet", (1e-5 * rng.standard_normal(5000)).astype(np.float32)),
            ("constant_int16", np.full(5000, 1000, dtype=np.int16)),
            ("one_sample", np.array([0.25], dtype=np.float32))]
