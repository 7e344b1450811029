"""Restatements of the three augmentation kernels' definitions (uvx_aug_gain, uvx_aug_iir, uvx_aug_noise: their comments in include/uvx.h) in
numpy, shared by test_aug_cpu.py, test_aug_gpu.py and tools/aug_ab.py.  Nothing here imports the package.

* gain: `gain_ref`, numpy's own float32 multiply and clip.
* filter: `iir_warm_ref` runs the warm-up recurrence with scipy.signal.lfilter per block (float64); `iir_truth` is the plain recurrence from sample
  0 in numpy's extended precision (longdouble), the truth both scipy and the kernel are measured against; `iir_bar` is the issue's per-element
  bound 2^-23 |truth| + 8 d with d the largest distance of scipy's float64 lfilter from the truth on the same case.
* noise: `normals` (Philox4x32-10 of sample_util.py and Box-Muller), `noise_ref` (white, or the shaped half spectrum through an inverse real
  FFT) and `mix_ref`; each takes the floating-point type to evaluate in: float64 is the restatement, float32 the CPU evaluation whose distance
  from it sets the GPU test's tolerance.
* `host_*`: the reference's own host definitions (numpy's generator, an FFT of length n), what tools/aug_ab.py times.
"""
import numpy as np

from sample_util import philox4x32_10

COLOURS = {"white": 0, "pink": 1, "brown": 2, "blue": 3, "violet": 4}
EXPONENT = {1: -0.5, 2: -1.0, 3: 0.5, 4: 1.0}      # amplitude factor f ** EXPONENT[colour]


def as_f32(x):
    """What a sample counts as: int16 is x * 2^-15 (exact in f32), f32 is itself."""
    x = np.asarray(x)
    return x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x.astype(np.float32)


# ------------------------------------------------------------------------------------------------ gain
def gain_ref(x, gain_db):
    """np.clip(x * 10^(gain_db / 20), -1, 1) on the f32 clip, in float32: the Python float is a weak scalar."""
    x = as_f32(x)
    y = np.clip(x * np.float32(10 ** (gain_db / 20)), np.float32(-1.0), np.float32(1.0))
    assert y.dtype == np.float32
    return y


# ------------------------------------------------------------------------------------------------ filter
def iir_warm_ref(b, a, x, warm, block):
    """Outputs [block * j, block * (j + 1)) from lfilter started with zero state at sample max(0, block * j - warm); float64."""
    from scipy.signal import lfilter
    x = np.asarray(x, dtype=np.float64)
    y = np.zeros(len(x))
    for k0 in range(0, len(x), block):
        s = max(0, k0 - warm)
        y[k0:k0 + block] = lfilter(b, a, x[s:k0 + block])[k0 - s:]
    return y


def iir_truth(b, a, x):
    """lfilter's recurrence (transposed direct form II) from sample 0 in longdouble -> longdouble [n]."""
    L = np.longdouble
    b, a = np.asarray(b, dtype=np.float64).astype(L), np.asarray(a, dtype=np.float64).astype(L)
    assert a[0] == 1 and len(a) == len(b)
    x = np.asarray(x, dtype=np.float64).astype(L)
    z = np.zeros(len(a), dtype=L)                  # z[order] stays 0
    y = np.zeros(len(x), dtype=L)
    for i in range(len(x)):
        y[i] = z[0] + b[0] * x[i]
        z[:-1] = z[1:] + b[1:] * x[i] - a[1:] * y[i]
    return y


def iir_bar(b, a, x, k=8.0):
    """-> (truth as longdouble [n], bar float64 [n], d): |out - (float)truth| <= 2^-23 |truth| + k d, d = max |lfilter_f64 - truth| on this case."""
    from scipy.signal import lfilter
    truth = iir_truth(b, a, x)
    d = float(np.max(np.abs(lfilter(b, a, np.asarray(x, dtype=np.float64)).astype(np.longdouble) - truth))) if len(x) else 0.0
    return truth, 2.0 ** -23 * np.abs(truth).astype(np.float64) + k * d, d


def iir_case(n, rng):
    """The issue's input: noise plus a step plus an impulse at the last sample, f32."""
    x = 0.1 * rng.standard_normal(n)
    x[n // 3:] += 0.25
    if n:
        x[-1] += 0.5
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------ noise
def normals(seed, offset, b, count, dtype=np.float64):
    """Normals 0 .. count - 1 of row b: key (seed_lo, seed_hi), counter (offset_lo, offset_hi, m >> 2, b); lanes 0, 1 = r cos(2 pi v), r sin(2 pi v) with
    r = sqrt(-2 ln u), u = ((w0 >> 9) + 0.5) * 2^-23, v = (w1 >> 8) * 2^-24, lanes 2, 3 the same from (w2, w3); evaluated in `dtype`."""
    q = (count + 3) // 4
    key = np.empty((q, 2), dtype=np.uint32)
    key[:, 0], key[:, 1] = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    ctr = np.empty((q, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF, np.arange(q, dtype=np.uint32), b
    w = philox4x32_10(key, ctr)
    T = dtype
    out = np.empty((q, 4), dtype=T)
    for pair in (0, 1):
        u = ((w[:, 2 * pair] >> np.uint32(9)).astype(T) + T(0.5)) * T(2.0 ** -23)
        v = (w[:, 2 * pair + 1] >> np.uint32(8)).astype(T) * T(2.0 ** -24)
        r = np.sqrt(T(-2.0) * np.log(u))
        ang = T(2.0 * np.pi) * v
        out[:, 2 * pair], out[:, 2 * pair + 1] = r * np.cos(ang), r * np.sin(ang)
    assert out.dtype == T
    return out.reshape(-1)[:count]


def grid_m(n):
    """M = max(2, smallest power of two >= n)"""
    return max(2, 1 << (int(n) - 1).bit_length())


def noise_ref(n, colour, seed, offset, b, dtype=np.float64):
    """The noise of a row before the mix, in `dtype` (float64: numpy's irfft; float32: scipy.fft.irfft on complex64 input)."""
    colour = COLOURS.get(colour, colour)
    T = dtype
    if colour == 0:
        return normals(seed, offset, b, n, T)
    M = grid_m(n)
    g = normals(seed, offset, b, M + 2, T)
    k = np.arange(M // 2 + 1)
    Z = (g[0::2] + 1j * g[1::2]) * np.sqrt(T(M / 2))
    Z[0], Z[-1] = g[0] * np.sqrt(T(M)), g[M] * np.sqrt(T(M))
    f = (np.maximum(k, 1) / M).astype(T)
    X = Z * f ** T(EXPONENT[colour])
    if T == np.float64:
        return np.fft.irfft(X, M)[:n]
    import scipy.fft
    y = scipy.fft.irfft(X.astype(np.complex64), M)
    assert y.dtype == np.float32
    return y[:n]


def mix_ref(x, noise, snr_db):
    """x + noise * sqrt(mean x^2 * 10^(-snr_db / 10) / mean noise^2) in float64 (unrounded); a row without signal or noise power comes back as it is."""
    x, noise = as_f32(x).astype(np.float64), np.asarray(noise).astype(np.float64)
    s2x, s2n = float(np.sum(x * x)), float(np.sum(noise * noise))
    if s2x == 0.0 or s2n == 0.0:
        return x
    n = len(x)
    return x + noise * np.sqrt((s2x / n) * 10 ** (-snr_db / 10) / (s2n / n))


def snr_db_of(x, y):
    """10 log10(sum x^2 / sum (y - x)^2)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return 10.0 * np.log10(np.sum(x * x) / np.sum((y - x) ** 2))


def periodogram_slope(noise):
    """Least-squares slope of log power against log frequency over the bins 1 .. M/2 - 1 of a row of length M."""
    P = np.abs(np.fft.rfft(noise)) ** 2
    k = np.arange(1, len(noise) // 2)
    return float(np.polyfit(np.log(k), np.log(P[k]), 1)[0])


# ------------------------------------------------------------------------------------------------ the host definitions the reference runs
def host_gain(x, gain_db):
    return np.clip(x * 10 ** (gain_db / 20), -1.0, 1.0)


def host_coloured_noise(x, colour, snr_db, rng=np.random):
    """White noise in time, an FFT of length n, the shaping on the grid k / n, an inverse FFT of length n, and the mix: float64."""
    colour = COLOURS.get(colour, colour)
    n = len(x)
    noise = rng.normal(0, 1, n)
    if colour:
        f = np.abs(np.fft.fftfreq(n))
        f[0] = f[1]
        noise = np.fft.ifft(np.fft.fft(noise) * f ** EXPONENT[colour]).real
    noise_power = np.mean(x ** 2) / 10 ** (snr_db / 10)
    return x + noise * np.sqrt(noise_power / np.mean(noise ** 2))


def host_bandpass(x, sample_rate=16000, lowcut=300, highcut=3400, order=5):
    from scipy.signal import butter, lfilter
    nyquist = sample_rate / 2
    b, a = butter(order, [lowcut / nyquist, highcut / nyquist], btype="band")
    return lfilter(b, a, x)
