"""(CPU) The raw-waveform normaliser without a GPU: the float64 yardstick of wavenorm_util.py against rational arithmetic, a numpy model of the
kernel's summation order against the yardstick's bar at the edges of its chunk, the entry points' exports, workspace size and argument checks,
ops.wave_norm's Python errors, and the extractor's unchanged host path."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import wavenorm_util as WU
from ultravox_amd import _lib, ops
from ultravox_amd.frontend import Wav2Vec2FeatureExtractor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = ops.WAVENORM_CHUNK


# ---------------------------------------------------------------- the yardstick
def test_the_yardstick_is_the_exact_definition_on_short_clips():
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 257):
        for x in ((0.3 * rng.standard_normal(n)).astype(np.float32), (0.5 + 0.01 * rng.standard_normal(n)).astype(np.float32),
                  WU.as_f32(rng.integers(-32768, 32768, n).astype(np.int16))):
            y, bar = WU.oracle(x)
            want = WU.exact(x)
            assert y.shape == bar.shape == (n,) and np.all(bar > 0)
            assert np.all(np.abs(y - want) <= 2.0 ** -52 * np.maximum(np.abs(want), 2.0 ** -40)), n      # float64 rounding of the yardstick's own result
    for name, x in WU.named_cases(np.random.default_rng(1)):
        y, bar = WU.oracle(WU.as_f32(x))
        assert np.all(np.isfinite(y)) and np.all(bar > 0), name
        if name in ("constant_int16", "one_sample"):
            assert np.all(y == 0.0), name


def kernel_model(x, acc=np.float64):
    """The summation order of uvx_wave_norm's comment in numpy: chunks of CHUNK from the row's start, 256 strided partial sums per chunk added in
    ascending order, a halving tree, the chunks' pairs in ascending order; `acc` is the accumulator type (float64: the definition)."""
    x = WU.as_f32(x)
    n = len(x)
    s1, s2 = acc(0), acc(0)
    for c0 in range(0, n, CHUNK):
        v = np.zeros(-(-min(CHUNK, n - c0) // 256) * 256, dtype=acc)
        v[:min(CHUNK, n - c0)] = x[c0:c0 + CHUNK]
        rows = v.reshape(-1, 256)
        p1, p2 = np.zeros(256, dtype=acc), np.zeros(256, dtype=acc)
        for r in rows:                                   # partial t: samples t, t + 256, ... in ascending order
            p1 = p1 + r
            p2 = p2 + r * r
        s = 128
        while s:
            p1[:s] = p1[:s] + p1[s:2 * s]
            p2[:s] = p2[:s] + p2[s:2 * s]
            s //= 2
        s1, s2 = s1 + p1[0], s2 + p2[0]
    mean = s1 / acc(n)
    var = max(acc(0), s2 / acc(n) - mean * mean)
    rstd = acc(1) / np.sqrt(var + acc(WU.EPS))
    return ((x.astype(acc) - mean) * rstd).astype(np.float32)


def test_the_bar_admits_float64_sums_and_refuses_float32_sums_at_the_chunk_edges():
    """The bar is derived, not measured; this shows that it discriminates at the sizes the GPU test uses: the kernel's order with float64
    accumulators stays within it, the same order with f32 accumulators and numpy's own f32 result do not."""
    rng = np.random.default_rng(2)
    clips = [(f"n={n}", (0.3 * rng.standard_normal(n)).astype(np.float32)) for n in (255, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)]
    clips += [(name, x) for name, x in WU.named_cases(rng) if name in ("dc_offset", "quiet")]
    for name, x in clips:
        y, bar = WU.oracle(WU.as_f32(x))
        assert np.all(np.abs(kernel_model(x).astype(np.float64) - y) <= bar), name
        assert np.any(np.abs(kernel_model(x, np.float32).astype(np.float64) - y) > bar), name
        assert np.any(np.abs(WU.host_f32(WU.as_f32(x)).astype(np.float64) - y) > bar), name


# ---------------------------------------------------------------- exports, workspace size, argument checks (no GPU work happens before them)
def test_both_entry_points_are_exported_and_declared():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "uvx.h")).read()
    for name in ("uvx_wave_norm_ws_bytes", "uvx_wave_norm"):
        assert name in _lib.EXPORTS and name + "(" in header and getattr(lib, name).argtypes is not None
    assert lib.uvx_wave_norm_ws_bytes.restype is C.c_size_t and lib.uvx_abi_version() == 19
    assert os.path.exists(os.path.join(ROOT, "ultravox_amd", "csrc", "wavenorm.hip"))
    assert f"constexpr int CHUNK = {CHUNK};" in open(os.path.join(ROOT, "ultravox_amd", "csrc", "wavenorm.h")).read()      # the Python mirror of the constant


def test_ws_bytes_is_sixteen_bytes_per_chunk_and_row():
    f = _lib.lib().uvx_wave_norm_ws_bytes
    assert [f(1, 1), f(1, CHUNK), f(1, CHUNK + 1), f(3, 2 * CHUNK + 1)] == [16, 16, 32, 3 * 3 * 16]
    assert f(8, 480000) == 8 * 30 * 16 and f(1, 1024 * CHUNK) == 16 * 1024
    assert [f(0, 5), f(-1, 5), f(3, 0), f(3, -7)] == [0, 0, 0, 0]
    assert f(65535, 2 ** 31 - 1) == 65535 * 131072 * 16                # no 32-bit product on the way


def _call(lib, **kw):
    a = dict(stream=None, fmt=1, pcm=64, row_offset=64, n=64, B=1, max_n=30, normalize=1, padding_value=0.0, out=64, out_stride=40, out_width=32,
             workspace=64, ws_bytes=16)
    a.update(kw)      # 64: a non-null address that is never read, every check comes before a launch
    return lib.uvx_wave_norm(a["stream"], a["fmt"], a["pcm"], a["row_offset"], a["n"], a["B"], a["max_n"], a["normalize"], a["padding_value"],
                             a["out"], a["out_stride"], a["out_width"], a["workspace"], a["ws_bytes"])


def test_every_invalid_argument_is_refused_with_a_message_before_any_device_work():
    lib = _lib.lib()
    bad_calls = [dict(pcm=None), dict(row_offset=None), dict(n=None), dict(out=None), dict(workspace=None), dict(ws_bytes=15),
                 dict(max_n=CHUNK + 1, out_width=CHUNK + 1, out_stride=CHUNK + 1, ws_bytes=31), dict(fmt=2), dict(fmt=-1), dict(B=-1), dict(B=65536),
                 dict(max_n=-1), dict(out_stride=31), dict(out_width=29), dict(padding_value=float("inf")), dict(padding_value=float("-inf")),
                 dict(padding_value=float("nan")), dict(normalize=0, workspace=None, ws_bytes=0, padding_value=float("nan"))]
    for bad in bad_calls:
        assert _call(lib, **bad) == -1, bad
        assert b"wave_norm" in lib.uvx_last_error(), bad
    assert _call(lib, out_width=29) == -1 and b"out_width=29" in lib.uvx_last_error() and b"max_n=30" in lib.uvx_last_error()
    assert _call(lib, B=0) == 0 and _call(lib, B=0, workspace=None, ws_bytes=0) == 0             # an empty batch is a no-op
    assert _call(lib, max_n=0, out_width=0, out_stride=0, workspace=None, ws_bytes=0) == 0       # so is an empty width
    with pytest.raises(ValueError, match="padding_value"):
        _lib.check(_call(lib, padding_value=float("inf")), "uvx_wave_norm")


def test_ops_wave_norm_checks_its_arguments_in_python():
    off, n = torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="int16 or float32"):
        ops.wave_norm(torch.zeros(4, dtype=torch.float64), off, n, max_n=1)
    with pytest.raises(ValueError, match="1-D"):
        ops.wave_norm(torch.zeros(2, 4), off, n, max_n=1)
    with pytest.raises(ValueError, match="contiguous"):
        ops.wave_norm(torch.zeros(8)[::2], off, n, max_n=1)
    with pytest.raises(ValueError, match="int64"):
        ops.wave_norm(torch.zeros(4), off.to(torch.int32), n, max_n=1)
    with pytest.raises(ValueError, match="int32"):
        ops.wave_norm(torch.zeros(4), off, n.to(torch.int64), max_n=1)
    with pytest.raises(ValueError, match="int64"):
        ops.wave_norm(torch.zeros(4), torch.zeros(2, dtype=torch.int64), n, max_n=1)
    for out in (torch.zeros(1, 4, dtype=torch.float64), torch.zeros(2, 4), torch.zeros(4), torch.zeros(1, 8)[:, ::2]):
        with pytest.raises(ValueError, match="out has to be f32"):
            ops.wave_norm(torch.zeros(4), off, n, max_n=1, out=out)
    with pytest.raises(ValueError, match="out has to be f32"):
        ops.wave_norm(torch.zeros(4), off, n, max_n=4, out=torch.zeros(1, 3), out_width=4)
    empty = ops.wave_norm(torch.zeros(4), off[:0], n[:0], max_n=0, out_width=5)
    assert empty.shape == (0, 5) and empty.dtype == torch.float32
    assert ops.WAVENORM_CHUNK == 16384


# ---------------------------------------------------------------- the extractor
def test_the_default_extractor_is_the_host_path_bit_for_bit():
    rng = np.random.default_rng(3)
    clips = [(0.1 * rng.standard_normal(n) + 0.01).astype(np.float32) for n in (700, 1, 1234)] + [rng.standard_normal(333)]      # the last: float64
    fe = Wav2Vec2FeatureExtractor(padding_value=-1.5)
    assert fe.normalize_on_device is False and fe.device is None
    got = fe(clips, sampling_rate=16000, pad_to_multiple_of=320, return_attention_mask=True)
    assert not got["input_values"].is_cuda and got["input_values"].dtype == torch.float32 and got["input_values"].shape == (4, 1280)
    want = np.full((4, 1280), -1.5, dtype=np.float32)
    for i, x in enumerate(clips):
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        x = (x - x.mean()) / np.sqrt(x.var() + 1e-7)
        want[i, : len(x)] = x
    assert np.array_equal(got["input_values"].numpy().view(np.uint32), want.view(np.uint32))
    assert got["attention_mask"].sum(-1).tolist() == [700, 1, 1234, 333] and got["attention_mask"].dtype == torch.int32
    plain = Wav2Vec2FeatureExtractor(do_normalize=False)(clips[0])
    assert set(plain) == {"input_values"} and np.array_equal(plain["input_values"].numpy()[0], clips[0])


def test_normalize_on_device_has_no_cpu_form():
    with pytest.raises(ValueError, match="no CPU form"):
        Wav2Vec2FeatureExtractor(normalize_on_device=True, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(ValueError, match="no CPU form"):
            Wav2Vec2FeatureExtractor(normalize_on_device=True)
