"""(CPU) The polyphase resampler without a GPU: the filter design and the float64 oracle against scipy, the 64-bit index helpers of
csrc/resample.h against Python integers, the entry point's argument checks, LocalInference's routing and the kernel's register budget.

The index test is where 32-bit overflow is caught: it needs no GPU and runs before any GPU run of the long clip (test_resample_gpu.py)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import resample_util as RU
from fake_tokenizer import FakeChatTokenizer
from ultravox_amd import _lib, build as B, ops
from ultravox_amd.inference import LocalInference, VoiceSample
from ultravox_amd.processing import UltravoxProcessor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the definition against scipy
def test_design_resample_taps_is_scipys_default_filter():
    """Pins the definition to scipy; passes with or without the device resampler as far as resample_util goes (ops.design_resample_taps is new)."""
    signal = pytest.importorskip("scipy.signal")
    for up, down in RU.RATIOS + [(320, 441)]:
        m = max(up, down)
        want = signal.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up
        got, half = ops.design_resample_taps(up, down)
        assert half == 10 * m and got.dtype == np.float64 and got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-15, (up, down)
        assert np.abs(RU.design_taps_f64(up, down)[0] - want).max() <= 1e-15, (up, down)


def test_float64_oracle_is_scipys_resample_poly():
    """Pins the test oracle to scipy.signal.resample_poly on float64 input.  It touches no code of the package, so it passes without the feature."""
    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(0)
    for rate in (48000, 44100, 8000, 22050, 24000, 11025):
        up, down = RU.ratio(rate)
        h, half = RU.design_taps_f64(up, down)
        for n in (1, 2, 3, 57, 441, 1000):
            x = rng.standard_normal(n)
            want = signal.resample_poly(x, up, down)
            got, _ = RU.oracle(x, up, down, h, half)
            assert got.shape == want.shape, (rate, n)
            assert np.abs(got - want).max() <= 1e-13, (rate, n)


# ---------------------------------------------------------------- csrc/resample.h against Python integers
def _py_first(k, up, down, half):
    a = k * down - half
    return 0 if a <= 0 else -(-a // up)


def _py_last(k, up, down, half, n):
    return min(n - 1, (k * down + half) // up)


def test_index_helpers_are_64_bit(tmp_path):
    gxx = shutil.which("g++") or shutil.which("c++")
    assert gxx, "a host C++ compiler is needed for the index test"
    src = tmp_path / "idx.cc"
    src.write_text('#include <cstdio>\n#include <cstdlib>\n#include "resample.h"\nusing namespace uvx::resample;\n'
                   'int main(int argc, char** argv) {\n'
                   '  for (int a = 1; a + 4 < argc; a += 5) {\n'
                   '    const int64_t k = atoll(argv[a]), n = atoll(argv[a + 1]), up = atoll(argv[a + 2]), down = atoll(argv[a + 3]), half = atoll(argv[a + 4]);\n'
                   '    const int64_t f = first_i(k, up, down, half), l = last_i(k, up, down, half, n);\n'
                   '    printf("%lld %lld %lld %lld %lld\\n", (long long)n_out(n, up, down), (long long)f, (long long)l,\n'
                   '           (long long)tap_index(k, f, up, down, half), (long long)tap_index(k, l, up, down, half));\n'
                   '  }\n  printf("%d %d %d\\n", TILE, MAX_RATIO, XCHUNK);\n  return 0;\n}\n')
    exe = tmp_path / "idx"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", str(B.CSRC), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cases = []
    n, up, down, half = 2 ** 24 + 5, 160, 441, 4410
    nout = RU.n_out(n, up, down)
    k31 = 2 ** 31 // down                       # k * down crosses 2^31 between k31 and k31 + 1
    ki31 = (2 ** 31 // up) * up // down         # an output whose inputs lie around i * up = 2^31
    for k in (0, 1, nout - 1, k31 - 1, k31, k31 + 1, k31 + 2, ki31 - 30, ki31, ki31 + 30):
        cases.append((k, n, up, down, half))
    assert k31 + 2 < nout and (k31 + 1) * down > 2 ** 31 > k31 * down and _py_last(ki31 + 30, up, down, half, n) * up > 2 ** 31 > _py_first(ki31 - 30, up, down, half) * up
    for up, down in RU.RATIOS:
        half = 10 * max(up, down)
        for n in (1, 2, 7, 1000):
            for k in {0, RU.n_out(n, up, down) // 2, RU.n_out(n, up, down) - 1}:
                cases.append((k, n, up, down, half))
    cases.append((2 ** 31 - 2, 2 ** 31 - 1, 1024, 1024, 10240))      # the widest products the 32-bit arguments allow
    cases.append((2 ** 21 - 1, 2 ** 31 - 1, 1, 1024, 10240))
    out = subprocess.run([str(exe)] + [str(v) for c in cases for v in c], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(cases) + 1
    for (k, n, up, down, half), line in zip(cases, lines):
        f, l = _py_first(k, up, down, half), _py_last(k, up, down, half, n)
        want = [RU.n_out(n, up, down), f, l, half + k * down - f * up, half + k * down - l * up]
        assert [int(v) for v in line.split()] == want, (k, n, up, down, half)
        assert 0 <= want[4] <= want[3] <= 2 * half, (k, n, up, down, half)
    assert [int(v) for v in lines[-1].split()][:2] == [ops.RESAMPLE_TILE, ops.RESAMPLE_MAX_RATIO]      # the Python mirrors of the header's constants


# ---------------------------------------------------------------- the entry point's argument checks (no GPU work happens before them)
def _call(lib, **kw):
    a = dict(stream=None, fmt=1, pcm=64, row_offset=64, n_in=64, B=1, max_n_in=30, up=1, down=3, taps=64, half=30, out=64, out_stride=16, out_width=10)
    a.update(kw)      # 64: a non-null address that is never read, every check comes before the launch
    return lib.uvx_resample_poly(a["stream"], a["fmt"], a["pcm"], a["row_offset"], a["n_in"], a["B"], a["max_n_in"], a["up"], a["down"], a["taps"],
                                 a["half"], a["out"], a["out_stride"], a["out_width"])


def test_entry_point_is_exported_and_checks_its_arguments():
    lib = _lib.lib()
    assert "uvx_resample_poly" in _lib.EXPORTS and lib.uvx_resample_poly.argtypes is not None
    for bad in (dict(pcm=None), dict(row_offset=None), dict(n_in=None), dict(taps=None), dict(out=None), dict(up=0), dict(down=0), dict(half=0),
                dict(fmt=2), dict(out_width=9), dict(out_stride=9), dict(B=-1)):
        assert _call(lib, **bad) == -1, bad
        assert b"resample_poly" in lib.uvx_last_error(), bad
    assert _call(lib, out_width=9) == -1 and b"out_width=9" in lib.uvx_last_error() and b"10 outputs" in lib.uvx_last_error()
    assert _call(lib, B=0) == 0                                       # an empty batch is a no-op
    with pytest.raises(ValueError, match="out_width"):
        _lib.check(_call(lib, out_width=9), "uvx_resample_poly")


def test_a_ratio_beyond_the_limit_is_refused_and_the_limit_is_named():
    lib = _lib.lib()
    lim = ops.RESAMPLE_MAX_RATIO
    assert lim >= 1024
    for kw in (dict(up=lim + 1, down=1, half=10, out_width=31 * (lim + 1)), dict(up=1, down=lim + 1, half=10), dict(half=10 * lim + 1)):
        kw.setdefault("out_stride", 1 << 20)
        assert _call(lib, **kw) == -4, kw                            # UVX_ERR_UNSUPPORTED
        assert str(lim).encode() in lib.uvx_last_error(), kw
    with pytest.raises(ValueError, match=str(lim)):                   # the Python side: a ValueError that names the limit, before any device work
        ops.resample_ratio(16001)
    with pytest.raises(ValueError, match=str(lim)):
        ops.resample_poly(torch.zeros(4), torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int32), lim + 1, 1, max_n_in=1)
    for rate in (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000):
        assert ops.resample_ratio(rate) == RU.ratio(rate)


# ---------------------------------------------------------------- LocalInference routing (the stub model of test_inference_cpu.py)
class StubModel:
    device = torch.device("cpu")
    dtype = torch.float32

    def __init__(self, tok, reply="the answer is 42 ."):
        self.tok, self.reply, self.calls = tok, reply, []

    def generate(self, **kw):
        self.calls.append(kw)
        ids = kw["input_ids"]
        new = (self.tok._tok(self.reply) + [kw["eos_token_id"][0]])[: kw["max_new_tokens"]]
        return torch.cat([ids, torch.tensor([new] * ids.shape[0])], dim=1)


def test_resample_on_device_needs_a_gpu_model_and_the_default_stays_scipy(monkeypatch):
    from oracle.reference_cpu import FeatureExtractorRef
    tok = FakeChatTokenizer()
    proc = UltravoxProcessor(FeatureExtractorRef(80), tokenizer=tok)
    with pytest.raises(ValueError, match="no CPU fallback"):
        LocalInference(StubModel(tok), proc, tok, dtype=torch.float32, resample_on_device=True)
    signal = pytest.importorskip("scipy.signal")
    calls = []
    real = signal.resample_poly
    monkeypatch.setattr(signal, "resample_poly", lambda *a, **k: (calls.append(a[1:3]), real(*a, **k))[1])
    model = StubModel(tok)
    inf = LocalInference(model, proc, tok, dtype=torch.float32)
    assert inf.resample_on_device is False
    inf.infer(VoiceSample.from_prompt_and_raw("<|audio|>", (np.ones(48000) * 1000).astype(np.int16), 48000), max_tokens=3)
    assert calls == [(1, 3)]
    assert model.calls[0]["audio_values"].shape == (1, 80, 100)


# ---------------------------------------------------------------- register budget
def test_no_resample_kernel_has_a_scratch_segment():
    src = B.CSRC / "resample.hip"
    cmd = [B._hipcc(), *B.FLAGS, *B.EXTRA_FLAGS.get(src.name, []), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", str(src),
           "-o", "/dev/null"]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    names = re.findall(r"Function Name: (\S+)", err)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
    assert len(names) == len(scratch) == 2, (names, scratch)          # the int16 and the f32 instance
    assert not any(scratch), list(zip(names, scratch))
