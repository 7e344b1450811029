"""(CPU) The augmentation layer without a GPU: the registry against the reference's table of named configs (tests/golden/aug_configs.json),
overrides and children, the types that are not built, the host randomness in the reference's call order, the filter's warm-up length, the numpy
restatements of aug_util.py held to account, and the three entry points' exports, workspace size and argument checks."""
import ctypes as C
import inspect
import json
import os
import random

import numpy as np
import pytest
import torch

import aug_util as AU
from ultravox_amd import _lib, aug, ops
from ultravox_amd.aug import AugmentationArgs, AugmentationConfig, AugRegistry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "aug_configs.json")))
BLOCK = ops.AUG_IIR_BLOCK


def butter(kind):
    from scipy.signal import butter as design
    return {"band5": lambda: design(5, [300 / 8000, 3400 / 8000], btype="band"), "low2": lambda: design(2, 3400 / 8000, btype="low"),
            "low5_100": lambda: design(5, 100 / 8000, btype="low")}[kind]()


# ---------------------------------------------------------------- registry
def test_the_registry_is_the_reference_table():
    assert {k: dict(type=c.type, params=c.params, description=c.description) for k, c in AugRegistry._configs.items()} == GOLDEN["configs"]
    for name, c in AugRegistry._configs.items():
        assert c.name == name and c.children is None and c.args.to_dict() == GOLDEN["args_defaults"]
    assert AugmentationArgs().to_dict() == GOLDEN["args_defaults"] and AugmentationArgs().param_names() == ["p", "sample_rate"]
    for type_name, defaults in GOLDEN["type_defaults"].items():
        sig = inspect.signature(AugRegistry.get_type(type_name).__init__).parameters
        got = {k: p.default for k, p in sig.items() if k not in ("self", "args", "device", "seed")}
        assert got == defaults, type_name
        assert sig["device"].default == "cuda"
    assert set(AugRegistry._aug_types) == set(GOLDEN["type_defaults"]) | set(GOLDEN["unbuilt_types"]) | {"null"}
    assert AugRegistry.get_type(None) is AugRegistry.get_type("null") is aug.Augmentation
    with pytest.raises(KeyError, match="not found"):
        AugRegistry.get_type("reverb")


def test_overrides_make_an_updated_copy_and_children_resolve_by_name():
    base = AugRegistry.get_config("random_gain")
    assert base is AugRegistry._configs["random_gain"]
    got = AugRegistry.get_config("random_gain", {"p": 0.25, "max_gain_db": 3.0, "description": "less"})
    assert got is not base and got.args.p == 0.25 and got.args.sample_rate == 16000 and got.description == "less"
    assert got.params == {"min_gain_db": -24.0, "max_gain_db": 3.0} and base.params["max_gain_db"] == 15.0 and base.args.p == 1.0
    new = AugRegistry.get_config("my_noise", {"type": "colored_noise", "noise_type": "brown", "p": 0.5})
    assert new.name == "my_noise" and new.type == "colored_noise" and new.params == {"noise_type": "brown"} and new.args.p == 0.5
    assert "my_noise" not in AugRegistry._configs
    chain = AugRegistry.get_config("phone", {"children": [{"name": "random_gain", "p": 0.5}, {"name": "telephone_bandpass"},
                                                           AugmentationConfig(name="x", type="gain", params={"gain_db": 1.0})], "p": 0.75})
    assert chain.type is None and chain.args.p == 0.75 and [c.name for c in chain.children] == ["random_gain", "telephone_bandpass", "x"]
    assert chain.children[0].args.p == 0.5 and chain.children[1] is AugRegistry._configs["telephone_bandpass"]
    for bad in ({}, None, {"p": 0.5}, {"type": "gain", "children": []}):
        with pytest.raises(AssertionError):
            AugRegistry.get_config("unknown", bad)
    for bad in ({"type": "gain"}, {"name": "other"}):
        with pytest.raises(AssertionError):
            AugRegistry.get_config("gain", bad)
    built = AugRegistry.create_augmentation(chain)
    assert type(built) is aug.Augmentation and built.p == 0.75 and [type(c).__name__ for c in built.children] == ["RandomGain", "BandpassFilter", "Gain"]
    assert built.children[0].p == 0.5 and built.children[2].gain_db == 1.0 and built.children[1].warm == 858
    with pytest.raises(AssertionError, match="both children"):
        AugRegistry.create_augmentation(AugmentationConfig(name="x", type="gain", children=[base]))
    seeded = AugRegistry.create_augmentation(AugRegistry.get_config("pink_noise", {"seed": 7, "device": "cuda:0"}))
    assert (seeded.seed, seeded.offset, seeded.noise_type, seeded.snr_db, seeded.device) == (7, 0, "pink", 20, "cuda:0")
    parent = AugRegistry.create_parent_augmentation([seeded])
    assert type(parent) is aug.Augmentation and parent.p == 1.0 and parent.children == [seeded]
    with pytest.raises(AssertionError):
        AugRegistry.create_augmentation(AugRegistry.get_config("gain", {"p": 1.5}))
    with pytest.raises(AssertionError):
        AugRegistry.create_augmentation(AugRegistry.get_config("white_noise", {"noise_type": "grey"}))


def test_unbuilt_types_and_a_cpu_device_are_refused():
    for name in GOLDEN["unbuilt_types"]:
        with pytest.raises(NotImplementedError, match="not built"):
            AugRegistry.create_augmentation(AugmentationConfig(name="x", type=name, params={"target_sr": 8000}))
    with pytest.raises(NotImplementedError, match="soxr_hq"):
        AugRegistry.get_type("resampling")(args=AugmentationArgs())
    with pytest.raises(NotImplementedError, match="ffmpeg"):
        AugRegistry.get_type("compression")(args=AugmentationArgs())
    for name in GOLDEN["type_defaults"]:
        with pytest.raises(ValueError, match="no CPU form"):
            AugRegistry.get_type(name)(args=AugmentationArgs(), device="cpu")


# ---------------------------------------------------------------- host randomness
class Sample:
    def __init__(self, audio):
        self.audio = audio


def test_decisions_and_draws_come_in_the_reference_call_order(monkeypatch):
    """A three-stage chain under a parent: per clip one random.random() for the parent, then per child one random.random() and - where the child
    applies - its np.random.uniform.  The device launch is replaced by a recorder, so this needs no GPU."""
    log = []
    monkeypatch.setattr(aug._DeviceAugmentation, "_run", lambda self, rows, values: (log.append((type(self).__name__, list(values))), rows)[1])
    ps = {"random_gain": 0.6, "random_pink_noise": 0.5, "telephone_bandpass": 0.7}
    chain = AugRegistry.create_parent_augmentation([AugRegistry.create_augmentation(AugRegistry.get_config(k, {"p": p})) for k, p in ps.items()])
    clips = [np.zeros(8, dtype=np.float32) for _ in range(40)]
    random.seed(11)
    np.random.seed(12)
    for x in clips:
        s = chain.apply_sample(Sample(x))
        assert s.audio is x
    assert chain.apply_sample(Sample(None)).audio is None and chain(None) is None      # the parent's draw is made, nothing else
    got, log[:] = list(log), []

    random.seed(11)
    np.random.seed(12)
    want = []
    for _ in clips:
        assert random.random() <= 1.0                                  # the parent, p = 1
        if random.random() <= ps["random_gain"]:
            want.append(("RandomGain", [np.random.uniform(-24.0, 15.0)]))
        if random.random() <= ps["random_pink_noise"]:
            want.append(("RandomColoredNoise", [np.random.uniform(0.0, 20.0)]))
        if random.random() <= ps["telephone_bandpass"]:
            want.append(("BandpassFilter", [None]))
    assert got == want and len({k for k, _ in got}) == 3 and 30 < len(got) < 100

    # the batch form: stage by stage, each stage's decisions in clip order, one launch per stage over the rows it applies to
    random.seed(11)
    np.random.seed(12)
    out = chain.apply_batch(clips + [None])
    assert all(a is b for a, b in zip(out, clips + [None]))
    random.seed(11)
    np.random.seed(12)
    assert all(random.random() <= 1.0 for _ in range(len(clips) + 1))
    want = []
    for name, (key, lo_hi) in zip(("RandomGain", "RandomColoredNoise", "BandpassFilter"),
                                  (("random_gain", (-24.0, 15.0)), ("random_pink_noise", (0.0, 20.0)), ("telephone_bandpass", None))):
        rows = [i for i in range(len(clips)) if random.random() <= ps[key]]
        want.append((name, [np.random.uniform(*lo_hi) if lo_hi else None for _ in rows]))
    assert log == want


def test_gain_and_noise_ratio_are_rounded_as_the_header_says():
    assert aug.gain_linear(10.0) == np.float32(10 ** 0.5) and aug.gain_linear(0.0) == 1.0 and type(aug.gain_linear(-3.0)) is np.float32
    x = np.array([0.3, -0.9, 0.5], dtype=np.float32)
    assert np.array_equal(AU.gain_ref(x, 7.3), np.clip(x * 10 ** (7.3 / 20), -1.0, 1.0)) and (x * 10 ** (7.3 / 20)).dtype == np.float32


# ---------------------------------------------------------------- the filter's warm-up
def test_warm_len_of_the_three_filters_and_the_limit():
    assert [aug.iir_warm_len(*butter(k)) for k in ("band5", "low2", "low5_100")] == [858, 34, 2309]
    bp = aug.BandpassFilter(AugmentationArgs())
    assert bp.warm == 858 and len(bp.a) == 11 and bp.a[0] == 1.0 and np.array_equal(bp.b, butter("band5")[0])
    assert aug.LowpassFilter(AugmentationArgs()).warm == 34
    with pytest.raises(ValueError, match="65536"):
        aug.iir_warm_len([1.0, 0.0], [1.0, -0.99999])
    with pytest.raises(ValueError, match="not a stable"):
        aug.iir_warm_len([1.0, 0.0], [1.0, -1.5])
    with pytest.raises(ValueError, match="orders 1 to 16"):
        aug.BandpassFilter(AugmentationArgs(), order=9)


# ---------------------------------------------------------------- the restatements hold themselves to account
def test_the_normals_have_mean_zero_and_variance_one():
    n = 1 << 16
    for seed, offset, b in ((1, 0, 0), (2 ** 63 + 5, 2 ** 40, 7)):
        g = AU.normals(seed, offset, b, n)
        assert abs(g.mean()) <= 5 / np.sqrt(n) and abs(g.var() - 1.0) <= 5 * np.sqrt(2 / n)
        assert np.array_equal(AU.normals(seed, offset, b, 37), g[:37])
    assert not np.array_equal(AU.normals(1, 0, 0, 64), AU.normals(1, 1, 0, 64)) and not np.array_equal(AU.normals(1, 0, 0, 64), AU.normals(1, 0, 1, 64))


def test_pink_and_brown_have_their_spectral_slopes():
    for colour, want in (("pink", -1.0), ("brown", -2.0)):
        slope = np.mean([AU.periodogram_slope(AU.noise_ref(4096, colour, seed, 0, 0)) for seed in range(64)])
        assert abs(slope - want) <= 0.1, (colour, slope)


def test_the_mix_reaches_the_requested_snr():
    rng = np.random.default_rng(3)
    for colour in AU.COLOURS:
        for n, snr in ((1, 3.0), (2, 20.0), (1000, 0.0), (4097, -7.5)):
            x = (0.2 * rng.standard_normal(n)).astype(np.float32)
            y = AU.mix_ref(x, AU.noise_ref(n, colour, 9, 2, 1), snr)
            assert abs(AU.snr_db_of(x, y) - snr) <= 1e-9, (colour, n)
    silent = np.zeros(5, dtype=np.float32)
    assert np.array_equal(AU.mix_ref(silent, AU.noise_ref(5, "pink", 1, 0, 0), 10.0), silent)
    assert AU.grid_m(1) == 2 and AU.grid_m(2) == 2 and AU.grid_m(3) == 4 and AU.grid_m(4096) == 4096 and AU.grid_m(4097) == 8192


@pytest.mark.parametrize("kind,warm", [("band5", 858), ("low2", 34), ("low5_100", 2309)])
def test_the_warm_up_restatement_is_within_the_bar_of_the_truth(kind, warm):
    b, a = butter(kind)
    rng = np.random.default_rng(4)
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, warm + BLOCK + 3, 3 * BLOCK + warm + 17):
        x = AU.iir_case(n, rng)
        truth, bar, d = AU.iir_bar(b, a, x)
        y = AU.iir_warm_ref(b, a, x, warm, BLOCK)
        assert np.all(np.abs(y.astype(np.longdouble) - truth) <= bar), (kind, n)
        assert d <= 1e-6 * max(float(np.sqrt(np.mean(truth.astype(np.float64) ** 2))), 1e-3)      # the realisation's noise is small against the signal
    # ... and the bar refuses a warm-up that is much too short
    x = AU.iir_case(3 * BLOCK + warm + 17, rng)
    truth, bar, _ = AU.iir_bar(b, a, x)
    assert np.any(np.abs(AU.iir_warm_ref(b, a, x, warm // 8, BLOCK).astype(np.longdouble) - truth) > bar)


# ---------------------------------------------------------------- exports, workspace size, argument checks (no GPU work happens before them)
def test_the_entry_points_are_exported_and_the_constants_are_mirrored():
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "uvx.h")).read()
    for name in ("uvx_aug_gain", "uvx_aug_iir", "uvx_aug_noise_ws_bytes", "uvx_aug_noise"):
        assert name in _lib.EXPORTS and name + "(" in header and getattr(lib, name).argtypes is not None
    assert lib.uvx_aug_noise_ws_bytes.restype is C.c_size_t and lib.uvx_abi_version() == 19
    consts = open(os.path.join(ROOT, "ultravox_amd", "csrc", "aug.h")).read()
    for text in (f"constexpr int BLOCK = {ops.AUG_IIR_BLOCK};", f"constexpr int MAX_ORDER = {ops.AUG_IIR_MAX_ORDER};",
                 f"constexpr int LDS_SPAN = {ops.AUG_FFT_LDS_SPAN};", "constexpr int LDS_LOG2 = 12;", "constexpr int MAX_LOG2_M = 21;",
                 "constexpr int CHUNK = 16384;"):
        assert text in consts, text
    assert ops.AUG_FFT_LDS_SPAN == 1 << 12 and ops.AUG_NOISE_MAX_N == 1 << 21 and ops.AUG_COLOURS == AU.COLOURS
    for src in ("aug.hip",):      # the float64 recurrences and sums are compiled as written
        assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "ultravox_amd", "csrc", src)).read()


def test_noise_ws_bytes():
    f = _lib.lib().uvx_aug_noise_ws_bytes
    assert [f(1, 1, 0), f(1, 16384, 0), f(1, 16385, 0), f(3, 2 * 16384 + 1, 0)] == [16, 16, 32, 3 * 3 * 16]
    assert [f(1, 1, 1), f(1, 2, 2), f(1, 3, 3), f(2, 4096, 4), f(2, 4097, 1)] == [16 + 8, 16 + 8, 16 + 16, 2 * (16 + 2048 * 8), 2 * (16 + 4096 * 8)]
    assert f(8, 480000, 1) == 8 * (30 * 16 + (1 << 18) * 8) and f(8, 480000, 0) == 8 * 30 * 16
    assert [f(0, 5, 1), f(-1, 5, 1), f(3, 0, 1), f(3, -7, 0), f(0, 0, 0)] == [0, 0, 0, 0, 0]
    assert f(65535, 2 ** 31 - 1, 0) == 65535 * 131072 * 16                # no 32-bit product on the way


LAYOUT = dict(stream=None, fmt=1, pcm=64, row_offset=64, n=64, B=1, max_n=30, out=64, out_stride=40, out_width=32)      # 64: never read


def _gain(lib, **kw):
    a = dict(LAYOUT, gain=64)
    a.update(kw)
    return lib.uvx_aug_gain(a["stream"], a["fmt"], a["pcm"], a["row_offset"], a["n"], a["B"], a["max_n"], a["gain"], a["out"], a["out_stride"],
                            a["out_width"])


def _iir(lib, **kw):
    a = dict(LAYOUT, b=64, a=64, order=2, warm=34)
    a.update(kw)
    return lib.uvx_aug_iir(a["stream"], a["fmt"], a["pcm"], a["row_offset"], a["n"], a["B"], a["max_n"], a["b"], a["a"], a["order"], a["warm"],
                           a["out"], a["out_stride"], a["out_width"])


def _noise(lib, **kw):
    a = dict(LAYOUT, colour=1, ratio=64, seed=1, offset=0, workspace=64, ws_bytes=16 + 16 * 8)
    a.update(kw)
    return lib.uvx_aug_noise(a["stream"], a["fmt"], a["pcm"], a["row_offset"], a["n"], a["B"], a["max_n"], a["colour"], a["ratio"], a["seed"],
                             a["offset"], a["out"], a["out_stride"], a["out_width"], a["workspace"], a["ws_bytes"])


def test_every_invalid_argument_is_refused_with_a_message_before_any_device_work():
    lib = _lib.lib()
    shared = [dict(pcm=None), dict(row_offset=None), dict(n=None), dict(out=None), dict(fmt=2), dict(fmt=-1), dict(B=-1), dict(B=65536),
              dict(max_n=-1), dict(out_stride=31), dict(out_width=29)]
    for call, tag, own in ((_gain, b"aug_gain", [dict(gain=None)]),
                           (_iir, b"aug_iir", [dict(b=None), dict(a=None), dict(order=0), dict(order=17), dict(order=-3), dict(warm=-1)]),
                           (_noise, b"aug_noise", [dict(ratio=None), dict(colour=-1), dict(colour=5), dict(workspace=None), dict(ws_bytes=16 + 16 * 8 - 1),
                                                   dict(colour=0, ws_bytes=15)])):
        for bad in shared + own:
            assert call(lib, **bad) == -1, (tag, bad)
            assert tag in lib.uvx_last_error(), (tag, bad)
        assert call(lib, B=0) == 0                                                  # an empty batch is a no-op
        assert call(lib, max_n=0, out_width=0, out_stride=0) == 0                  # so is an empty width
    assert _iir(lib, order=17) == -1 and b"order=17" in lib.uvx_last_error()
    assert _noise(lib, B=0, workspace=None, ws_bytes=0) == 0 and _noise(lib, max_n=0, out_width=0, out_stride=0, workspace=None, ws_bytes=0) == 0
    big = (1 << 21) + 1
    assert _noise(lib, max_n=big, out_width=big, out_stride=big, ws_bytes=1 << 40) == -4      # coloured noise beyond its limit is refused ...
    assert b"2097152" in lib.uvx_last_error() and b"white" in lib.uvx_last_error()
    assert _noise(lib, colour=0, B=0, max_n=big, out_width=big, out_stride=big) == 0          # ... white noise has none
    with pytest.raises(ValueError, match="order"):
        _lib.check(_iir(lib, order=0), "uvx_aug_iir")
    with pytest.raises(_lib.UvxError, match="2097152"):
        _lib.check(_noise(lib, max_n=big, out_width=big, out_stride=big, ws_bytes=1 << 40), "uvx_aug_noise")


def test_the_python_wrappers_check_their_arguments():
    off, n = torch.zeros(1, dtype=torch.int64), torch.ones(1, dtype=torch.int32)
    coef = torch.ones(3, dtype=torch.float64)
    for call in (lambda **kw: ops.aug_gain(kw.pop("pcm", torch.zeros(4)), kw.pop("off", off), kw.pop("n", n), [1.0], max_n=1, **kw),
                 lambda **kw: ops.aug_iir(kw.pop("pcm", torch.zeros(4)), kw.pop("off", off), kw.pop("n", n), coef, coef, 3, max_n=1, **kw),
                 lambda **kw: ops.aug_noise(kw.pop("pcm", torch.zeros(4)), kw.pop("off", off), kw.pop("n", n), [0.1], colour="pink", seed=1, offset=0,
                                            max_n=1, **kw)):
        with pytest.raises(ValueError, match="int16 or float32"):
            call(pcm=torch.zeros(4, dtype=torch.float64))
        with pytest.raises(ValueError, match="1-D"):
            call(pcm=torch.zeros(2, 4))
        with pytest.raises(ValueError, match="int64"):
            call(off=off.to(torch.int32))
        with pytest.raises(ValueError, match="int32"):
            call(n=n.to(torch.int64))
        with pytest.raises(ValueError, match="out has to be f32"):
            call(out=torch.zeros(2, 4))
        assert call(off=off[:0], n=n[:0], out_width=5).shape == (0, 5)
    with pytest.raises(ValueError, match="float64"):
        ops.aug_iir(torch.zeros(4), off, n, coef.float(), coef, 3, max_n=1)
    with pytest.raises(ValueError, match="gain has to be"):
        ops.aug_gain(torch.zeros(4), off, n, [1.0, 2.0], max_n=1)
    with pytest.raises(KeyError):
        ops.aug_noise(torch.zeros(4), off, n, [0.1], colour="grey", seed=1, offset=0, max_n=1)

