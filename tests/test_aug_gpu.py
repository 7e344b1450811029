"""(GPU) uvx_aug_gain, uvx_aug_iir and uvx_aug_noise against the restatements of aug_util.py at the smallest shapes where they can go wrong, then
the augmentation layer through UltravoxDataproc.

* gain: bit for bit against numpy's float32 multiply and clip; both formats, an int16 row at an odd element offset, gains that clip on both
  sides, n in {0, 1, 255, 256, 257} with the empty row in the middle of a ragged batch, padding and the stride's tail.
* filter: the three filters of the issue at n in {0, 1, BLOCK - 1, BLOCK, BLOCK + 1, warm + BLOCK + 3, 3 BLOCK + warm + 17}: a block that starts at
  sample 0, one that starts exactly `warm` back, one that looks back across several blocks.  Per element |out - (float)truth| <= 2^-23 |truth| +
  8 d with the longdouble recurrence as truth and d the distance of scipy's float64 lfilter from it on the same case.
* noise: five colours, n in {1, 2, 3, M/2 + 1, M - 1, M} for M = 4, the largest M inside the LDS span of csrc/aug.h (8192), the next one (one
  global pass) and the one after (two).  max |noise_dev - noise_ref| <= t rms(noise_ref), the noise seen through `out` (out - x under a signal
  40 dB below the noise); t = 4 x the largest distance of the same definition evaluated in float32 on the CPU from the float64 restatement
  over the same cases, measured here before the device is looked at, and required to stay below 1e-4.  The figures are printed as AUG-EDGE
  lines (profiles/aug_edges.txt holds them).
"""
import functools
import random
import types

import numpy as np
import pytest
import torch

import aug_util as AU
from ultravox_amd import aug, ops
from ultravox_amd.aug import AugRegistry

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 777.0          # what the out buffer holds beyond out_width: the kernels must leave it
BLOCK = ops.AUG_IIR_BLOCK
SPAN = ops.AUG_FFT_LDS_SPAN


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(fn, clips, out_width=None, stride=None, offs=None, **kw):
    """One call of an ops wrapper over `clips` laid out in one buffer, row b from element offs[b] on (what lies between the rows holds a loud value
    that would show in the result) -> out [B, stride] on the host."""
    lens = [len(x) for x in clips]
    if offs is None:
        offs = [int(v) for v in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    assert all(o + m <= p for o, m, p in zip(offs, lens, offs[1:]))
    out_width = max(lens) if out_width is None else out_width
    stride = out_width if stride is None else stride
    buf = np.full(offs[-1] + lens[-1] + 1, 12345 if clips[0].dtype == np.int16 else 1.0e6, dtype=clips[0].dtype)
    for o, x in zip(offs, clips):
        buf[o:o + len(x)] = x
    out = torch.full((len(clips), stride), SENT, device=DEV, dtype=torch.float32)
    got = fn(torch.from_numpy(buf).to(DEV), torch.tensor(offs, dtype=torch.int64, device=DEV), torch.tensor(lens, dtype=torch.int32, device=DEV),
             max_n=max(lens), out=out, out_width=out_width, **kw)
    assert got is out
    return out.cpu().numpy()


def check_edges(row, n, out_width, what):
    assert np.array_equal(bits(row[n:out_width]), bits(np.zeros(out_width - n))), f"{what}: padding is not +0.0 bit for bit"
    assert np.all(row[out_width:] == SENT), f"{what}: the kernel wrote beyond out_width"


# ================================================================ gain
def gain_clip(n, fmt, rng):
    if fmt == "int16":
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        if n:
            x[0] = -32768
        if n > 1:
            x[-1] = 32767
        return x
    return (rng.standard_normal(n) * 0.3).astype(np.float32)


@pytest.mark.parametrize("fmt", ["f32", "int16"])
def test_gain_is_numpy_bit_for_bit(fmt):
    rng = np.random.default_rng(5)
    lens, dbs = [1, 255, 0, 256, 257], [15.0, -24.0, 3.0, 20.0, 0.0]         # 15 and 20 dB clip on both sides; the empty row lies in the middle
    clips = [gain_clip(n, fmt, rng) for n in lens]
    offs = [1, 4, 300, 301, 600]                                             # odd element offsets among them
    gains = np.array([aug.gain_linear(g) for g in dbs], dtype=np.float32)
    out = run(lambda *a, **kw: ops.aug_gain(*a, gains, **kw), clips, out_width=260, stride=263, offs=offs)
    for b, (x, db) in enumerate(zip(clips, dbs)):
        want = AU.gain_ref(x, db)
        assert np.array_equal(bits(out[b, :len(x)]), bits(want)), (fmt, len(x))
        check_edges(out[b], len(x), 260, f"gain {fmt} n={len(x)}")
    big = AU.gain_ref(clips[3], 20.0)
    assert big.max() == 1.0 and big.min() == -1.0 and np.abs(AU.gain_ref(clips[1], -24.0)).max() < 1.0      # the case does clip, on both sides
    alone = run(lambda *a, **kw: ops.aug_gain(*a, gains[4:], **kw), clips[4:], offs=[0])                     # a row's bits do not depend on the batch
    assert np.array_equal(bits(alone[0]), bits(out[4, :257]))
    empty = run(lambda *a, **kw: ops.aug_gain(*a, gains[:1], **kw), [clips[2]], out_width=3, stride=5, offs=[0])
    check_edges(empty[0], 0, 3, "gain n=0")


# ================================================================ filter
FILTERS = {"band5": (858, lambda design: design(5, [300 / 8000, 3400 / 8000], btype="band")), "low2": (34, lambda design: design(2, 3400 / 8000, btype="low")),
           "low5_100": (2309, lambda design: design(5, 100 / 8000, btype="low"))}


@functools.lru_cache(maxsize=None)
def iir_cases(kind):
    """(b, a, warm, [(x, truth, bar, d)]) of one filter, computed once and shared (and never modified)."""
    from scipy.signal import butter
    warm, design = FILTERS[kind]
    b, a = design(butter)
    assert aug.iir_warm_len(b, a) == warm
    rng = np.random.default_rng(6)
    cases = []
    for n in (0, 1, BLOCK - 1, BLOCK, BLOCK + 1, warm + BLOCK + 3, 3 * BLOCK + warm + 17):
        x = AU.iir_case(n, rng)
        cases.append((x,) + AU.iir_bar(b, a, x))
    return b, a, warm, cases


def iir_fn(b, a, warm):
    bd, ad = torch.from_numpy(np.asarray(b)).to(DEV), torch.from_numpy(np.asarray(a)).to(DEV)
    return lambda *args, **kw: ops.aug_iir(*args, bd, ad, warm, **kw)


@pytest.mark.parametrize("kind", list(FILTERS))
def test_the_filter_is_within_the_bar_of_the_truth(kind):
    b, a, warm, cases = iir_cases(kind)
    fn = iir_fn(b, a, warm)
    worst = 0.0
    for x, truth, bar, d in cases:
        n = len(x)
        out = run(fn, [x], out_width=n + 3, stride=n + 8, offs=[1])
        want = truth.astype(np.float32).astype(np.float64)                  # (float)truth
        err = np.abs(out[0, :n].astype(np.float64) - want)
        if n:
            worst = max(worst, float(np.max(err / bar)))
            rms = float(np.sqrt(np.mean(truth.astype(np.float64) ** 2)))
            print(f"AUG-EDGE iir {kind} n={n} warm={warm} d={d:.3e} d/rms={d / rms:.3e} worst_err/bar={np.max(err / bar):.3f}")
        assert np.all(err <= bar), f"{kind} n={n}: output {int(np.argmax(err / bar))} is off by {err.max():.3e}"
        check_edges(out[0], n, n + 3, f"iir {kind} n={n}")
    assert worst <= 1.0      # (0 where every output is the rounded truth itself, as for the order-2 low-pass)


def test_a_filtered_row_does_not_depend_on_its_batch():
    b, a, warm, cases = iir_cases("low2")
    fn = iir_fn(b, a, warm)
    xs = [c[0] for c in cases[1:]]
    batch = run(fn, xs, out_width=max(len(x) for x in xs) + 5, stride=max(len(x) for x in xs) + 64)
    for i, x in enumerate(xs):
        alone = run(fn, [x], out_width=len(x), stride=len(x) + 1, offs=[3])
        assert np.array_equal(bits(alone[0, :len(x)]), bits(batch[i, :len(x)])), len(x)
        check_edges(batch[i], len(x), max(len(v) for v in xs) + 5, f"iir batch row {i}")
    # int16 input: the same samples as f32 give the same bits
    q = np.random.default_rng(7).integers(-32768, 32768, 2 * BLOCK + 5).astype(np.int16)
    assert np.array_equal(bits(run(fn, [q], offs=[1])), bits(run(fn, [AU.as_f32(q)], offs=[2])))


# ================================================================ noise
NOISE_M = [4, 2 * SPAN, 4 * SPAN, 8 * SPAN]
NOISE_N = [1, 2, 3, 4] + [n for M in NOISE_M[1:] for n in (M // 2 + 1, M - 1, M)]
SEED, OFFSET, SNR_LOUD = 0x1234567887654321, 3 + (1 << 33), -40.0


@functools.lru_cache(maxsize=None)
def noise_clips():
    rng = np.random.default_rng(8)
    return [(2.0 ** -10 * rng.standard_normal(n)).astype(np.float32) for n in NOISE_N]


@functools.lru_cache(maxsize=None)
def noise_case(colour):
    """Per row b of the ragged launch: (float64 mix of the float64 noise, rms of its noise part, distance of the float32 CPU evaluation from it in
    that rms); computed once and shared."""
    rows = []
    for b, x in enumerate(noise_clips()):
        n = len(x)
        ref = AU.mix_ref(x, AU.noise_ref(n, colour, SEED, OFFSET, b), SNR_LOUD)
        cpu32 = AU.mix_ref(x, AU.noise_ref(n, colour, SEED, OFFSET, b, np.float32), SNR_LOUD).astype(np.float32)
        rms = float(np.sqrt(np.mean((ref - x) ** 2)))
        rows.append((ref, rms, float(np.max(np.abs(cpu32.astype(np.float64) - ref))) / rms))
    return rows


@functools.lru_cache(maxsize=None)
def tolerance():
    """t = 4 x the largest distance of the float32 CPU evaluation from the float64 restatement over all cases of all colours."""
    measured = max(r[2] for colour in AU.COLOURS for r in noise_case(colour))
    return measured, 4.0 * measured


def noise_fn(colour, snr_db, B, seed=SEED, offset=OFFSET):
    ratio = np.full(B, 10 ** (-snr_db / 10), dtype=np.float64)
    return lambda *a, **kw: ops.aug_noise(*a, ratio, colour=colour, seed=seed, offset=offset, **kw)


def test_the_lengths_cover_the_transform_paths():
    assert [AU.grid_m(n) for n in NOISE_N] == [2, 2, 4, 4] + [M for M in NOISE_M[1:] for _ in range(3)]
    assert NOISE_M[1] // 2 == SPAN and NOISE_M[2] // 2 == 2 * SPAN and NOISE_M[3] // 2 == 4 * SPAN      # no, one and two global passes
    measured, t = tolerance()
    print(f"AUG-EDGE noise float32-on-CPU distance from the float64 restatement (max over {len(NOISE_N)} lengths x 5 colours, in rms) = {measured:.3e}; t = {t:.3e}")
    assert 0.0 < t < 1e-4


@pytest.mark.parametrize("colour", list(AU.COLOURS))
def test_the_noise_is_the_restatement(colour):
    clips, rows = noise_clips(), noise_case(colour)
    _, t = tolerance()
    W = max(NOISE_N) + 3
    out = run(noise_fn(colour, SNR_LOUD, len(clips)), clips, out_width=W, stride=W + 5)
    worst = 0.0
    for b, (x, (ref, rms, _)) in enumerate(zip(clips, rows)):
        n = len(x)
        dist = float(np.max(np.abs(out[b, :n].astype(np.float64) - ref))) / rms
        worst = max(worst, dist)
        assert dist <= t, f"{colour} n={n}: distance {dist:.3e} of the noise's rms, t = {t:.3e}"
        check_edges(out[b], n, W, f"noise {colour} n={n}")
    print(f"AUG-EDGE noise {colour}: largest device distance = {worst:.3e} rms (t = {t:.3e})")


@pytest.mark.parametrize("fmt", ["f32", "int16"])
def test_the_requested_snr_is_reached_and_silence_stays_silent(fmt):
    rng = np.random.default_rng(9)
    lens = [1, 2, 3, 257, SPAN + 1, 16384 + 5, 40, 2 * SPAN]
    clips = [gain_clip(n, fmt, rng) for n in lens]
    clips[6] = np.zeros(40, dtype=clips[0].dtype)                       # a silent row
    offs = [int(v) for v in np.concatenate([[1], 1 + np.cumsum([n + 1 for n in lens])[:-1]])]
    for colour in ("white", "pink", "violet"):
        snrs = np.array([0.0, 20.0, 3.0, -5.0, 10.0, 12.5, 10.0, 30.0])
        ratio = 10 ** (-snrs / 10)
        out = run(lambda *a, **kw: ops.aug_noise(*a, ratio, colour=colour, seed=5, offset=0, **kw), clips, offs=offs)
        for b, (x, snr) in enumerate(zip(clips, snrs)):
            xf = AU.as_f32(x)
            if b == 6:
                assert np.array_equal(bits(out[b, :40]), bits(xf))
                continue
            assert abs(AU.snr_db_of(xf, out[b, :len(x)]) - snr) <= 1e-3, (colour, fmt, len(x))
            check_edges(out[b], len(x), max(lens), f"noise {colour} {fmt} n={len(x)}")


def test_seed_and_offset_fix_the_bits_and_rows_do_not_depend_on_the_batch():
    clips = noise_clips()
    W = max(NOISE_N)
    for colour in ("white", "brown"):
        first = run(noise_fn(colour, 10.0, len(clips)), clips)
        again = run(noise_fn(colour, 10.0, len(clips)), clips, out_width=W + 7, stride=W + 9)
        assert np.array_equal(bits(first), bits(again[:, :W]))
        other = run(noise_fn(colour, 10.0, len(clips), offset=OFFSET + 1), clips)
        reseed = run(noise_fn(colour, 10.0, len(clips), seed=SEED + 1), clips)
        for b, x in enumerate(clips):
            if len(x) > 1:      # (one sample: the mix is x +- |x| sqrt(ratio) whatever was drawn, so two draws may well agree)
                assert not np.array_equal(first[b, :len(x)], other[b, :len(x)]) and not np.array_equal(first[b, :len(x)], reseed[b, :len(x)]), (colour, len(x))
        # rows of different M in one launch equal the same rows launched alone with the same b (the other rows empty)
        for b in (0, 3, 5, 9, len(clips) - 1):
            alone = [x if i == b else x[:0] for i, x in enumerate(clips)]
            got = run(noise_fn(colour, 10.0, len(clips)), alone)
            assert np.array_equal(bits(got[b, :len(clips[b])]), bits(first[b, :len(clips[b])])), (colour, b)
            assert all(np.all(got[i, :len(clips[b])] == 0.0) for i in range(len(clips)) if i != b)


# ================================================================ through the public surface
MESSAGES = [[{"role": "user", "content": "Transcribe\n<|audio|>"}, {"role": "assistant", "content": "the quick brown fox jumps"}],
            [{"role": "system", "content": "You are helpful ."}, {"role": "user", "content": "Listen to <|audio|> and answer briefly"},
             {"role": "assistant", "content": "it says hello world"}],
            [{"role": "user", "content": "What is two plus two ?"}, {"role": "assistant", "content": "four"}]]
SECONDS = [1.0, 0.37, None]


def dataset(on_device=False):
    out = []
    for i, (messages, seconds) in enumerate(zip(MESSAGES, SECONDS)):
        audio = None if seconds is None else (0.1 * np.random.RandomState(i).randn(int(16000 * seconds))).astype(np.float32)
        if on_device and audio is not None:
            audio = torch.from_numpy(audio).to(DEV)
        out.append(types.SimpleNamespace(messages=[dict(m) for m in messages], audio=audio, sample_rate=16000, audio_transcript=""))
    return out


def chain(p):
    return AugRegistry.create_parent_augmentation([AugRegistry.create_augmentation(AugRegistry.get_config(name, dict(extra, p=p)))
                                                   for name, extra in (("random_gain", {}), ("random_pink_noise", {"seed": 21}), ("telephone_bandpass", {}))])


def process(augmentation, on_device=False):
    from fake_tokenizer import FakeChatTokenizer
    from ultravox_amd.config import LossMaskType
    from ultravox_amd.data_proc import UltravoxDataproc
    from ultravox_amd.frontend import WhisperFeatureExtractor
    from ultravox_amd.processing import UltravoxProcessor
    tok = FakeChatTokenizer(padding_side="right")
    tok.pad_token_id = tok.eos_token_id
    random.seed(31)
    np.random.seed(32)
    dp = UltravoxDataproc(dataset(on_device), UltravoxProcessor(WhisperFeatureExtractor(80, device=DEV), tokenizer=tok), LossMaskType.LAST_ASSISTANT,
                          augmentation=augmentation)
    return list(dp)


def test_a_chain_through_ultravox_dataproc():
    plain, augmented, skipped, from_device = process(None), process(chain(1.0)), process(chain(0.0)), process(chain(1.0), on_device=True)
    assert len(plain) == len(augmented) == 3 and "audio_values" not in plain[2] and "audio_values" not in augmented[2]
    for a, b, c, d in zip(plain, augmented, skipped, from_device):
        for other in (b, c, d):
            assert set(other) == set(a) and torch.equal(other["input_ids"], a["input_ids"]) and other["labels"] == a["labels"]
            for key in ("audio_lens", "audio_token_len", "audio_batch_size"):
                assert key not in a or torch.equal(other[key], a[key]), key
        if "audio_values" not in a:
            continue
        assert b["audio_values"].is_cuda and b["audio_values"].dtype == a["audio_values"].dtype and b["audio_values"].shape == a["audio_values"].shape
        assert bool(torch.isfinite(b["audio_values"]).all()) and not torch.equal(b["audio_values"], a["audio_values"])
        assert torch.equal(c["audio_values"], a["audio_values"])            # every p = 0: bit for bit the run without an augmentation
        assert torch.equal(d["audio_values"], b["audio_values"])            # a numpy clip and the same clip as a CUDA tensor: the same bits


def test_apply_and_apply_batch_return_device_clips():
    rng = np.random.default_rng(10)
    clips = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in (1000, 1, 700)] + [rng.integers(-3000, 3000, 500).astype(np.int16)]
    stage = AugRegistry.create_augmentation(AugRegistry.get_config("gain_minus_10db"))
    y = stage(clips[0])
    assert isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.shape == (1000,)
    assert np.array_equal(bits(y.cpu().numpy()), bits(AU.gain_ref(clips[0], -10.0)))
    assert stage(y).data_ptr() != y.data_ptr() and np.array_equal(bits(stage(y).cpu().numpy()), bits(AU.gain_ref(AU.gain_ref(clips[0], -10.0), -10.0)))
    whole = chain(1.0)
    random.seed(1)
    np.random.seed(2)
    outs = whole.apply_batch(clips + [None])
    assert outs[-1] is None and [tuple(o.shape) for o in outs[:-1]] == [(1000,), (1,), (700,), (500,)]
    assert all(o.is_cuda and o.dtype == torch.float32 and bool(torch.isfinite(o).all()) for o in outs[:-1])
    assert whole.children[1].offset == 1                                    # one launch of the noise stage for the whole batch
    # the batch form of a deterministic stage is the per-clip form, bit for bit
    lp = AugRegistry.create_augmentation(AugRegistry.get_config("telephone_lowpass"))
    for one, x in zip(lp.apply_batch(clips), clips):
        assert torch.equal(one, lp(x))
    nothing = chain(0.0).apply_batch(clips)
    assert all(a is b for a, b in zip(nothing, clips))
