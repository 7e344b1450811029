"""(GPU) uvx_resample_poly against the float64 oracle of resample_util.py, output by output, at the smallest shapes where it can go wrong: one
and two samples, a clip shorter than the filter, n_out on either side of the tile, the two edges of the ceil, both input formats with the int16
extremes, a ragged batch on 2-byte-aligned rows that must reproduce the single-clip bits, and one clip long enough for k * down and i * up to
pass 2^31 (its index arithmetic is checked on the CPU first: test_resample_cpu.py::test_index_helpers_are_64_bit).  Every comparison is with
the oracle: none is with scipy's f32 output, none with the kernel itself - except the bit-identity of a batch row and the same clip alone.

Where a ratio cannot produce an n_out (2/1 gives even counts only; 640/441 skips some), the smallest n with n_out at or above the target is used.
"""
import functools

import numpy as np
import pytest
import torch

import resample_util as RU
from ultravox_amd import ops

pytestmark = pytest.mark.gpu

TILE = ops.RESAMPLE_TILE
SENT = 777.0          # what the out buffer holds beyond out_width: the kernel must leave it
DEV = "cuda"


def lengths(up, down):
    half = 10 * max(up, down)
    span = 2 * half // up + 1
    ns = [1, 2, max(3, span // 2)]
    for target in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        ns.append((target - 1) * down // up + 1)                       # the smallest n with n * up > (target - 1) * down: n_out >= target
        assert RU.n_out(ns[-1], up, down) >= target > RU.n_out(ns[-1] - 1, up, down)
        assert up > down or RU.n_out(ns[-1], up, down) == target
    base = span + 10
    ns.append(next(n for n in range(base, base + down) if n * up % down == 0))
    if down > 1:
        ns.append(next(n for n in range(base, base + down) if n * up % down == 1))
    return ns


def make_clip(n, fmt, rng):
    if fmt == "int16":
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        x[0] = -32768
        if n > 1:
            x[-1] = 32767
        return x
    return (rng.standard_normal(n) * 0.3).astype(np.float32)


def as_f32(x):
    return x.astype(np.float32) * np.float32(2.0 ** -15) if x.dtype == np.int16 else x


@functools.lru_cache(maxsize=None)
def case(up, down, fmt):
    """The clips of one ratio and format with their oracle results, computed once and shared (and never modified)."""
    rng = np.random.default_rng(1000 * up + down + (7 if fmt == "int16" else 0))
    hf, half = RU.taps_f32(up, down)
    clips = [make_clip(n, fmt, rng) for n in lengths(up, down)]
    return clips, [RU.oracle(as_f32(x), up, down, hf, half) for x in clips]


def run(clips, up, down, out_width, stride, offs=None):
    """One launch over `clips` laid out in one buffer, row b from element offs[b] on (what lies between the rows holds a value that would show
    in the result) -> out [B, stride] on the host."""
    lens = [len(x) for x in clips]
    offs = [0] * len(clips) if offs is None else offs
    assert all(o + n <= p for o, n, p in zip(offs, lens, offs[1:]))
    buf = np.full(offs[-1] + lens[-1] + 1, 12345 if clips[0].dtype == np.int16 else 1.0e6, dtype=clips[0].dtype)
    for o, x in zip(offs, clips):
        buf[o:o + len(x)] = x
    pcm = torch.from_numpy(buf).to(DEV)
    out = torch.full((len(clips), stride), SENT, device=DEV, dtype=torch.float32)
    got = ops.resample_poly(pcm, torch.tensor(offs, dtype=torch.int64, device=DEV), torch.tensor(lens, dtype=torch.int32, device=DEV), up, down,
                            max_n_in=max(lens), out=out, out_width=out_width)
    assert got is out and out.is_cuda
    return out.cpu().numpy()


def check_row(row, y, bar, out_width, what):
    n_out = len(y)
    err = np.abs(row[:n_out].astype(np.float64) - y)
    worst = int(np.argmax(err / bar))
    assert np.all(err <= bar), f"{what}: output {worst} is off by {err[worst]:.3e}, bar {bar[worst]:.3e}"
    assert np.all(row[n_out:out_width] == 0.0) and not np.any(np.signbit(row[n_out:out_width])), f"{what}: padding is not +0.0"
    assert np.all(row[out_width:] == SENT), f"{what}: the kernel wrote beyond out_width"


@pytest.mark.parametrize("fmt", ["int16", "f32"])
@pytest.mark.parametrize("up,down", RU.RATIOS)
def test_every_output_is_within_the_f32_dot_product_bar(up, down, fmt):
    clips, want = case(up, down, fmt)
    for x, (y, bar) in zip(clips, want):
        assert len(y) == RU.n_out(len(x), up, down)
        out_width = len(y) + 3
        out = run([x], up, down, out_width, out_width + 5, offs=[3 if len(x) % 2 else 0])
        check_row(out[0], y, bar, out_width, f"{up}/{down} {fmt} n={len(x)}")


@pytest.mark.parametrize("fmt", ["int16", "f32"])
@pytest.mark.parametrize("up,down", RU.RATIOS)
def test_a_ragged_batch_gives_the_bits_of_each_clip_alone(up, down, fmt):
    clips, want = case(up, down, fmt)
    pick = [6, 0, 3]                                                   # n_out past two tiles, one sample, n_out = TILE - 1 (or just above)
    rows = [clips[i] for i in pick]
    out_width = max(len(want[i][0]) for i in pick) + 7
    offs = [1]                                                         # rows at odd element offsets: an int16 row is 2-byte aligned only
    for x in rows[:-1]:
        offs.append((offs[-1] + len(x) + 1) | 1)
    assert all(o % 2 == 1 for o in offs)
    batch = run(rows, up, down, out_width, out_width + 9, offs=offs)
    for b, i in enumerate(pick):
        y, bar = want[i]
        check_row(batch[b], y, bar, out_width, f"{up}/{down} {fmt} row {b}")
        alone_width = len(y) + 1
        alone = run([clips[i]], up, down, alone_width, alone_width + 2)
        assert np.array_equal(batch[b, :len(y)].view(np.uint32), alone[0, :len(y)].view(np.uint32)), f"{up}/{down} {fmt} row {b}: bits differ"


@pytest.mark.parametrize("up,down,n", [(1, 64, 257 * 64 + 5), (1, 1024, 20 * 1024 + 3), (1024, 1, 3)])
def test_the_paths_only_extreme_ratios_take(up, down, n):
    """The kernel stages at most XCHUNK = 16384 inputs per pass and asks for more than the default 64 KB of LDS when the tap table is large.  No
    audio rate gets there (192 kHz stages 3 312 inputs next to 241 taps), so three ratios up to the limit do: 1/64 walks a tile's span in two
    passes; 1/1024 does so next to the largest table (20 481 taps, 147 KB of LDS in all); 1024/1 reads that table at every phase."""
    assert max(up, down) <= ops.RESAMPLE_MAX_RATIO
    rng = np.random.default_rng(up + down)
    hf, half = RU.taps_f32(up, down)
    for fmt in ("int16", "f32"):
        x = make_clip(n, fmt, rng)
        y, bar = RU.oracle(as_f32(x), up, down, hf, half)
        out_width = len(y) + 3
        out = run([x], up, down, out_width, out_width + 5, offs=[1])
        check_row(out[0], y, bar, out_width, f"{up}/{down} {fmt} n={n}")


def test_one_long_clip_past_the_32_bit_products():
    """n = 2^24 + 5 at 160/441 (44.1 kHz), int16 from the counter pattern: 256 outputs against the oracle - the first 64, the last 64, and 64 on
    each side of k * down = 2^31 (i * up passes 2^31 in the same neighbourhood: an output's inputs lie within half_len of k * down)."""
    up, down = 160, 441
    n = 2 ** 24 + 5
    hf, half = RU.taps_f32(up, down)
    n_out = RU.n_out(n, up, down)
    k31 = 2 ** 31 // down
    ks = np.concatenate([np.arange(64), np.arange(k31 - 63, k31 + 65), np.arange(n_out - 64, n_out)]).astype(np.int64)
    assert len(ks) == 256 and ks[64 + 63] * down < 2 ** 31 < ks[64 + 64] * down
    y, bar = RU.oracle_at(ks, n, up, down, hf, half, lambda i: RU.counter_pcm(i).astype(np.float32) * np.float32(2.0 ** -15))
    i = torch.arange(n, dtype=torch.int64, device=DEV)
    pcm = ((((i * 2654435761) >> 7) & 0xFFFF) - 32768).to(torch.int16)
    del i
    probe = torch.tensor([0, 1, 12345678, n - 1], device=DEV)
    assert pcm[probe].cpu().tolist() == RU.counter_pcm(probe.cpu().numpy()).tolist()
    out_width = n_out + 2
    out = torch.full((1, out_width + 3), SENT, device=DEV, dtype=torch.float32)
    ops.resample_poly(pcm, torch.zeros(1, dtype=torch.int64, device=DEV), torch.tensor([n], dtype=torch.int32, device=DEV), up, down, max_n_in=n,
                      out=out, out_width=out_width)
    got = out[0, torch.from_numpy(ks).to(DEV)].cpu().numpy().astype(np.float64)
    err = np.abs(got - y)
    worst = int(np.argmax(err / bar))
    assert np.all(err <= bar), f"output {ks[worst]} is off by {err[worst]:.3e}, bar {bar[worst]:.3e}"
    assert np.abs(y).max() > 0.01                                      # the comparison is not of zeros
    assert out[0, n_out:out_width].cpu().tolist() == [0.0, 0.0] and out[0, out_width:].cpu().tolist() == [SENT] * 3


def test_resample_device_casts_pads_and_feeds_the_logmel():
    from ultravox_amd.frontend import WhisperFeatureExtractor, resample_device
    rng = np.random.default_rng(5)
    x64 = rng.standard_normal(4801) * 0.2
    x16 = make_clip(2000, "int16", rng)
    out, n_out = resample_device([x64, torch.from_numpy(x16)], 48000, DEV, pad_to_multiple_of=160)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
    assert n_out == [1601, 667] and out.shape == (2, 1760) and out.shape[1] % 160 == 0
    host = out.cpu().numpy()
    for row, x in zip(host, (x64.astype(np.float32), as_f32(x16))):      # float64 is cast to f32 on the host; int16 next to float goes up as x / 32768
        y, bar = RU.oracle(x, 1, 3)
        check_row(np.concatenate([row, [SENT]]), y, bar, out.shape[1], "resample_device")
    alone, n_alone = resample_device([x16], 48000, DEV)                 # int16 alone is uploaded as int16
    assert n_alone == [667] and alone.shape == (1, 667) and np.array_equal(alone.cpu().numpy()[0].view(np.uint32), host[1, :667].view(np.uint32))
    fe = WhisperFeatureExtractor(80, device=DEV)
    mel = fe.logmel_device(out)
    assert mel.is_cuda and mel.shape == (2, 80, 11) and bool(torch.isfinite(mel).all())
    feats = fe([out[0, :n_out[0]], out[1, :n_out[1]]], sampling_rate=16000, pad_to_multiple_of=160)      # device clips through the HF call contract
    assert feats["input_features"].is_cuda and torch.equal(feats["input_features"], mel)
    assert feats["attention_mask"].sum(-1).tolist() == [11, 5]
    with pytest.raises(ValueError, match="float64 or float32 or int16"):
        resample_device([np.ones(100, dtype=np.int32)], 48000, DEV)
    with pytest.raises(ValueError, match=str(ops.RESAMPLE_MAX_RATIO)):
        resample_device([x16], 16001, DEV)


class GpuStubModel:
    device = torch.device("cuda")
    dtype = torch.float32

    def __init__(self, tok):
        self.tok, self.calls = tok, []

    def generate(self, **kw):
        self.calls.append(kw)
        ids = kw["input_ids"]
        new = (self.tok._tok("the answer is 42 .") + [kw["eos_token_id"][0]])[: kw["max_new_tokens"]]
        return torch.cat([ids, torch.tensor([new] * ids.shape[0], device=ids.device)], dim=1)


def test_local_inference_resamples_on_the_device_without_scipy(monkeypatch):
    from fake_tokenizer import FakeChatTokenizer
    from ultravox_amd.frontend import WhisperFeatureExtractor
    from ultravox_amd.inference import LocalInference, VoiceSample
    from ultravox_amd.processing import UltravoxProcessor
    signal = pytest.importorskip("scipy.signal")

    class Reached(Exception):
        pass

    def refuse(*a, **k):
        raise Reached()

    monkeypatch.setattr(signal, "resample_poly", refuse)
    tok = FakeChatTokenizer()
    proc = UltravoxProcessor(WhisperFeatureExtractor(80, device=DEV), tokenizer=tok)
    sample = VoiceSample.from_prompt_and_raw("<|audio|>", (np.ones(48000) * 1000).astype(np.int16), 48000)
    model = GpuStubModel(tok)
    inf = LocalInference(model, proc, tok, dtype=torch.float32, resample_on_device=True)
    out = inf.infer(sample, max_tokens=3)
    kw = model.calls[0]
    assert kw["audio_values"].is_cuda and kw["audio_values"].shape == (1, 80, 100) and kw["audio_token_len"].item() == 7
    assert out.output_tokens == 3
    short = proc(audio=torch.full((100,), 0.5, device=DEV), text="<|audio|>", sampling_rate=16000)      # a device clip below two hops is padded there
    assert short["audio_values"].is_cuda and short["audio_values"].shape == (1, 80, 2) and short["audio_lens"].tolist() == [2]
    with pytest.raises(Reached):                                       # the flag off: the same call does reach scipy
        LocalInference(GpuStubModel(tok), proc, tok, dtype=torch.float32).infer(sample, max_tokens=3)
