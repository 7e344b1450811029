"""(GPU) uvx_wave_norm against the float64 yardstick of wavenorm_util.py, element by element, at the smallest shapes where it can go wrong: one,
two and three samples, n on either side of the block (256) and of the chunk (16 384), past two chunks, both input formats with the int16
extremes, rows at odd element offsets, both padding values, a ragged batch that must reproduce the single-clip bits, the conversion-only mode,
clamped lengths, and one clip of 2^22 + 3 samples (256 chunks).  Then the layers above it: the extractor, the resampler chained in front,
LocalInference and the real wav2vec2 tower.  Every value comparison is with the yardstick; only the bit-identity checks compare the kernel
with itself.
"""
import functools

import numpy as np
import pytest
import torch

import resample_util as RU
import wavenorm_util as WU
from ultravox_amd import ops

pytestmark = pytest.mark.gpu

CHUNK = ops.WAVENORM_CHUNK
LENGTHS = [1, 2, 3, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
SENT = 777.0          # what the out buffer holds beyond out_width: the kernel must leave it
DEV = "cuda"


def make_clip(n, fmt, rng):
    if fmt == "int16":
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        x[0] = -32768
        if n > 1:
            x[-1] = 32767
        return x
    return (rng.standard_normal(n) * 0.3).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(fmt):
    """The clips of one format with their yardstick results, computed once and shared (and never modified)."""
    rng = np.random.default_rng(7 if fmt == "int16" else 8)
    clips = [make_clip(n, fmt, rng) for n in LENGTHS]
    return clips, [WU.oracle(WU.as_f32(x)) for x in clips]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(clips, out_width, stride, offs=None, pad=0.0, normalize=True, n=None, max_n=None):
    """One call over `clips` laid out in one buffer, row b from element offs[b] on (what lies between the rows holds a loud value that would
    show in the result) -> out [B, stride] on the host.  n / max_n: what the kernel is told, where that is not the clips' lengths."""
    lens = [len(x) for x in clips]
    offs = [0] * len(clips) if offs is None else offs
    assert all(o + m <= p for o, m, p in zip(offs, lens, offs[1:]))
    buf = np.full(offs[-1] + lens[-1] + 1, 12345 if clips[0].dtype == np.int16 else 1.0e6, dtype=clips[0].dtype)
    for o, x in zip(offs, clips):
        buf[o:o + len(x)] = x
    out = torch.full((len(clips), stride), SENT, device=DEV, dtype=torch.float32)
    got = ops.wave_norm(torch.from_numpy(buf).to(DEV), torch.tensor(offs, dtype=torch.int64, device=DEV),
                        torch.tensor(lens if n is None else n, dtype=torch.int32, device=DEV), max_n=max(lens) if max_n is None else max_n,
                        normalize=normalize, padding_value=pad, out=out, out_width=out_width)
    assert got is out and out.device.type == DEV
    return out.cpu().numpy()


def check_row(row, y, bar, out_width, pad, what):
    n = len(y)
    err = np.abs(row[:n].astype(np.float64) - y)
    worst = int(np.argmax(err / bar)) if n else 0
    assert np.all(err <= bar), f"{what}: output {worst} is off by {err[worst]:.3e}, bar {bar[worst]:.3e}"
    assert np.array_equal(bits(row[n:out_width]), bits(np.full(out_width - n, pad))), f"{what}: padding is not {pad!r} bit for bit"
    assert np.all(row[out_width:] == SENT), f"{what}: the kernel wrote beyond out_width"


@pytest.mark.parametrize("pad", [0.0, -1.5])
@pytest.mark.parametrize("fmt", ["int16", "f32"])
def test_every_output_is_within_its_bar(fmt, pad):
    clips, want = case(fmt)
    for x, (y, bar) in zip(clips, want):
        out_width = len(x) + 3
        out = run([x], out_width, out_width + 5, offs=[3 if len(x) % 2 else 1], pad=pad)
        check_row(out[0], y, bar, out_width, pad, f"{fmt} n={len(x)}")


def test_the_named_cases():
    for name, x in WU.named_cases(np.random.default_rng(11)):
        y, bar = WU.oracle(WU.as_f32(x))
        out = run([x], len(x) + 2, len(x) + 4, offs=[1])
        check_row(out[0], y, bar, len(x) + 2, 0.0, name)
        if name in ("constant_int16", "one_sample"):                   # the sums are exact: every output is exactly +0.0
            assert not np.any(bits(out[0, :len(x)])), name
        else:
            assert np.abs(y).max() > 0.05, name                        # the comparison is not of zeros (the quiet clip stays small: 1e-7 dominates its variance)


@pytest.mark.parametrize("fmt", ["int16", "f32"])
def test_a_ragged_batch_gives_the_bits_of_each_clip_alone(fmt):
    clips, want = case(fmt)
    pick = [LENGTHS.index(2 * CHUNK + 1), LENGTHS.index(1), LENGTHS.index(255)]
    rows = [clips[pick[0]], clips[pick[1]], clips[0][:0], clips[pick[2]]]      # the third row has n = 0: all padding
    out_width = 2 * CHUNK + 1 + 7
    offs = [1]                                                         # rows at odd element offsets: an int16 row is 2-byte aligned only
    for x in rows[:-1]:
        offs.append((offs[-1] + len(x) + 1) | 1)
    assert all(o % 2 == 1 for o in offs)
    batch = run(rows, out_width, out_width + 9, offs=offs, pad=-1.5)
    check_row(batch[2], np.zeros(0), np.zeros(0), out_width, -1.5, f"{fmt} empty row")
    for b, i, extra in ((0, pick[0], 1), (1, pick[1], 4), (3, pick[2], 130)):
        y, bar = want[i]
        check_row(batch[b], y, bar, out_width, -1.5, f"{fmt} row {b}")
        alone = run([clips[i]], len(y) + extra, len(y) + extra + b + 2)         # another width, another stride, offset 0, another batch size
        assert np.array_equal(bits(batch[b, :len(y)]), bits(alone[0, :len(y)])), f"{fmt} row {b}: bits differ"


@pytest.mark.parametrize("fmt", ["int16", "f32"])
def test_without_normalize_the_output_is_the_f32_conversion_bit_for_bit(fmt):
    clips, _ = case(fmt)
    rows = [clips[LENGTHS.index(CHUNK + 1)], clips[LENGTHS.index(3)]]
    if fmt == "f32":
        rows[1] = np.array([-0.0, 1e-45, -3.0e38], dtype=np.float32)   # a signed zero, a subnormal and a large value come through as they are
    out_width = CHUNK + 4
    out = run(rows, out_width, out_width + 2, offs=[1, CHUNK + 5], pad=-1.5, normalize=False)      # ops.wave_norm hands over a null workspace here
    for b, x in enumerate(rows):
        assert np.array_equal(bits(out[b, :len(x)]), bits(WU.as_f32(x))), (fmt, b)
        assert np.array_equal(bits(out[b, len(x):out_width]), bits(np.full(out_width - len(x), -1.5))) and np.all(out[b, out_width:] == SENT)


def test_a_length_above_max_n_is_clamped_and_a_negative_one_counts_as_zero():
    x = make_clip(300, "f32", np.random.default_rng(12))
    y, bar = WU.oracle(x[:257])
    out = run([x, x], 260, 262, offs=[1, 303], n=[300, -5], max_n=257)
    check_row(out[0], y, bar, 260, 0.0, "n above max_n")
    check_row(out[1], np.zeros(0), np.zeros(0), 260, 0.0, "negative n")
    alone = run([x[:257]], 257, 257)
    assert np.array_equal(bits(out[0, :257]), bits(alone[0]))


def test_one_long_clip_of_256_chunks():
    """n = 2^22 + 3 int16 samples of the counter pattern, built on the device: the first 64, the last 64 and 64 outputs across a chunk boundary
    against the yardstick (its mean and variance from the closed-form host array, the bar with this n's gamma)."""
    n = 2 ** 22 + 3
    idx = np.concatenate([np.arange(64), np.arange(128 * CHUNK - 32, 128 * CHUNK + 32), np.arange(n - 64, n)])
    y, bar = WU.oracle(WU.as_f32(RU.counter_pcm(np.arange(n)).astype(np.int16)))
    i = torch.arange(n, dtype=torch.int64, device=DEV)
    pcm = ((((i * 2654435761) >> 7) & 0xFFFF) - 32768).to(torch.int16)
    del i
    probe = torch.tensor([0, 1, 1234567, n - 1], device=DEV)
    assert pcm[probe].cpu().tolist() == RU.counter_pcm(probe.cpu().numpy()).tolist()
    out_width = n + 2
    out = torch.full((1, out_width + 3), SENT, device=DEV, dtype=torch.float32)
    ops.wave_norm(pcm, torch.zeros(1, dtype=torch.int64, device=DEV), torch.tensor([n], dtype=torch.int32, device=DEV), max_n=n, out=out,
                  out_width=out_width)
    got = out[0, torch.from_numpy(idx).to(DEV)].cpu().numpy().astype(np.float64)
    err = np.abs(got - y[idx])
    worst = int(np.argmax(err / bar[idx]))
    assert np.all(err <= bar[idx]), f"output {idx[worst]} is off by {err[worst]:.3e}, bar {bar[idx][worst]:.3e}"
    assert np.abs(y[idx]).max() > 1.0                                  # the comparison is not of zeros
    assert out[0, n:out_width].cpu().tolist() == [0.0, 0.0] and out[0, out_width:].cpu().tolist() == [SENT] * 3


def test_the_extractor_uploads_casts_pads_and_keeps_device_clips_on_the_device():
    from ultravox_amd.frontend import Wav2Vec2FeatureExtractor
    rng = np.random.default_rng(13)
    x64 = rng.standard_normal(4801) * 0.2 + 0.05
    x16 = make_clip(2000, "int16", rng)
    fe = Wav2Vec2FeatureExtractor(device=DEV, normalize_on_device=True, padding_value=-1.5)
    got = fe([x64, torch.from_numpy(x16)], sampling_rate=16000, pad_to_multiple_of=320, return_attention_mask=True)
    vals = got["input_values"]
    assert vals.is_cuda and vals.dtype == torch.float32 and vals.shape == (2, 5120) and vals.is_contiguous()
    assert not got["attention_mask"].is_cuda and got["attention_mask"].sum(-1).tolist() == [4801, 2000]
    host = vals.cpu().numpy()
    for row, x in zip(host, (x64.astype(np.float32), WU.as_f32(x16))):      # float64 is cast to f32 on the host; int16 next to float counts as x / 32768
        y, bar = WU.oracle(x)
        check_row(np.concatenate([row, [SENT]]), y, bar, 5120, -1.5, "extractor")
    same = Wav2Vec2FeatureExtractor(padding_value=-1.5)([torch.from_numpy(x64).to(DEV), torch.from_numpy(x16).to(DEV)], sampling_rate=16000,
                                                        pad_to_multiple_of=320)      # clips on the GPU take the device path without the flag
    assert same["input_values"].is_cuda and "attention_mask" not in same and np.array_equal(bits(same["input_values"].cpu().numpy()), bits(host))
    raw = Wav2Vec2FeatureExtractor(device=DEV, normalize_on_device=True, do_normalize=False)([x16])["input_values"]      # int16 alone goes up as int16
    assert raw.is_cuda and np.array_equal(bits(raw.cpu().numpy()[0]), bits(WU.as_f32(x16)))


def test_chained_behind_the_device_resampler():
    from ultravox_amd.frontend import Wav2Vec2FeatureExtractor, resample_device
    x16 = make_clip(48000, "int16", np.random.default_rng(14))
    res, n_out = resample_device([x16], 48000, DEV)
    assert n_out == [16000]
    got = Wav2Vec2FeatureExtractor()(res[0, :n_out[0]], sampling_rate=16000, return_attention_mask=True)
    assert got["input_values"].is_cuda and got["input_values"].shape == (1, 16000) and got["attention_mask"].sum().item() == 16000
    y, bar = WU.oracle(res[0, :n_out[0]].cpu().numpy())               # the yardstick on the resampler's own output, read back
    check_row(np.concatenate([got["input_values"].cpu().numpy()[0], [SENT]]), y, bar, 16000, 0.0, "behind the resampler")


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


def test_local_inference_keeps_a_raw_waveform_clip_on_the_device(monkeypatch):
    """48 kHz and 16 kHz int16 clips through LocalInference(resample_on_device=True) with a device-normalising extractor: neither scipy nor the
    host normaliser is reached.  numpy.ndarray is an immutable type, so its `var` cannot be replaced; the tripwire for the host normaliser is
    numpy.sqrt, which that path calls once per clip right after `var` (`np.sqrt(x.var() + 1e-7)`) and nothing else on the way calls through
    the module attribute.  With both flags off the same calls do reach the tripwires."""
    from fake_tokenizer import FakeChatTokenizer
    from ultravox_amd.frontend import Wav2Vec2FeatureExtractor
    from ultravox_amd.inference import LocalInference, VoiceSample
    from ultravox_amd.processing import UltravoxProcessor, _wav2vec2_frames
    signal = pytest.importorskip("scipy.signal")

    class Reached(Exception):
        pass

    def refuse(*a, **k):
        raise Reached()

    rng = np.random.default_rng(15)
    clip48, clip16 = make_clip(48000, "int16", rng), make_clip(16000, "int16", rng)
    want16 = WU.oracle(WU.as_f32(clip16))
    tok = FakeChatTokenizer()
    proc = UltravoxProcessor(Wav2Vec2FeatureExtractor(normalize_on_device=True, device=DEV), tokenizer=tok)
    plain = UltravoxProcessor(Wav2Vec2FeatureExtractor(), tokenizer=tok)
    model = GpuStubModel(tok)
    inf = LocalInference(model, proc, tok, dtype=torch.float32, resample_on_device=True)
    with monkeypatch.context() as m:
        m.setattr(signal, "resample_poly", refuse)
        m.setattr(np, "sqrt", refuse)
        for clip, rate in ((clip48, 48000), (clip16, 16000)):
            out = inf.infer(VoiceSample.from_prompt_and_raw("<|audio|>", clip, rate), max_tokens=3)
            assert out.output_tokens == 3
        for clip, rate in ((clip48, 48000), (clip16, 16000)):          # both flags off: the same calls reach scipy and the host normaliser
            with pytest.raises(Reached):
                LocalInference(GpuStubModel(tok), plain, tok, dtype=torch.float32).infer(VoiceSample.from_prompt_and_raw("<|audio|>", clip, rate),
                                                                                         max_tokens=3)
    for kw in model.calls:
        assert kw["audio_values"].is_cuda and kw["audio_values"].dtype == torch.float32 and kw["audio_values"].shape == (1, 16000)
        assert kw["audio_lens"].tolist() == [_wav2vec2_frames(16000)] == [49] and kw["audio_token_len"].tolist() == [7]
    check_row(np.concatenate([model.calls[1]["audio_values"].cpu().numpy()[0], [SENT]]), *want16, 16000, 0.0, "16 kHz int16 through LocalInference")


# ---------------------------------------------------------------- the real tower (the smallest config tests/test_wav2vec2_gpu.py builds, restated)
W2V_SMALL = {"model_type": "wav2vec2", "hidden_size": 128, "num_hidden_layers": 2, "num_attention_heads": 2, "intermediate_size": 256,
             "conv_dim": [64] * 7, "num_conv_pos_embeddings": 16, "num_conv_pos_embedding_groups": 4}
TEXT_SMALL = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2,
                  vocab_size=512, eos_token_id=2)


def test_the_tower_moves_no_further_than_under_one_rounding_step_of_its_input():
    """Encoder output from device-normalised values against output from host-normalised values of the same clips (f32 tower).  There is no derivable
    bound for this; the scale is measured on the reference side: how far the output moves when every host-normalised input element is moved by
    one f32 rounding step (up or down, seeded).  The device path has to stay within 4x that distance: its input is within about one rounding step
    per element of the exact value and so is numpy's (factor 2); another factor of 2 is for accumulation order inside the tower.  Both distances
    are recorded (profiles/wave_norm_parity.txt holds those of the run that added the kernel)."""
    from parity_util import record
    from ultravox_amd.config import UltravoxConfig
    from ultravox_amd.frontend import Wav2Vec2FeatureExtractor
    from ultravox_amd.model import UltravoxModel
    from ultravox_amd.weights import random_state_dict
    cfg = UltravoxConfig(audio_config=W2V_SMALL, text_config=TEXT_SMALL, hidden_size=256, projector_ln_mid=True)
    model = UltravoxModel(cfg, state_dict=random_state_dict(cfg, seed=5), device=DEV, dtype=torch.float32)
    rng = np.random.default_rng(16)
    clips = [(0.1 * rng.standard_normal(9000) + 0.01).astype(np.float32) for _ in range(3)]      # 9000 samples -> 27 frames
    host = Wav2Vec2FeatureExtractor()(clips)["input_values"]
    dev = Wav2Vec2FeatureExtractor(device=DEV, normalize_on_device=True)(clips)["input_values"]
    assert not host.is_cuda and dev.is_cuda and host.shape == dev.shape == (3, 9000)
    h = host.numpy()
    stepped = torch.from_numpy(np.nextafter(h, np.where(rng.integers(0, 2, h.shape) == 1, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)))
    assert stepped.dtype == torch.float32 and bool((stepped != host).all())
    t_host = model.audio_tower_forward(host.to(DEV), None).double()
    t_step = model.audio_tower_forward(stepped.to(DEV), None).double()
    t_dev = model.audio_tower_forward(dev, None).double()
    d_step, d_dev = (t_step - t_host).norm().item(), (t_dev - t_host).norm().item()
    record("wave_norm_tower_parity", {"one_rounding_step_of_the_host_input": d_step, "device_normalised_input": d_dev, "output_norm": t_host.norm().item(),
                                      "input_elements_that_differ": int((dev.cpu() != host).sum()), "input_elements": host.numel()})
    print(f"tower output moves by {d_step:.6e} under one rounding step of the host-normalised input, by {d_dev:.6e} under the device-normalised input")
    assert d_step > 0.0
    assert d_dev <= 4.0 * d_step, (d_dev, d_step)
