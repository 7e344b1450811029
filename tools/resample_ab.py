"""A/B of the device resampler (uvx_resample_poly) against the host path of LocalInference._dataproc, on the GPU; writes the table of
profiles/resample_ab.txt.

  python tools/resample_ab.py OUT.txt

For one int16 clip of 5 s and of 30 s at 48 000, 44 100 and 8 000 Hz (seeded noise), from the numpy array to the log-mel features on the device:
(a) host: x / 32768 (f32) -> scipy.signal.resample_poly -> torch.from_numpy -> WhisperFeatureExtractor.__call__ as UltravoxProcessor calls it
    (builds the padded batch on the host, uploads it at 16 kHz, runs uvx_logmel);
(b) device: frontend.resample_device (uploads the int16 at its native rate, uvx_resample_poly into the padded batch) -> logmel_device.
Host clock from the numpy array to the end of a torch.cuda.synchronize(), the two paths alternating, REPS times each after WARM untimed rounds;
median [min .. max].  The kernel alone: device events around blocks of 20 launches on resident buffers, 5 blocks, per-launch mean.
The last column is the largest difference between the two paths' log-mel features (they differ by the resamplers' f32 rounding only).
"""
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS, WARM = 25, 5


def spread(v, w=8, p=3):
    return f"{statistics.median(v):{w}.{p}f} [{min(v):{w}.{p}f} .. {max(v):{w}.{p}f}]"


def main():
    from scipy.signal import resample_poly
    from ultravox_amd import ops
    from ultravox_amd.frontend import WhisperFeatureExtractor, resample_device
    out_path = sys.argv[1]
    dev = "cuda"
    fe = WhisperFeatureExtractor(80, device=dev)
    rng = np.random.default_rng(0)
    lines = [f"# uvx_resample_poly against the host resampler (tools/resample_ab.py; MI355X - torch names the device '{torch.cuda.get_device_name(0)}' -, one process, one call; "
             f"scipy {__import__('scipy').__version__}, {torch.get_num_threads()} torch threads)",
             f"ms from the int16 numpy clip to the log-mel on the device, median [min .. max] of {REPS} alternating repeats; kernel alone: us per launch, "
             "5 blocks of 20",
             f"{'rate':>6} {'clip':>5} {'(a) host: scipy + upload + logmel':>36} {'(b) device: upload + resample + logmel':>40} {'a / b':>6} "
             f"{'uvx_resample_poly alone, us':>34} {'max |mel a - b|':>16}"]
    for seconds in (5, 30):
        for rate in (48000, 44100, 8000):
            pcm = (rng.standard_normal(seconds * rate) * 3000).clip(-32768, 32767).astype(np.int16)
            g = math.gcd(16000, rate)
            up, down = 16000 // g, rate // g

            def host():
                audio = pcm / np.float32(32768.0)
                audio = resample_poly(audio, up, down, axis=-1).astype(audio.dtype)
                audio_input = torch.from_numpy(np.ascontiguousarray(audio))           # what _dataproc hands to the processor,
                feats = fe([audio_input.numpy()], sampling_rate=16000, padding="longest", pad_to_multiple_of=160,      # and the processor's call
                           truncation=False, return_attention_mask=True)
                return feats["input_features"]

            def device():
                batch, _ = resample_device([pcm], rate, dev, pad_to_multiple_of=160)
                return fe.logmel_device(batch)

            paths = {"a": host, "b": device}
            ms = {k: [] for k in paths}
            for r in range(WARM + REPS):
                for k, f in paths.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    torch.cuda.synchronize()
                    if r >= WARM:
                        ms[k].append((time.perf_counter() - t0) * 1e3)
            diff = float((host() - device()).abs().max())
            # the kernel alone, on resident buffers
            x = torch.from_numpy(pcm).to(dev)
            off = torch.zeros(1, dtype=torch.int64, device=dev)
            n_in = torch.tensor([len(pcm)], dtype=torch.int32, device=dev)
            width = -(-ops.resample_n_out(len(pcm), up, down) // 160) * 160
            out = torch.empty(1, width, device=dev, dtype=torch.float32)
            call = lambda: ops.resample_poly(x, off, n_in, up, down, max_n_in=len(pcm), out=out, out_width=width)
            for _ in range(10):
                call()
            us = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(20):
                    call()
                b.record()
                torch.cuda.synchronize()
                us.append(a.elapsed_time(b) * 1e3 / 20)
            lines.append(f"{rate:>6} {seconds:>4}s {spread(ms['a']):>36} {spread(ms['b']):>40} {statistics.median(ms['a']) / statistics.median(ms['b']):5.1f}x "
                         f"{spread(us, 7, 1):>34} {diff:16.3e}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
