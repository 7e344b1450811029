"""The device normaliser of raw-waveform clips (uvx_wave_norm) next to the host path of frontend.Wav2Vec2FeatureExtractor, on the GPU; writes the
table of profiles/wave_norm.txt.

  python tools/wave_norm_ab.py OUT.txt

For 1 and 8 f32 clips of 30 s at 16 kHz (seeded noise with a small offset), from the numpy clips to `input_values` on the device:
(a) host: Wav2Vec2FeatureExtractor() - numpy mean and variance per clip, the padded batch built on the host - and the upload of that batch;
(b) device: Wav2Vec2FeatureExtractor(normalize_on_device=True) - one upload of the clips, one uvx_wave_norm call (its workspace allocated).
Host clock from the numpy clips to the end of a torch.cuda.synchronize(), the two paths alternating, REPS times each after WARM untimed rounds;
median [min .. max].  The two launches alone: device events around blocks of 20 calls on resident buffers, 5 blocks, per-call mean.
The last column is the largest difference between the two paths' outputs (numpy's f32 rounding against float64 sums rounded once).
"""
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
    from ultravox_amd import ops
    from ultravox_amd.frontend import Wav2Vec2FeatureExtractor
    out_path = sys.argv[1]
    dev = "cuda"
    fe_host, fe_dev = Wav2Vec2FeatureExtractor(), Wav2Vec2FeatureExtractor(device=dev, normalize_on_device=True)
    rng = np.random.default_rng(0)
    lines = [f"# uvx_wave_norm next to the host normaliser (tools/wave_norm_ab.py; MI355X - torch names the device '{torch.cuda.get_device_name(0)}' -, one process, "
             f"one call; numpy {np.__version__}, {torch.get_num_threads()} torch threads)",
             f"ms from the f32 numpy clips (30 s at 16 kHz each) to input_values on the device, median [min .. max] of {REPS} alternating repeats; the two launches "
             "alone: us per call, 5 blocks of 20",
             f"{'clips':>6} {'(a) host: numpy + upload':>36} {'(b) device: upload + uvx_wave_norm':>40} {'a / b':>6} {'the two launches alone, us':>34} {'max |a - b|':>12}"]
    for B in (1, 8):
        clips = [(0.1 * rng.standard_normal(30 * 16000) + 0.01).astype(np.float32) for _ in range(B)]
        paths = {"a": lambda: fe_host(clips, sampling_rate=16000)["input_values"].to(dev), "b": lambda: fe_dev(clips, sampling_rate=16000)["input_values"]}
        ms = {k: [] for k in paths}
        for r in range(WARM + REPS):
            for k, f in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                if r >= WARM:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
        diff = float((paths["a"]() - paths["b"]()).abs().max())
        # the two launches alone, on resident buffers (the workspace comes from torch's caching allocator: no device allocation in the loop)
        n = len(clips[0])
        x = torch.from_numpy(np.concatenate(clips)).to(dev)
        off = torch.arange(B, dtype=torch.int64, device=dev) * n
        n_dev = torch.full((B,), n, dtype=torch.int32, device=dev)
        out = torch.empty(B, n, device=dev, dtype=torch.float32)
        call = lambda: ops.wave_norm(x, off, n_dev, max_n=n, out=out, out_width=n)
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
        lines.append(f"{B:>6} {spread(ms['a']):>36} {spread(ms['b']):>40} {statistics.median(ms['a']) / statistics.median(ms['b']):5.1f}x "
                     f"{spread(us, 7, 1):>34} {diff:12.3e}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
