"""The device augmentations (ultravox_amd.aug: uvx_aug_gain, uvx_aug_noise, uvx_aug_iir) next to the host definitions the reference runs
(numpy / scipy, as restated in tests/aug_util.py), on the GPU; writes the table of profiles/aug_ab.txt.

  python tools/aug_ab.py OUT.txt

For 8 int16 clips of 30 s at 16 kHz (seeded noise), for each of `random_gain`, `random_pink_noise`, `telephone_bandpass` and the chain of the three:
(a) host: the definition on the clip as float32 (x / 32768), clip by clip in float64 where numpy / scipy go there; host clock; the result stays on
    the host (the reference's next stage reads it there), so no upload is counted for it;
(b) device: `apply_batch` over the numpy int16 clips - the upload of the PCM, one launch sequence per stage, the workspace allocated - under device
    events from before the upload to after the last kernel (the host draws and the packing of the clips lie inside the window).
WARM untimed rounds, then REPS timed ones, the two paths alternating; median [min .. max].  The kernels alone: device events around blocks of
10 calls of the ops wrapper on resident buffers, 5 blocks, per-call mean.  There is no pass / fail threshold; the figure that matters is the chain's
(b) against the 78 ms training step that consumes these 8 clips.
"""
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPS, WARM, B, SECONDS = 15, 3, 8, 30


def spread(v, w=8, p=3):
    return f"{statistics.median(v):{w}.{p}f} [{min(v):{w}.{p}f} .. {max(v):{w}.{p}f}]"


def device_ms(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main():
    import aug_util as AU
    from ultravox_amd import ops
    from ultravox_amd.aug import AugRegistry
    from ultravox_amd.frontend import _pack_clips
    out_path = sys.argv[1]
    dev = "cuda"
    rng = np.random.default_rng(0)
    clips = [np.clip(3000.0 * rng.standard_normal(SECONDS * 16000), -32768, 32767).astype(np.int16) for _ in range(B)]
    as_f32 = [AU.as_f32(x) for x in clips]
    make = lambda name, **kw: AugRegistry.create_augmentation(AugRegistry.get_config(name, kw) if kw else AugRegistry.get_config(name))
    stages = {"random_gain": make("random_gain"), "random_pink_noise": make("random_pink_noise", seed=1), "telephone_bandpass": make("telephone_bandpass")}
    host = {"random_gain": lambda x: AU.host_gain(x, np.random.uniform(-24.0, 15.0)),
            "random_pink_noise": lambda x: AU.host_coloured_noise(x, "pink", np.random.uniform(0.0, 20.0)),
            "telephone_bandpass": lambda x: AU.host_bandpass(x)}

    def host_chain(x):
        for f in host.values():
            x = f(x)
        return x

    rows = [(name, host[name], stages[name]) for name in stages]
    rows.append(("chain of the three", host_chain, AugRegistry.create_parent_augmentation(list(stages.values()))))
    lines = [f"# the device augmentations next to the host definitions (tools/aug_ab.py; MI355X - torch names the device '{torch.cuda.get_device_name(0)}' -, one "
             f"process; numpy {np.__version__}, scipy {__import__('scipy').__version__})",
             f"ms for {B} clips of {SECONDS} s at 16 kHz, median [min .. max] of {REPS} alternating repeats after {WARM} warm-up rounds.  (a) host clock, one thread of "
             "numpy / scipy, float32 clips in, result on the host; (b) device events, int16 numpy clips in (upload included), result on the device",
             f"{'augmentation':>20} {'(a) host definition':>36} {'(b) device, upload included':>36} {'a / b':>7}"]
    for name, host_f, dev_aug in rows:
        ms = {"a": [], "b": []}
        for r in range(WARM + REPS):
            random.seed(r)
            np.random.seed(r)
            t0 = time.perf_counter()
            for x in as_f32:
                host_f(x)
            ta = (time.perf_counter() - t0) * 1e3
            tb = device_ms(lambda: dev_aug.apply_batch(clips))
            if r >= WARM:
                ms["a"].append(ta)
                ms["b"].append(tb)
        lines.append(f"{name:>20} {spread(ms['a']):>36} {spread(ms['b']):>36} {statistics.median(ms['a']) / statistics.median(ms['b']):6.1f}x")

    # the kernels alone, on resident buffers (workspaces come from torch's caching allocator: no device allocation in the loop)
    pcm, row_offset, n, lens = _pack_clips(clips, dev, "aug_ab")
    out = torch.empty(B, max(lens), device=dev, dtype=torch.float32)
    bp = stages["telephone_bandpass"]
    bd, ad = torch.from_numpy(bp.b).to(dev), torch.from_numpy(bp.a).to(dev)
    gain = torch.full((B,), 0.5, device=dev, dtype=torch.float32)
    ratio = torch.full((B,), 0.1, device=dev, dtype=torch.float64)
    calls = {"uvx_aug_gain": lambda: ops.aug_gain(pcm, row_offset, n, gain, max_n=max(lens), out=out),
             "uvx_aug_noise, white": lambda: ops.aug_noise(pcm, row_offset, n, ratio, colour="white", seed=1, offset=0, max_n=max(lens), out=out),
             "uvx_aug_noise, pink": lambda: ops.aug_noise(pcm, row_offset, n, ratio, colour="pink", seed=1, offset=0, max_n=max(lens), out=out),
             f"uvx_aug_iir, order 10, warm {bp.warm}": lambda: ops.aug_iir(pcm, row_offset, n, bd, ad, bp.warm, max_n=max(lens), out=out)}
    lines.append("")
    lines.append(f"the launches alone on resident int16 buffers ({B} x {max(lens)} samples), us per call, 5 blocks of 10: median [min .. max]")
    for name, call in calls.items():
        for _ in range(3):
            call()
        us = [device_ms(lambda: [call() for _ in range(10)]) * 1e3 / 10 for _ in range(5)]
        lines.append(f"{name:>40} {spread(us, 9, 1)}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
