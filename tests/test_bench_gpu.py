"""`bench.py` end to end on the GPU at plumbing size (`--workload c1`): a plain run prints the headline line without the --full
extras, and `--dump-outputs` writes what its last timed step computed - identically in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "c1", *extra], env=env, capture_output=True, text=True, timeout=600)      # (a later --workload wins)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_reproducibly(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    out = run_bench("--dump-outputs", str(a))
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "audio-seconds/sec" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert abs(out["value"] - 4.0 / (out["ms_per_step"] * 1e-3)) < 1e-6 * out["value"]      # 1 clip x 4 s per step
    assert not {"roofline", "cpu_baseline", "parity"} & set(out)                              # --full only
    names = sorted(f[:-4] for f in os.listdir(a))
    assert "loss" in names and any(n.startswith("param.multi_modal_projector.") for n in names) and any(n.startswith("grad.") for n in names)
    assert sum(os.path.getsize(a / (n + ".npy")) for n in names) < 64e6
    loss = np.load(a / "loss.npy")
    assert loss.dtype == np.float32 and abs(float(loss) - out["loss"]) < 1e-6 * abs(out["loss"])
    run_bench("--dump-outputs", str(b))
    for n in names:
        x, y = np.load(a / (n + ".npy")), np.load(b / (n + ".npy"))
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all() and np.array_equal(x, y), n


@pytest.mark.gpu
def test_inference_workload_dumps_the_generated_tokens(tmp_path):
    """`--workload c4t --dump-outputs DIR`: the last timed generate() call's token ids (prompt + new tokens), exact as float64."""
    out = run_bench("--workload", "c4t", "--dump-outputs", str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["tokens.npy"]
    tok = np.load(tmp_path / "tokens.npy")
    assert tok.dtype == np.float64 and list(tok.shape) == out["output_shape"] and tok.shape[1] == out["config"]["prompt_len"] + 8
    assert np.array_equal(tok, np.round(tok)) and tok.min() >= 0
