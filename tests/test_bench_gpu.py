"""GPU: `bench.py --dump-outputs DIR` writes what the last timed step computed, and two runs with the same arguments compute the same step
(seeded inputs, masks and initialisation), so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loss", "grad_norm", "params")


def _run(*args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--resolution", "32", "--backbone", "swin_t"] + list(args)
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _bench(out_dir):
    d = _run("--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-kernel-timing", "--no-sweep", "--dump-outputs", str(out_dir))
    return d, {n: np.load(os.path.join(out_dir, n + ".npy")) for n in NAMES}


def test_bench_plain_run_is_lean():
    """without --full the line carries the headline figure of the timed steps and none of the extra measurements"""
    d = _run("--steps", "2", "--warmup", "1")
    assert d["steps"] == 2 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["unit"] == "grids/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert "roofline" not in d and "cpu_baseline" not in d
    assert list(d["config"]["sweep"]) == ["%d_grids_per_gpu" % d["config"]["grids_per_gpu"]]
    assert not {"fp32_mode", "other_backbones", "timed_kernel_ms_per_step"} & set(d["config"])


def test_bench_dump_outputs(tmp_path):
    d, a = _bench(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in NAMES)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / (n + ".npy")) for n in NAMES) <= 64 << 20
    assert a["loss"].shape == (3,) and abs(a["loss"][0] - d["config"]["final_loss"]) < 1e-5
    assert a["grad_norm"].shape == (1,) and a["grad_norm"][0] > 0
    assert a["params"].ndim == 1 and a["params"].size > 0

    _, b = _bench(tmp_path / "b")
    # same inputs, same step: the fp32 atomic reductions of the weight gradients round in a different order from run to run, and the training
    # steps carry that into the state of the last one, so two runs agree within the bf16 unit roundoff (2^-8) of the computation, not bit for bit
    tol = 2.0 ** -8
    np.testing.assert_allclose(b["loss"], a["loss"], rtol=tol)
    np.testing.assert_allclose(b["grad_norm"], a["grad_norm"], rtol=tol)
    assert np.linalg.norm(b["params"] - a["params"]) <= tol * np.linalg.norm(a["params"])
