"""`python bench.py --gpus 1 --steps K --warmup W` on the GPU: the plain run reports the K timed steps
(ms_per_step) and leaves every --full leg null; --dump-outputs writes the last timed step's loss, flat gradient and flat
parameters, and two runs with the same arguments start from the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("host_ms_per_step", "roofline", "end_to_end", "batch32", "predict", "dedup", "other_configs", "ref_headline",
             "cpu_baseline")


def _bench(out_dir, steps=3, warmup=1):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    outs = {n: np.load(os.path.join(out_dir, n + ".npy")) for n in ("loss", "grad", "params")}
    return line, outs


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    line, outs = _bench(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "pairs/s" and line["dtype"] == "f32"
    assert line["higher_is_better"] is True
    for k in FULL_ONLY:
        assert line[k] is None, k
    assert all(a.dtype == np.float32 for a in outs.values())
    assert outs["loss"].shape == (1,) and abs(float(outs["loss"][0]) - line["config"]["loss"]) <= 1e-5
    assert outs["grad"].ndim == 1 and outs["grad"].shape == outs["params"].shape
    assert all(np.isfinite(a).all() for a in outs.values())
    assert np.abs(outs["grad"]).max() > 0

    # same arguments, same inputs: loss and gradient agree up to float32 summation order (the embedding gradient sums in LDS
    # with atomics).  Adam moves an entry by up to alpha = 1e-3 per step whatever the size of its gradient, so an entry whose
    # gradient is rounding noise (analytically zero) may move either way: the parameters are held to that bound.
    _, again = _bench(tmp_path / "b")
    for n in ("loss", "grad"):
        a, b = outs[n], again[n]
        assert np.abs(a - b).max() <= 1e-4 * max(float(np.abs(a).max()), 1e-6), n
    assert np.abs(outs["params"] - again["params"]).max() <= 2e-3 * (3 + 1)
