"""bench.py as it is run for every change: a plain run times --steps steps and prints the headline line alone, --dump-outputs
writes what the timed path returned in its last step (the same on a second run with the same arguments), and --full adds the
legs that take runs of their own.  Config 2 keeps the runs short."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2", "--steps", "3", "--warmup", "1", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_ones_outputs(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    out = _bench("--dump-outputs", str(a))
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] == out["value"] > 0
    assert not {"cpu_baseline", "variants", "secondary"} & set(out), sorted(out)
    _bench("--dump-outputs", str(b))
    got = {}
    for name in ("top_scores", "top_indices", "alpha"):
        x, y = np.load(a / f"{name}.npy"), np.load(b / f"{name}.npy")
        assert x.dtype == np.float64 and x.shape == y.shape and np.all(np.isfinite(x)), name
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=0, err_msg=name)
        got[name] = x
    assert got["top_scores"].shape == (100,) and got["alpha"].shape == (1024,)
    assert np.array_equal(got["top_indices"], np.load(b / "top_indices.npy"))
    assert got["top_scores"][0] == out["top1"]["score"] and got["top_indices"][0] == out["top1"]["index"]


@pytest.mark.gpu
def test_full_run_adds_the_variants():
    out = _bench("--full", "--no-cpu-baseline")
    assert out["steps"] == 3 and out["value"] > 0
    assert out["variants"]["scores_to_host_ms"] > 0 and "cpu_baseline" not in out
