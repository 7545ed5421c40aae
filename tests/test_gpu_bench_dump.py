"""bench.py --dump-outputs: what the last timed step computed (output representations, weight gradients) as .npy files -
the same from run to run of the same arguments, so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, extra=()):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TFGNN_BENCH_SINGLE_DEVICE"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
                          "--no-alt-mode", "--no-roofline", "--dump-outputs", str(out_dir), *extra], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    return json.loads([l for l in res.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.parametrize("workload", ["tiny", "qm9-tiny"])
def test_dumped_outputs_are_the_same_from_run_to_run(tmp_path, workload):
    """Two runs (each with its own settle loop, whose length depends on timing) dump the same arrays: the inputs, weights
    and dropout masks of the last timed step do not depend on anything but the arguments."""
    first = _bench(tmp_path / "a", ["--workload", workload])
    _bench(tmp_path / "b", ["--workload", workload])
    assert first["steps"] == 3 and first["ms_per_step"] > 0
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert "node_representations.npy" in names and sum(n.startswith("grad_") for n in names) >= 4
    if workload == "qm9-tiny":
        assert "graph_representations.npy" in names
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= 64 * 10**6
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), n
        # the same inputs through the same kernels; a different dropout mask or batch would differ by O(|a|)
        assert np.allclose(a, b, rtol=1e-5, atol=1e-6 * float(np.abs(a).max())), n
