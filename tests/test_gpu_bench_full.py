"""bench.py without --full measures the headline and nothing else; --full adds the comparison GEMM mode, the rooflines, the
step breakdown, the CPU baseline and (ppi) the host time and the replayed step."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DETAIL_PREFIX = "BENCH_DETAIL "


def _bench(extra):
    """-> the complete record of one single-rank run (its BENCH_DETAIL line); the last line is the short one"""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TFGNN_BENCH_SINGLE_DEVICE"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", *extra], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert lines[-1].startswith("{") and len(lines[-1]) < 4096
    detail = [l[len(DETAIL_PREFIX):] for l in lines if l.startswith(DETAIL_PREFIX)]
    assert len(detail) == 1, res.stdout[-2000:]
    return json.loads(detail[0])


def test_plain_run_times_the_headline_only_and_full_adds_the_rest():
    plain = _bench(["--workload", "tiny"])
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["config"]["products_per_step"]["gather"] + plain["config"]["products_per_step"]["gather_sp"] > 0
    for k in ("roofline", "cpu_baseline", "step_breakdown", "other_configs"):
        assert k not in plain, k
    assert "alt_gemm_mode" not in plain["config"]

    full = _bench(["--workload", "tiny", "--full", "--cpu-baseline-seconds", "1"])
    assert full["steps"] == 3 and full["metric"] == plain["metric"] and full["unit"] == plain["unit"]
    assert full["roofline"]["bound"] in ("hbm", "mfma") and 0 < full["roofline"]["frac"] <= 1.0
    assert full["cpu_baseline"]["value"] > 0 and full["step_breakdown"]["top"]
    assert full["config"]["alt_gemm_mode"]["gemm_mode_name"] == "bf16x3" and full["config"]["alt_gemm_mode"]["value"] > 0
    assert "other_configs" not in full  # only the rmat30k headline times the other workloads


def test_ppi_replay_and_host_time_come_with_full():
    plain = _bench(["--workload", "ppi"])
    assert plain["value"] > 0 and plain["graphs_per_s"] > 0 and plain["batches"] == 8
    for k in ("host_ms_per_step", "eager", "replay_only", "replay_static_batch"):
        assert k not in plain, k

    full = _bench(["--workload", "ppi", "--full"])
    assert full["host_ms_per_step"] > 0 and full["eager"]["device_ms_one_step_alone"] > 0
    assert full["replay_only"]["ms_per_step"] > 0 and full["replay_static_batch"]["ms_per_step"] > 0
    assert full["bound"] in ("host", "device") and full["config"]["loss"] > 0
