"""Range-level in-stream repair of the grouped weight-gradient product (include/tfgnn.h tfgnn_sp_gemm_tn_grouped under
tfgnn_sp_guard_repair), the part that needs no GPU: the workspace query is exported, declared and bound, the ABI number did not
move, the query grows by exactly the tail of the trip words while the environment arms the repair, and the arithmetic the repair
kernel performs - modelled on the CPU - gets the operands of the GPU test right with room to spare."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests import tn_repair_grouped_reference as grp
from tests.test_gpu_gemm_sp_tn_edges import mag, ref

ROOT = Path(__file__).resolve().parent.parent
NEW = "tfgnn_sp_gemm_tn_grouped_workspace_bytes"
SHAPES = [(128, 128, 128, 64, 9), (640, 128, 640, 320, 3), (512, 512, 512, 256, 512)]  # M, N, a_total_cols, a_scale_block, ranges
GPU_BOUND = 2e-6  # tests/test_gpu_tn_repair.py BOUND


def _tail_bytes():
    text = (ROOT / "tf2_gnn_amd" / "csrc" / "tn_repair.hpp").read_text()
    ranges = int(re.search(r"constexpr int kTnRepairGroupedMaxRanges = (\d+);", text).group(1))
    assert re.search(r"constexpr size_t kTnRepairGroupedTailBytes =", text)
    return ranges, ((ranges + 1) * 4 + 255) // 256 * 256


def test_the_query_is_exported_declared_and_bound_and_the_abi_stays_5():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert hasattr(lib, NEW)
    assert re.search(r"\bsize_t\s+%s\s*\(" % NEW, header)
    assert NEW in {row[0] for row in _lib._SIGNATURES} and NEW in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5
    assert "#define TFGNN_ABI_VERSION 5" in text


def _sizes_in_child(env_value):
    code = (
        "from tf2_gnn_amd import _lib\n"
        "lib = _lib.load()\n"
        "print('STATE', lib.tfgnn_sp_guard_repair(-1))\n"
        f"for s in {SHAPES!r}:\n"
        f"    print('BYTES', lib.{NEW}(*s))\n"
    )
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("TFGNN_GUARD_REPAIR", None)
    if env_value is not None:
        env["TFGNN_GUARD_REPAIR"] = env_value
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    lines = res.stdout.splitlines()
    state = [int(l.split()[1]) for l in lines if l.startswith("STATE")]
    sizes = [int(l.split()[1]) for l in lines if l.startswith("BYTES")]
    assert len(state) == 1 and len(sizes) == len(SHAPES)
    return state[0], sizes


def test_the_query_is_the_documented_size_and_grows_by_exactly_the_tail_while_armed():
    """The state is read from TFGNN_GUARD_REPAIR once per process (hence child processes); the query touches no device.
    Disarmed: roundup256(4 * 512 * nblk) + num_splits * roundup(M, 128) * N * 4, as include/tfgnn.h documents."""
    ranges, tail = _tail_bytes()
    assert ranges == 512 and tail == 2304 and tail % 256 == 0
    off_state, off = _sizes_in_child(None)
    zero_state, zero = _sizes_in_child("0")
    on_state, on = _sizes_in_child("1")
    assert (off_state, zero_state, on_state) == (0, 0, 1)
    documented = [(4 * 512 * (cols // sb) + 255) // 256 * 256 + s * ((M + 127) // 128 * 128) * N * 4 for M, N, cols, sb, s in SHAPES]
    assert off == documented and zero == documented
    assert on == [d + tail for d in documented]


def test_the_cuts_of_the_model_are_those_of_the_row_groups():
    """``ranges_of`` against what the issue's operands are built around: 9 K ranges, group 6 cut into 1376 + 1376 + 1348 rows
    with the deficient rows (local rows >= 2752) in the last one only, group 4 into 1024 + 993."""
    off = grp.offsets()
    rs = grp.ranges_of(off)
    assert sum(len(r) for r in rs) == 9
    assert [n for _, n in rs[6]] == [1376, 1376, 1348] and rs[6][2][0] == off[6] + 2752
    assert [n for _, n in rs[4]] == [1024, 993] and [n for _, n in rs[3]] == [2016] and rs[0] == []
    assert all(n <= grp.MAX_CHUNK for r in rs for _, n in r)


@pytest.mark.parametrize("M,N,sb", grp.SHAPES, ids=[f"m{s[0]}_sb{s[2]}" for s in grp.SHAPES])
def test_cpu_model_of_the_repaired_grouped_product_meets_half_the_gpu_bound(M, N, sb):
    """SP16 decode (power-of-two scales per (row, block)), fp32 accumulation in ascending k per K range, slabs added in range
    order - on the GPU test's own operands, every range taken as repaired: max error against fp64 relative to sum |a||b| must
    stay under half the GPU bound of 2e-6, so the inputs are ones the arithmetic alone gets right.
    Measured (worst group): M = 128, sb = 64: 4.2e-7 (group 3, every range of it repaired); M = 256, sb = 128: 3.8e-7; the
    one-row group, where only the SP16 decode rounds: 2.8e-7."""
    a, b, off = grp.tripping_case(M, N, sb, 40 + M)
    got = grp.repaired_model(a, b, sb, off).double()
    worst = 0.0
    for gi in range(len(off) - 1):
        sl = slice(off[gi], off[gi + 1])
        r, m = ref(a[sl], b[sl]), mag(a[sl], b[sl])
        zero = m == 0
        assert torch.equal(got[gi][zero], r[zero]), gi
        if bool((~zero).any()):
            e = float(((got[gi] - r).abs()[~zero] / m[~zero]).max())
            print(f"group {gi} ({off[gi + 1] - off[gi]} rows): model err / sum |a||b| = {e:.3e}")
            worst = max(worst, e)
    print(f"M={M} sb={sb}: worst {worst:.3e}")
    assert worst <= GPU_BOUND / 2, worst
