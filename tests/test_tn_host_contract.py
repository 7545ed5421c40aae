"""The host contract of the split-operand weight-gradient (TN) product, the part that needs no GPU: what the three workspace
queries return and what the three entry points answer to arguments they reject (return code and the exact text of
tfgnn_last_error), with the in-stream repair switch off and on.  tests/golden/tn_host_contract_parent.json is what
``contract()`` below returned at the commit before the plain and the grouped product were given one workspace layout and one
launch path (csrc/gemm_sp.hip): Python allocates from these sizes, include/tfgnn.h documents them, and callers match the texts.

Every call here returns before the library touches a device, so the operand and table pointers are arbitrary aligned non-null
values.  The repair switch is read from TFGNN_GUARD_REPAIR once per process, hence one child process per state (as
tests/test_tn_repair_host.py does)."""
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "tn_host_contract_parent.json"

# (M, N, K, a_total_cols, a_scale_block); the last three are unsupported and give 0
PLAIN_SIZES = [(256, 128, 2017, 256, 64), (128, 128, 131088, 128, 128), (640, 320, 6053, 640, 320), (144, 128, 17, 160, 32),
               (1280, 320, 30000, 1280, 320), (256, 128, 1032193, 256, 64), (256, 96, 2017, 256, 64), (0, 128, 2017, 256, 64),
               (256, 128, 2017, 256, 0)]
# (M, N, a_total_cols, a_scale_block, num_splits)
GROUPED_SIZES = [(128, 128, 128, 64, 9), (640, 128, 640, 320, 3), (512, 512, 512, 256, 512), (256, 128, 256, 64, 0)]

A, INV_A, B, INV_B, C, OFFSETS, TABLE, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x100000
BIG = 1 << 40


def plain_args(**over):
    """A valid call of tfgnn_sp_gemm_tn / _wide: [2017, 256] (blocks of 64 columns) ^T [2017, 128]"""
    a = dict(M=256, N=128, K=2017, A=A, lda=1024, a0=0, inv_a=INV_A, a_total=256, sb=64, B=B, ldb=512, b0=0, inv_b=INV_B, C=C,
             group_rows=256, stride_group=0, stride_row=128, stride_col=1, accumulate=0, ws=WS, ws_bytes=BIG, stream=None)
    a.update(over)
    return tuple(a.values())


def grouped_args(**over):
    """A valid call of tfgnn_sp_gemm_tn_grouped: seven groups in nine K ranges, [R, 128] (blocks of 64 columns) ^T [R, 128]"""
    a = dict(M=128, N=128, A=A, lda=512, inv_a=INV_A, a_total=128, sb=64, B=B, ldb=512, inv_b=INV_B, groups=7, offsets=OFFSETS,
             splits=9, table=TABLE, C=C, c_group_stride=128 * 128, stride_row=128, stride_col=1, ws=WS, ws_bytes=BIG, stream=None)
    a.update(over)
    return tuple(a.values())


REJECTIONS = [
    ("tn null operand", "tfgnn_sp_gemm_tn", plain_args(A=None)),
    ("tn N=96", "tfgnn_sp_gemm_tn", plain_args(N=96)),
    ("tn M=24", "tfgnn_sp_gemm_tn", plain_args(M=24, group_rows=24)),
    ("tn a_scale_block=16", "tfgnn_sp_gemm_tn", plain_args(sb=16)),
    ("tn lda=1000", "tfgnn_sp_gemm_tn", plain_args(lda=1000)),
    ("tn first column 8", "tfgnn_sp_gemm_tn", plain_args(M=128, a0=8, group_rows=128)),
    ("tn group_rows=0", "tfgnn_sp_gemm_tn", plain_args(group_rows=0)),
    ("tn 32-column blocks, first column 16", "tfgnn_sp_gemm_tn", plain_args(M=128, a0=16, sb=32, group_rows=128)),
    ("tn workspace of 1024 bytes", "tfgnn_sp_gemm_tn", plain_args(ws_bytes=1024)),
    ("tn workspace not 256-byte aligned", "tfgnn_sp_gemm_tn", plain_args(ws=WS + 16)),
    ("wide K=512*2016+1", "tfgnn_sp_gemm_tn_wide", plain_args(K=512 * 2016 + 1)),
    ("wide no scales of B", "tfgnn_sp_gemm_tn_wide", plain_args(inv_b=None)),
    ("grouped null table", "tfgnn_sp_gemm_tn_grouped", grouped_args(table=None)),
    ("grouped 513 ranges", "tfgnn_sp_gemm_tn_grouped", grouped_args(splits=513)),
    ("grouped N=96", "tfgnn_sp_gemm_tn_grouped", grouped_args(N=96)),
    ("grouped workspace of 1024 bytes", "tfgnn_sp_gemm_tn_grouped", grouped_args(ws_bytes=1024)),
]


def contract():
    """-> {"armed", "sizes": {query and arguments: bytes}, "rejections": {case: [return code, error text]}} of THIS process"""
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    sizes = {}
    for s in PLAIN_SIZES:
        sizes["plain %r" % (s,)] = lib.tfgnn_sp_gemm_tn_workspace_bytes(*s)
        sizes["wide %r" % (s,)] = lib.tfgnn_sp_gemm_tn_wide_workspace_bytes(*s)
    for s in GROUPED_SIZES:
        sizes["grouped %r" % (s,)] = lib.tfgnn_sp_gemm_tn_grouped_workspace_bytes(*s)
    rejections = {}
    for name, fn, args in REJECTIONS:
        rc = getattr(lib, fn)(*args)
        rejections[name] = [rc, lib.tfgnn_last_error().decode("utf-8", "replace")]
    return {"armed": lib.tfgnn_sp_guard_repair(-1), "sizes": sizes, "rejections": rejections}


def contract_in_child(env_value):
    code = "import json\nfrom tests.test_tn_host_contract import contract\nprint('CONTRACT', json.dumps(contract(), sort_keys=True))\n"
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("TFGNN_GUARD_REPAIR", None)
    if env_value is not None:
        env["TFGNN_GUARD_REPAIR"] = env_value
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120, cwd=str(ROOT))
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("CONTRACT ")]
    assert len(lines) == 1
    return json.loads(lines[0][len("CONTRACT "):])


def record():
    return {"repair_off": contract_in_child(None), "repair_on": contract_in_child("1")}


def test_the_record_is_what_the_issue_lists():
    want = json.loads(GOLDEN.read_text())
    for state, armed in (("repair_off", 0), ("repair_on", 1)):
        rec = want[state]
        assert rec["armed"] == armed
        assert len(rec["sizes"]) == 2 * len(PLAIN_SIZES) + len(GROUPED_SIZES) and len(rec["rejections"]) == len(REJECTIONS)
        for key, n in rec["sizes"].items():
            unsupported = any(key.endswith(repr(s)) for s in PLAIN_SIZES[-3:])
            assert (n == 0) == unsupported, key
        for name, (rc, text) in rec["rejections"].items():
            assert rc != 0 and text.startswith("tfgnn_sp_gemm_tn"), name
    # the tail of the trip words is all that the switch changes
    for key, n in want["repair_off"]["sizes"].items():
        tail = 0 if n == 0 else (2304 if key.startswith("grouped") else 256)
        assert want["repair_on"]["sizes"][key] == n + tail, key


def test_sizes_and_rejections_are_those_of_the_parent_commit():
    want = json.loads(GOLDEN.read_text())
    got = record()
    for state in ("repair_off", "repair_on"):
        for part in ("sizes", "rejections"):
            differing = {k: (got[state][part].get(k), v) for k, v in want[state][part].items() if got[state][part].get(k) != v}
            assert not differing, (state, part, differing)
        assert got[state] == want[state]


if __name__ == "__main__":
    print(json.dumps(record(), indent=1, sort_keys=True))
