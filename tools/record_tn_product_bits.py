"""SHA-256 of what the split-operand weight-gradient (TN) product computes through every branch of its host path: the record
that pins the product bit for bit across a change of how the host code lays out its workspace and issues its launches.

    python tools/record_tn_product_bits.py > tests/golden/tn_product_parent_bits.json

Per case of ``cases()``: the hash of the output tensor, the spread flag afterwards, the launches counted for the family
``sp_tn`` (``ops.launch_counts``) and, with the in-stream repair armed, ``ops.repair_stats()``.  The operands come from the
seeded host generators of tests/test_gpu_gemm_sp_tn_edges.py (``structured``, ``zero_block_case``), tests/test_gpu_tn_repair.py
(``orphan_case``) and tests/tn_repair_grouped_reference.py, so the hashes depend on the kernels alone.  The cases that need the
separate factor pass (TFGNN_TN_FIK=0, read once per process) run together in one child process.  The recorder runs every case
twice in one process and refuses to write a record if two runs of a case differ: the product adds its slabs in a fixed order,
so no case is exempt from the comparison.  tests/test_gpu_tn_product_bits.py runs the same cases through ``cases()`` /
``run_case()`` / ``run_factor_pass_cases()`` and compares with the committed record."""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

QUIET = (5, 7, 9)  # row deficits the one-factor form takes (its guard: 2^20)
WIDE = (32, 36, 40, 44)  # ... and the two-factor form (2^22 per factor)
EMPTY_GROUPS = [0, 0, 0, 0]


def case(name, kind, **kw):
    return dict(name=name, kind=kind, factor_pass=False, armed=False, **kw)


def cases():
    """The smallest shapes that reach every branch of the host path.  kind "plain": sb, M, N, K (+ wide / a_cols / b_cols /
    scatter / accumulate / trip); kind "grouped": M, N, sb, transposed (+ trip / empty)"""
    out = []
    # one factor, computed in the kernel; (320, 640, ..): a tile straddles two blocks
    for sb, M, N, K in ((64, 256, 128, 2017), (320, 640, 128, 6053), (128, 128, 128, 17), (128, 128, 128, 1)):
        out.append(case(f"plain_sb{sb}_M{M}_K{K}", "plain", sb=sb, M=M, N=N, K=K))
    out.append(case("plain_column_ranges_padded_M", "plain", sb=64, M=256, N=256, K=2017, a_cols=(64, 144), b_cols=(128, 128)))
    # the call of the one-call layer backward pass (mp_layer.hip): dW [L, D, H] from [K, L H]^T [K, D]
    L, H, D = 2, 128, 128
    for acc in (True, False):
        out.append(case("plain_scattered" + ("_accumulating" if acc else ""), "plain", sb=H, M=L * H, N=D, K=2017,
                        scatter=(H, D * H, 1, H), accumulate=acc))
    for K in (2016, 2017, 6053):
        out.append(case(f"wide_K{K}", "plain", sb=64, M=256, N=128, K=K, wide=True))
    # the separate factor pass; K > 131072: its two-stage maxima
    for sb, M, N, K in ((64, 256, 128, 2017), (128, 128, 128, 131088)):
        c = case(f"factor_pass_sb{sb}_K{K}", "plain", sb=sb, M=M, N=N, K=K)
        c["factor_pass"] = True
        out.append(c)
    for M, N, sb in ((128, 128, 64), (256, 128, 128)):
        for transposed in (False, True):
            out.append(case(f"grouped_M{M}_sb{sb}" + ("_transposed" if transposed else ""), "grouped", M=M, N=N, sb=sb,
                            transposed=transposed))
    out.append(case("grouped_all_groups_empty", "grouped", M=128, N=128, sb=64, transposed=False, empty=True))
    armed = [case("armed_plain_quiet", "plain", sb=64, M=256, N=128, K=2017),
             case("armed_plain_tripping", "plain", sb=64, M=256, N=128, K=2017, trip=True),
             case("armed_grouped_quiet", "grouped", M=128, N=128, sb=64, transposed=False),
             case("armed_grouped_tripping", "grouped", M=128, N=128, sb=64, transposed=False, trip=True)]
    for c in armed:
        c["armed"] = True
    return out + armed


def seed_of(c):
    return 100 + sum(ord(ch) for ch in c["name"])


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _plain(c, dev, ops):
    import torch

    from tests.test_gpu_gemm_sp_tn_edges import zero_block_case
    from tests.test_gpu_tn_repair import orphan_case

    sb, M, N, K, wide = c["sb"], c["M"], c["N"], c["K"], c.get("wide", False)
    if c.get("trip"):
        a, b = orphan_case(K, M, N, sb, 30, 0, seed_of(c))  # rows 2^-30 below the others: beyond the one-factor guard
    else:
        a, b = zero_block_case(K, M, N, sb, seed_of(c), WIDE if wide else QUIET, b_spread=3 if wide else 4)
    a_sp, b_sp = ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev))
    Mc = c["a_cols"][1] if c.get("a_cols") else M
    Nc = c["b_cols"][1] if c.get("b_cols") else N
    out = None
    if c.get("scatter"):
        out = torch.randn((Mc * Nc,), generator=torch.Generator().manual_seed(seed_of(c) + 7)).to(dev)
    return ops.sp_gemm_tn(a_sp, b_sp, a_cols=c.get("a_cols"), b_cols=c.get("b_cols"), out=out, scatter=c.get("scatter"),
                          accumulate=c.get("accumulate", False), wide=wide)


def _grouped(c, dev, ops):
    import torch

    from tests import tn_repair_grouped_reference as grp
    from tests.test_gpu_gemm_sp_tn_edges import structured

    M, N, sb = c["M"], c["N"], c["sb"]
    if c.get("trip"):
        a, b, off = grp.tripping_case(M, N, sb, seed_of(c))
    else:
        off = grp.offsets()
        g = torch.Generator().manual_seed(seed_of(c))
        R = off[-1]
        a = structured(R, M, sb, seed_of(c) + 1, deficit=torch.randint(0, 4, (R, M // sb), generator=g))
        b = structured(R, N, N, seed_of(c) + 2, deficit=torch.randint(0, 4, (R, 1), generator=g))
    a_sp, b_sp = ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev))
    if c.get("empty"):  # no rows in any group: no K range, the reduce pass alone (it writes zeros)
        off = EMPTY_GROUPS
        a_sp = ops.SplitOperand(a_sp.data, a_sp.inv_scale, 0, M, sb)
        b_sp = ops.SplitOperand(b_sp.data, b_sp.inv_scale, 0, N, N)
    groups = ops.RowGroups(off, dev)
    out = torch.full((groups.num_groups, N, M) if c["transposed"] else (groups.num_groups, M, N), float("nan"), device=dev)
    return ops.sp_gemm_tn_grouped(a_sp, b_sp, groups, out, transposed=c["transposed"])


def run_case(c, dev):
    """-> {"sha", "flag", "sp_tn"} and, armed, {"repair": ops.repair_stats()}.  Leaves mode f16x2, the flag down, repair off."""
    import torch

    from tf2_gnn_amd import _lib, ops

    ops.set_gemm_mode("f16x2")
    was = ops.set_guard_repair(c["armed"])
    if c["armed"]:
        ops.repair_stats(reset=True)
    try:
        before = ops.launch_counts()["sp_tn"]
        out = (_plain if c["kind"] == "plain" else _grouped)(c, dev, ops)
        res = {"sp_tn": ops.launch_counts()["sp_tn"] - before}
        torch.cuda.synchronize()
        res["flag"] = _lib.load().tfgnn_sp_spread_flag(0)
        res["sha"] = sha(out)
        if c["armed"]:
            res["repair"] = ops.repair_stats(reset=True)
    finally:
        torch.cuda.synchronize()
        ops.set_guard_repair(was)
        ops.set_gemm_mode("f16x2")
    return res


def run_twice(cs, dev):
    out = {}
    for c in cs:
        first, second = run_case(c, dev), run_case(c, dev)
        if first != second:
            raise SystemExit(f"{c['name']}: two runs in one process differ - a finding, not a case to exempt:\n{first}\n{second}")
        out[c["name"]] = first
    return out


def run_factor_pass_cases(twice=False):
    """The cases with ``factor_pass`` in ONE child process with TFGNN_TN_FIK=0 -> {name: result}"""
    env = dict(os.environ, TFGNN_TN_FIK="0", PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, str(Path(__file__).resolve()), "--factor-pass-child"] + (["--twice"] if twice else [])
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    lines = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
    if res.returncode != 0 or len(lines) != 1:
        raise RuntimeError("factor-pass child failed:\n" + res.stdout[-2000:] + res.stderr[-3000:])
    return json.loads(lines[0][len("RESULT "):])


if __name__ == "__main__":
    import torch

    device = torch.device("cuda", 0)
    if "--factor-pass-child" in sys.argv:
        assert os.environ.get("TFGNN_TN_FIK") == "0"
        mine = [c for c in cases() if c["factor_pass"]]
        got = run_twice(mine, device) if "--twice" in sys.argv else {c["name"]: run_case(c, device) for c in mine}
        print("RESULT " + json.dumps(got, sort_keys=True))
    else:
        record = run_twice([c for c in cases() if not c["factor_pass"]], device)
        record.update(run_factor_pass_cases(twice=True))
        print(json.dumps(record, indent=1, sort_keys=True))
