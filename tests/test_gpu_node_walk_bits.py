"""The R-GCN basis gather and the block-diagonal walk compute, bit for bit and launch for launch, what they computed before
the skeleton they share moved into one place (csrc/node_walk.hpp, csrc/node_walk.hip): tests/golden/node_walk_parent_bits.json
is what tools/record_node_walk_bits.py printed on an MI355X at the commit before that change - per case the SHA-256 of each
output (basis: Z, dX, dcoeff; block-diagonal: pre, dX, dQb) and the launch-count deltas of one forward and one backward call.

Cases and shapes: tools/record_node_walk_bits.py - the FLOAT family of every entry of ``CASES`` in
tests/test_gpu_basis_gather.py and tests/test_gpu_blockdiag_ops.py, the smallest shapes that reach every (VEC, LPR)
instantiation, rows of 31 .. 33 and 511 .. 513 edges in both directions, hubs of several items (the combine launch) and
one-type hubs.  No fp64 reference is computed here.  No case is exempt: the recorder ran every case twice in one process and
would have refused to write the record had two runs differed."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _load_recorder():
    spec = importlib.util.spec_from_file_location("record_node_walk_bits", ROOT / "tools" / "record_node_walk_bits.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _load_recorder()
CASES = rec.cases()
GOLDEN = json.loads((ROOT / "tests" / "golden" / "node_walk_parent_bits.json").read_text())


def test_the_record_covers_the_cases():
    assert sorted(GOLDEN) == sorted(c["name"] for c in CASES) and len(GOLDEN) == len(CASES)
    for c in CASES:
        want = GOLDEN[c["name"]]
        outputs = ["Z", "dX", "dcoeff"] if c["kind"] == "basis" else ["pre", "dX", "dQb"]
        assert sorted(want) == ["launches", "sha"] and sorted(want["sha"]) == sorted(outputs), c["name"]
        assert sorted(want["launches"]) == ["backward", "forward"], c["name"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_walk_computes_and_launches_what_the_parent_commit_did(dev, case):
    got = rec.run_case(case, dev)
    print(case["name"], json.dumps(got, sort_keys=True))
    assert got == GOLDEN[case["name"]]
