"""The split-operand weight-gradient (TN) product computes, bit for bit, what it computed before the plain and the grouped
product were given one workspace layout and one launch path (csrc/gemm_sp.hip): tests/golden/tn_product_parent_bits.json is
what tools/record_tn_product_bits.py printed on an MI355X at the commit before that change - per case the SHA-256 of the
output, the spread flag afterwards, the launches counted for the family ``sp_tn`` and, with the in-stream repair armed, the
repair counters.

Cases and shapes: tools/record_tn_product_bits.py - the smallest that reach every branch of the host path (the three factor
forms, the two-stage maxima of the factor pass, column ranges with a padded M, the scattered and accumulating reduce, the
grouped product with an empty group and with no K range at all, repair armed on quiet and on tripping operands).  No case is
exempt: the recorder ran every case twice in one process and would have refused to write the record had two runs differed."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _load_recorder():
    spec = importlib.util.spec_from_file_location("record_tn_product_bits", ROOT / "tools" / "record_tn_product_bits.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _load_recorder()
CASES = rec.cases()
IN_PROCESS = [c for c in CASES if not c["factor_pass"]]
GOLDEN = json.loads((ROOT / "tests" / "golden" / "tn_product_parent_bits.json").read_text())


def test_the_record_covers_the_cases():
    assert sorted(GOLDEN) == sorted(c["name"] for c in CASES)
    for c in CASES:
        want = GOLDEN[c["name"]]
        assert sorted(want) == sorted(["sha", "flag", "sp_tn"] + (["repair"] if c["armed"] else [])), c["name"]
        assert want["sp_tn"] == (0 if c.get("empty") else 1), c["name"]  # no K range: the reduce pass alone
        assert want["flag"] == 0, c["name"]  # quiet operands, or repaired on the stream
        if c["armed"]:
            assert want["repair"] == {"armed_products": 1, "repaired_products": 1 if c.get("trip") else 0}, c["name"]


@pytest.mark.parametrize("case", IN_PROCESS, ids=[c["name"] for c in IN_PROCESS])
def test_product_computes_what_the_parent_commit_computed(dev, case):
    got = rec.run_case(case, dev)
    print(case["name"], json.dumps(got, sort_keys=True))
    assert got == GOLDEN[case["name"]]


def test_separate_factor_pass_computes_what_the_parent_commit_computed(dev):
    got = rec.run_factor_pass_cases()
    print(json.dumps(got, sort_keys=True))
    assert got == {c["name"]: GOLDEN[c["name"]] for c in CASES if c["factor_pass"]}
