"""Every formulation of the GNN_Edge_MLP family computes, bit for bit, what it computed before the layer's choice of formulation
was moved into one method and every route got a forward and a backward function of its own: tests/golden/
edge_mlp_routes_parent_bits.json is what tools/record_edge_mlp_routes.py printed on an MI355X at the commit before that change -
per case the route taken (``ctx["path"]``, ``ctx["f16x2"]``, ``_grouped_tn_used``), the launches per kernel family and the
SHA-256 of the output, of d(node states) and of every weight gradient of one forward pass and one ``backward_with_epilogue``.

Cases and shapes: tools/record_edge_mlp_routes.py - the smallest that still take each route (H = 128, V = 384 .. 400, a few
thousand edges; 3 000 nodes for the grouped split-operand products).  No array is exempt: the recorder ran every case twice in
one process and found none whose hashes differ (it would list them under ``not_reproducible``; path A on split operands and on
the exact kernels may never have one)."""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _load_recorder():
    spec = importlib.util.spec_from_file_location("record_edge_mlp_routes", ROOT / "tools" / "record_edge_mlp_routes.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _load_recorder()
CASES = rec.cases()
GOLDEN = json.loads((ROOT / "tests" / "golden" / "edge_mlp_routes_parent_bits.json").read_text())


def test_the_record_covers_the_cases():
    assert sorted(GOLDEN) == sorted(c["name"] for c in CASES)
    for name, want in GOLDEN.items():
        if name.startswith("A_"):
            assert "not_reproducible" not in want, name
    # the routes the cases are named after were taken when the record was made
    assert [GOLDEN[n]["path"] for n in ("A_bf16x3", "Ac", "B_dense", "Bc", "C_exact_kernels")] == ["A", "Ac", "B", "Bc", "C"]
    assert GOLDEN["A_f16x2_one_call"]["f16x2"] is True and GOLDEN["A_per_edge_bf16x3"]["f16x2"] is False
    assert GOLDEN["A_mode_demoted_before_backward"]["products"].get("sp_tn", 0) == 0  # (the dense backward pass)
    assert GOLDEN["Bc_grouped_split"]["grouped_tn_used"] and GOLDEN["C_first_layer_split"]["grouped_tn_used"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_route_computes_what_the_parent_commit_computed(dev, case):
    got = rec.run_case(case, dev)
    print(case["name"], json.dumps(got, sort_keys=True))
    want = GOLDEN[case["name"]]
    skipped = want.get("not_reproducible", {})
    assert (got["path"], got["f16x2"], got["grouped_tn_used"]) == (want["path"], want["f16x2"], want["grouped_tn_used"])
    assert got["products"] == want["products"]
    assert sorted(got["sha"]) == sorted(want["sha"])
    differing = [k for k, h in want["sha"].items() if k not in skipped and got["sha"][k] != h]
    assert not differing, differing
