"""What the GNN_Edge_MLP family answers a layer stack before a pass - ``graph_parts``, ``recomputes_input_dropout``,
``weight_operand_requests`` - held against the record taken before the layer's choice of formulation was moved into one method
(tools/record_edge_mlp_plan.py, tests/golden/edge_mlp_plan_parent.json): every point of the grid, no case left out.  Host code
only: the layers are built on the meta device and no kernel runs."""
import importlib.util
import json
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "edge_mlp_plan_parent.json"


def _load_recorder():
    spec = importlib.util.spec_from_file_location("record_edge_mlp_plan", ROOT / "tools" / "record_edge_mlp_plan.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


plan = _load_recorder()


def test_every_answer_to_the_stack_equals_the_parent_record():
    want = json.loads(GOLDEN.read_text())
    got = plan.record()
    assert [list(p) for p in plan.points()] == want["points"]
    assert sorted(got["layers"]) == sorted(want["layers"]) == sorted(name for name, *_ in plan.layers())
    drift = []
    for name, row in want["layers"].items():
        mine = got["layers"][name]
        assert len(mine) == len(row) == len(want["points"]), name
        for i, (a, b) in enumerate(zip(mine, row)):
            a, b = got["answers"][plan.ALPHABET.index(a)], want["answers"][plan.ALPHABET.index(b)]
            if a != b:
                drift.append((name, tuple(want["points"][i]), "now " + a, "parent " + b))
    assert not drift, (len(drift), drift[:5])
