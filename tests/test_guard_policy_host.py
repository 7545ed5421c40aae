"""The spread-guard policy of the f16x2 mode (tf2_gnn_amd/guard.py) held, transition by transition, against the record taken
before its state moved into one object per stack (tools/record_guard_policy.py, tests/golden/guard_policy_parent.json): every
scenario of the grid, field for field.  Host code only: the library's three entry points, the stream wait and the backward walk
are the recorder's fakes."""
import ast
import importlib.util
import itertools
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "guard_policy_parent.json"


def _load_recorder():
    spec = importlib.util.spec_from_file_location("record_guard_policy", ROOT / "tools" / "record_guard_policy.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


recorder = _load_recorder()


def test_every_scenario_replays_the_parent_record():
    from tf2_gnn_amd import guard

    want = json.loads(GOLDEN.read_text())
    guard.reset_warned()  # (the record was taken in a fresh process)
    try:
        got = recorder.record()
    finally:
        guard.reset_warned()  # (... and the tests after this one expect one too)
    assert sorted(got["scenarios"]) == sorted(want["scenarios"])
    assert {name for name, *_ in recorder.grid()} < set(want["scenarios"]) and len(recorder.grid()) == 6 * 3 * 2 * 3 * 2 * 4 * 2
    drift = []
    for name, row in want["scenarios"].items():
        mine = got["scenarios"][name]
        assert len(mine) == len(row), name
        for call, (a, b) in enumerate(zip(mine, row)):
            a, b = got["steps"][a], want["steps"][b]
            assert sorted(a) == sorted(b)
            drift.extend((name, call, field, "now", a[field], "parent", b[field]) for field in b if a[field] != b[field])
    assert not drift, (len(drift), drift[:5])


def test_the_stage_is_what_the_parent_inferred_from_its_flags():
    """The parent kept ``_dense_tn_wide``, ``_dense_split_ok`` and ``_tn_demoted_epoch`` and read the stage off them."""
    from tf2_gnn_amd import guard

    def inferred(dense_tn_wide, dense_split_ok, tn_demoted):
        stage = "none"
        if dense_tn_wide:
            stage = "1a"
        if not dense_split_ok:
            stage = "1b"
        if tn_demoted:
            stage = "2"
        return stage

    policy = guard.GuardPolicy(None)
    for dense, grouped_tn in itertools.product(("split", "wide", "exact"), ("split", "exact")):
        policy.dense, policy.grouped_tn = dense, grouped_tn
        assert policy.stage == inferred(dense != "split", dense != "exact", grouped_tn == "exact"), (dense, grouped_tn)
    # ... and every pair is reachable: ``advance`` walks dense split -> wide -> exact while Dense products are possible, and
    # takes grouped_tn from any of the three when they are not
    layer = recorder.StubLayer(True)
    for steps in range(3):
        policy, layer._grouped_tn_split_ok, layer._grouped_tn_used = guard.GuardPolicy(None), True, True
        seen = [policy.advance([layer], True) for _ in range(steps)] + [policy.advance([layer], False)]
        assert all(seen) and (policy.dense, policy.grouped_tn) == (("split", "wide", "exact")[steps], "exact")
        assert layer._grouped_tn_split_ok is False and policy.advance([layer], False) is None


def test_guard_does_not_import_ops():
    """guard.py needs ``_lib`` and torch only: ``ops`` imports it, never the other way round."""
    tree = ast.parse((ROOT / "tf2_gnn_amd" / "guard.py").read_text())
    relative, absolute = set(), set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            absolute.update(a.name.split(".")[0] for a in node.names)
        elif isinstance(node, ast.ImportFrom) and node.level:
            relative.update([node.module] if node.module else [a.name for a in node.names])
        elif isinstance(node, ast.ImportFrom):
            absolute.add(node.module.split(".")[0])
    assert relative == {"_lib"}, relative
    assert absolute - set(sys.stdlib_module_names) == {"torch"}, absolute
    assert "importlib" not in absolute and "__import__" not in {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)}
