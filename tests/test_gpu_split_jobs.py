"""The weight splits of a training step are built as jobs and launched by whoever built them (``ops.sp_split_*_jobs``,
``ops.aux_flush``) instead of waiting in a process-global queue that the next library call drained.  The step must launch what
it launched before: tests/golden/aux_launch_sequence_parent.json is what tools/record_aux_launches.py printed on an MI355X at
the commit before the queue was removed - per layer family, every tfgnn_aux_launch of one forward + backward pass from a cleared
weight-operand cache (the kinds of its non-empty jobs, whether its stream is the current one) and the step's launches per
kernel family.  The expected values come from that file, never from the code under test.

Cases and shapes: tools/record_aux_launches.py (V = 500, E = 5000, L = 3, D = H = 128; D = 512 for the long kernel stack whose
split takes two launches; sources of the compact-row case drawn from 200 nodes so that the layer takes that formulation)."""
import importlib.util
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def _load_recorder():
    spec = importlib.util.spec_from_file_location("record_aux_launches", ROOT / "tools" / "record_aux_launches.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _load_recorder()
CASES = rec.cases()
GOLDEN = json.loads((ROOT / "tests" / "golden" / "aux_launch_sequence_parent.json").read_text())


def test_the_record_covers_the_cases():
    assert sorted(GOLDEN) == sorted(c[0] for c in CASES)
    # the long kernel stack splits inside the layer in two consecutive launches, the column maxima (kind 6) first
    assert GOLDEN["edge_mlp_A_long_stack"]["launches"][:2] == [[[6], True], [[2], True]]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_step_launches_what_the_parent_commit_launched(dev, case):
    got, first = rec.run_case(case, dev)
    print(case[0], json.dumps(got, sort_keys=True))
    assert any(got["products"].get(f, 0) > 0 for f in rec.SPLIT_FAMILIES), got["products"]  # the split-operand route ran
    want = GOLDEN[case[0]]
    assert got["launches"] == want["launches"]
    assert got["products"] == want["products"]
    again, second = rec.run_case(case, dev)  # a fresh layer with the same seed, the cache cleared again
    assert again == got
    assert len(first) == len(second) and len(first) >= 3
    for a, b in zip(first, second):
        assert torch.equal(a, b)
