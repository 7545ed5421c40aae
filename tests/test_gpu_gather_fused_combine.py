"""The gather combines its multi-item rows inside its own launch (csrc/spmm.hip finish_multi_row): the item workgroup of a row
that stores its partial sums last adds the row's partial rows in item order.  Nothing else changed - same sums, same order,
same operands - so the checks are: the fp64 reference, bit-identity with the parent commit (recorded hashes), no dependence
on which workgroup arrives last (back-to-back launches, replays, two handles on two streams), the arrival counters back at
zero, and the launch structure of a training step.

Graph: tools/record_gather_bits.py (V = 300, L = 3, type 2 empty; in- and out-degrees 48, 49, 513, 1025, 2600 of type 0 around
the plan's limits - typed threshold 48, 512-edge items).

Bounds (those of tests/test_gpu_graph_gather.py for the same views, from arithmetic, not from the code under test):
  fp32 sums   |out - ref| <= 2e-6 * l1, l1 = sum |terms| * max(1, |row_scale|)
  max         two fp32 roundings: |out - ref| <= 2^-22 * |ref|; empty rows are the lowest float
  SP16 sums   the same sum bound plus what the format adds to an exact fp32 value (tests/test_gpu_gemm_sp.py
              test_gather_sp_matches_fp32_gather): 2^-22 * |ref| + 2^-37 * (largest |ref| of the row)"""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import gather_reference as gr
from tests.helpers import decode_sp16, random_graph, to_dev

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SUM_TOL = 2e-6
MAX_TOL = 2.0 ** -22


def _load_recorder():
    spec = importlib.util.spec_from_file_location("record_gather_bits", ROOT / "tools" / "record_gather_bits.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _load_recorder()
CASES = rec.cases()


class _Shared:
    """the graph, every case's device inputs, results of ONE eager run and fp64 references (computed once, read only)"""

    def __init__(self, dev):
        self.dev = dev
        self.graph = rec.make_graph(dev)
        self.lists = rec.adjacency_lists()
        self._inputs, self._results, self._views = {}, {}, {}

    def inputs(self, case):
        key = (case[1], case[2])
        if key not in self._inputs:
            self._inputs[key] = tuple(torch.from_numpy(a).to(self.dev) for a in rec.host_inputs(case[1], case[2]))
        return self._inputs[key]

    def run(self, case):
        return rec.run_case(self.graph, case, self.dev, self.inputs(case))

    def result(self, case):
        if case[0] not in self._results:
            res = self.run(case)
            torch.cuda.synchronize()
            self._results[case[0]] = res
        return self._results[case[0]]

    def host_view(self, view):
        if view not in self._views:
            from tf2_gnn_amd import ops

            pos = self.graph.array(ops.G_PATTERN_POS_BY_DST).cpu().numpy() if view == gr.VIEW_BY_DST_TYPED_PATTERN else None
            self._views[view] = gr.view_rows(self.lists, rec.NUM_NODES, view, pattern_pos=pos)
        return self._views[view]


@pytest.fixture(scope="module")
def shared(dev):
    return _Shared(dev)


def test_the_graph_has_the_planned_rows(shared):
    """degrees at both sides of the limits read from the library; 2 + 3 + 6 partial slots per hub side"""
    from oracle import adjacency_oracle as ao
    from tf2_gnn_amd import _lib

    for by, hubs in (("dst", rec.HUB_TARGETS), ("src", rec.HUB_SOURCES)):
        rowptr, _, _ = ao.bucket_edges(shared.lists, rec.NUM_NODES, by=by)
        lens = np.diff(rowptr).reshape(rec.NUM_NODES, 3)
        assert tuple(int(lens[v, 0]) for v in hubs) == rec.HUB_DEGREES
        assert int(lens[:, 2].sum()) == 0 and int(lens[:, 1].sum()) == 300
        rest = np.delete(lens[:, 0], hubs)
        assert int(rest.max()) <= 48  # every other bucket is a short row
    lib = _lib.load()
    for view in (0, 2, 6):
        assert lib.tfgnn_graph_gather_workspace_bytes(shared.graph._h, view, 64) == (2 + 3 + 6) * 64 * 4
    assert lib.tfgnn_graph_gather_workspace_bytes(shared.graph._h, 1, 64) == (2 + 3 + 6) * 64 * 4


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_against_fp64(shared, case):
    name, view, width, weighted, kind = case
    rowptr, col, out_rows = shared.host_view(view)
    X, ew, rs = (t.cpu() for t in shared.inputs(case))
    ref, l1, _ = gr.gather_reference(rowptr, col, X, edge_weight=ew if weighted else None, row_scale=rs if weighted else None,
                                     reduce="max" if kind == "max" else "sum")
    if out_rows is not None:
        ref, l1 = ref[out_rows], l1[out_rows]
    res = shared.result(case)
    if kind == "sp":
        from tf2_gnn_amd import ops

        op = ops.SplitOperand(res["data"], res["inv_scale"].reshape(-1, 1), ref.shape[0], width, width)
        got = torch.from_numpy(decode_sp16(op))
        fmt = ref.abs() * 2.0 ** -22 + ref.abs().amax(dim=1, keepdim=True) * 2.0 ** -37
        excess = (got - ref).abs() - fmt
        worst = float((excess / l1.clamp(min=1e-300)).masked_fill(l1 == 0, 0).max())
        print(f"{name}: error beyond the format's {worst:.3e} of l1 (bound {SUM_TOL:.1e})")
        assert bool((excess[l1 == 0] <= 0).all()), f"{name}: a row without edges is not zero"
        assert worst <= SUM_TOL, f"{name}: {worst:.3e} of the row's l1 mass"
        return
    got = res["rows"].cpu().double()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    if kind == "max":
        empty = ref == gr.FLOAT_LOWEST
        assert torch.equal(got[empty], ref[empty])
        worst = float(((got - ref).abs()[~empty] / ref.abs()[~empty]).max())
        print(f"{name}: max relative error {worst:.3e} (bound 2^-22)")
        assert worst <= MAX_TOL
        return
    diff = (got - ref).abs()
    assert bool((diff[l1 == 0] == 0).all()), f"{name}: a row without edges is not exactly zero"
    worst = float((diff / l1.clamp(min=1e-300)).masked_fill(l1 == 0, 0).max())
    print(f"{name}: {worst:.3e} of l1 (bound {SUM_TOL:.1e})")
    assert worst <= SUM_TOL, f"{name}: {worst:.3e} of the row's l1 mass"


def test_bits_equal_the_parent_commit(shared):
    """tests/golden/gather_combine_parent_bits.json: what tools/record_gather_bits.py printed on an MI355X at the commit before
    the combine moved into the gather launch"""
    golden = json.loads((ROOT / "tests" / "golden" / "gather_combine_parent_bits.json").read_text())
    got = {}
    for case in CASES:
        for arr, t in shared.result(case).items():
            got[f"{case[0]} {arr}"] = rec.sha(rec.bucket_order(shared.graph, case[1], t))
    assert sorted(got) == sorted(golden)
    wrong = [k for k in golden if got[k] != golden[k]]
    assert not wrong, wrong


def _arrival_counters(graph):
    from tf2_gnn_amd import ops

    return [graph.array(ops.G_GATHER_ARRIVALS_VIEW0 + v) for v in range(4)]


@pytest.mark.parametrize("case", [c for c in CASES if c[2] in (320, 1280) and c[3]], ids=lambda c: c[0])
def test_twenty_launches_back_to_back_agree_and_leave_the_counters_at_zero(shared, case):
    outs = [shared.run(case) for _ in range(20)]  # fresh outputs, no synchronisation in between
    torch.cuda.synchronize()
    first = shared.result(case)
    for o in outs:
        for arr in first:
            assert torch.equal(o[arr], first[arr]), arr
    counters = _arrival_counters(shared.graph)
    assert sum(c.numel() for c in counters) == 4 * 3 * 8  # three multi-item rows per view, eight counters each
    for c in counters:
        assert int(c.abs().sum()) == 0


def test_captured_pair_replays_to_the_eager_bits(shared):
    """a forward (by target) and a backward (by source) gather captured into one hipGraph and replayed three times"""
    from tf2_gnn_amd import CapturedStep

    fwd = next(c for c in CASES if c[0] == "sp view0 w320 weighted")
    bwd = next(c for c in CASES if c[0] == "sp view2 w320 weighted")
    wide = next(c for c in CASES if c[0] == "fp32 view0 w1280 plain")

    def step():
        a, b, c = shared.run(fwd), shared.run(bwd), shared.run(wide)
        return a["data"], a["inv_scale"], b["data"], b["inv_scale"], c["rows"]

    eager = [shared.result(fwd)["data"], shared.result(fwd)["inv_scale"], shared.result(bwd)["data"], shared.result(bwd)["inv_scale"],
             shared.result(wide)["rows"]]
    cap = CapturedStep(step)
    cap.capture()
    for _ in range(3):
        out = cap.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got, want)
    for c in _arrival_counters(shared.graph):
        assert int(c.abs().sum()) == 0


def test_two_handles_on_two_streams(shared, dev):
    """the counters live in the handle: gathers over two handles may be in flight at once"""
    other = rec.make_graph(dev)
    case = next(c for c in CASES if c[0] == "sp view0 w320 weighted")
    wide = next(c for c in CASES if c[0] == "fp32 view2 w1280 weighted")
    want = [shared.result(case), shared.result(wide)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    main = torch.cuda.current_stream()
    shared.inputs(case), shared.inputs(wide)
    torch.cuda.synchronize()
    got1, got2 = [], []
    for _ in range(5):
        with torch.cuda.stream(s1):
            got1.append([rec.run_case(shared.graph, c, dev, shared.inputs(c)) for c in (case, wide)])
        with torch.cuda.stream(s2):
            got2.append([rec.run_case(other, c, dev, shared.inputs(c)) for c in (case, wide)])
    main.wait_stream(s1)
    main.wait_stream(s2)
    torch.cuda.synchronize()
    for got in got1 + got2:
        for res, ref in zip(got, want):
            for arr in ref:
                assert torch.equal(res[arr], ref[arr]), arr
    other.close()


def test_training_step_launches_small_passes_twice_then_never(dev, monkeypatch):
    """The benchmarked RGCN stack at V = 2500: with a cleared weight-operand cache the only small-pass launches of a training
    step are the two at the start of its passes (all stale weights split at once); a second step with unchanged weights
    launches none.  The layer-level entry points are handed no weight to split (``stale`` False), so nothing is launched
    inside them either - their gathers return no combine job.  Both routes give the same bits."""
    import bench
    from tf2_gnn_amd import _lib, ops
    from tf2_gnn_amd.layers import GNN, GNNInput
    from tf2_gnn_amd.layers.message_passing import set_seed

    V, E, L, H = 2500, 60000, 4, 320
    adjs = to_dev(random_graph(V, E, L, seed=3, hub=(5, 300)), dev)
    gen = torch.Generator().manual_seed(5)
    X = torch.randn((V, H), generator=gen).to(dev)
    dOut = torch.randn((V, H), generator=gen).to(dev)
    n2g = torch.zeros(V, dtype=torch.int32, device=dev)
    lib = _lib.load()
    real = lib.tfgnn_aux_launch
    launches = []

    def spy(jobs, n, stream):
        launches.append(sum(1 for i in range(n) if jobs[i].kind != 0 and jobs[i].num_blocks != 0))
        return real(jobs, n, stream)

    stale_flags = []
    real_for_call = ops._weight_operand_for_call

    def for_call(w, kind, rows, cols):
        op, stale = real_for_call(w, kind, rows, cols)
        stale_flags.append(stale)
        return op, stale

    monkeypatch.setattr(lib, "tfgnn_aux_launch", spy)
    monkeypatch.setattr(ops, "_weight_operand_for_call", for_call)
    results = {}
    for entry in ("1", "0"):
        monkeypatch.setenv("TFGNN_MP_ENTRY", entry)
        set_seed(0)
        gnn = GNN(bench.model_params("rgcn", H, 4, None))
        gnn.dropout_seed = 7
        graph = ops.Graph(adjs, V, parts=ops.G_PARTS_ALL)
        inp = GNNInput(X, graph, n2g, 1)

        def step():
            gnn._dropout_calls = 0
            out = gnn(inp, training=True)
            dx = gnn.backward(dOut, need_input_grad=True)
            torch.cuda.synchronize()
            return [out.clone(), dx.clone()] + [v.grad.clone() for v in gnn.trainable_variables]

        for _ in range(4):  # the stack's first backward passes are checked synchronously; same launches
            step()
        ops.clear_weight_operand_cache()
        del launches[:], stale_flags[:]
        first = step()
        assert [n for n in launches if n] and len([n for n in launches if n]) == 2, launches
        assert not any(stale_flags), stale_flags
        if entry == "1":
            assert len(stale_flags) == 8  # four layers, two passes: every call found its operand built
        del launches[:], stale_flags[:]
        second = step()
        assert not [n for n in launches if n], launches
        assert not any(stale_flags)
        for a, b in zip(first, second):
            assert torch.equal(a, b)
        results[entry] = first
        graph.close()
    for a, b in zip(results["1"], results["0"]):
        assert torch.equal(a, b)
