"""tfgnn_pool_forward / tfgnn_pool_backward (csrc/pool_fused.hip) against tests/pool_reference.py, a float64 restatement of the
header's contract, on chosen inputs: tiles that own both workspace slots, empty graphs next to chunked ones, chunk edges on
tile edges, heads that are no power of two or more than 64, rows of 1 to 1024 floats on the float4 and the scalar path, scores
that need the maximum subtracted, activations exactly on the clip bounds, NaN and inf.  The inputs and the comparison are
tests/pool_cases.py's, shared with tests/test_pool_reference_host.py, which shows on the host that this comparison fails for
each of a list of planted defects.  The C ABI is called directly: every buffer is a slice of a wider one."""
import numpy as np
import pytest
import torch

from tests import pool_cases as pc
from tests.helpers import record_parity
from tests.pool_abi import _raw_backward, _raw_forward

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def _ids(sizes):
    return torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes).astype(np.int32))


def _padded(dev, rows, width, left, right, fill, data=None):
    """[rows, left + width + right] filled with ``fill`` -> (buffer, its columns [left, left + width), holding ``data``)"""
    buf = torch.full((rows, left + width + right), fill, dtype=torch.float32, device=dev)
    view = buf[:, left:left + width]
    if data is not None:
        view.copy_(torch.from_numpy(np.array(data, dtype=np.float32)).to(dev))  # a copy: the cases' inputs are read-only
    return buf, view


def _untouched(buf, left, width, fill):
    outside = torch.cat([buf[:, :left], buf[:, left + width:]], dim=1)
    return bool((outside == fill).all())


def run_readout(dev, case, kind, lo, hi, T=None, S=None):
    """One forward and one backward call on the case's inputs (or on ``T`` / ``S``, S as the kernels get it) -> dict(out, w, dT,
    dS) of float32 numpy arrays (w None unless softmax, dS None without scores).  T and S sit in buffers padded with NaN - a
    read outside the slice poisons a result - and w, dT, dS in buffers padded with a sentinel that must survive."""
    from tf2_gnn_amd.layers.nodes_to_graph_representation import segment_offsets

    T0, S0, dOut = pc.inputs(case)
    T = T0 if T is None else T
    S = pc.scores_for(kind, S0) if S is None else S
    V, G, GD, heads, col0 = case.V, case.G, case.GD, case.heads, case.col0
    ids = _ids(case.sizes).to(dev)
    ptr = segment_offsets(ids, G)
    assert ptr.cpu().tolist() == case.ptr.tolist()
    nan = float("nan")
    _, Td = _padded(dev, V, GD, col0, 12 - col0, nan, T)
    Sd = None if S is None else _padded(dev, V, heads, 1, 2, nan, S)[1]
    g = torch.from_numpy(dOut.copy()).to(dev)
    w_buf, w = _padded(dev, V, heads, 2, 3, SENTINEL)
    out = _raw_forward(kind, ptr, Td, Sd, heads, lo, hi, w=w)
    w_used = w if kind == "softmax" else Sd
    dT_buf, dT = _padded(dev, V, GD, col0, 12 - col0, SENTINEL)
    dS_buf, dS = _padded(dev, V, heads, 1, 1, SENTINEL)
    _raw_backward(kind, ptr, ids, g, Td, w_used, heads, lo, hi, dT, dS if w_used is not None else None)
    torch.cuda.synchronize()
    assert _untouched(w_buf, 2, heads, SENTINEL) and _untouched(dT_buf, col0, GD, SENTINEL) and _untouched(dS_buf, 1, heads, SENTINEL)
    if kind != "softmax":  # w is an output of the softmax alone
        assert bool((w == SENTINEL).all())
    if w_used is None:
        assert bool((dS == SENTINEL).all())
    host = lambda t: t.contiguous().cpu().numpy()
    return {"out": host(out), "w": host(w) if kind == "softmax" else None, "dT": host(dT),
            "dS": host(dS) if w_used is not None else None}


def _bounds_id(b):
    return "nobounds" if b == (None, None) else f"{'lo' if b[0] is not None else ''}{'hi' if b[1] is not None else ''}"


PARAMS = [pytest.param(c.name, kind, b, id=f"{c.name}-{kind}-{_bounds_id(b)}") for c in pc.cases() for kind in c.kinds for b in c.bounds]


def test_chunk_size_is_the_librarys():
    from tf2_gnn_amd import _lib

    assert pc.C == _lib.POOL_CHUNK_NODES


@pytest.mark.parametrize("name, kind, bounds", PARAMS)
def test_readout_against_the_fp64_reference(dev, name, kind, bounds):
    """Bounds: tests/pool_cases.py (1e-5 scaled, plus the allowance derived there for the cases of more than 256 columns)."""
    from tf2_gnn_amd import ops

    case = pc.by_name(name)
    lo, hi = bounds
    pc.assert_conditions(case, kind, lo, hi)
    before = ops.pool_launch_counts()
    got = run_readout(dev, case, kind, lo, hi)
    r = pc.reference(case, kind, lo, hi)
    if case.V == 0:  # nothing is launched and nothing written: out still holds what _raw_forward filled it with
        assert ops.pool_launch_counts() == before and np.isnan(got["out"]).all() and got["out"].shape == (case.G, case.GD)
        return
    if case.scores != "randn":
        assert all(np.isfinite(x).all() for x in got.values() if x is not None)
        # the weights of a (graph, head) sum to s / (s + 1e-7), s = its sum of exponentials, from the reference
        for g in range(case.G):
            a, b = int(case.ptr[g]), int(case.ptr[g + 1])
            if b > a:
                want = r["w"][a:b].sum(axis=0)
                assert np.all(want > 0.99) and np.abs(got["w"][a:b].astype(np.float64).sum(axis=0) - want).max() <= pc.TOL
    if case.ties:
        T, _, dOut = pc.inputs(case)
        tie = np.zeros(T.shape, dtype=bool)
        for bound in (lo, hi):
            if bound is not None:
                tie |= T == bound
        through = np.repeat(r["w"], case.GD // case.heads, axis=1) * dOut[pc.node_graph(case)]
        assert tie.mean() >= 0.02 and np.abs(through[tie]).min() > 0  # at a tie dT is w * dOut, not 0
        assert np.abs(got["dT"][tie] - through[tie]).max() <= pc.TOL * max(1.0, np.abs(through[tie]).max())
    worst = pc.compare(case, kind, lo, hi, got, r=r)
    for what, e in worst.items():
        print(f"pool reference {name} {kind} {_bounds_id(bounds)} {what}: error / bound {e:.3f}")
        record_parity(f"pool reference {name} {kind} {what}", max_error_over_bound=e, bound=1.0)


def test_rows_of_more_than_1024_floats_are_refused(dev):
    from tf2_gnn_amd import ops

    case = pc.Case("too_wide", [5, 3], 1028, 4)
    ids = _ids(case.sizes).to(dev)
    from tf2_gnn_amd.layers.nodes_to_graph_representation import segment_offsets

    ptr = segment_offsets(ids, case.G)
    T = torch.zeros((case.V, 1028), device=dev)
    S = torch.zeros((case.V, 4), device=dev)
    w = torch.zeros((case.V, 4), device=dev)
    dOut = torch.zeros((case.G, 1028), device=dev)
    before = ops.pool_launch_counts()
    with pytest.raises(RuntimeError, match="not supported"):
        _raw_forward("softmax", ptr, T, S, 4, None, None, w=w)
    with pytest.raises(RuntimeError, match="not supported"):
        _raw_backward("softmax", ptr, ids, dOut, T, w, 4, None, None, torch.zeros_like(T), torch.zeros_like(S))
    assert ops.pool_launch_counts() == before


PLANT_PARAMS = [pytest.param(p, b, where, id=f"{p[0]}_{'nan' if np.isnan(p[1]) else 'inf'}-{_bounds_id(b)}-{where}")
                for p in pc.PLANTS for b in pc.BOUNDS for where in pc.PLANT_SPOTS]


@pytest.mark.parametrize("plant, bounds, where", PLANT_PARAMS)
def test_nonfinite_inputs_stay_in_their_graph_and_show(dev, plant, bounds, where):
    """A NaN or +inf as a VALUE of T or S (never an index) in one graph of several: non-finite results exactly where the
    reference has them, every other graph bit-equal to the run without the plant.  tests/pool_cases.py check_planted."""
    what, value, kinds = plant
    lo, hi = bounds
    case = pc.NONFINITE_CASE
    for kind in kinds:
        worst = pc.check_planted(case, kind, lo, hi, what, value, where, lambda T, S: run_readout(dev, case, kind, lo, hi, T=T, S=S))
        for name, e in worst.items():
            record_parity(f"pool reference planted {what} {kind} {name}", max_error_over_bound=e, bound=1.0)


# ---- the op-level kernels (csrc/pool.hip), which two tests of test_gpu_pool_entry.py use as their yardstick ----------------
OP_CASES = [c.name for c in pc.cases() if c.name.startswith("heads_") or c.name in ("scores_const", "scores_const_cycle")]


@pytest.mark.parametrize("bounds", pc.BOUNDS, ids=_bounds_id)
@pytest.mark.parametrize("name", OP_CASES)
def test_op_level_kernels_against_the_fp64_reference(dev, name, bounds):
    """tfgnn_segment_softmax, tfgnn_segment_weighted_sum and their two backward calls on contiguous inputs, same comparison."""
    from tests.test_gpu_pool_entry import _op_level_backward, _op_level_forward
    from tf2_gnn_amd.layers.nodes_to_graph_representation import segment_offsets

    case = pc.by_name(name)
    lo, hi = bounds
    T, S, dOut = pc.inputs(case)
    ids = _ids(case.sizes).to(dev)
    ptr = segment_offsets(ids, case.G)
    for kind in case.kinds:
        pc.assert_conditions(case, kind, lo, hi)
        Td = torch.from_numpy(T.copy()).to(dev)
        Sd = torch.from_numpy(pc.scores_for(kind, S).copy()).to(dev)
        out, w, R = _op_level_forward(kind, ptr, Td, Sd, case.heads, lo, hi)
        dT, dS = _op_level_backward(kind, ptr, ids, torch.from_numpy(dOut.copy()).to(dev), Td, R, w, case.heads, lo, hi)
        torch.cuda.synchronize()
        got = {"out": out.cpu().numpy(), "w": w.cpu().numpy() if kind == "softmax" else None, "dT": dT.cpu().numpy(), "dS": dS.cpu().numpy()}
        worst = pc.compare(case, kind, lo, hi, got)
        for what, e in worst.items():
            record_parity(f"pool op-level {name} {kind} {what}", max_error_over_bound=e, bound=1.0)
