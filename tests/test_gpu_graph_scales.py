"""tfgnn_graph_scales, tfgnn_graph_target_multiplier (csrc/graph.hip) and the per-edge arrays of a graph handle against
tests/edge_reference.py, which builds them on the host from oracle.adjacency_oracle.bucket_edges and the formulas of
include/tfgnn.h.

The graphs: the four small ones of tests/test_gpu_edge_ops.py (an empty type, a 700-edge hub, a single edge type) and a large one,
V = 1 100 000, L = 2, E = 2 300 000 with nodes of in-degree 0 and a 5000-edge hub: R = V L = 2 200 000, R + 1 and E all lie past the
8 192 x 256 threads of the three kernels' grids and R != E, so the grid-stride loops take a second trip and graph_scales_kernel
runs both of its halves (i < R, i < E) with different ends.  The small graphs have R < E (and R > E where a type is empty), all
inside one trip.

tfgnn_graph_scales: with mode 0 (sum) the outputs are ones or copies of the handle's 1 / (c + 1e-7) arrays and EQUAL the
reference.  With modes 1 (mean) and 2 (sqrt_n) every element is within a relative 1.01 x 4 x 2^-24 of the fp64 value: a reciprocal
or a reciprocal square root, a division and a product, four roundings at most - derived, not measured; the worst ratio is
recorded in the parity log.  Every output carries a guard element behind its last one."""
import numpy as np
import pytest
import torch

from tests import edge_reference as ref
from tests.edge_reference import guard_untouched, guarded, untouched
from tests.helpers import random_graph, record_parity, to_dev
from tests.test_gpu_edge_ops import GRAPHS

pytestmark = pytest.mark.gpu

GRID_THREADS = 8192 * 256
BIG_V, BIG_L, BIG_E, BIG_HUB = 1100000, 2, 2300000, (123457, 5000)
REL_BOUND = 1.01 * 4 * ref.U32


class _Case:
    """a graph on the host (lists, the oracle's buckets) and its handle"""

    def __init__(self, adjs, V, dev, parts=None):
        from tf2_gnn_amd import ops

        self.adjs, self.V, self.L = adjs, V, len(adjs)
        self.buckets = ref.host_buckets(adjs, V)
        self.g = ops.Graph(to_dev(adjs, dev), V) if parts is None else ops.Graph(to_dev(adjs, dev), V, parts=parts)
        self.E = self.g.num_edges
        self.R = V * self.L
        self.tag = f"V={V} E={self.E} L={self.L}"


@pytest.fixture(scope="module")
def big(dev):
    adjs = random_graph(BIG_V, BIG_E - BIG_HUB[1], BIG_L, seed=5, hub=BIG_HUB)
    case = _Case(adjs, BIG_V, dev)
    assert case.E == BIG_E and case.R != case.E and min(case.R, case.E) > GRID_THREADS
    indeg = np.diff(case.buckets[0].astype(np.int64)).reshape(BIG_V, BIG_L)
    assert (indeg.sum(axis=1) == 0).sum() > 1000 and indeg[BIG_HUB[0], 0] >= BIG_HUB[1]
    yield case
    case.g.close()


@pytest.fixture(scope="module", params=range(len(GRAPHS)), ids=[f"V{v}-E{e}-L{l}" for v, e, l, _ in GRAPHS])
def small(request, dev):
    V, E, L, kw = GRAPHS[request.param]
    case = _Case(random_graph(V, E, L, seed=V + E, **kw), V, dev)
    yield case
    case.g.close()


def _lib_ops():
    from tf2_gnn_amd import _lib, ops

    return _lib.load(), ops


# ---- tfgnn_graph_scales ---------------------------------------------------------------------------------------------------------
def _call_graph_scales(dev, case, normalize, mode):
    lib, ops = _lib_ops()
    bufs = [guarded(n, 1, dev) for n in (case.R, case.V, case.E, case.E)]
    rc = lib.tfgnn_graph_scales(case.g._h, normalize, mode, *(ops._ptr(b) for b in bufs), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"tfgnn_graph_scales returned {rc}"
    return bufs


def _relative(entry, what, got, want):
    """every element within REL_BOUND of the fp64 value, relative; an exact 0 where the value is 0"""
    got, want = got.cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err = np.abs(got - want)
    assert not (err[want == 0] > 0).any(), f"{entry} {what}: not 0 where the value is 0"
    ratio = float((err[want != 0] / (np.abs(want[want != 0]) * REL_BOUND)).max()) if (want != 0).any() else 0.0
    print(f"{entry} {what}: max relative error / (1.01 x 4 x 2^-24) = {ratio:.3e}")
    record_parity(entry, max_error_over_bound=ratio, bound=1.0)
    assert ratio <= 1.0, f"{entry} {what}: relative error {ratio:.3f} x the bound"


def _check_graph_scales(dev, case, normalize, mode):
    _, ops = _lib_ops()
    names = ("row_scale", "node_scale", "edge_weight_by_src", "edge_weight_by_dst")
    bufs = _call_graph_scales(dev, case, normalize, mode)
    want = ref.graph_scales(case.adjs, case.V, normalize, mode, case.buckets)
    tag = f"{case.tag} normalize={normalize} mode={mode}"
    for buf, exp, name in zip(bufs, want, names):
        n = buf.shape[0] - 1
        if mode == 0:
            assert exp.dtype == np.float64
            ref.compare_equal("tfgnn_graph_scales", f"{name} {tag}", buf[:n, 0], exp.astype(np.float32))
            assert np.array_equal(exp.astype(np.float32).astype(np.float64), exp)  # (ones or fp32 values: nothing was rounded)
        else:
            _relative("tfgnn_graph_scales", f"{name} {tag}", buf[:n, 0], exp)
        guard_untouched(buf, f"graph_scales {name} {tag}")
    # ew_by_src[p] belongs to the TARGET at by-src position p - through the handle's own column array and bucket pointers, not
    # through the reference's order: the weight is (normalize ? 1 / (c[target, type] + 1e-7) : 1) * m[target]
    L = case.L
    col_s = case.g.array(ops.G_COL_BY_SRC).cpu().numpy().astype(np.int64)
    typ_s = ref.row_of_position(case.g.array(ops.G_ROWPTR_BY_SRC).cpu().numpy()) % max(L, 1)
    inv = ref.invdeg(case.buckets[0]).astype(np.float64) if normalize else np.ones(case.R)
    exp_s = inv[col_s * L + typ_s] * want[1][col_s]
    if mode == 0:
        ref.compare_equal("tfgnn_graph_scales", f"edge_weight_by_src through G_COL_BY_SRC {tag}", bufs[2][:case.E, 0], exp_s.astype(np.float32))
    else:
        _relative("tfgnn_graph_scales", f"edge_weight_by_src through G_COL_BY_SRC {tag}", bufs[2][:case.E, 0], exp_s)
    return bufs


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("normalize", [0, 1])
def test_graph_scales(dev, small, normalize, mode):
    _check_graph_scales(dev, small, normalize, mode)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("normalize", [0, 1])
def test_graph_scales_past_the_grid(dev, big, normalize, mode):
    _check_graph_scales(dev, big, normalize, mode)


def test_graph_scales_of_the_layers(dev, small):
    """layers/graph_scales.py graph_scales(): the None pattern of (False, "sum"), the handle's arrays for (True, "sum"), the
    kernel's outputs otherwise, and the cached objects on a second call"""
    _, ops = _lib_ops()
    from tf2_gnn_amd.layers.graph_scales import GraphScales, graph_scales

    g = small.g
    assert graph_scales(g, False, "sum") == GraphScales(None, None, None, None)
    assert graph_scales(g, False, "max") == GraphScales(None, None, None, None)
    s = graph_scales(g, True, "sum")
    assert s.node_scale is None
    assert s.row_scale is g.array(ops.G_INVDEG_BY_DST) and s.edge_weight_by_dst is g.array(ops.G_INVDEG_EDGE_BY_DST)
    assert s.edge_weight_by_src is g.array(ops.G_INVDEG_EDGE_BY_SRC)
    for normalize in (False, True):
        for aggregation, mode in (("mean", 1), ("sqrt_n", 2)):
            s = graph_scales(g, normalize, aggregation)
            torch.cuda.synchronize()
            row, node, ew_s, ew_d = _call_graph_scales(dev, small, int(normalize), mode)
            assert torch.equal(s.row_scale, row[:-1, 0]) and torch.equal(s.node_scale, node[:-1, 0])
            assert torch.equal(s.edge_weight_by_src, ew_s[:-1, 0])
            if normalize:
                assert torch.equal(s.edge_weight_by_dst, ew_d[:-1, 0])
            else:
                assert s.edge_weight_by_dst is None  # all ones
            again = graph_scales(g, normalize, aggregation)
            assert again is s and all(a is b for a, b in zip(again, s))
    assert graph_scales(g, True, "sum") is graph_scales(g, True, "sum")


# ---- tfgnn_graph_target_multiplier ----------------------------------------------------------------------------------------------
def _check_target_multiplier(dev, case, row_scale):
    """row_scale: None or a device tensor [R]"""
    lib, ops = _lib_ops()
    R = case.R
    k = guarded(R, 1, dev)
    ident, node_of_row = guarded(R + 1, 1, dev, dtype=torch.int32), guarded(R, 1, dev, dtype=torch.int32)
    rc = lib.tfgnn_graph_target_multiplier(case.g._h, ops._ptr(row_scale), ops._ptr(k), ops._ptr(ident), ops._ptr(node_of_row),
                                           ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"tfgnn_graph_target_multiplier returned {rc}"
    want_k, want_ident, want_node = ref.target_multiplier(case.buckets[0], None if row_scale is None else row_scale.cpu().numpy(), case.L)
    tag = f"{case.tag} row_scale={'NULL' if row_scale is None else 'given'}"
    ref.compare_equal("tfgnn_graph_target_multiplier", f"k {tag}", k[:R, 0], want_k)  # one fp32 product: the same bits
    ref.compare_equal("tfgnn_graph_target_multiplier", f"ident_ptr {tag}", ident[:R + 1, 0], want_ident)
    ref.compare_equal("tfgnn_graph_target_multiplier", f"node_of_row {tag}", node_of_row[:R, 0], want_node)
    for buf, what in ((k, "k"), (ident, "ident_ptr"), (node_of_row, "node_of_row")):
        guard_untouched(buf, f"target_multiplier {what} {tag}")


def _row_scales(dev, case):
    """None, and the device's own row scales of (normalize, sqrt_n) and of (no normalize, mean)"""
    yield None
    for normalize, mode in ((1, 2), (0, 1)):
        yield _call_graph_scales(dev, case, normalize, mode)[0][:-1, 0].contiguous()


def test_target_multiplier(dev, small):
    for row_scale in _row_scales(dev, small):
        _check_target_multiplier(dev, small, row_scale)


def test_target_multiplier_past_the_grid(dev, big):
    assert big.R + 1 > GRID_THREADS
    for row_scale in _row_scales(dev, big):
        _check_target_multiplier(dev, big, row_scale)


def test_target_multiplier_without_rows(dev):
    """R = 0 (no edge types): only ident_ptr[0] = 0 is written"""
    lib, ops = _lib_ops()
    g = ops.Graph([], 5, parts=0)
    k, node_of_row = guarded(3, 1, dev), guarded(3, 1, dev, dtype=torch.int32)
    ident = guarded(1, 1, dev, dtype=torch.int32)
    for kp, np_ in ((ops._ptr(k), ops._ptr(node_of_row)), (None, None)):
        ident[0, 0] = 77
        assert lib.tfgnn_graph_target_multiplier(g._h, None, kp, ops._ptr(ident), np_, ops._stream()) == 0
        torch.cuda.synchronize()
        assert int(ident[0, 0]) == 0
        guard_untouched(ident, "target_multiplier ident_ptr at R = 0")
        untouched(k, "k at R = 0")
        untouched(node_of_row, "node_of_row at R = 0")
    g.close()


# ---- the derived arrays of the handle -------------------------------------------------------------------------------------------
def _check_derived(case):
    _, ops = _lib_ops()
    from oracle import adjacency_oracle as ao

    g, V, L = case.g, case.V, case.L
    by_src, by_dst, target, pattern = ref.per_edge_derived(case.adjs, V, case.buckets)
    ref.compare_equal("graph arrays", f"G_INVDEG_EDGE_BY_SRC {case.tag}", g.array(ops.G_INVDEG_EDGE_BY_SRC), by_src)
    ref.compare_equal("graph arrays", f"G_INVDEG_EDGE_BY_DST {case.tag}", g.array(ops.G_INVDEG_EDGE_BY_DST), by_dst)
    ref.compare_equal("graph arrays", f"G_TARGET_BY_DST {case.tag}", g.array(ops.G_TARGET_BY_DST), target)
    # nodes ordered by the emptiness pattern of their by-SOURCE buckets: the order inside a pattern is free, the sequence of
    # patterns and the tile masks are not (the assertions tests/test_gpu_graph.py makes for the by-target side)
    node_at = g.array(ops.G_PATTERN_NODE_BY_SRC).cpu().numpy()
    tmask = g.array(ops.G_PATTERN_TILEMASK_BY_SRC).cpu().numpy()
    assert g.parts & ops.G_PART_DST_PATTERN
    if L > 8:
        assert node_at.size == 0 and tmask.size == 0
        return
    rp_s = g.array(ops.G_ROWPTR_BY_SRC).cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(rp_s, case.buckets[1])
    np.testing.assert_array_equal(np.sort(node_at), np.arange(V))
    seq = pattern[node_at]
    popcount = np.array([bin(m).count("1") for m in range(256)])
    key = (8 - popcount[seq]) * 256 + seq
    assert np.all(np.diff(key) >= 0), f"{case.tag}: by-source patterns out of order"  # many non-empty buckets first, equal patterns adjacent
    assert tmask.dtype == np.uint8 and tmask.shape[0] == -(-V // 128)
    np.testing.assert_array_equal(tmask, ao.tile_masks(seq))
    # the by-target side of the same handle, against the oracle's own pattern function
    node_d = g.array(ops.G_PATTERN_NODE_BY_DST).cpu().numpy()
    seq_d = ao.bucket_emptiness_patterns(case.adjs, V)[node_d]
    assert np.all(np.diff(ao.pattern_order_key(seq_d)) >= 0)
    np.testing.assert_array_equal(g.array(ops.G_PATTERN_TILEMASK_BY_DST).cpu().numpy(), ao.tile_masks(seq_d))


def test_derived_arrays(small):
    _check_derived(small)


def test_derived_arrays_past_the_grid(big):
    _check_derived(big)


def test_derived_arrays_with_more_than_eight_types(dev):
    case = _Case(random_graph(40, 360, 9, seed=9), 40, dev)
    _check_derived(case)
    case.g.close()
