"""The planned graph gather with per-head weights that also writes one inner product per edge and head (csrc/spmm.hip
tfgnn_graph_gather_reduce_dot, MODE_HEADS_DOT, ``ops.graph_gather_dot``: RGAT's backward pass) on the planned graphs of
tests/test_gpu_graph_gather.py, in the four plain views: short rows at both sides of the threshold, whole-row items, rows of two
and three items.

The calls go to the C entry with buffers of the test's own - sums and products are filled with a sentinel first and carry one
guard row - and ``ops.graph_gather_dot`` is held to the same bits.

  sums      bit-equal to ``ops.graph_gather`` with the same [E, K] weights (pinned to fp64 by test_per_head_weights), and
            within that test's bound of the fp64 reference: 2e-6 of the row's l1 mass
  products  per edge e and head k:  |dot - ref| <= 4e-7 * sum_f |in[col(e), f]| * |dot_rows[row(e), f]|  over the head's
            columns, ref in fp64 from the host arrays of gather_reference.view_rows (the factor of
            test_edge_products_riding_on_the_by_source_gather); the worst ratio is reported per row length
  mapping   product (e, k) stands at dot_pos[e] * K + k (None: e), every slot is written, nothing else is"""
import numpy as np
import pytest
import torch

from tests import gather_reference as gr
from tests.helpers import record_parity
from tests.test_gpu_graph_gather import NUM_NODES, PARTIAL_SLOTS, SENTINEL, Spec, _Case, _check

pytestmark = pytest.mark.gpu

PLAIN_VIEWS = (gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE, gr.VIEW_BY_SRC_TYPED, gr.VIEW_BY_SRC_NODE)
# every head-to-lane shape tfgnn_graph_gather_dot_supported admits: 8-lane groups (32, 2); one float4 per head (64, 16);
# 8 lanes per head on 16 x 1 (64, 2); the split reduction on 16 x 2 (128, 8) and 16 x 4 (256, 8); 16 lanes per head on 16 x 5
# (320, 5); 32-lane groups (512, 8)
SHAPES = ((32, 2), (64, 16), (64, 2), (128, 8), (256, 8), (320, 5), (512, 8))
UNSUPPORTED = ((96, 8), (256, 2), (64, 1))  # heads of 12 floats, a head of 128 floats, one head
DOT_TOL = 4e-7


@pytest.fixture(scope="module")
def case(dev):
    return _Case(dev)


def _path(case, view, n):
    """the work unit that takes a row of ``n`` edges (graph.hpp: typed threshold 48, node threshold 32, 512-edge items)"""
    threshold = 32 if _Case.kind(view) == "node" else 48
    if n <= threshold:
        return "short row"
    items = -(-n // 512)
    return "whole-row item" if items == 1 else f"{items} items"


def _operands(case, view, width, heads):
    """(X, ew [E, K], dot_rows [rows, width]) as CPU tensors"""
    X, ew, _ = case.inputs(view, width, heads)
    rowptr = case.host(view)[0]
    Y = torch.randn((rowptr.shape[0] - 1, width), generator=torch.Generator().manual_seed(31 * view + width + heads))
    return X, ew, Y


def _positions(case, view, kind):
    """dot_pos of the call as a host array (None: the view's own order)"""
    from tf2_gnn_amd import ops

    E = case.num_edges(view)
    if kind == "none":
        return None
    if kind == "perm":
        return np.random.default_rng(1000 + view).permutation(E).astype(np.int32)
    pos = case.handle(view).array(ops.G_SRC2DST_POS).cpu().numpy()
    assert pos.shape == (E,) and np.array_equal(np.sort(pos), np.arange(E)), "the edge map is not a permutation"
    return pos


def _call(case, view, width, heads, X, ew, Y, pos):
    """tfgnn_graph_gather_reduce_dot on sentinel-filled, guarded buffers -> (rc, sums [rows + 1, width], products [E + 1, K])"""
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    g = case.handle(view)
    g.wait()
    g.ensure(ops._VIEW_PARTS[view])
    rows, E = case.num_out_rows(view), case.num_edges(view)
    sums = torch.full((rows + 1, width), SENTINEL, dtype=torch.float32, device=case.dev)
    dots = torch.full((E + 1, heads), SENTINEL, dtype=torch.float32, device=case.dev)
    ws = torch.full((PARTIAL_SLOTS + 1, width), SENTINEL, dtype=torch.float32, device=case.dev)
    nbytes = int(lib.tfgnn_graph_gather_workspace_bytes(g._h, view, width))
    assert nbytes == PARTIAL_SLOTS * width * 4
    Xd, ewd, Yd = X.to(case.dev), ew.to(case.dev), Y.to(case.dev)
    posd = None if pos is None else torch.from_numpy(pos).to(case.dev)
    rc = lib.tfgnn_graph_gather_reduce_dot(g._h, view, ops._ptr(ewd), heads, ops._ptr(Xd), Xd.stride(0), width, ops._ptr(sums), width,
                                           ops._ptr(Yd), Yd.stride(0), ops._ptr(posd), ops._ptr(dots), ops._ptr(ws), nbytes,
                                           ops._stream())
    torch.cuda.synchronize()
    assert bool((ws[-1] == SENTINEL).all()), "the row behind the partial slots was written"
    return rc, sums, dots


# dot_pos: none, a fixed random permutation of the edges and, where the view is by source, the handle's by-source to by-target map
VIEW_POSITIONS = [(v, k) for v in PLAIN_VIEWS for k in ("none", "perm") + (("src2dst",) if _Case.by_src(v) else ())]


@pytest.mark.parametrize("width,heads", SHAPES)
@pytest.mark.parametrize("view,pos_kind", VIEW_POSITIONS)
def test_sums_products_and_mapping(case, view, width, heads, pos_kind):
    from tf2_gnn_amd import _lib, ops

    assert ops.graph_gather_dot_supported(width, heads)
    what = f"view {view} width {width} heads {heads} dot_pos {pos_kind}"
    X, ew, Y = _operands(case, view, width, heads)
    pos = _positions(case, view, pos_kind)
    rc, sums, dots = _call(case, view, width, heads, X, ew, Y, pos)
    assert rc == 0, _lib.load().tfgnn_last_error().decode()
    rows, E = case.num_out_rows(view), case.num_edges(view)
    assert bool((sums[-1] == SENTINEL).all()), f"{what}: the guard row behind the sums was written"
    assert bool((dots[-1] == SENTINEL).all()), f"{what}: the guard row behind the products was written"
    # sums: the per-head weighted gather, bit for bit, and its fp64 bound
    spec = Spec(ew=heads)
    assert torch.equal(sums[:-1].cpu(), case.run(view, width, spec)), f"{what}: the sums differ from ops.graph_gather"
    ref, l1 = case.reference(view, width, spec)
    _check(sums[:-1].cpu(), ref, l1, spec, what, "graph_gather_dot sums")
    # mapping: every slot written, product (e, k) at pos[e]
    got = dots[:-1].cpu().numpy()
    unwritten = np.flatnonzero((got == SENTINEL).any(axis=1))
    assert unwritten.size == 0, f"{what}: {unwritten.size} product rows were never written, the first one at position {unwritten[0]}"
    if pos is not None:
        got = got[pos]
    # products against fp64, edge by edge
    rowptr, col, _ = case.host(view)
    lens = np.diff(rowptr)
    row_of_edge = np.repeat(np.arange(rows), lens)
    terms = X.double().numpy()[col] * Y.double().numpy()[row_of_edge]
    want = terms.reshape(E, heads, width // heads).sum(axis=2)
    mag = np.abs(terms).reshape(E, heads, width // heads).sum(axis=2)
    ratio = np.abs(got.astype(np.float64) - want) / (DOT_TOL * mag)
    worst_of = {}
    for n in sorted(set(int(x) for x in lens if x)):
        worst_of[n] = float(ratio[lens[row_of_edge] == n].max())
    print(f"{what}: worst error / bound per row length: " + ", ".join(f"{n}: {w:.2f}" for n, w in worst_of.items()))
    worst = float(ratio.max())
    record_parity("graph_gather_dot products", max_error_to_bound=worst, bound=1.0)
    if worst > 1.0:
        e, k = np.unravel_index(int(ratio.argmax()), ratio.shape)
        r = int(row_of_edge[e])
        over = {n: round(w, 2) for n, w in worst_of.items() if w > 1.0}
        raise AssertionError(f"{what}: product of edge {e} (edge {e - int(rowptr[r])} of row {r}, {int(lens[r])} edges: "
                             f"{_path(case, view, int(lens[r]))}), head {k} is {got[e, k]!r}, fp64 {want[e, k]!r}: {worst:.3e} of its "
                             f"bound; row lengths over the bound: {over}")


@pytest.mark.parametrize("view", PLAIN_VIEWS)
def test_wrapper_returns_the_bits_of_the_c_entry(case, view):
    from tf2_gnn_amd import ops

    width, heads = 256, 8
    X, ew, Y = _operands(case, view, width, heads)
    for pos in (None, _positions(case, view, "perm")):
        rc, sums, dots = _call(case, view, width, heads, X, ew, Y, pos)
        assert rc == 0
        posd = None if pos is None else torch.from_numpy(pos).to(case.dev)
        s2, d2 = ops.graph_gather_dot(case.handle(view), view, X.to(case.dev), edge_weight=ew.to(case.dev), dot_rows=Y.to(case.dev),
                                      dot_pos=posd)
        assert torch.equal(s2, sums[:-1]) and torch.equal(d2, dots[:-1])
    for bad in (gr.VIEW_BY_DST_TYPED_COMPACT, gr.VIEW_BY_SRC_TYPED_COMPACT, gr.VIEW_BY_DST_TYPED_PATTERN):
        with pytest.raises(ValueError):
            ops.graph_gather_dot(case.handle(bad), bad, X.to(case.dev), edge_weight=ew.to(case.dev), dot_rows=Y.to(case.dev))


@pytest.mark.parametrize("width,heads", UNSUPPORTED)
def test_unsupported_head_shapes_are_refused(case, width, heads):
    """heads of 12 floats, a head wider than 64 floats and a single head: refused by the query, by the wrapper and by the C
    entry, which writes nothing"""
    from tf2_gnn_amd import _lib, ops

    assert not ops.graph_gather_dot_supported(width, heads)
    view = gr.VIEW_BY_SRC_TYPED
    E = case.num_edges(view)
    gen = torch.Generator().manual_seed(width + heads)
    X, Y = torch.randn((NUM_NODES, width), generator=gen), torch.randn((case.num_out_rows(view), width), generator=gen)
    ew = torch.rand((E, heads), generator=gen)
    rc, sums, dots = _call(case, view, width, heads, X, ew, Y, None)
    assert rc != 0, "an unsupported head shape was accepted"
    message = _lib.load().tfgnn_last_error().decode()
    assert "per-head edge weights only" in message if heads == 1 else "unsupported head width" in message, message
    assert bool((sums == SENTINEL).all()) and bool((dots == SENTINEL).all()), "a refused call wrote to its outputs"
    with pytest.raises(ValueError):
        ops.graph_gather_dot(case.handle(view), view, X.to(case.dev), edge_weight=ew.to(case.dev), dot_rows=Y.to(case.dev))
