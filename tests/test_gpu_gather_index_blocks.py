"""The planned graph gather's edge walk (csrc/spmm.hip accumulate_edges, EdgeBlocks) at every row length at which it changes
shape: a lane group reads its column indices and edge weights in blocks of LPR = 16 consecutive edges, one edge per lane, and
hands them round inside the group; the plain-sum walk does not load rows past the end of its run.  The variants that walk
two edges per round do so (widths 256 and 320 here); widths 64 and 128 and the max reduce keep one index load per edge and
must give the same sums.

One graph (V = 200, L = 3, type 2 without edges, in the style of tools/record_gather_bits.py) puts in- and out-degrees of
type 0 at
  0, 1, 2, 3        the opening of a row, odd and even lengths (rounds of two edges: a masked second edge)
  15, 16, 17        one index block / two
  31, 32, 33        two blocks / three; 32 is also the node views' long-row threshold (and a block of a 32-lane variant)
  47, 48            the last short typed rows (three blocks)
  49                one item: 16 lane groups with runs of 4, 4, .., 1, 0 edges at two edges per round
  300               one item whose lane groups walk 20 (24 at width 64) edges each: an index block ends inside a run
  513               two items; the second holds one edge, most runs are empty
The hubs' other ends are drawn from the plain nodes, which so get rows of about seven edges; type 1 holds 200 random edges.

Checks (bounds from the arithmetic and the project's precedent, none from the code under test):
  plain sums, no weights or weights of 1.0, with and without a row scale
      fp32 output: byte-equal to a host restatement in fp32 - rows added one at a time in the handle's CSR order, in the
      order of the plan (graph.hpp; a row up to the threshold: one running sum; a longer row: items of 512 edges, an item's
      edges dealt to 16 lane groups in runs of ceil(n / 16) rounded up to the round length, the runs' sums added in group
      order, the items' sums in item order), one multiplication by the row scale at the end.  Exact whatever the compiler
      contracts: 1.0f * x + acc has one rounding either way.
      SP16 output: tests/sp16_reference.encode of that same host result, byte-equal.
  random weights + row scale (fp32 and SP16 output), and one max case (MODE_GENERAL)
      against tests/gather_reference.gather_reference in fp64 with the bounds of tests/test_gpu_graph_gather.py
      (sums 2e-6 * l1, max 2^-22 relative) and tests/test_gpu_graph_gather_sp.py (+ the format's bound)."""
import numpy as np
import pytest
import torch

from tests import gather_reference as gr
from tests import sp16_reference as sp
from tests.helpers import record_parity, to_dev

pytestmark = pytest.mark.gpu

NUM_NODES = 200
LENGTHS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 300, 513)
HUB_TARGETS = tuple(range(0, len(LENGTHS)))    # in-degree LENGTHS[i] in type 0
HUB_SOURCES = tuple(range(20, 20 + len(LENGTHS)))  # out-degree LENGTHS[i] in type 0
FIRST_PLAIN_NODE = 40
VIEWS = (gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_TYPED_PATTERN, gr.VIEW_BY_SRC_TYPED, gr.VIEW_BY_DST_NODE)
WIDTHS = (64, 128, 256, 320)
# the plan (graph.hpp) and the dispatch (spmm.hip gather_dispatch) as documented: 16 lanes per row at these widths
TYPED_THRESHOLD, NODE_THRESHOLD, ITEM_EDGES, ITEM_GROUPS = 48, 32, 512, 16
ROUND_EDGES = {64: 8, 128: 4, 256: 2, 320: 2}
SUM_TOL = 2e-6       # tests/test_gpu_graph_gather.py
MAX_TOL = 2.0 ** -22  # tests/test_gpu_graph_gather.py: two fp32 roundings (w * x, * row_scale)


def adjacency_lists():
    rng = np.random.default_rng(4612)
    plain = lambda n: rng.integers(FIRST_PLAIN_NODE, NUM_NODES, size=n)
    src, tgt = [], []
    for node, deg in zip(HUB_TARGETS, LENGTHS):
        src.append(plain(deg))
        tgt.append(np.full(deg, node))
    for node, deg in zip(HUB_SOURCES, LENGTHS):
        src.append(np.full(deg, node))
        tgt.append(plain(deg))
    a0 = np.stack([np.concatenate(src), np.concatenate(tgt)], axis=1)
    rng.shuffle(a0, axis=0)
    a1 = np.stack([plain(200), plain(200)], axis=1)
    return [a0.astype(np.int32), a1.astype(np.int32), np.zeros((0, 2), dtype=np.int32)]


def planned_row_sum(rows32, threshold, round_edges):
    """fp32 sum of the rows of one CSR row in the order of the plan (module docstring)"""
    n, width = rows32.shape

    def run(part):
        acc = np.zeros(width, dtype=np.float32)
        for r in part:
            acc = acc + r
        return acc

    if n <= threshold:
        return run(rows32)
    total = None
    for i0 in range(0, n, ITEM_EDGES):
        item = rows32[i0:i0 + ITEM_EDGES]
        per = -(-item.shape[0] // ITEM_GROUPS)
        per = -(-per // round_edges) * round_edges
        s = run(item[:per])
        for g in range(1, ITEM_GROUPS):
            s = s + run(item[g * per:(g + 1) * per])
        total = s if total is None else total + s
    return total


class _Case:
    def __init__(self, dev):
        from tf2_gnn_amd import ops

        self.dev = dev
        self.lists = adjacency_lists()
        self.graph = ops.Graph(to_dev(self.lists, dev), NUM_NODES, parts=ops.G_PARTS_ALL)
        g = self.graph
        host = lambda a: g.array(a).cpu().numpy().astype(np.int64)
        # the handle's own CSR arrays: the order the exact restatement follows
        self.csr = {
            gr.VIEW_BY_DST_TYPED: (host(ops.G_ROWPTR_BY_DST), host(ops.G_COL_BY_DST)),
            gr.VIEW_BY_SRC_TYPED: (host(ops.G_ROWPTR_BY_SRC), host(ops.G_COL_BY_SRC)),
            gr.VIEW_BY_DST_NODE: (host(ops.G_NODEPTR_BY_DST), host(ops.G_COLL_BY_DST)),
        }
        self.csr[gr.VIEW_BY_DST_TYPED_PATTERN] = self.csr[gr.VIEW_BY_DST_TYPED]
        pos = g.array(ops.G_PATTERN_POS_BY_DST).cpu().numpy()
        self.out_rows = {v: gr.view_rows(self.lists, NUM_NODES, v, pattern_pos=pos)[2] for v in VIEWS}
        self.hosted = {v: gr.view_rows(self.lists, NUM_NODES, v, pattern_pos=pos)[:2] for v in VIEWS}
        self._inputs, self._exact, self._refs, self._dev_inputs = {}, {}, {}, {}

    def inputs(self, view, width):
        """(X [input rows, width], edge weights [E], row scales [CSR rows]) as fp32 numpy arrays"""
        key = (view, width)
        if key not in self._inputs:
            rowptr, col = self.csr[view]
            rng = np.random.default_rng(1000 * view + width)
            node = view == gr.VIEW_BY_DST_NODE
            X = rng.standard_normal((NUM_NODES * (len(self.lists) if node else 1), width)).astype(np.float32)
            ew = (rng.random(col.shape[0]) + 0.5).astype(np.float32)
            rs = (rng.random(rowptr.shape[0] - 1) * 0.7 + 0.3).astype(np.float32)
            self._inputs[key] = (X, ew, rs)
            self._dev_inputs[key] = tuple(torch.from_numpy(a).to(self.dev) for a in (X, ew, rs))
        return self._inputs[key]

    def dev_inputs(self, view, width):
        self.inputs(view, width)
        return self._dev_inputs[view, width]

    def in_output_rows(self, view, a):
        rows = self.out_rows[view]
        return a if rows is None else a[rows]

    def lengths(self, view):
        return self.in_output_rows(view, np.diff(self.csr[view][0]))

    def exact(self, view, width, scaled):
        """the host restatement, fp32 [output rows, width]"""
        key = (view, width, scaled)
        if key not in self._exact:
            rowptr, col = self.csr[view]
            X, _, rs = self.inputs(view, width)
            threshold = NODE_THRESHOLD if view == gr.VIEW_BY_DST_NODE else TYPED_THRESHOLD
            out = np.zeros((rowptr.shape[0] - 1, width), dtype=np.float32)
            for r in range(out.shape[0]):
                if rowptr[r + 1] > rowptr[r]:
                    out[r] = planned_row_sum(X[col[rowptr[r]:rowptr[r + 1]]], threshold, ROUND_EDGES[width])
            if scaled:
                out = out * rs[:, None]
            self._exact[key] = self.in_output_rows(view, out)
        return self._exact[key]

    def reference(self, view, width, reduce):
        """fp64 (out, l1) of the weighted and scaled call, in output rows, from the host's own bucketing of the edge lists"""
        key = (view, width, reduce)
        if key not in self._refs:
            rowptr, col = self.hosted[view]
            X, ew, rs = self.inputs(view, width)
            out, l1, _ = gr.gather_reference(rowptr, col, torch.from_numpy(X), edge_weight=torch.from_numpy(ew),
                                             row_scale=torch.from_numpy(rs), reduce=reduce)
            self._refs[key] = (self.in_output_rows(view, out.numpy()), self.in_output_rows(view, l1.numpy()))
        return self._refs[key]

    def run(self, view, width, out, weights, scaled, reduce="sum"):
        """one gather -> fp32 numpy rows, or (h, l, inv) of an SP16 result"""
        from tf2_gnn_amd import ops

        X, ew, rs = self.dev_inputs(view, width)
        if weights == "ones":
            ew = torch.ones_like(ew)
        kw = dict(edge_weight=ew if weights else None, row_scale=rs if scaled else None)
        if out == "sp":
            op = ops.graph_gather_sp(self.graph, view, X, **kw)
            torch.cuda.synchronize()
            h, l = sp.unpack(op.data.cpu().numpy(), width)
            return h, l, op.inv_scale.cpu().numpy().reshape(-1)
        res = ops.graph_gather(self.graph, view, X, reduce=ops.REDUCE_MAX if reduce == "max" else ops.REDUCE_SUM, **kw)
        torch.cuda.synchronize()
        return res.cpu().numpy()


@pytest.fixture(scope="module")
def case(dev):
    return _Case(dev)


def test_graph_has_the_planned_rows(case):
    n = len(LENGTHS)
    for view in (gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_SRC_TYPED):
        hubs = HUB_SOURCES if view == gr.VIEW_BY_SRC_TYPED else HUB_TARGETS
        for rowptr, col in (case.csr[view], case.hosted[view]):
            lens = np.diff(rowptr).reshape(NUM_NODES, 3)
            assert tuple(lens[list(hubs), 0]) == LENGTHS
            assert int(lens[:, 2].sum()) == 0 and int(lens[:FIRST_PLAIN_NODE, 1].sum()) == 0
            assert int(lens[FIRST_PLAIN_NODE:, 0].max()) <= TYPED_THRESHOLD  # the plain nodes' rows are short rows
    deg = np.diff(case.csr[gr.VIEW_BY_DST_NODE][0])
    assert tuple(deg[:n]) == LENGTHS
    assert case.csr[gr.VIEW_BY_DST_NODE][1].shape[0] == 2 * sum(LENGTHS) + 200
    # the handle's arrays are the host's own bucketing of the lists (columns ascending inside a bucket)
    for view in VIEWS:
        assert all(np.array_equal(a, b) for a, b in zip(case.csr[view], case.hosted[view])), f"view {view}"
    # the pattern view writes every bucket; its rows are a permutation of the typed view's
    assert np.array_equal(np.sort(case.out_rows[gr.VIEW_BY_DST_TYPED_PATTERN]), np.arange(NUM_NODES * 3))


def _first_difference(got, want, lens, what):
    diff = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if diff.any():
        r, c = np.argwhere(diff)[0]
        raise AssertionError(f"{what}: output row {r} ({int(lens[r])} edges), column {c} is {got[r, c]!r}, the restatement gives "
                             f"{want[r, c]!r} ({int(diff.sum())} entries in {np.unique(np.argwhere(diff)[:, 0]).size} rows differ)")


@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "row-scale"])
@pytest.mark.parametrize("weights", [None, "ones"], ids=["no-weights", "unit-weights"])
@pytest.mark.parametrize("out", ["fp32", "sp"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("view", VIEWS)
def test_plain_sums_are_the_restatement_bit_for_bit(case, view, width, out, weights, scaled):
    what = f"view {view} width {width} {out} weights={weights} scaled={scaled}"
    want = case.exact(view, width, scaled)
    lens = case.lengths(view)
    if out == "fp32":
        got = case.run(view, width, out, weights, scaled)
        assert got.shape == want.shape
        _first_difference(got.view(np.uint32), want.view(np.uint32), lens, what)
        return
    h, l, inv = case.run(view, width, out, weights, scaled)
    wh, wl, winv = sp.encode(want, width)
    bad = np.flatnonzero(inv != winv[:, 0])
    assert bad.size == 0, f"{what}: inverse scale of output row {bad[0]} ({int(lens[bad[0]])} edges) is {inv[bad[0]]}, not {winv[bad[0], 0]}"
    _first_difference(h.view(np.uint16), np.ascontiguousarray(wh).view(np.uint16), lens, what + " h")
    _first_difference(l.view(np.uint16), np.ascontiguousarray(wl).view(np.uint16), lens, what + " l")


@pytest.mark.parametrize("out", ["fp32", "sp"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("view", VIEWS)
def test_weighted_sums_against_fp64(case, view, width, out):
    what = f"view {view} width {width} {out} weighted"
    ref, l1 = case.reference(view, width, "sum")
    lens = case.lengths(view)
    if out == "fp32":
        got = case.run(view, width, out, "random", True).astype(np.float64)
        bound = SUM_TOL * l1
    else:
        h, l, inv = case.run(view, width, out, "random", True)
        got = sp.decode(h, l, inv, width)
        bound = SUM_TOL * l1 + sp.format_bound(ref, sp.blockmax(ref, width))
    assert got.shape == ref.shape and np.all(np.isfinite(got))
    assert np.all(got[lens == 0] == 0), f"{what}: a row without edges is not exactly zero"
    err = np.abs(got - ref)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max())
    record_parity("graph_gather index blocks weighted", max_error_to_bound=worst, bound=1.0)
    print(f"{what}: worst error / bound {worst:.3e}")
    if worst > 1.0:
        r, c = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{what}: error {err[r, c]:.3e} is {worst:.3e} of its bound at output row {r} ({int(lens[r])} edges), column {c}")


@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_weighted_max_against_fp64(case, view):
    """MODE_GENERAL: the walk that keeps its own index and weight loads"""
    width = 64
    ref, _ = case.reference(view, width, "max")
    got = case.run(view, width, "fp32", "random", True, reduce="max").astype(np.float64)
    empty = ref == gr.FLOAT_LOWEST
    assert np.array_equal(empty.all(axis=1), case.lengths(view) == 0)
    assert np.array_equal(got[empty], ref[empty]), "an empty max row is not the lowest float"
    err = np.abs(got - ref)[~empty] / np.abs(ref)[~empty]
    worst = float(err.max())
    record_parity("graph_gather index blocks max", max_relative_error=worst, bound=MAX_TOL)
    print(f"view {view} max: worst relative error {worst:.3e}")
    assert worst <= MAX_TOL, f"view {view}: max relative error {worst:.3e} > 2^-22"
