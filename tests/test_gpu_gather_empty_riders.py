"""Empty (node, type) buckets of the planned graph gather (csrc/spmm.hip gather_rows_block, EmptyRiders): in the plain-sum
walks with two-edge rounds (widths 256 - 384 here) an empty short row has no lane group of its own any more; the group of
non-empty slot i of the length-ordered list also writes the zero rows of the empty slots i + n_ne, i + 2 n_ne, ..  What is
stored for an empty bucket must be what a group of its own stored: zero sums times the row's scale through the same epilogue.
Width 64 (rounds of eight edges), the max reduce (MODE_GENERAL) and the compact views keep one group per row / no row.

Graphs (L = 4, V = 200 - 300): type l has the buckets (v, l), v < m_l, with d_l edges each, from the sources (v + 1 + j) mod m_l,
so the by-target and the by-source typed views have the same m_l non-empty buckets of d_l edges per type.  Every graph but the
empty one also holds HUB_EDGES copies of one self-loop per hub bucket: a long row in both views (items, no short row), which
puts the edge count above 1.5 edges per walked row - below that the dispatch (spmm.hip graph_gather_impl, kMultiAvgLen) sends
the short rows two to a lane group through gather_rows_block_multi, which this change leaves alone.

The reference is the host restatement of the parent's arithmetic (fp32, rows added one at a time in the handle's CSR order,
long rows in the order of the plan as in tests/test_gpu_gather_index_blocks.py; one multiplication by the row scale) and, for
SP16 output, tests/sp16_reference.encode of it.  Every output row - inverse scales included - must be equal bit for bit; where
both sides hold a NaN (an empty row with a scale of inf or NaN: 0 * inf) the payloads are not compared, the host's and the
device's default NaNs differ in sign.  Outputs are pre-filled with 0xFF bytes (an fp32 / fp16 NaN that no producer writes), so
a row nobody wrote shows, and have a guard band of rows behind the last one that must stay untouched."""
import numpy as np
import pytest
import torch

from tests import gather_reference as gr
from tests import sp16_reference as sp
from tests.helpers import to_dev

pytestmark = pytest.mark.gpu

L = 4
HUB_EDGES = 2500
TYPED_THRESHOLD, ITEM_EDGES = 48, 512  # graph.hpp: LONG_ROW_THRESHOLD_TYPED, ITEM_CHUNK_TYPED
WIDTHS = (64, 256, 320, 384)
ROUND_EDGES = {64: 8, 256: 2, 320: 2, 384: 2}    # spmm.hip gather_dispatch
ITEM_GROUPS = {64: 16, 256: 16, 320: 16, 384: 8}  # 256 threads / lanes per row (32 lanes above 320 floats)
GUARD_ROWS = 8
FULL_VIEWS = (gr.VIEW_BY_DST_TYPED_PATTERN, gr.VIEW_BY_SRC_TYPED)
COMPACT_VIEWS = (gr.VIEW_BY_DST_TYPED_COMPACT, gr.VIEW_BY_SRC_TYPED_COMPACT)

# name -> (V, m_l, d_l, hub buckets): n_ne = non-empty short rows, empties = 4 V - hubs - long buckets - n_ne
GRAPHS = {
    "none-empty": (200, (200, 200, 200, 199), (3, 1, 2, 5), 1),       # no empty bucket at all: the parent's launch
    "fewer-empties": (300, (300, 60, 300, 150), (3, 50, 2, 7), 1),    # n_ne 750, 60 long buckets, 389 empties
    "as-many": (300, (300, 299, 0, 0), (4, 9, 0, 0), 2),              # n_ne 599 = empties
    "3.5-times": (295, (100, 100, 62, 0), (1, 2, 16, 0), 1),          # n_ne 262, 917 empties: the rider loop runs 3 and 4 times
    "n_ne-1": (200, (1, 0, 0, 0), (1, 0, 0, 0), 1),                   # one lane group writes 798 zero rows
    "n_ne-15": (200, (15, 0, 0, 0), (3, 0, 0, 0), 1),                 # the workgroup edges at 16 lane groups
    "n_ne-16": (200, (16, 0, 0, 0), (3, 0, 0, 0), 1),
    "n_ne-17": (200, (17, 0, 0, 0), (3, 0, 0, 0), 1),
    "all-empty": (200, (0, 0, 0, 0), (0, 0, 0, 0), 0),                # no edge: the parent's path
    "all-long": (200, (64, 0, 0, 0), (60, 0, 0, 0), 1),               # items only, no row workgroup to host a rider
}
COUNTS = {"none-empty": (799, 0), "fewer-empties": (750, 389), "as-many": (599, 599), "3.5-times": (262, 917), "n_ne-1": (1, 798),
          "n_ne-15": (15, 784), "n_ne-16": (16, 783), "n_ne-17": (17, 782), "all-empty": (0, 800), "all-long": (0, 735)}


def adjacency_lists(name):
    V, m, d, hubs = GRAPHS[name]
    rng = np.random.default_rng(len(name) + V)
    lists = []
    for l in range(L):
        v = np.repeat(np.arange(m[l]), d[l])
        j = np.tile(np.arange(d[l]), m[l])
        a = np.stack([(v + 1 + j) % max(m[l], 1), v], axis=1)
        if l >= L - hubs:  # the hub buckets (V - 1, 3), (V - 1, 2): m_l <= V - 1 there
            assert m[l] <= V - 1
            a = np.concatenate([a, np.full((HUB_EDGES, 2), V - 1)], axis=0)
        rng.shuffle(a, axis=0)
        lists.append(a.astype(np.int32).reshape(-1, 2))
    return lists


def restate(rowptr, col, X, width):
    """fp32 row sums [CSR rows, width] in the order of the plan"""
    R = rowptr.shape[0] - 1
    lens = np.diff(rowptr)
    out = np.zeros((R, width), dtype=np.float32)
    short = lens <= TYPED_THRESHOLD
    for j in range(int(lens[short].max()) if short.any() else 0):  # a short row: one running sum, edge by edge
        rows = np.flatnonzero(short & (lens > j))
        out[rows] = out[rows] + X[col[rowptr[rows] + j]]

    def run(part):
        acc = np.zeros(width, dtype=np.float32)
        for r in part:
            acc = acc + r
        return acc

    groups, round_edges = ITEM_GROUPS[width], ROUND_EDGES[width]
    for r in np.flatnonzero(~short):  # items of 512 edges, an item's edges dealt to the lane groups in runs, sums in group / item order
        rows32 = X[col[rowptr[r]:rowptr[r + 1]]]
        total = None
        for i0 in range(0, rows32.shape[0], ITEM_EDGES):
            item = rows32[i0:i0 + ITEM_EDGES]
            per = -(-item.shape[0] // groups)
            per = -(-per // round_edges) * round_edges
            s = run(item[:per])
            for g in range(1, groups):
                s = s + run(item[g * per:(g + 1) * per])
            total = s if total is None else total + s
        out[r] = total
    return out


def same_bits(got, want):
    """equal bit for bit, or a NaN on both sides"""
    bits = {2: np.uint16, 4: np.uint32}[got.dtype.itemsize]
    return (np.ascontiguousarray(got).view(bits) == np.ascontiguousarray(want).view(bits)) | (np.isnan(got) & np.isnan(want))


def assert_same(got, want, lens, what):
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    diff = ~same_bits(got, want)
    if diff.any():
        idx = np.argwhere(diff)[0]
        r = int(idx[0])
        raise AssertionError(f"{what}: output row {r} ({int(lens[r])} edges) at {tuple(int(i) for i in idx[1:])} is {got[tuple(idx)]!r}, the "
                             f"restatement gives {want[tuple(idx)]!r} ({np.unique(np.argwhere(diff)[:, 0]).size} rows differ)")


class _Graph:
    def __init__(self, name, dev):
        from tf2_gnn_amd import ops

        self.name, self.dev = name, dev
        self.V = GRAPHS[name][0]
        self.lists = adjacency_lists(name)
        self.graph = ops.Graph(to_dev(self.lists, dev), self.V, parts=ops.G_PARTS_ALL)
        g = self.graph
        host = lambda a: g.array(a).cpu().numpy().astype(np.int64)
        by_dst, by_src = (host(ops.G_ROWPTR_BY_DST), host(ops.G_COL_BY_DST)), (host(ops.G_ROWPTR_BY_SRC), host(ops.G_COL_BY_SRC))
        self.csr = {gr.VIEW_BY_DST_TYPED_PATTERN: by_dst, gr.VIEW_BY_DST_TYPED_COMPACT: by_dst, gr.VIEW_BY_SRC_TYPED: by_src,
                    gr.VIEW_BY_SRC_TYPED_COMPACT: by_src}
        pos = g.array(ops.G_PATTERN_POS_BY_DST).cpu().numpy()
        self.hosted = {v: gr.view_rows(self.lists, self.V, v, pattern_pos=pos) for v in self.csr}
        self.out_rows = {v: np.arange(self.V * L) if self.hosted[v][2] is None else self.hosted[v][2] for v in self.csr}
        self._inputs, self._sums = {}, {}

    def inputs(self, view, width):
        """(X [V, width], row scales [V * L]) as fp32 numpy arrays and on the device"""
        key = (view in (gr.VIEW_BY_SRC_TYPED, gr.VIEW_BY_SRC_TYPED_COMPACT), width)
        if key not in self._inputs:
            rng = np.random.default_rng(7 * width + key[0])
            X = rng.standard_normal((self.V, width)).astype(np.float32)
            rs = (rng.random(self.V * L) * 0.7 + 0.3).astype(np.float32)
            self._inputs[key] = (X, rs, torch.from_numpy(X).to(self.dev), torch.from_numpy(rs).to(self.dev))
        return self._inputs[key]

    def lens(self, view):
        return np.diff(self.csr[view][0])

    def sums(self, view, width):
        """the unscaled restatement in CSR rows (shared by the full and the compact view of a direction)"""
        key = (view in (gr.VIEW_BY_SRC_TYPED, gr.VIEW_BY_SRC_TYPED_COMPACT), width)
        if key not in self._sums:
            rowptr, col = self.csr[view]
            self._sums[key] = restate(rowptr, col, self.inputs(view, width)[0], width)
        return self._sums[key]

    def expected(self, view, width, rs):
        """(restatement in output rows, edges per output row); rs: fp32 [CSR rows] or None"""
        out = self.sums(view, width)
        if rs is not None:
            with np.errstate(invalid="ignore"):
                out = out * rs[:, None]
        rows = self.out_rows[view]
        return out[rows], self.lens(view)[rows]

    def num_edges(self):
        return sum(a.shape[0] for a in self.lists)

    def run_fp32(self, view, width, n_rows, weights, rs_dev, reduce="sum"):
        """-> (rows [n_rows, width], guard band [GUARD_ROWS, width] as bytes)"""
        from tf2_gnn_amd import ops

        X = self.inputs(view, width)[2]
        buf = torch.full((n_rows + GUARD_ROWS, width * 4), 0xFF, dtype=torch.uint8, device=self.dev).view(torch.float32)
        ew = torch.ones(self.num_edges(), device=self.dev) if weights else None
        ops.graph_gather(self.graph, view, X, edge_weight=ew, row_scale=rs_dev, out=buf[:n_rows],
                         reduce=ops.REDUCE_MAX if reduce == "max" else ops.REDUCE_SUM)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        return got[:n_rows], got[n_rows:].view(np.uint8)

    def run_sp(self, view, width, n_rows, weights, rs_dev):
        """tfgnn_graph_gather_reduce_sp into pre-filled buffers of this test (ops.graph_gather_sp allocates its own)
        -> (h, l [n_rows, width], inv [n_rows], guard bytes of the data, guard bytes of the scales)"""
        from tf2_gnn_amd import _lib, ops

        lib = _lib.load()
        X = self.inputs(view, width)[2]
        data = torch.full((n_rows + GUARD_ROWS, width * 4), 0xFF, dtype=torch.uint8, device=self.dev)
        inv = torch.full((n_rows + GUARD_ROWS, 4), 0xFF, dtype=torch.uint8, device=self.dev).view(torch.float32).reshape(-1)
        ew = torch.ones(self.num_edges(), device=self.dev) if weights else None
        self.graph.ensure(ops._VIEW_PARTS[view])
        ws_bytes = lib.tfgnn_graph_gather_workspace_bytes(self.graph._h, view, width)
        ws = ops._workspace(self.dev, ws_bytes) if ws_bytes else None
        _lib.check(lib.tfgnn_graph_gather_reduce_sp(self.graph._h, view, None, ops._ptr(ew), ops._ptr(rs_dev), ops._ptr(X), width, width,
                                                    ops._ptr(data), width * 4, ops._ptr(inv), None, ops._ptr(ws),
                                                    ws.numel() if ws is not None else 0, ops._stream()))
        torch.cuda.synchronize()
        data, inv = data.cpu().numpy(), inv.cpu().numpy()
        h, l = sp.unpack(data[:n_rows], width)
        return h, l, inv[:n_rows], data[n_rows:], inv[n_rows:].view(np.uint8)


_graphs = {}


@pytest.fixture
def graph_of(dev):
    def get(name):
        if name not in _graphs:
            _graphs[name] = _Graph(name, dev)
        return _graphs[name]

    return get


def check_call(g, view, width, out, weights, rs_host, rs_dev, what):
    want, lens = g.expected(view, width, rs_host)
    n_rows = want.shape[0]
    if out == "fp32":
        got, guard = g.run_fp32(view, width, n_rows, weights, rs_dev)
        assert_same(got, want, lens, what)
        assert np.all(guard == 0xFF), f"{what}: the rows behind the last output row were written"
        return
    h, l, inv, guard, guard_inv = g.run_sp(view, width, n_rows, weights, rs_dev)
    wh, wl, winv = sp.encode(want, width)
    assert_same(inv, winv[:, 0], lens, what + " inverse scale")
    assert_same(h, wh, lens, what + " h")
    assert_same(l, wl, lens, what + " l")
    assert np.all(guard == 0xFF) and np.all(guard_inv == 0xFF), f"{what}: the rows behind the last output row were written"


@pytest.mark.parametrize("name", list(GRAPHS))
def test_graphs_hold_the_planned_buckets(graph_of, name):
    g = graph_of(name)
    V, m, d, hubs = GRAPHS[name]
    assert g.num_edges() == 0 or g.num_edges() > 1.5 * V * L, "the short rows would go two to a lane group"
    for view in FULL_VIEWS:
        assert all(np.array_equal(a, b) for a, b in zip(g.csr[view], g.hosted[view][:2])), "the handle's CSR is not the host's bucketing"
        lens = g.lens(view)
        short = lens <= TYPED_THRESHOLD
        assert (int((short & (lens > 0)).sum()), int((lens == 0).sum())) == COUNTS[name]
        assert int((~short).sum()) == hubs + sum(m[l] for l in range(L) if d[l] > TYPED_THRESHOLD)
    assert np.array_equal(np.sort(g.out_rows[gr.VIEW_BY_DST_TYPED_PATTERN]), np.arange(V * L))


@pytest.mark.parametrize("out", ["fp32", "sp"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("view", FULL_VIEWS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_every_row_is_the_restatement_bit_for_bit(graph_of, name, view, width, out):
    g = graph_of(name)
    _, rs, _, rs_dev = g.inputs(view, width)
    for weights in (False, True):
        for scaled in (False, True):
            check_call(g, view, width, out, weights, rs if scaled else None, rs_dev if scaled else None,
                       f"{name} view {view} width {width} {out} unit-weights={weights} row-scale={scaled}")


@pytest.mark.parametrize("out", ["fp32", "sp"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("view", FULL_VIEWS + COMPACT_VIEWS)
@pytest.mark.parametrize("name", ["fewer-empties", "3.5-times", "n_ne-17"])
def test_scales_of_inf_nan_and_zero_on_empty_rows(graph_of, name, view, width, out):
    """0 * inf and 0 * NaN still show in the row of an empty bucket (and its inverse scale is 1), 0 * 0 is the all-zero row"""
    g = graph_of(name)
    rs = g.inputs(view, width)[1].copy()
    empty = np.flatnonzero(g.lens(view) == 0)
    rs[empty[0::4]] = np.inf
    rs[empty[1::4]] = np.nan
    rs[empty[2::4]] = 0.0
    check_call(g, view, width, out, False, rs, torch.from_numpy(rs).to(g.dev), f"{name} view {view} width {width} {out} special scales")
    if view in FULL_VIEWS and out == "fp32":
        got, _ = g.run_fp32(view, width, g.V * L, False, torch.from_numpy(rs).to(g.dev))
        assert int(np.isnan(got).all(axis=1).sum()) == empty[0::4].size + empty[1::4].size


@pytest.mark.parametrize("out", ["fp32", "sp"])
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("view", COMPACT_VIEWS)
@pytest.mark.parametrize("name", ["none-empty", "fewer-empties", "as-many", "3.5-times", "n_ne-16", "all-long"])
def test_compact_views_have_no_row_for_an_empty_bucket(graph_of, name, view, width, out):
    g = graph_of(name)
    _, rs, _, rs_dev = g.inputs(view, width)
    want, lens = g.expected(view, width, rs)
    assert want.shape[0] == int((g.lens(view) > 0).sum()) and np.all(lens > 0)
    assert want.shape[0] == g.graph.nonempty_offsets(view == gr.VIEW_BY_SRC_TYPED_COMPACT)[-1]
    for scaled in (False, True):
        check_call(g, view, width, out, False, rs if scaled else None, rs_dev if scaled else None,
                   f"{name} compact view {view} width {width} {out} row-scale={scaled}")


@pytest.mark.parametrize("width", [64, 320])
@pytest.mark.parametrize("view", FULL_VIEWS)
@pytest.mark.parametrize("name", ["fewer-empties", "3.5-times", "n_ne-1", "all-empty"])
def test_max_reduce_keeps_the_lowest_float_in_empty_rows(graph_of, name, view, width):
    """MODE_GENERAL: one lane group per row as before; the maximum of fp32 values is exact, an empty row is not scaled"""
    g = graph_of(name)
    X, rs, _, rs_dev = g.inputs(view, width)
    rowptr, col = g.csr[view]
    want = np.full((g.V * L, width), gr.FLOAT_LOWEST, dtype=np.float32)
    for r in np.flatnonzero(np.diff(rowptr) > 0):
        want[r] = X[col[rowptr[r]:rowptr[r + 1]]].max(axis=0) * rs[r]
    rows = g.out_rows[view]
    got, guard = g.run_fp32(view, width, g.V * L, False, rs_dev, reduce="max")
    assert_same(got, want[rows], g.lens(view)[rows], f"{name} view {view} width {width} max")
    assert np.all(guard == 0xFF)
