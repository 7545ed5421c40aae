"""Graph-owned gather operands (ops.Graph.gather_operand, tfgnn_graph_gather_reduce_sp_keep_empty, agg_filled / g_filled of the
layer-level calls): which (node, type) buckets are empty depends on the graph, so only the first gather into the pair a graph
keeps per (view, width, stream) writes their zero rows and marker scales; later gathers launch over the non-empty buckets only.

Graphs as in tests/test_gpu_gather_empty_riders.py (L = 4, V = 200 - 300, the same buckets in both directions, one long
self-loop bucket per graph so that the edge count stays above 1.5 edges per walked row) plus one molecule-like graph below
that, whose short rows go two to a lane group (gather_rows_block_multi).  The reference is the host restatement of the
gather's arithmetic (fp32, a short row one edge at a time in CSR order, a long row in the order of the plan) and
tests/sp16_reference.encode of it; a second reference is the library's own filling gather into a fresh buffer.  Buffers are
pre-filled with 0xFF bytes (an fp16 / fp32 NaN no producer writes) and have a guard band behind the last row.  Everything is
compared byte for byte: no tolerance is involved."""
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
WIDTHS = (64, 128, 320, 384)
ROUND_EDGES = {64: 8, 128: 4, 320: 2, 384: 2}    # spmm.hip gather_dispatch: edges per round of the SP16 variants
ITEM_GROUPS = {64: 16, 128: 16, 320: 16, 384: 8}  # 256 threads / lanes per row (32 lanes above 320 floats)
GUARD_ROWS = 8
FORWARD_VIEWS = (gr.VIEW_BY_DST_TYPED_PATTERN, gr.VIEW_BY_DST_TYPED)
FULL_VIEWS = FORWARD_VIEWS + (gr.VIEW_BY_SRC_TYPED,)
PATTERN = 0xA5

# name -> (V, m_l, d_l, hub buckets): type l has the buckets (v, l), v < m_l, with d_l edges each from the sources
# (v + 1 + j) mod m_l; n_ne = non-empty short rows
GRAPHS = {
    "none-empty": (200, (200, 200, 200, 199), (3, 1, 2, 5), 1),     # no empty bucket: a request changes nothing
    "fewer-empties": (300, (300, 60, 300, 150), (3, 50, 2, 7), 1),  # n_ne 750, 60 long buckets, 389 empties
    "as-many": (300, (300, 299, 0, 0), (4, 9, 0, 0), 2),            # n_ne 599 = empties
    "3.5-times": (295, (100, 100, 62, 0), (1, 2, 16, 0), 1),        # n_ne 262, 917 empties
    "n_ne-1": (200, (1, 0, 0, 0), (1, 0, 0, 0), 1),
    "n_ne-15": (200, (15, 0, 0, 0), (3, 0, 0, 0), 1),               # the workgroup edges at 16 lane groups
    "n_ne-16": (200, (16, 0, 0, 0), (3, 0, 0, 0), 1),
    "n_ne-17": (200, (17, 0, 0, 0), (3, 0, 0, 0), 1),
    "all-empty": (200, (0, 0, 0, 0), (0, 0, 0, 0), 0),              # no edge at all: a keeping gather launches nothing
    "all-long": (200, (64, 0, 0, 0), (60, 0, 0, 0), 1),             # items only: a keeping gather has no row workgroup
    "molecule": (240, (200, 150, 0, 100), (1, 1, 0, 2), 0),         # 550 edges in 960 buckets: two short rows per lane group
}
COUNTS = {"none-empty": (799, 0), "fewer-empties": (750, 389), "as-many": (599, 599), "3.5-times": (262, 917), "n_ne-1": (1, 798),
          "n_ne-15": (15, 784), "n_ne-16": (16, 783), "n_ne-17": (17, 782), "all-empty": (0, 800), "all-long": (0, 735),
          "molecule": (450, 510)}


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


def first_difference(got, want, what):
    diff = np.argwhere(got != want)
    assert diff.size == 0, (f"{what}: byte {tuple(int(i) for i in diff[0])} is {got[tuple(diff[0])]:#x}, expected {want[tuple(diff[0])]:#x} "
                            f"({np.unique(diff[:, 0]).size} rows differ)")


class _Graph:
    def __init__(self, name, dev):
        from tf2_gnn_amd import ops

        self.name, self.dev = name, dev
        self.V = GRAPHS[name][0]
        self.lists = adjacency_lists(name)
        self.graph = ops.Graph(to_dev(self.lists, dev), self.V, parts=ops.G_PARTS_ALL)
        pos = self.graph.array(ops.G_PATTERN_POS_BY_DST).cpu().numpy()
        self.hosted = {v: gr.view_rows(self.lists, self.V, v, pattern_pos=pos) for v in FULL_VIEWS + (gr.VIEW_BY_DST_TYPED_COMPACT,)}
        self._inputs, self._want = {}, {}

    def inputs(self, by_src, width, which):
        """input `which` (0: the first gather's, 1: the one under test): (X [V, width], row scales [V * L]), host and device"""
        key = (by_src, width, which)
        if key not in self._inputs:
            rng = np.random.default_rng(7 * width + by_src + 1000 * which)
            X = rng.standard_normal((self.V, width)).astype(np.float32)
            rs = (rng.random(self.V * L) * 0.7 + 0.3).astype(np.float32)
            self._inputs[key] = (X, rs, torch.from_numpy(X).to(self.dev), torch.from_numpy(rs).to(self.dev))
        return self._inputs[key]

    def lens(self, view):
        """edges per OUTPUT row"""
        rowptr, _, out_rows = self.hosted[view]
        lens = np.diff(rowptr)
        return lens if out_rows is None else lens[out_rows]

    def want(self, view, width, scaled):
        """the expected operand of input 1: (packed data bytes [rows, 4 width], inverse scales [rows])"""
        by_src = view == gr.VIEW_BY_SRC_TYPED
        key = (view, width, scaled)
        if key not in self._want:
            rowptr, col, out_rows = self.hosted[view]
            skey = ("sums", by_src, width)
            if skey not in self._want:
                self._want[skey] = restate(rowptr, col, self.inputs(by_src, width, 1)[0], width)
            out = self._want[skey]
            if scaled:
                out = out * self.inputs(by_src, width, 1)[1][:, None]
            if out_rows is not None:
                out = out[out_rows]
            h, l, inv = sp.encode(out, width)
            self._want[key] = (sp.pack(h, l), inv[:, 0].copy())
        return self._want[key]

    # ---- the pair under test: the graph's own, placed in buffers with a guard band -------------------------------------------
    def install_pair(self, view, width, fill=0xFF):
        """-> (pair, whole data buffer, whole scale buffer as bytes): a fresh, never-filled pair of the graph for (view, width)
        whose arrays are the leading rows of buffers filled with `fill`"""
        from tf2_gnn_amd import ops

        compact = view == gr.VIEW_BY_DST_TYPED_COMPACT
        rows = int(self.graph.nonempty_offsets(False)[-1]) if compact else self.V
        per = 1 if compact else L
        data = torch.full((rows + GUARD_ROWS, per * width * 4), fill, dtype=torch.uint8, device=self.dev)
        inv = torch.full((rows + GUARD_ROWS, per * 4), fill, dtype=torch.uint8, device=self.dev)
        pair = ops._GatherOperand(data[:rows], inv.view(torch.float32)[:rows])
        self.graph._gather_operands[(int(view), int(width), ops._stream())] = pair
        return pair, data, inv

    def gather(self, view, width, which, scaled):
        """ops.graph_gather_sp_owned of input `which` into the graph's pair (the row scales are those of input 1 either way: a
        stack's layers share them)"""
        from tf2_gnn_amd import ops

        by_src = view == gr.VIEW_BY_SRC_TYPED
        X, rs = self.inputs(by_src, width, which)[2], self.inputs(by_src, width, 1)[3]
        return ops.graph_gather_sp_owned(self.graph, view, X, row_scale=rs if scaled else None)

    def fresh(self, view, width, scaled):
        """the library's filling gather of input 1 into fresh 0xFF buffers -> (data bytes, scale bytes) with their guard rows"""
        from tf2_gnn_amd import _lib, ops

        lib = _lib.load()
        _, _, X, rs = self.inputs(view == gr.VIEW_BY_SRC_TYPED, width, 1)
        rows = self.V * L
        data = torch.full((rows + GUARD_ROWS * L, width * 4), 0xFF, dtype=torch.uint8, device=self.dev)
        inv = torch.full((rows + GUARD_ROWS * L, 4), 0xFF, dtype=torch.uint8, device=self.dev)
        ws_bytes = lib.tfgnn_graph_gather_workspace_bytes(self.graph._h, view, width)
        ws = ops._workspace(self.dev, ws_bytes) if ws_bytes else None
        _lib.check(lib.tfgnn_graph_gather_reduce_sp(self.graph._h, view, None, None, ops._ptr(rs) if scaled else None, ops._ptr(X), width,
                                                    width, ops._ptr(data), width * 4, ops._ptr(inv), None, ops._ptr(ws),
                                                    ws.numel() if ws is not None else 0, ops._stream()))
        torch.cuda.synchronize()
        return data.cpu().numpy(), inv.cpu().numpy()


_graphs = {}


@pytest.fixture
def graph_of(dev):
    def get(name):
        if name not in _graphs:
            _graphs[name] = _Graph(name, dev)
        return _graphs[name]

    return get


def rows_of(buf, n_rows, width_bytes):
    """a [V + guard, L * bytes] buffer as (output rows [n_rows, bytes], guard bytes)"""
    flat = buf.reshape(-1, width_bytes)
    return flat[:n_rows], flat[n_rows:]


def check_written(g, view, width, scaled, data, inv, what, skip_rows=None):
    """every output row (but `skip_rows`) and its scale equal the restatement; the guard band is untouched"""
    compact = view == gr.VIEW_BY_DST_TYPED_COMPACT
    n_rows = data.shape[0] - GUARD_ROWS if compact else g.V * L
    want_data, want_inv = g.want(view, width, scaled)
    got, guard = rows_of(data.cpu().numpy(), n_rows, width * 4)
    got_inv, guard_inv = rows_of(inv.cpu().numpy(), n_rows, 4)
    keep = np.ones(n_rows, dtype=bool)
    if skip_rows is not None:
        keep[skip_rows] = False
    first_difference(got[keep], want_data[keep], what + " data")
    first_difference(got_inv[keep], want_inv.view(np.uint8).reshape(-1, 4)[keep], what + " inverse scales")
    assert np.all(guard == 0xFF) and np.all(guard_inv == 0xFF), f"{what}: the rows behind the last output row were written"
    return got, got_inv


@pytest.mark.parametrize("name", list(GRAPHS))
def test_graphs_hold_the_planned_buckets(graph_of, name):
    g = graph_of(name)
    V = g.V
    multi = name == "molecule"
    E = sum(a.shape[0] for a in g.lists)
    assert E == 0 or (E <= 1.5 * V * L) == multi, "the short rows would take the other walk"
    for view in FULL_VIEWS:
        lens = np.diff(g.hosted[view][0])
        short = lens <= TYPED_THRESHOLD
        assert (int((short & (lens > 0)).sum()), int((lens == 0).sum())) == COUNTS[name]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_a_keeping_gather_leaves_the_operand_a_filling_gather_writes(graph_of, name, width):
    """1. Bits: two gathers into one graph-owned pair with different inputs; after the second, every byte of the operand and
    every scale - the empty buckets' included - is what a filling gather of the second input writes into a fresh buffer, and
    what sp16_reference.encode gives for the host restatement"""
    g = graph_of(name)
    for view in FULL_VIEWS:
        for scaled in (False, True):
            what = f"{name} view {view} width {width} row-scale={scaled}"
            pair, data, inv = g.install_pair(view, width)
            g.gather(view, width, 0, scaled)
            assert pair.filled is not None
            g.gather(view, width, 1, scaled)
            torch.cuda.synchronize()
            got, got_inv = check_written(g, view, width, scaled, data, inv, what)
            fresh_data, fresh_inv = g.fresh(view, width, scaled)
            first_difference(data.cpu().numpy().reshape(-1, width * 4), fresh_data, what + " against a fresh filling gather")
            first_difference(inv.cpu().numpy().reshape(-1, 4), fresh_inv, what + " scales against a fresh filling gather")


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", list(GRAPHS))
def test_the_empty_rows_are_left_alone(graph_of, name, width):
    """2. After the first gather the empty buckets' rows and scales are overwritten from the host (behind the library's back);
    a second gather of the same description must leave that pattern where it is and write every other row"""
    g = graph_of(name)
    for view in FULL_VIEWS:
        for scaled in (False, True):
            what = f"{name} view {view} width {width} row-scale={scaled}"
            pair, data, inv = g.install_pair(view, width)
            g.gather(view, width, 0, scaled)
            torch.cuda.synchronize()
            empty = np.flatnonzero(g.lens(view) == 0)
            assert empty.size == COUNTS[name][1]
            rows_d, rows_i = data[:g.V].view(g.V * L, width * 4), inv[:g.V].view(g.V * L, 4)
            idx = torch.from_numpy(empty).to(g.dev)
            rows_d[idx] = PATTERN
            rows_i[idx] = PATTERN
            g.gather(view, width, 1, scaled)
            torch.cuda.synchronize()
            got, got_inv = check_written(g, view, width, scaled, data, inv, what, skip_rows=empty)
            assert np.all(got[empty] == PATTERN) and np.all(got_inv[empty] == PATTERN), f"{what}: an empty bucket's row was written"


def refill(data, inv):
    data.fill_(0xFF)
    inv.fill_(0xFF)


@pytest.mark.parametrize("name", ["fewer-empties", "3.5-times", "molecule"])
def test_what_does_not_match_the_record_writes_every_row(graph_of, name):
    """3. Fallbacks, each into a pair whose bytes are 0xFF again: a first use; another width; another row_scale tensor; the
    same tensor modified in place; a compact view"""
    g = graph_of(name)
    view, width = gr.VIEW_BY_SRC_TYPED, 320
    # a request on a first use
    pair, data, inv = g.install_pair(view, width)
    assert pair.filled is None and pair.begin(None) is False
    g.gather(view, width, 1, True)
    check_written(g, view, width, True, data, inv, f"{name}: first use")
    # another width: another pair, which is on its first use
    other, data_o, inv_o = g.install_pair(view, 128)
    g.gather(view, 128, 1, True)
    check_written(g, view, 128, True, data_o, inv_o, f"{name}: another width")
    assert pair.filled is not None  # (the first pair keeps its record)
    # another row_scale tensor with the same values
    _, rs_host, X, rs = g.inputs(True, width, 1)
    from tf2_gnn_amd import ops

    refill(data, inv)
    ops.graph_gather_sp_owned(g.graph, view, X, row_scale=rs.clone())
    check_written(g, view, width, True, data, inv, f"{name}: another row_scale tensor")
    # the same tensor modified in place (the values are put back first: the reference is the one of `rs`)
    mine = rs.clone()
    ops.graph_gather_sp_owned(g.graph, view, X, row_scale=mine)
    refill(data, inv)
    mine.mul_(2.0).mul_(0.5)
    ops.graph_gather_sp_owned(g.graph, view, X, row_scale=mine)
    check_written(g, view, width, True, data, inv, f"{name}: row_scale modified in place")
    # ... and the control: nothing changed, the empty rows stay 0xFF
    refill(data, inv)
    ops.graph_gather_sp_owned(g.graph, view, X, row_scale=mine)
    torch.cuda.synchronize()
    empty = np.flatnonzero(g.lens(view) == 0)
    got, _ = check_written(g, view, width, True, data, inv, f"{name}: control", skip_rows=empty)
    assert np.all(got[empty] == 0xFF)
    # a call that fails leaves the pair unfilled: the record is taken away before the call and set again behind it
    assert pair.filled is not None
    with pytest.raises(Exception):
        ops.graph_gather_sp_owned(g.graph, view, X, row_scale=mine, edge_weight=torch.ones(3))  # not a device tensor
    assert pair.filled is None
    ops.graph_gather_sp_owned(g.graph, view, X, row_scale=mine)
    assert pair.filled is not None
    # a compact view has no empty row: a second gather writes all of it
    cview = gr.VIEW_BY_DST_TYPED_COMPACT
    _, _, Xd, rsd = g.inputs(False, width, 1)
    pair_c, data_c, inv_c = g.install_pair(cview, width)
    ops.graph_gather_sp_owned(g.graph, cview, Xd, row_scale=rsd)
    refill(data_c, inv_c)
    ops.graph_gather_sp_owned(g.graph, cview, Xd, row_scale=rsd)
    check_written(g, cview, width, True, data_c, inv_c, f"{name}: compact view")


def test_a_view_without_empty_rows_is_written_in_full(graph_of):
    g = graph_of("none-empty")
    for view in FULL_VIEWS:
        pair, data, inv = g.install_pair(view, 320)
        g.gather(view, 320, 0, True)
        refill(data, inv)
        g.gather(view, 320, 1, True)
        check_written(g, view, 320, True, data, inv, f"none-empty view {view}")


# ---- 4. the layer-level calls --------------------------------------------------------------------------------------------------
def layer_calls(g, H, pattern, fresh):
    """four mp_forward and four mp_backward calls in a row on one graph, as a four-layer stack makes them
    -> every out, split result, dX and dW as byte tensors.  fresh: the graph's pairs are dropped before every call"""
    from tf2_gnn_amd import ops

    graph, V, dev = g.graph, g.V, g.dev
    gen = torch.Generator().manual_seed(H + pattern)
    Ws = [(torch.randn((L, H, H), generator=gen) / np.sqrt(L * H)).to(dev) for _ in range(4)]
    x = torch.randn((V, H), generator=gen).to(dev)
    d = torch.randn((V, H), generator=gen).to(dev)
    rs = torch.from_numpy(g.inputs(False, 320, 1)[1]).to(dev)
    view = ops.VIEW_BY_DST_TYPED_PATTERN if pattern else ops.VIEW_BY_DST_TYPED
    fwd = dict(tile_kmask=graph.array(ops.G_PATTERN_TILEMASK_BY_DST), row_map=graph.array(ops.G_PATTERN_NODE_BY_DST)) if pattern else {}
    node_by_src = graph.array(ops.G_PATTERN_NODE_BY_SRC)
    skip = dict(tile_kmask=graph.array(ops.G_PATTERN_TILEMASK_BY_SRC), a_rows=node_by_src, row_map=node_by_src) if pattern else None
    results, xs = [], []
    ops.clear_weight_operand_cache()
    graph.release_gather_operands()
    for W in Ws:
        if fresh:
            graph.release_gather_operands()
        xs.append(ops.sp_split_rows(x))
        out, op = ops.mp_forward(graph, view, x, W, row_scale=rs, act="relu", want_split=True, **fwd)
        results += [out.view(torch.uint8).clone(), op.data.clone(), op.inv_scale.view(torch.uint8).clone()]
        x = out
    for W, x_sp in zip(reversed(Ws), reversed(xs)):
        if fresh:
            graph.release_gather_operands()
        dX, _, dW = ops.mp_backward(graph, d, W, x_sp, skip=skip)
        results += [dX.view(torch.uint8).clone(), dW.view(torch.uint8).clone()]
        d = dX
    torch.cuda.synchronize()
    if not fresh:
        filled = [p.filled is not None for p in graph._gather_operands.values()]
        assert len(filled) == 2 and all(filled)  # one pair per direction, both filled
    return results


@pytest.mark.parametrize("pattern", [0, 1])
@pytest.mark.parametrize("H", [128, 320])
@pytest.mark.parametrize("name", ["fewer-empties", "3.5-times", "molecule"])
def test_layer_calls_on_one_graph_equal_the_calls_on_fresh_operands(graph_of, name, H, pattern):
    g = graph_of(name)
    kept = layer_calls(g, H, pattern, fresh=False)
    fresh = layer_calls(g, H, pattern, fresh=True)
    assert len(kept) == len(fresh) == 4 * 3 + 4 * 2
    for i, (a, b) in enumerate(zip(kept, fresh)):
        assert torch.equal(a, b), f"{name} H {H} pattern {pattern}: result {i} differs"
    g.graph.release_gather_operands()


def test_training_step_eager_captured_and_replayed(dev):
    """a 2-layer RGCN training step at H = 320: eager, captured and replayed twice, byte-equal"""
    from bench import model_params
    from tf2_gnn_amd import CapturedStep, ops
    from tf2_gnn_amd.layers import GNN, GNNInput
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tests.helpers import random_graph

    V, E, H = 1200, 9000, 320  # 4 800 buckets, most of them empty
    gen = torch.Generator().manual_seed(7)
    X = torch.randn((V, H), generator=gen).to(dev)
    dOut = torch.randn((V, H), generator=gen).to(dev)
    adj = to_dev(random_graph(V, E, L, seed=11, hub=(5, 300)), dev)
    set_seed(13)
    params = model_params("rgcn", H, 2)
    params["layer_input_dropout_rate"] = 0.0
    gnn = GNN(params)
    inp = GNNInput(X, adj, torch.zeros(V, dtype=torch.int32, device=dev), 1)

    def step():
        out = gnn(inp, training=True)
        dX = gnn.backward(dOut, need_input_grad=True)
        return out, dX, [v.grad for v in gnn.trainable_variables]

    def snapshot(res):
        torch.cuda.synchronize()
        return [res[0].clone(), res[1].clone()] + [t.clone() for t in res[2]]

    eager = snapshot(step())
    cap = CapturedStep(step)
    cap.capture()  # (records the launches; the replays run them)
    runs = [snapshot(cap.replay()), snapshot(cap.replay()), snapshot(step())]
    assert ops.get_gemm_mode() == ops.GEMM_F16X2
    for k, run in enumerate(runs):
        assert len(run) == len(eager)
        for i, (a, b) in enumerate(zip(run, eager)):
            assert torch.equal(a, b), f"run {k} (replay, replay, eager again), tensor {i}"


# ---- 5. lifetime -----------------------------------------------------------------------------------------------------------------
def test_close_releases_the_pairs_and_a_later_graph_is_served(dev):
    from tf2_gnn_amd import ops

    def layer_call(g):
        H = 128
        gen = torch.Generator().manual_seed(5)
        W = (torch.randn((L, H, H), generator=gen) / 16).to(dev)
        x = torch.randn((g.V, H), generator=gen).to(dev)
        ops.clear_weight_operand_cache()
        out, _ = ops.mp_forward(g.graph, ops.VIEW_BY_DST_TYPED, x, W)
        dX, _, _ = ops.mp_backward(g.graph, out, W, None, need_weight_grad=False)
        torch.cuda.synchronize()

    warm = _Graph("fewer-empties", dev)  # workspaces and other first-use allocations of the process
    layer_call(warm)
    warm.graph.close()
    g = _Graph("3.5-times", dev)
    ops.clear_weight_operand_cache()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    layer_call(g)
    assert len(g.graph._gather_operands) == 2
    pair_bytes = sum(p.data.numel() + 4 * p.inv_scale.numel() for p in g.graph._gather_operands.values())
    ops.clear_weight_operand_cache()
    assert torch.cuda.memory_allocated() >= before + pair_bytes
    g.graph.close()
    assert g.graph._gather_operands == {}
    assert torch.cuda.memory_allocated() == before
    # a second graph of another shape, created afterwards: case 1 on it
    g2 = _Graph("as-many", dev)
    for view in FULL_VIEWS:
        pair, data, inv = g2.install_pair(view, 320)
        g2.gather(view, 320, 0, True)
        g2.gather(view, 320, 1, True)
        check_written(g2, view, 320, True, data, inv, f"second graph view {view}")
    g2.graph.close()
