"""The planned graph gather (csrc/spmm.hip tfgnn_graph_gather_reduce, ``ops.graph_gather``) and the backward pass through a
general aggregation (csrc/edge.hip tfgnn_edge_aggregate_backward) against the fp64 references of tests/gather_reference.py.

Two graphs put every work unit of the long-row plan (graph.hpp: typed threshold 48, node threshold 32, 512-edge items) on
known rows: short rows at both sides of the threshold, whole-row items (49 edges: the last lane groups get empty slices),
rows of two and three items whose last item holds one edge (513, 1025), and the combine pass.  The by-source views run on
a second handle built from the same lists with the columns swapped, so they see the same row lengths.

Bounds (from arithmetic and the project's precedent, not from the code under test):
  sums                    |out - ref| <= 2e-6 * l1, l1 = sum |terms| * max(1, |row_scale|)   (test_gather_reduce_matches_oracle;
                          a strictly sequential fp32 sum over these rows stays at 2.1e-7 * l1, one dropped or doubled edge
                          of the 1100-edge row is ~1e-3 * l1)
  max, no activation      two fp32 roundings (w * x, * row_scale): |out - ref| <= 2^-22 * |ref|; empty rows are the lowest float
  with pre / post act     max: 2e-6 * max(1, |ref|); sums: 2e-6 * l1 + 2e-6 * max(1, |ref|)   (the device activations' tolerance
                          in tests/test_gpu_ops.py)
  backward                5e-6 * max(1, |ref|)   (the activation-backward tolerance of tests/test_gpu_ops.py)"""
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from oracle import adjacency_oracle as ao
from tests import gather_reference as gr
from tests.helpers import assert_close, record_parity, to_dev

pytestmark = pytest.mark.gpu

TYPED_LENGTHS = (0, 1, 2, 3, 47, 48, 49, 64, 511, 512, 513, 1024, 1025, 1100)
NODE_DEGREES = (0, 1, 2, 3, 31, 32, 33, 64, 511, 512, 513, 1024, 1025, 1100)
NUM_NODES = 1300
PARTIAL_SLOTS = 10  # 513 -> 2, 1024 -> 2, 1025 -> 3, 1100 -> 3
SENTINEL = -12345.5
ACTS = ["relu", "tanh", "leaky_relu", "elu", "selu", "gelu", "sigmoid"]
ALL_VIEWS = tuple(range(7))
DISPATCH_WIDTHS = (7, 70, 8, 32, 64, 96, 128, 256, 320, 1280, 384, 512, 1024)
SUM_TOL = 2e-6
MAX_TOL = 2.0 ** -22
ACT_TOL = 2e-6
BWD_TOL = 5e-6


@dataclass(frozen=True)
class Spec:
    """one form of the call: ew = 0 (no edge weights), 1 ([E]) or K > 1 ([E, K])"""
    ew: int = 0
    rs: bool = False
    reduce: str = "sum"
    pre: str = None
    post: str = None


PLAIN = Spec()
WEIGHTED = Spec(ew=1, rs=True, post="relu")


def _typed_lists(rng):
    """L = 3: bucket (i, 0) holds TYPED_LENGTHS[i] edges, bucket (i, 1) two edges for even i, type 2 is empty"""
    tgt = np.repeat(np.arange(len(TYPED_LENGTHS)), TYPED_LENGTHS)
    a0 = np.stack([rng.integers(0, NUM_NODES, size=tgt.size), tgt], axis=1)
    tgt1 = np.repeat(np.arange(0, len(TYPED_LENGTHS), 2), 2)
    a1 = np.stack([rng.integers(0, NUM_NODES, size=tgt1.size), tgt1], axis=1)
    rng.shuffle(a0, axis=0)
    rng.shuffle(a1, axis=0)
    return [a0.astype(np.int32), a1.astype(np.int32), np.zeros((0, 2), dtype=np.int32)]


def _node_lists(rng):
    """L = 2: node i has in-degree NODE_DEGREES[i], split at random over the two types"""
    tgt = np.repeat(np.arange(len(NODE_DEGREES)), NODE_DEGREES)
    src = rng.integers(0, NUM_NODES, size=tgt.size)
    typ = rng.integers(0, 2, size=tgt.size)
    order = rng.permutation(tgt.size)
    src, tgt, typ = src[order], tgt[order], typ[order]
    return [np.stack([src[typ == l], tgt[typ == l]], axis=1).astype(np.int32) for l in range(2)]


class _Case:
    """Both graphs, their handles (lists as given: by-target views; columns swapped: by-source views), the host arrays of
    every view and the inputs and fp64 references shared by the tests below (computed once, read only)."""

    def __init__(self, dev):
        from tf2_gnn_amd import ops

        self.dev = dev
        rng = np.random.default_rng(29)
        self.lists = {"typed": _typed_lists(rng), "node": _node_lists(rng)}
        self.swapped = {k: [np.ascontiguousarray(a[:, ::-1]) for a in v] for k, v in self.lists.items()}
        self.handles = {}
        for kind in ("typed", "node"):
            self.handles[kind, False] = ops.Graph(to_dev(self.lists[kind], dev), NUM_NODES, parts=ops.G_PARTS_ALL)
            self.handles[kind, True] = ops.Graph(to_dev(self.swapped[kind], dev), NUM_NODES, parts=ops.G_PARTS_ALL)
        self._host, self._inputs, self._refs = {}, {}, {}

    @staticmethod
    def kind(view):
        return "node" if view in (gr.VIEW_BY_DST_NODE, gr.VIEW_BY_SRC_NODE) else "typed"

    @staticmethod
    def by_src(view):
        return view in (gr.VIEW_BY_SRC_TYPED, gr.VIEW_BY_SRC_NODE, gr.VIEW_BY_SRC_TYPED_COMPACT)

    def handle(self, view):
        return self.handles[self.kind(view), self.by_src(view)]

    def host_lists(self, view):
        return (self.swapped if self.by_src(view) else self.lists)[self.kind(view)]

    def host(self, view):
        """(rowptr, col, out_rows) of the view, from the edge lists"""
        if view not in self._host:
            from tf2_gnn_amd import ops

            pos = None
            if view == gr.VIEW_BY_DST_TYPED_PATTERN:
                pos = self.handle(view).array(ops.G_PATTERN_POS_BY_DST).cpu().numpy()
            self._host[view] = gr.view_rows(self.host_lists(view), NUM_NODES, view, pattern_pos=pos)
        return self._host[view]

    def num_edges(self, view):
        return int(self.host(view)[1].shape[0])

    def inputs(self, view, width, heads=1):
        """(X [input rows, width], edge weights [E] or [E, heads], row scales [CSR rows]) as CPU tensors"""
        key = (view, width, heads)
        if key not in self._inputs:
            rowptr, col, _ = self.host(view)
            L = len(self.host_lists(view))
            gen = torch.Generator().manual_seed(1000 * view + width + 7 * heads)
            X = torch.randn((NUM_NODES * (L if self.kind(view) == "node" else 1), width), generator=gen)
            ew = torch.rand((col.shape[0],) if heads == 1 else (col.shape[0], heads), generator=gen) + 0.5
            rs = torch.rand(rowptr.shape[0] - 1, generator=gen) * 0.7 + 0.3
            self._inputs[key] = (X, ew, rs)
        return self._inputs[key]

    def reference(self, view, width, spec):
        """(out64, l1) in the view's output rows"""
        key = (view, width, spec)
        if key not in self._refs:
            rowptr, col, out_rows = self.host(view)
            X, ew, rs = self.inputs(view, width, max(spec.ew, 1))
            out, l1, _ = gr.gather_reference(rowptr, col, X, edge_weight=ew if spec.ew else None, row_scale=rs if spec.rs else None,
                                             reduce=spec.reduce, pre_act=spec.pre, post_act=spec.post)
            if out_rows is not None:
                out, l1 = out[out_rows], l1[out_rows]
            self._refs[key] = (out, l1)
        return self._refs[key]

    def num_out_rows(self, view):
        rowptr, _, out_rows = self.host(view)
        return int(rowptr.shape[0] - 1 if out_rows is None else out_rows.shape[0])

    def guarded_out(self, view, width):
        return torch.full((self.num_out_rows(view) + 1, width), SENTINEL, dtype=torch.float32, device=self.dev)

    def run(self, view, width, spec, inp=None, out=None, col=None):
        """one ops.graph_gather call; the output carries one guard row behind its last row -> the rows (a CPU copy)"""
        from tf2_gnn_amd import ops

        X, ew, rs = self.inputs(view, width, max(spec.ew, 1))
        buf = None
        if out is None:
            buf = self.guarded_out(view, width)
            out = buf[:-1]
        ops.graph_gather(self.handle(view), view, X.to(self.dev) if inp is None else inp, col=col,
                         edge_weight=ew.to(self.dev) if spec.ew else None, row_scale=rs.to(self.dev) if spec.rs else None,
                         reduce=ops.REDUCE_MAX if spec.reduce == "max" else ops.REDUCE_SUM, pre_act=spec.pre, post_act=spec.post,
                         out=out)
        torch.cuda.synchronize()
        if buf is not None:
            _guard_untouched(buf, f"view {view} width {width} {spec}")
        return out.cpu()


@pytest.fixture(scope="module")
def case(dev):
    return _Case(dev)


def _guard_untouched(buf, what):
    assert bool((buf[-1] == SENTINEL).all()), f"{what}: the guard row behind the last row was written"


def _check(got, ref, l1, spec, what, group):
    """the bound of the module docstring for ``spec``; the measured error goes to the parity log under ``group``"""
    got = got.double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    acts = spec.pre is not None or spec.post is not None
    if spec.reduce == "max":
        if acts:
            assert_close(got, ref, tol=ACT_TOL, what=group)
            return
        empty = ref == gr.FLOAT_LOWEST
        assert torch.equal(got[empty], ref[empty]), f"{what}: an empty max row is not the lowest float"
        err = (got - ref).abs()[~empty] / ref.abs()[~empty]
        worst = float(err.max()) if err.numel() else 0.0
        record_parity(group, max_relative_error=worst, bound=MAX_TOL)
        assert worst <= MAX_TOL, f"{what}: max relative error {worst:.3e} > 2^-22"
        return
    scale = l1 + ref.abs().clamp(min=1.0) if acts else l1
    diff = (got - ref).abs()
    zero = scale == 0  # rows without edges: nothing to round
    assert bool((diff[zero] == 0).all()), f"{what}: a row without edges is not exactly zero"
    err = diff[~zero] / scale[~zero]
    worst = float(err.max()) if err.numel() else 0.0
    record_parity(group, max_scaled_error=worst, bound=SUM_TOL)
    if worst > SUM_TOL:
        where = int((diff / scale.clamp(min=1e-300)).masked_fill(zero, 0).argmax())
        r, c = divmod(where, got.shape[1])
        raise AssertionError(f"{what}: error {worst:.3e} of the row's l1 mass > {SUM_TOL:.1e} at output row {r}, column {c}")


# ---- 2. the graphs -----------------------------------------------------------------------------------------------------------
def test_graphs_have_the_planned_rows(case):
    n = len(TYPED_LENGTHS)
    for swapped in (False, True):
        lists = (case.swapped if swapped else case.lists)["typed"]
        rowptr, _, _ = ao.bucket_edges(lists, NUM_NODES, by="src" if swapped else "dst")
        lens = np.diff(rowptr).reshape(NUM_NODES, 3)
        assert tuple(lens[:n, 0]) == TYPED_LENGTHS
        assert tuple(lens[:n, 1]) == tuple(2 if i % 2 == 0 else 0 for i in range(n))
        assert int(lens[:, 2].sum()) == 0 and int(lens[n:].sum()) == 0
        lists = (case.swapped if swapped else case.lists)["node"]
        rowptr, _, typ = ao.bucket_edges(lists, NUM_NODES, by="src" if swapped else "dst")
        deg = np.diff(rowptr[::2])
        assert tuple(deg[:n]) == NODE_DEGREES and int(deg[n:].sum()) == 0
        assert 0 < int(typ.sum()) < typ.size  # both types hold edges
    assert case.num_edges(gr.VIEW_BY_DST_TYPED) == sum(TYPED_LENGTHS) + 2 * ((n + 1) // 2)
    assert case.num_edges(gr.VIEW_BY_DST_NODE) == sum(NODE_DEGREES)
    # compact rows: the non-empty buckets; pattern rows: every bucket
    nz = sum(1 for x in TYPED_LENGTHS if x) + (n + 1) // 2
    assert case.num_out_rows(gr.VIEW_BY_DST_TYPED_COMPACT) == case.num_out_rows(gr.VIEW_BY_SRC_TYPED_COMPACT) == nz
    assert case.handle(gr.VIEW_BY_DST_TYPED_COMPACT).nonempty_offsets(False)[-1] == nz
    assert case.handle(gr.VIEW_BY_SRC_TYPED_COMPACT).nonempty_offsets(True)[-1] == nz
    assert case.num_out_rows(gr.VIEW_BY_DST_TYPED_PATTERN) == NUM_NODES * 3


@pytest.mark.parametrize("view", ALL_VIEWS)
def test_plan_has_ten_partial_slots(case, view):
    """513 -> 2, 1024 -> 2, 1025 -> 3, 1100 -> 3 items of multi-item rows: if the plan constants move, this fails instead of
    the tests below quietly no longer covering the item paths"""
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    for w in (7, 64):
        assert lib.tfgnn_graph_gather_workspace_bytes(case.handle(view)._h, view, w) == PARTIAL_SLOTS * w * 4


# ---- 3. forward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["1", "21"])
@pytest.mark.parametrize("width", [64, 128])
@pytest.mark.parametrize("view", ALL_VIEWS)
def test_views_plain_sum_both_walks(case, monkeypatch, view, width, walk):
    monkeypatch.setenv("TFGNN_GATHER_MULTI", walk)
    got = case.run(view, width, PLAIN)
    ref, l1 = case.reference(view, width, PLAIN)
    assert got.shape == (case.num_out_rows(view), width)
    _check(got, ref, l1, PLAIN, f"view {view} width {width} walk {walk}", "graph_gather views plain sum")


def test_pattern_view_allocates_a_row_per_bucket(case):
    """without ``out=`` the wrapper sizes the result itself: V * L rows in pattern order, not the V rows of a node view"""
    from tf2_gnn_amd import ops

    view = gr.VIEW_BY_DST_TYPED_PATTERN
    got = ops.graph_gather(case.handle(view), view, case.inputs(view, 64)[0].to(case.dev))
    assert got.shape == (NUM_NODES * 3, 64)
    assert torch.equal(got.cpu(), case.run(view, 64, PLAIN))


@pytest.mark.parametrize("width", [64, 128])
@pytest.mark.parametrize("view", ALL_VIEWS)
def test_views_weights_scales_relu(case, view, width):
    got = case.run(view, width, WEIGHTED)
    ref, l1 = case.reference(view, width, WEIGHTED)
    _check(got, ref, l1, WEIGHTED, f"view {view} width {width} weighted", "graph_gather views weights + scales + relu")


@pytest.mark.parametrize("walk", ["1", "21"])
@pytest.mark.parametrize("width", DISPATCH_WIDTHS)
@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_dispatch_variants_plain_sum_both_walks(case, monkeypatch, view, width, walk):
    """scalar path (7, 70: one window, two windows with a dead tail), 8 x 1 (8, 32), 16 x 1 (64), 16 x 2 (96, 128), 16 x 4 (256),
    16 x 5 (320; 1280: four windows), 32 x 4 (384, 512; 1024: two windows): items, partial slots and the combine pass run
    for every window"""
    monkeypatch.setenv("TFGNN_GATHER_MULTI", walk)
    got = case.run(view, width, PLAIN)
    ref, l1 = case.reference(view, width, PLAIN)
    _check(got, ref, l1, PLAIN, f"view {view} width {width} walk {walk}", "graph_gather dispatch plain sum")


@pytest.mark.parametrize("width", DISPATCH_WIDTHS)
@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_dispatch_variants_weights_scales_relu(case, view, width):
    got = case.run(view, width, WEIGHTED)
    ref, l1 = case.reference(view, width, WEIGHTED)
    _check(got, ref, l1, WEIGHTED, f"view {view} width {width} weighted", "graph_gather dispatch weights + scales + relu")


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("width", [64, 320])
@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_max(case, view, width, weights):
    """MODE_GENERAL over short rows, items and the combine pass; empty rows are the lowest float, not scaled"""
    spec = Spec(ew=1 if weights else 0, rs=weights, reduce="max")
    got = case.run(view, width, spec)
    ref, l1 = case.reference(view, width, spec)
    if not weights:
        assert torch.equal(got.double(), ref)  # no arithmetic at all
    _check(got, ref, l1, spec, f"view {view} width {width} max weights={weights}", "graph_gather max")


@pytest.mark.parametrize("reduce", ["sum", "max"])
@pytest.mark.parametrize("pre", ["relu", "tanh", "gelu"])
@pytest.mark.parametrize("width", [64, 320])
@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_pre_activation(case, view, width, pre, reduce):
    spec = Spec(ew=1, reduce=reduce, pre=pre)
    got = case.run(view, width, spec)
    ref, l1 = case.reference(view, width, spec)
    _check(got, ref, l1, spec, f"view {view} width {width} {pre} {reduce}", f"graph_gather pre_act {reduce}")


@pytest.mark.parametrize("width,heads", [(64, 2), (24, 3), (18, 3), (256, 8)])
@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_per_head_weights(case, view, width, heads):
    """MODE_HEADS over items; (18, 3): 6-float heads take the scalar path"""
    spec = Spec(ew=heads)
    got = case.run(view, width, spec)
    ref, l1 = case.reference(view, width, spec)
    _check(got, ref, l1, spec, f"view {view} width {width} heads {heads}", "graph_gather per-head weights")


@pytest.mark.parametrize("offset", [4, 1])
@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_input_as_a_column_slice(case, view, offset):
    """16-byte aligned offset: the float4 path with a leading dimension; an offset of one float: the scalar path"""
    width = 64
    X = case.inputs(view, width)[0]
    wide = torch.full((X.shape[0], width + 8), 3.25)
    wide[:, offset:offset + width] = X
    got = case.run(view, width, PLAIN, inp=wide.to(case.dev)[:, offset:offset + width])
    ref, l1 = case.reference(view, width, PLAIN)
    _check(got, ref, l1, PLAIN, f"view {view} input slice at {offset}", "graph_gather operands")


@pytest.mark.parametrize("offset", [20, 21])
@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_output_as_a_column_slice(case, view, offset):
    width = 64
    wide = torch.full((case.num_out_rows(view) + 1, 100), SENTINEL, dtype=torch.float32, device=case.dev)
    got = case.run(view, width, WEIGHTED, out=wide[:-1, offset:offset + width])
    ref, l1 = case.reference(view, width, WEIGHTED)
    _check(got, ref, l1, WEIGHTED, f"view {view} output slice at {offset}", "graph_gather operands")
    assert bool((wide[:, :offset] == SENTINEL).all()) and bool((wide[:, offset + width:] == SENTINEL).all())
    _guard_untouched(wide, "output slice")


@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_NODE, gr.VIEW_BY_SRC_NODE])
def test_column_override_with_per_edge_rows(case, view):
    """col = the identity over [E, width] per-edge rows, as RGAT and the per-edge message forms use the node views"""
    width = 64
    rowptr, col, _ = case.host(view)
    E = col.shape[0]
    msgs = torch.randn((E, width), generator=torch.Generator().manual_seed(view))
    ident = np.arange(E)
    got = case.run(view, width, PLAIN, inp=msgs.to(case.dev), col=torch.from_numpy(ident.astype(np.int32)).to(case.dev))
    ref, l1, _ = gr.gather_reference(rowptr, ident, msgs)
    _check(got, ref, l1, PLAIN, f"view {view} col override", "graph_gather operands")


@pytest.mark.parametrize("view", ALL_VIEWS)
def test_workspace_and_output_guards_at_the_c_entry(case, view):
    """tfgnn_graph_gather_reduce called directly with a workspace that is one row larger than required: neither the row
    behind the partial slots nor the row behind the output may change"""
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    width = 64
    g = case.handle(view)
    X, ew, rs = case.inputs(view, width)
    nbytes = int(lib.tfgnn_graph_gather_workspace_bytes(g._h, view, width))
    assert nbytes == PARTIAL_SLOTS * width * 4
    ws = torch.full((PARTIAL_SLOTS + 1, width), SENTINEL, dtype=torch.float32, device=case.dev)
    out = case.guarded_out(view, width)
    Xd, ewd, rsd = X.to(case.dev), ew.to(case.dev), rs.to(case.dev)
    rc = lib.tfgnn_graph_gather_reduce(g._h, view, None, ops._ptr(ewd), 1, ops._ptr(rsd), ops._ptr(Xd), width, width, ops._ptr(out),
                                       width, ops.REDUCE_SUM, ops.ACT_NONE, ops.ACT_RELU, ops._ptr(ws), nbytes, ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.tfgnn_last_error().decode()
    _guard_untouched(ws, f"view {view} workspace")
    _guard_untouched(out, f"view {view} output")
    assert bool((ws[:-1] != SENTINEL).all())  # every partial slot was written
    ref, l1 = case.reference(view, width, WEIGHTED)
    _check(out[:-1].cpu(), ref, l1, WEIGHTED, f"view {view} C entry", "graph_gather views weights + scales + relu")
    # one byte short of the requirement is an error, not a write past the end
    rc = lib.tfgnn_graph_gather_reduce(g._h, view, None, None, 1, None, ops._ptr(Xd), width, width, ops._ptr(out), width,
                                       ops.REDUCE_SUM, ops.ACT_NONE, ops.ACT_NONE, ops._ptr(ws), nbytes - 1, ops._stream())
    assert rc != 0 and "workspace" in lib.tfgnn_last_error().decode()


@pytest.mark.parametrize("spec", [PLAIN, WEIGHTED, Spec(ew=1, reduce="max", pre="tanh"), Spec(ew=8)], ids=["plain", "weighted", "max", "heads"])
@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE, gr.VIEW_BY_SRC_TYPED_COMPACT])
def test_same_call_twice_same_bits(case, view, spec):
    assert torch.equal(case.run(view, 320, spec), case.run(view, 320, spec))


# ---- 4. backward through a general aggregation -------------------------------------------------------------------------------
POOL_ROWS = 40
BWD_NODES = 16


class _BackwardCase:
    """One edge type, in-degrees TYPED_LENGTHS (node threshold 32: every row from 47 edges on goes through item workgroups,
    513 and up through the combine pass).  Edge arrays are in the handle's by-target order.  Messages come from a pool of 40
    rows and the edge weight is a function of the pool row, so duplicate edges tie exactly."""

    def __init__(self, dev):
        from tf2_gnn_amd import ops

        self.dev = dev
        rng = np.random.default_rng(23)
        tgt = np.repeat(np.arange(len(TYPED_LENGTHS)), TYPED_LENGTHS)
        adj = np.stack([rng.integers(0, BWD_NODES, size=tgt.size), tgt], axis=1).astype(np.int32)
        rng.shuffle(adj, axis=0)
        self.g = ops.Graph(to_dev([adj], dev), BWD_NODES)
        rowptr, _, _ = ao.bucket_edges([adj], BWD_NODES, by="dst")
        assert tuple(np.diff(rowptr)[: len(TYPED_LENGTHS)]) == TYPED_LENGTHS
        self.E = int(tgt.size)
        self.target = torch.from_numpy(np.repeat(np.arange(BWD_NODES), np.diff(rowptr))).int()
        self.msg_row = torch.from_numpy(rng.integers(0, POOL_ROWS, size=self.E)).int()
        self.pool_weight = torch.from_numpy(np.where(rng.integers(0, 2, size=POOL_ROWS) == 1, 1.25, 0.75)).float()
        self.ident = torch.arange(self.E, dtype=torch.int32, device=dev)

    def operands(self, width, pooled, pad=3):
        """(message rows inside a tensor ``pad`` columns wider, msg_row or None, edge weights [E], node scales, grad_agg)"""
        gen = torch.Generator().manual_seed(width + (100 if pooled else 0))
        rows = POOL_ROWS if pooled else self.E
        wide = torch.randn((rows, width + pad), generator=gen)
        if pooled:
            ew = self.pool_weight[self.msg_row.long()]
        else:
            ew = torch.rand(self.E, generator=gen) + 0.5
        ns = torch.rand(BWD_NODES, generator=gen) + 0.5
        grad = torch.randn((BWD_NODES, width), generator=gen)
        return wide, (self.msg_row if pooled else None), ew, ns, grad


@pytest.fixture(scope="module")
def bwd(dev):
    return _BackwardCase(dev)


def _dev(t, dev):
    return None if t is None else t.to(dev)


@pytest.mark.parametrize("width", [5, 64])
@pytest.mark.parametrize("act", [None] + ACTS)
def test_edge_aggregate_backward_sum(bwd, act, width):
    from tf2_gnn_amd import ops

    for pooled, with_ew, with_ns in ((True, True, True), (False, False, False), (False, True, False), (True, False, True)):
        wide, msg_row, ew, ns, grad = bwd.operands(width, pooled)
        ew, ns = (ew if with_ew else None), (ns if with_ns else None)
        msg = wide[:, 2:2 + width]
        ref = gr.aggregate_backward_reference(msg, bwd.target, grad, num_targets=BWD_NODES, msg_row=msg_row, edge_weight=ew,
                                              node_scale=ns, pre_act=act)
        msg_d = wide.to(bwd.dev)[:, 2:2 + width]
        assert msg_d.stride(0) == width + 3  # ld_msg > width
        got = ops.edge_aggregate_backward(msg_d, bwd.target.to(bwd.dev), grad.to(bwd.dev), msg_row=_dev(msg_row, bwd.dev),
                                          edge_weight=_dev(ew, bwd.dev), node_scale=_dev(ns, bwd.dev), pre_act=act)
        assert got.shape == (bwd.E, width)
        assert_close(got, ref, tol=BWD_TOL, what="edge_aggregate_backward sum")


@pytest.mark.parametrize("offset", [4, 2], ids=["float4", "scalar"])
@pytest.mark.parametrize("pooled", [True, False], ids=["pool", "per-edge"])
@pytest.mark.parametrize("act", [None] + ACTS)
def test_edge_aggregate_backward_max(bwd, act, pooled, offset):
    """The max branch selects by bit equality, z == agg_max[t], between the value edge.hip recomputes per edge and the maximum
    the MODE_GENERAL gather took over item workgroups and the combine pass: phase 0 must mark exactly the reference's edges,
    and at least one per (non-empty target, column).  The messages are a column slice at a 16-byte aligned offset (the gather's
    float4 kernels, what the layers run) and at an offset of two floats (its scalar kernels)."""
    from tf2_gnn_amd import ops

    width = 32
    wide, msg_row, ew, _, grad = bwd.operands(width, pooled, pad=offset + 4)
    msg = wide[:, offset:offset + width]
    sel, ties, ref, gap = gr.aggregate_backward_reference(msg, bwd.target, grad, num_targets=BWD_NODES, msg_row=msg_row,
                                                          edge_weight=ew, pre_act=act, reduce="max")
    # precondition on the reference alone: no cell is decided by less than fp32 rounding (no cell is excluded)
    assert float(gap.min()) > 1e-6, f"ambiguous maximum in the test data: gap {float(gap.min()):.3e}"
    if pooled:
        assert int((ties > 1).sum()) > 0  # exact ties are part of the case
    dev = bwd.dev
    msg_d = wide.to(dev)[:, offset:offset + width]
    target_d, row_d, ew_d, grad_d = bwd.target.to(dev), _dev(msg_row, dev), ew.to(dev), grad.to(dev)
    col = row_d if pooled else bwd.ident
    agg_max = ops.graph_gather(bwd.g, ops.VIEW_BY_DST_NODE, msg_d, col=col, edge_weight=ew_d, reduce=ops.REDUCE_MAX, pre_act=act)
    got_sel = ops.edge_aggregate_backward(msg_d, target_d, None, msg_row=row_d, edge_weight=ew_d, pre_act=act,
                                          reduce=ops.REDUCE_MAX, agg_max=agg_max, phase=0)
    sel_cpu = got_sel.cpu()
    per_target = torch.zeros((BWD_NODES, width)).index_add_(0, bwd.target.long(), sel_cpu)
    nonempty = torch.bincount(bwd.target.long(), minlength=BWD_NODES) > 0
    missing = int((per_target[nonempty] < 1).sum())
    assert missing == 0, f"{missing} (target, column) cells lost their maximum: z != agg_max bit for bit"
    assert torch.equal(sel_cpu, sel.float())
    nsel = ops.graph_gather(bwd.g, ops.VIEW_BY_DST_NODE, got_sel, col=bwd.ident)
    assert torch.equal(nsel.cpu().double(), ties)
    got = ops.edge_aggregate_backward(msg_d, target_d, grad_d, msg_row=row_d, edge_weight=ew_d, pre_act=act, reduce=ops.REDUCE_MAX,
                                      agg_max=agg_max, num_selected=nsel).cpu()
    assert bool((got[~sel] == 0).all())
    assert_close(got, ref, tol=BWD_TOL, what="edge_aggregate_backward max")


def test_edge_aggregate_backward_argument_checks(bwd):
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    width = 8
    wide, _, _, _, grad = bwd.operands(width, False)
    msg_d, target_d, grad_d = wide.to(bwd.dev), bwd.target.to(bwd.dev), grad.to(bwd.dev)
    out = torch.full((bwd.E + 1, width), SENTINEL, dtype=torch.float32, device=bwd.dev)

    def call(ld, reduce, agg_max, nsel, phase):
        return lib.tfgnn_edge_aggregate_backward(bwd.E, width, ops._ptr(msg_d), ld, None, ops._ptr(target_d), None, None, ops.ACT_NONE,
                                                 reduce, ops._ptr(grad_d), ops._ptr(agg_max), ops._ptr(nsel), phase, ops._ptr(out),
                                                 ops._stream())

    assert call(width + 3, ops.REDUCE_SUM, None, None, 0) != 0  # phase 0 is for max
    assert "phase 0" in lib.tfgnn_last_error().decode()
    assert call(width + 3, ops.REDUCE_MAX, None, None, 1) != 0  # max without agg_max
    assert "agg_max" in lib.tfgnn_last_error().decode()
    assert call(width - 1, ops.REDUCE_SUM, None, None, 1) != 0  # ld_msg < width
    assert "leading dimension" in lib.tfgnn_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())  # a refused call writes nothing
    assert call(width + 3, ops.REDUCE_SUM, None, None, 1) == 0
    torch.cuda.synchronize()
    _guard_untouched(out, "edge_aggregate_backward")


# ---- 5. ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (4, 64, 320), (3, 0, 5)])
def test_permute_021(dev, shape):
    from tf2_gnn_amd import ops

    x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
    out = ops.permute_021(x.to(dev))
    assert out.shape == (shape[1], shape[0], shape[2])
    assert torch.equal(out.cpu(), x.permute(1, 0, 2).contiguous())
