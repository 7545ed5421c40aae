"""tfgnn_blockdiag_forward / tfgnn_blockdiag_backward on the device against the op-level loops of
tests/rgcn_blockdiag_reference.py (float64, with the bound derived from the stated sum orders).  Not run per GEMM mode: no
product is involved.

Two input families.  EXACT: X, dPre and Qb small integers, no weights - every partial sum is an integer below 2^24 (asserted
from the degrees and the ranges), so every order gives the same fp32 value and the results must equal the reference bit for
bit.  FLOAT: randn inputs with the degree normalisation and the mean aggregator's scales as tfgnn_graph_scales computes them
(read back and handed to the reference as its inputs): every value within its bound, an error where the bound is 0 must be 0.

Graphs (V = 50 unless stated): every one has an edge type without edges (type L - 2 when L >= 3), node 7 without in-edges,
node 9 without out-edges, self loops and duplicated edges.  "hub": node 2 gets 2100 in-edges and node 3 2050 out-edges (several
512-edge items each, so the combine launch runs in both directions) and nodes 10 .. 15 in-degrees - and 16 .. 21 out-degrees -
of exactly 31, 32, 33, 511, 512, 513, which straddle the plan's long-row threshold (32) and its item size (512).  "hub1": the
same with every hub edge of ONE type, so a run of one type crosses segment and item boundaries.  "chunks": six types with
0, 1, 255, 256, 257 and 600 edges, the boundaries of the weight gradient's 256-edge chunks.  X and dPre sit inside wider
arrays; pre and dX are written into wider arrays whose other columns must stay as they were."""
import functools

import numpy as np
import pytest
import torch

from tests import rgcn_blockdiag_reference as ref
from tests.helpers import KernelsUsed

pytestmark = pytest.mark.gpu

PAD_LEFT, PAD_RIGHT = 4, 4  # rows stay 16-byte aligned where the width allows it; "misaligned" cases shift them by one float
SENTINEL = 7.5
STRADDLE = (31, 32, 33, 511, 512, 513)
CHUNK_COUNTS = (0, 1, 255, 256, 257, 600)
# (graph kind, V, L, D, H, C, misaligned)
CASES = [
    ("plain", 1, 1, 4, 4, 2, False), ("plain", 2, 4, 6, 9, 3, False),
    ("hub", 50, 4, 64, 64, 2, False),       # vector path, one window, 16 lane groups per item
    ("hub", 50, 4, 64, 64, 2, True),        # the same widths on the scalar path: base pointers off by one float
    ("hub", 50, 4, 8, 8, 1, False),         # one dense block
    ("hub", 50, 256, 8, 8, 8, False),       # diagonal; many types
    ("hub", 50, 37, 20, 20, 4, False),      # di = 5 is no multiple of the vector width; many runs per row
    ("hub1", 50, 3, 12, 20, 4, False),      # di != ho; runs across segment and item boundaries
    ("hub1", 50, 3, 128, 64, 2, False),     # di != ho on the vector path: more input lanes than output lanes
    ("hub", 50, 37, 320, 320, 64, False),   # the paper's 5 x 5 blocks: six windows of 12 blocks, the last one short
    ("hub", 50, 4, 320, 320, 8, False),     # vector path, three windows of 3 + 3 + 2 blocks of 40 x 40
    ("hub", 50, 4, 7, 7, 7, False), ("hub", 50, 4, 6, 9, 3, False),  # scalar path, odd widths
    ("chunks", 50, 6, 20, 20, 4, False), ("chunks", 50, 6, 24, 16, 2, False),  # di = 12: two tiles of 8 block rows in stage 1
    ("plain", 3001, 37, 64, 64, 16, False),  # many workgroups of short rows; one target row of two items
]


def _edges(kind, V, L, rng):
    """per type an int32 [E_l, 2] array of (source, target)"""
    per_type = [[] for _ in range(L)]
    if kind == "chunks":
        srcs = np.array([v for v in range(V) if v != 9])
        tgts = np.array([v for v in range(V) if v != 7])
        return [np.stack([rng.choice(srcs, n), rng.choice(tgts, n)], axis=1).astype(np.int32) for n in CHUNK_COUNTS]
    empty = L - 2 if L >= 3 else None
    types = [l for l in range(L) if l != empty]

    def add(src, tgt, one_type=None):
        t = rng.choice(types, size=len(src)) if one_type is None else np.full(len(src), one_type)
        for l in types:
            sel = t == l
            if sel.any():
                per_type[l].append(np.stack([src[sel], tgt[sel]], axis=1))

    if V < 50:
        n = 5 * V
        add(rng.integers(0, V, n), rng.integers(0, V, n))
        add(np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64))  # self loops, twice
    else:
        hub = kind in ("hub", "hub1")
        fixed_in, fixed_out = (set(range(10, 16)), set(range(16, 22))) if hub else (set(), set())
        srcs = np.array([v for v in range(V) if v != 9 and v not in fixed_out])
        tgts = np.array([v for v in range(V) if v != 7 and v not in fixed_in])
        n = 3 * V if V > 50 else 600
        s, t = rng.choice(srcs, n), rng.choice(tgts, n)
        add(s, t)
        add(s[:20], t[:20])                               # duplicated edges
        loops = np.array([0, 1, 4, 5]); add(loops, loops)  # self loops
        if hub:
            one = types[0] if kind == "hub1" else None
            add(rng.choice(srcs, 2100), np.full(2100, 2), one)
            add(np.full(2050, 3), rng.choice(tgts, 2050), one)
            for node, deg in zip(range(10, 16), STRADDLE):
                add(rng.choice(srcs, deg), np.full(deg, node), one)
            for node, deg in zip(range(16, 22), STRADDLE):
                add(np.full(deg, node), rng.choice(tgts, deg), one)
        elif V > 1000:
            add(rng.choice(srcs, 700), np.full(700, 2))    # two items
            add(np.full(40, 3), rng.choice(tgts, 40))
    return [np.concatenate(p).astype(np.int32) if p else np.zeros((0, 2), np.int32) for p in per_type]


@functools.lru_cache(maxsize=None)
def _graph_case(kind, V, L):
    rng = np.random.default_rng(104729 * V + 131 * L + len(kind))
    adjs = _edges(kind, V, L, rng)
    indeg, outdeg = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64)
    for a in adjs:
        np.add.at(outdeg, a[:, 0], 1)
        np.add.at(indeg, a[:, 1], 1)
    if V >= 50:
        assert indeg[7] == 0 and outdeg[9] == 0
    if kind == "chunks":
        assert tuple(a.shape[0] for a in adjs) == CHUNK_COUNTS
    elif V >= 50:
        assert L < 3 or adjs[L - 2].shape[0] == 0
    if kind in ("hub", "hub1"):
        assert indeg[2] >= 2100 and outdeg[3] >= 2050
        assert tuple(indeg[10:16]) == STRADDLE and tuple(outdeg[16:22]) == STRADDLE
    return adjs, indeg, outdeg


@functools.lru_cache(maxsize=None)
def _case(family, kind, V, L, D, H, C):
    """inputs and the (shared, read-only) references of one case; the FLOAT family's scales come from the device run"""
    adjs, indeg, outdeg = _graph_case(kind, V, L)
    rng = np.random.default_rng(7919 * V + 31 * D + 7 * L + C + 3 * H)
    di, ho = D // C, H // C
    if family == "exact":
        X = rng.integers(-2, 3, size=(V, D)).astype(np.float32)
        Qb = rng.integers(-2, 3, size=(L, di, H)).astype(np.float32)
        dPre = rng.integers(-1, 2, size=(V, H)).astype(np.float32)
        # every partial sum of every result is an integer of magnitude below 2^24: exact in fp32, whatever the order
        assert indeg.max(initial=0) * di * 2 * 2 < 2 ** 24 and outdeg.max(initial=0) * ho * 2 * 1 < 2 ** 24
        assert max(a.shape[0] for a in adjs) * 2 * 1 < 2 ** 24
    else:
        X = rng.standard_normal((V, D)).astype(np.float32)
        Qb = rng.standard_normal((L, di, H)).astype(np.float32)
        dPre = rng.standard_normal((V, H)).astype(np.float32)
    return {"adjs": adjs, "X": X, "Qb": Qb, "dPre": dPre, "ref": {}}


def _wide(a, dev, left=PAD_LEFT):
    w = torch.full((a.shape[0], left + a.shape[1] + PAD_RIGHT), SENTINEL)
    w[:, left:left + a.shape[1]] = torch.from_numpy(a)
    w = w.to(dev)
    return w, w[:, left:left + a.shape[1]]


def _pads_untouched(w, left=PAD_LEFT):
    return bool((w[:, :left] == SENTINEL).all()) and bool((w[:, w.shape[1] - PAD_RIGHT:] == SENTINEL).all())


def _ratio(err, bound):
    """the largest error / bound; an error where the bound is 0 must be 0"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.all(err[bound == 0] == 0), "an error where the bound is exactly 0"
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def _scale_tables(g, V, L):
    """the device's mean / normalised scales as [V, L] tables (constant per (target, type) bucket: asserted) and m [V]"""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers.graph_scales import graph_scales

    sc = graph_scales(g, True, "mean")
    tables = []
    for ew, coll, tgt in ((sc.edge_weight_by_dst, g.array(ops.G_COLL_BY_DST), g.array(ops.G_TARGET_BY_DST)),
                          (sc.edge_weight_by_src, g.array(ops.G_COLL_BY_SRC), None)):
        ew, coll = ew.cpu().numpy().astype(np.float64), coll.cpu().numpy().astype(np.int64)
        t = tgt.cpu().numpy().astype(np.int64) if tgt is not None else coll // L
        tab = np.ones((V, L))
        tab[t, coll % L] = ew
        assert np.array_equal(tab[t, coll % L], ew), "an edge weight that is not constant over its (target, type) bucket"
        tables.append(tab)
    return sc, tables[0], tables[1], sc.node_scale.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("family", ["exact", "float"])
@pytest.mark.parametrize("kind,V,L,D,H,C,misaligned", CASES)
def test_blockdiag_forward_and_backward(dev, family, kind, V, L, D, H, C, misaligned):
    from tf2_gnn_amd import ops

    c = _case(family, kind, V, L, D, H, C)
    adjs = c["adjs"]
    _, indeg, outdeg = _graph_case(kind, V, L)
    g = ops.Graph([torch.from_numpy(a).to(dev) for a in adjs], V)
    ew_d = ew_s = ns = s = s_src = m = None
    if family == "float":
        sc, s, s_src, m = _scale_tables(g, V, L)
        ew_d, ew_s, ns = sc.edge_weight_by_dst, sc.edge_weight_by_src, sc.node_scale
    if not c["ref"]:
        c["ref"]["pre"] = ref.forward(adjs, V, c["Qb"], c["X"], C, s, m)
        c["ref"]["dX"] = ref.backward_dx(adjs, V, c["Qb"], c["dPre"], C, s_src)
        c["ref"]["dQb"] = ref.backward_dq(adjs, V, C, D, H, c["X"], c["dPre"], s, m)
    rP, rdX, rdQ = (c["ref"][k] for k in ("pre", "dX", "dQb"))  # shared between the runs of a case, never written
    for val, _ in (rP, rdX, rdQ):
        assert family == "float" or np.abs(val).max(initial=0) < 2 ** 24

    left = PAD_LEFT - 1 if misaligned else PAD_LEFT
    qflat = torch.zeros(c["Qb"].size + 4, device=dev)
    Qb = qflat[1 if misaligned else 0:][:c["Qb"].size].view(c["Qb"].shape)
    Qb.copy_(torch.from_numpy(c["Qb"]))
    assert (Qb.data_ptr() % 16 != 0) == misaligned
    Xw, X = _wide(c["X"], dev, left)
    dPw, dPre = _wide(c["dPre"], dev, left)
    Pw, P = _wide(np.zeros((V, H), np.float32), dev, left)
    dXw, dX = _wide(np.zeros((V, D), np.float32), dev, left)
    P.fill_(-3.0), dX.fill_(-3.0)
    kw = dict(edge_weight_by_dst=ew_d, edge_weight_by_src=ew_s, node_scale=ns)
    ops.blockdiag_backward(g, Qb, dPre, X, C, **kw)  # builds the per-graph tables, so the counted calls below only launch
    n0 = ops.blockdiag_launch_counts()
    with KernelsUsed() as used:
        assert ops.blockdiag_forward(g, Qb, X, C, edge_weight=ew_d, node_scale=ns, out=P) is P
        n1 = ops.blockdiag_launch_counts()
        P1 = P.cpu().numpy().copy()
        P.fill_(5.0)
        ops.blockdiag_forward(g, Qb, X, C, edge_weight=ew_d, node_scale=ns, out=P)
        n2 = ops.blockdiag_launch_counts()
        got_dX, got_dQ = ops.blockdiag_backward(g, Qb, dPre, X, C, out_dx=dX, **kw)
        n3 = ops.blockdiag_launch_counts()
        assert got_dX is dX
        dX1, dQ1 = dX.cpu().numpy().copy(), got_dQ.cpu().numpy().copy()
        dX_alone, none = ops.blockdiag_backward(g, Qb, dPre, None, C, want_dq=False, **kw)
        n4 = ops.blockdiag_launch_counts()
        assert none is None
        none, dQ_alone = ops.blockdiag_backward(g, Qb, dPre, X, C, want_dx=False, **kw)
        n5 = ops.blockdiag_launch_counts()
        assert none is None
        dX.fill_(5.0)
        _, dQ2 = ops.blockdiag_backward(g, Qb, dPre, X, C, out_dx=dX, **kw)
    assert not any(used.delta.values()), used.delta  # no product (or plain gather) family moved

    # launches per call as the header states them: the walks 1 (+ 1 when a row has several 512-edge items), dQb 2
    fwd, dx = 1 + int(indeg.max() > 512), 1 + int(outdeg.max() > 512)
    delta = lambda a, b: {k: b[k] - a[k] for k in a}
    assert delta(n0, n1) == {"fwd": fwd, "dx": 0, "dq": 0} and delta(n1, n2) == {"fwd": fwd, "dx": 0, "dq": 0}
    assert delta(n2, n3) == {"fwd": 0, "dx": dx, "dq": 2}
    assert delta(n3, n4) == {"fwd": 0, "dx": dx, "dq": 0} and delta(n4, n5) == {"fwd": 0, "dx": 0, "dq": 2}

    # the same bits: a second call, and each backward output alone or together with the other
    assert np.array_equal(P1, P.cpu().numpy()) and np.array_equal(dX1, dX.cpu().numpy()) and np.array_equal(dQ1, dQ2.cpu().numpy())
    assert np.array_equal(dX1, dX_alone.cpu().numpy()) and np.array_equal(dQ1, dQ_alone.cpu().numpy())
    assert all(_pads_untouched(w, left) for w in (Pw, dXw, Xw, dPw))
    assert np.array_equal(X.cpu().numpy(), c["X"]) and np.array_equal(dPre.cpu().numpy(), c["dPre"])
    assert np.array_equal(Qb.cpu().numpy(), c["Qb"]) and not qflat[-3:].any()

    figures = {}
    for name, got, (val, bound) in (("pre", P1, rP), ("dX", dX1, rdX), ("dQb", dQ1, rdQ)):
        err = np.abs(got.astype(np.float64) - val)
        figures[name] = (float(err.max(initial=0)), _ratio(err, bound))
    print(f"blockdiag {family} {kind} V={V} L={L} D={D} H={H} C={C} misaligned={misaligned}: (max error, max error / bound) {figures}")
    for name, (err, ratio) in figures.items():
        if family == "exact":
            assert err == 0.0, (name, err)
        else:
            assert ratio <= 1.0, (name, err, ratio)
    if V >= 50:
        assert not P1[7].any() and not dX1[9].any()
        empty = 0 if kind == "chunks" else L - 2 if L >= 3 else None
        assert empty is None or not dQ1[empty].any()


def test_no_edges_give_zeros_and_no_nodes_launch_nothing(dev):
    from tf2_gnn_amd import ops

    L, C, D, H = 3, 2, 8, 4
    Qb = torch.ones((L, D // C, H), device=dev)
    for V in (5, 0):
        g = ops.Graph([torch.zeros((0, 2), dtype=torch.int32, device=dev) for _ in range(L)], V,
                      parts=ops.G_PART_PLAN_NODE | ops.G_PART_EDGE_IDS)
        X = torch.ones((V, D), device=dev)
        before = ops.blockdiag_launch_counts()
        P = ops.blockdiag_forward(g, Qb, X, C, out=torch.full((V, H), 3.0, device=dev))
        dX, dQ = ops.blockdiag_backward(g, Qb, torch.ones((V, H), device=dev), X, C, out_dx=torch.full((V, D), 3.0, device=dev))
        after = ops.blockdiag_launch_counts()
        assert P.shape == (V, H) and not P.any() and dX.shape == (V, D) and not dX.any()
        assert dQ.shape == (L, D // C, H) and not dQ.any()
        # without edges dQb is one memset; without nodes nothing is launched at all
        assert {k: after[k] - before[k] for k in after} == ({"fwd": 1, "dx": 1, "dq": 0} if V else {"fwd": 0, "dx": 0, "dq": 0})


def test_limits_that_need_a_graph_handle(dev):
    """strides smaller than the rows and a handle without PLAN_NODE are refused by the C entries before any launch"""
    import ctypes

    from tf2_gnn_amd import _lib, ops

    V, L, C, D, H = 6, 2, 2, 8, 4
    adjs = [torch.tensor([[0, 1], [2, 3]], dtype=torch.int32, device=dev) for _ in range(L)]
    g = ops.Graph(adjs, V, parts=ops.G_PART_PLAN_NODE)
    bare = ops.Graph(adjs, V, parts=0)
    Qb, X, P = torch.ones((L, D // C, H), device=dev), torch.ones((V, D), device=dev), torch.ones((V, H), device=dev)
    lib = _lib.load()

    def fwd(graph, **over):
        a = _lib.BlockdiagForwardArgs()
        a.struct_size = ctypes.sizeof(a)
        a.graph, a.C, a.D, a.H = graph._h, C, D, H
        a.Qb, a.X, a.ldX, a.pre, a.ldpre = Qb.data_ptr(), X.data_ptr(), D, P.data_ptr(), H
        for k, v in over.items():
            setattr(a, k, v)
        return lib.tfgnn_blockdiag_forward(ctypes.byref(a), None)

    def bwd(graph, **over):
        a = _lib.BlockdiagBackwardArgs()
        a.struct_size = ctypes.sizeof(a)
        a.graph, a.C, a.D, a.H = graph._h, C, D, H
        a.Qb, a.dPre, a.lddPre, a.dX, a.lddX = Qb.data_ptr(), P.data_ptr(), H, X.data_ptr(), D
        for k, v in over.items():
            setattr(a, k, v)
        return lib.tfgnn_blockdiag_backward(ctypes.byref(a), None)

    before = ops.blockdiag_launch_counts()
    assert fwd(bare) == -1 and b"PLAN_NODE" in lib.tfgnn_last_error()
    assert bwd(bare) == -1 and b"PLAN_NODE" in lib.tfgnn_last_error()
    assert fwd(g, ldX=D - 1) == -1 and b"row stride" in lib.tfgnn_last_error()
    assert fwd(g, ldpre=H - 1) == -1 and b"row stride" in lib.tfgnn_last_error()
    assert fwd(g, X=None) == -1 and b"NULL pointer" in lib.tfgnn_last_error()
    assert bwd(g, lddPre=H - 1) == -1 and b"row stride" in lib.tfgnn_last_error()
    assert bwd(g, lddX=D - 1) == -1 and b"row stride" in lib.tfgnn_last_error()
    assert bwd(g, dQb=X.data_ptr(), X=None, dX=None) == -1 and b"dQb needs X" in lib.tfgnn_last_error()
    assert ops.blockdiag_launch_counts() == before
    torch.cuda.synchronize()


def test_wrappers_refuse_bad_arguments_before_the_call(dev):
    from tf2_gnn_amd import ops

    V, L = 6, 2
    g = ops.Graph([torch.tensor([[0, 1], [2, 3]], dtype=torch.int32, device=dev) for _ in range(L)], V)
    X = torch.ones((V, 8), device=dev)
    Qb = torch.ones((L, 4, 6), device=dev)  # C = 2: D = 8, H = 6
    for bad in (lambda: ops.blockdiag_forward(g, torch.ones((L + 1, 4, 6), device=dev), X, 2),
                lambda: ops.blockdiag_forward(g, Qb, X, 0),
                lambda: ops.blockdiag_forward(g, Qb, X, 4),                       # 4 does not divide H = 6
                lambda: ops.blockdiag_forward(g, Qb, X, 1),                       # D would be 4
                lambda: ops.blockdiag_forward(g, torch.ones((L, 65, 6), device=dev), torch.ones((V, 130), device=dev), 2),
                lambda: ops.blockdiag_forward(g, Qb, X[:5], 2),
                lambda: ops.blockdiag_forward(g, Qb, X, 2, edge_weight=torch.ones(3, device=dev)),
                lambda: ops.blockdiag_forward(g, Qb, X, 2, node_scale=torch.ones(V + 1, device=dev)),
                lambda: ops.blockdiag_forward(g, Qb, X, 2, out=torch.ones((V, 7), device=dev)),
                lambda: ops.blockdiag_backward(g, Qb, torch.ones((V, 5), device=dev), X, 2),
                lambda: ops.blockdiag_backward(g, Qb, torch.ones((V, 6), device=dev), None, 2),
                lambda: ops.blockdiag_backward(g, Qb, torch.ones((V, 6), device=dev), X[:, :3], 2)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.blockdiag_forward(g, Qb.double(), X, 2)
