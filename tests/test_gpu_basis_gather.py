"""tfgnn_basis_gather_forward / tfgnn_basis_gather_backward on the device against the op-level loops of
tests/rgcn_basis_reference.py (float64, with the bound an fp32 evaluation in any order is held to).  Not run per GEMM mode: no
product is involved.

Two input families.  EXACT: X, dZ and coeff small integers, no weights - every partial sum is an integer below 2^24 (asserted
from the degrees and the ranges), so every order gives the same fp32 value and the results must equal the reference bit for
bit.  FLOAT: randn inputs with the degree normalisation and the mean aggregator's scales as tfgnn_graph_scales computes them
(read back and handed to the reference as its inputs): every value within its bound, an error where the bound is 0 must be 0.

Every case with V >= 50 has an edge type without edges (type L - 2 when L >= 3), node 7 without in-edges, node 9 without
out-edges, self loops and duplicated edges.  The hub cases (V = 50) give node 2 >= 2000 in-edges and node 3 >= 2000 out-edges
(several 512-edge items each) and nodes 10 .. 15 in-degrees - and 16 .. 21 out-degrees - of exactly 31, 32, 33, 511, 512, 513,
which straddle the plan's long-row threshold (32) and its item size (512).  X and dZ sit inside wider arrays; Z and dX are
written into wider arrays whose other columns must stay as they were."""
import functools

import numpy as np
import pytest
import torch

from tests import rgcn_basis_reference as ref
from tests.helpers import KernelsUsed

pytestmark = pytest.mark.gpu

PAD_LEFT, PAD_RIGHT = 4, 4  # rows stay 16-byte aligned where the width allows it; _MISALIGNED cases shift them by one float
_MISALIGNED = {(3001, 64, 37, 8), (50, 320, 37, 8)}  # D % 4 == 0 on the scalar path
SENTINEL = 7.5
STRADDLE = (31, 32, 33, 511, 512, 513)
# (V, D, L, B, hub)
CASES = [
    (1, 1, 1, 1, False), (1, 64, 4, 2, False), (2, 3, 4, 8, False), (2, 1024, 1, 2, False),
    (50, 64, 4, 8, True), (50, 65, 37, 2, True), (50, 3, 256, 64, True), (50, 320, 37, 8, True), (50, 1, 4, 1, False),
    (50, 1024, 4, 2, False), (50, 128, 256, 8, False),
    (3001, 64, 37, 8, False), (3001, 65, 4, 2, False), (3001, 320, 4, 1, False), (3001, 3, 1, 64, False),
]


def _edges(V, L, hub, rng):
    """per type an int32 [E_l, 2] array of (source, target)"""
    per_type = [[] for _ in range(L)]
    empty = L - 2 if L >= 3 else None
    types = [l for l in range(L) if l != empty]

    def add(src, tgt):
        t = rng.choice(types, size=len(src))
        for l in types:
            sel = t == l
            if sel.any():
                per_type[l].append(np.stack([src[sel], tgt[sel]], axis=1))

    if V < 50:
        n = 5 * V
        add(rng.integers(0, V, n), rng.integers(0, V, n))
        add(np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int64))  # self loops, twice
    else:
        fixed_in, fixed_out = (set(range(10, 16)), set(range(16, 22))) if hub else (set(), set())
        srcs = np.array([v for v in range(V) if v != 9 and v not in fixed_out])
        tgts = np.array([v for v in range(V) if v != 7 and v not in fixed_in])
        n = 3 * V if V > 50 else 600
        s, t = rng.choice(srcs, n), rng.choice(tgts, n)
        add(s, t)
        add(s[:20], t[:20])                               # duplicated edges
        loops = np.array([0, 1, 4, 5]); add(loops, loops)  # self loops
        if hub:
            add(rng.choice(srcs, 2100), np.full(2100, 2))
            add(np.full(2050, 3), rng.choice(tgts, 2050))
            for node, deg in zip(range(10, 16), STRADDLE):
                add(rng.choice(srcs, deg), np.full(deg, node))
            for node, deg in zip(range(16, 22), STRADDLE):
                add(np.full(deg, node), rng.choice(tgts, deg))
        elif V > 1000:
            add(rng.choice(srcs, 700), np.full(700, 2))    # two items
            add(np.full(40, 3), rng.choice(tgts, 40))
    return [np.concatenate(p).astype(np.int32) if p else np.zeros((0, 2), np.int32) for p in per_type]


@functools.lru_cache(maxsize=None)
def _graph_case(V, L, hub):
    rng = np.random.default_rng(104729 * V + 131 * L + int(hub))
    adjs = _edges(V, L, hub, rng)
    indeg, outdeg = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int64)
    for a in adjs:
        np.add.at(outdeg, a[:, 0], 1)
        np.add.at(indeg, a[:, 1], 1)
    if V >= 50:
        assert indeg[7] == 0 and outdeg[9] == 0 and (L < 3 or adjs[L - 2].shape[0] == 0)
    if hub:
        assert indeg[2] >= 2000 and outdeg[3] >= 2000
        assert tuple(indeg[10:16]) == STRADDLE and tuple(outdeg[16:22]) == STRADDLE
    return adjs, indeg, outdeg


@functools.lru_cache(maxsize=None)
def _case(family, V, D, L, B, hub):
    """inputs and the (shared, read-only) references of one case; the FLOAT family's scales come from the device run"""
    adjs, indeg, outdeg = _graph_case(V, L, hub)
    rng = np.random.default_rng(7919 * V + 31 * D + 7 * L + B)
    if family == "exact":
        X = rng.integers(-2, 3, size=(V, D)).astype(np.float32)
        coeff = rng.integers(-2, 3, size=(L, B)).astype(np.float32)
        dZ = rng.integers(-1, 2, size=(V, B * D)).astype(np.float32)
        # every partial sum of every result is an integer of magnitude below 2^24: exact in fp32, whatever the order
        assert indeg.max(initial=0) * 2 * 2 < 2 ** 24 and outdeg.max(initial=0) * B * 2 * 1 < 2 ** 24
        assert max(a.shape[0] for a in adjs) * D * 2 * 1 < 2 ** 24
    else:
        X = rng.standard_normal((V, D)).astype(np.float32)
        coeff = rng.standard_normal((L, B)).astype(np.float32)
        dZ = rng.standard_normal((V, B * D)).astype(np.float32)
    return {"adjs": adjs, "X": X, "coeff": coeff, "dZ": dZ, "ref": {}}


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
@pytest.mark.parametrize("V,D,L,B,hub", CASES)
def test_basis_gather_forward_and_backward(dev, family, V, D, L, B, hub):
    from tf2_gnn_amd import ops

    c = _case(family, V, D, L, B, hub)
    adjs = c["adjs"]
    g = ops.Graph([torch.from_numpy(a).to(dev) for a in adjs], V)
    ew_d = ew_s = ns = s = s_src = m = None
    if family == "float":
        sc, s, s_src, m = _scale_tables(g, V, L)
        ew_d, ew_s, ns = sc.edge_weight_by_dst, sc.edge_weight_by_src, sc.node_scale
    if not c["ref"]:
        c["ref"]["Z"] = ref.gather_forward(adjs, V, c["coeff"], c["X"], s, m)
        c["ref"]["dX"] = ref.gather_backward_dx(adjs, V, c["coeff"], c["dZ"], s_src)
        c["ref"]["dcoeff"] = ref.gather_backward_dcoeff(adjs, V, (L, B), c["X"], c["dZ"], s, m)
    rZ, rdX, rdc = (c["ref"][k] for k in ("Z", "dX", "dcoeff"))  # shared between the runs of a case, never written
    for val, _ in (rZ, rdX, rdc):
        assert family == "float" or np.abs(val).max(initial=0) < 2 ** 24

    coeff = torch.from_numpy(c["coeff"]).to(dev)
    left = PAD_LEFT - 1 if (V, D, L, B) in _MISALIGNED else PAD_LEFT
    Xw, X = _wide(c["X"], dev, left)
    dZw, dZ = _wide(c["dZ"], dev, left)
    Zw, Z = _wide(np.zeros((V, B * D), np.float32), dev, left)
    dXw, dX = _wide(np.zeros((V, D), np.float32), dev, left)
    Z.fill_(-3.0), dX.fill_(-3.0)
    before = ops.basis_launch_counts()
    with KernelsUsed() as used:
        assert ops.basis_gather_forward(g, coeff, X, edge_weight=ew_d, node_scale=ns, out=Z) is Z
        Z1 = Z.cpu().numpy().copy()
        Z.fill_(5.0)
        ops.basis_gather_forward(g, coeff, X, edge_weight=ew_d, node_scale=ns, out=Z)
        kw = dict(edge_weight_by_dst=ew_d, edge_weight_by_src=ew_s, node_scale=ns)
        got_dX, got_dc = ops.basis_gather_backward(g, coeff, dZ, X, out_dx=dX, **kw)
        assert got_dX is dX
        dX1, dc1 = dX.cpu().numpy().copy(), got_dc.cpu().numpy().copy()
        dX_alone, none = ops.basis_gather_backward(g, coeff, dZ, None, want_dcoeff=False, **kw)
        assert none is None
        none, dc_alone = ops.basis_gather_backward(g, coeff, dZ, X, want_dx=False, **kw)
        assert none is None
        dX.fill_(5.0)
        _, dc2 = ops.basis_gather_backward(g, coeff, dZ, X, out_dx=dX, **kw)
    after = ops.basis_launch_counts()
    assert all(after[k] > before[k] for k in ("basis_fwd", "basis_dx", "basis_dcoeff")), (before, after)
    assert not any(used.delta.values()), used.delta  # no product (or plain gather) family moved

    # the same bits: a second call, and each backward output alone or together with the other
    assert np.array_equal(Z1, Z.cpu().numpy()) and np.array_equal(dX1, dX.cpu().numpy()) and np.array_equal(dc1, dc2.cpu().numpy())
    assert np.array_equal(dX1, dX_alone.cpu().numpy()) and np.array_equal(dc1, dc_alone.cpu().numpy())
    assert all(_pads_untouched(w, left) for w in (Zw, dXw, Xw, dZw))
    assert np.array_equal(X.cpu().numpy(), c["X"]) and np.array_equal(dZ.cpu().numpy(), c["dZ"])

    figures = {}
    for name, got, (val, bound) in (("Z", Z1, rZ), ("dX", dX1, rdX), ("dcoeff", dc1, rdc)):
        err = np.abs(got.astype(np.float64) - val)
        figures[name] = (float(err.max(initial=0)), _ratio(err, bound))
    print(f"basis gather {family} V={V} D={D} L={L} B={B} hub={hub}: (max error, max error / bound) {figures}")
    for name, (err, ratio) in figures.items():
        if family == "exact":
            assert err == 0.0, (name, err)
        else:
            assert ratio <= 1.0, (name, err, ratio)
    if V >= 50:
        assert not Z1[7].any() and not dX1[9].any() and (L < 3 or not dc1[L - 2].any())


def test_no_edges_and_no_nodes_give_zeros(dev):
    from tf2_gnn_amd import ops

    L, B, D = 3, 4, 8
    coeff = torch.ones((L, B), device=dev)
    for V in (5, 0):
        g = ops.Graph([torch.zeros((0, 2), dtype=torch.int32, device=dev) for _ in range(L)], V, parts=ops.G_PART_PLAN_NODE)
        X = torch.ones((V, D), device=dev)
        Z = ops.basis_gather_forward(g, coeff, X, out=torch.full((V, B * D), 3.0, device=dev))
        dX, dc = ops.basis_gather_backward(g, coeff, torch.ones((V, B * D), device=dev), X,
                                           out_dx=torch.full((V, D), 3.0, device=dev))
        assert Z.shape == (V, B * D) and not Z.any() and dX.shape == (V, D) and not dX.any()
        assert dc.shape == (L, B) and not dc.any()


def test_wrappers_refuse_bad_arguments_before_the_call(dev):
    from tf2_gnn_amd import ops

    V, L = 6, 2
    g = ops.Graph([torch.tensor([[0, 1], [2, 3]], dtype=torch.int32, device=dev) for _ in range(L)], V)
    X = torch.ones((V, 4), device=dev)
    coeff = torch.ones((L, 3), device=dev)
    for bad in (lambda: ops.basis_gather_forward(g, torch.ones((L + 1, 3), device=dev), X),
                lambda: ops.basis_gather_forward(g, torch.ones((L, 65), device=dev), X),
                lambda: ops.basis_gather_forward(g, torch.ones((L, 0), device=dev), X),
                lambda: ops.basis_gather_forward(g, coeff, X[:5]),
                lambda: ops.basis_gather_forward(g, coeff, X, edge_weight=torch.ones(3, device=dev)),
                lambda: ops.basis_gather_forward(g, coeff, X, node_scale=torch.ones(V + 1, device=dev)),
                lambda: ops.basis_gather_forward(g, coeff, X, out=torch.ones((V, 11), device=dev)),
                lambda: ops.basis_gather_backward(g, coeff, torch.ones((V, 13), device=dev), X),
                lambda: ops.basis_gather_backward(g, coeff, torch.ones((V, 12), device=dev), None),
                lambda: ops.basis_gather_backward(g, coeff, torch.ones((V, 12), device=dev), X[:, :3])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.basis_gather_forward(g, coeff.double(), X)
