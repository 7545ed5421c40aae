"""tfgnn_graph_scales_edge_dropout on the device: the keep pattern against tests/edge_dropout_reference.py in both edge orders,
and the values pinned to code that exists without the feature - tfgnn_graph_scales on the graph made of the kept edges, bit for
bit - instead of to a host guess at device rounding.  The kept counts are also recovered from the values as integers.

Every case with V >= 50 has an edge type without edges (type L - 2 when L >= 3), node 7 without in-edges, self loops and
duplicated edges.  The hub case (V = 50) gives node 2 >= 2000 in-edges (buckets that cross many 64-edge chunks of the kernel's
walk) and nodes 10 .. 15 in-degrees of exactly 31, 32, 33, 511, 512, 513."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import dropout_reference as dr
from tests import edge_dropout_reference as ref

pytestmark = pytest.mark.gpu

STRADDLE = (31, 32, 33, 511, 512, 513)
CASES = [(V, L) for V in (1, 2, 50, 3001) for L in (1, 4, 37)]
COMBOS = [(normalize, mode) for normalize in (False, True) for mode in (0, 1, 2)]
SEED = 0x5EED0000ED6E


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
            add(rng.choice(srcs, 700), np.full(700, 2))    # a row of eleven chunks
            add(np.full(40, 3), rng.choice(tgts, 40))
    return [np.concatenate(p).astype(np.int32) if p else np.zeros((0, 2), np.int32) for p in per_type]


@functools.lru_cache(maxsize=None)
def _graph_case(V, L):
    hub = V == 50
    rng = np.random.default_rng(104729 * V + 131 * L + int(hub))
    adjs = _edges(V, L, hub, rng)
    indeg = np.zeros(V, dtype=np.int64)
    for a in adjs:
        np.add.at(indeg, a[:, 1], 1)
    if V >= 50:
        assert indeg[7] == 0 and (L < 3 or adjs[L - 2].shape[0] == 0)
    if hub:
        assert indeg[2] >= 2000 and tuple(indeg[10:16]) == STRADDLE
    return adjs


def _zero_type(adjs, V):
    """the type that stays at rate 0 in the "extreme" set: the non-empty type most nodes with in-edges receive nothing of, so that
    a node can lose every edge although one type keeps all of its own; where every node receives every non-empty type (the
    hubs' graph with 4 types) the type without edges; none with a single type"""
    L = len(adjs)
    if L == 1:
        return None
    full = np.zeros((V, L), dtype=np.int64)
    for l, a in enumerate(adjs):
        np.add.at(full[:, l], a[:, 1], 1)
    lacking = ((full == 0) & (full.sum(axis=1, keepdims=True) > 0)).sum(axis=0)
    live = [l for l in range(L) if adjs[l].shape[0] > 0 and lacking[l] > 0]
    if live:
        return max(live, key=lambda l: (lacking[l], l))
    return L - 2 if L >= 3 else L - 1


def _rate_sets(adjs, V):
    L = len(adjs)
    extreme = [0.999] * L
    zero = _zero_type(adjs, V)
    if zero is not None:
        extreme[zero] = 0.0  # one type at 0 next to the others at 0.999
    return {"half": [0.5] * L, "paper": [0.2] + [0.4] * (L - 1), "extreme": extreme, "zero": [0.0] * L}


def _plain_device_scales(g, normalize, mode):
    """tfgnn_graph_scales, every array -> (node_scale, by_src, by_dst) as numpy"""
    from tf2_gnn_amd import _lib, ops

    dev = g.device
    row = torch.empty(g.num_nodes * g.num_edge_types, dtype=torch.float32, device=dev)
    ns = torch.empty(g.num_nodes, dtype=torch.float32, device=dev)
    ews = torch.empty(g.num_edges, dtype=torch.float32, device=dev)
    ewd = torch.empty(g.num_edges, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().tfgnn_graph_scales(g._h, int(normalize), mode, ops._ptr(row), ops._ptr(ns), ops._ptr(ews), ops._ptr(ewd),
                                              ops._stream()))
    return ns.cpu().numpy(), ews.cpu().numpy(), ewd.cpu().numpy()


def _eids(g):
    from tf2_gnn_amd import ops

    return (g.array(ops.G_EID_BY_DST).cpu().numpy().astype(np.int64), g.array(ops.G_EID_BY_SRC).cpu().numpy().astype(np.int64))


def _by_eid(values, eid):
    out = np.full(eid.shape[0], np.float32(np.nan), dtype=np.float32)
    out[eid] = values
    return out


def _dropped(g, normalize, mode, rates_dev, seed, eid_d, eid_s):
    from tf2_gnn_amd import ops

    ns, ews, ewd = ops.graph_scales_edge_dropout(g, normalize, mode, rates_dev, seed)
    return ns.cpu().numpy(), _by_eid(ews.cpu().numpy(), eid_s), _by_eid(ewd.cpu().numpy(), eid_d)


@pytest.mark.parametrize("V,L", CASES)
def test_pattern_and_values_in_both_edge_orders(dev, V, L):
    from tf2_gnn_amd import ops

    adjs = _graph_case(V, L)
    per = [a.shape[0] for a in adjs]
    t, tgt = ref.edge_types(adjs), ref.edge_targets(adjs)
    full = np.zeros((V, L), dtype=np.int64)
    np.add.at(full, (tgt, t), 1)
    g = ops.Graph([torch.from_numpy(a).to(dev) for a in adjs], V)
    eid_d, eid_s = _eids(g)
    assert np.array_equal(np.sort(eid_d), np.arange(sum(per))) and np.array_equal(np.sort(eid_s), np.arange(sum(per)))
    epoch = ops.dropout_epoch()
    before = ops.edge_dropout_launch_counts()["edge_dropout_scales"]
    launches = 0
    for name, rates in _rate_sets(adjs, V).items():
        rates_dev = torch.tensor(rates, dtype=torch.float32, device=dev)
        keep = ref.keep_edges(per, rates, SEED, epoch)
        kept_factor = np.array([dr.scale(r) for r in rates], dtype=np.float32)
        r0 = ref.scales_of_kept(adjs, V, keep, True, 1, kept_factor)
        if name == "extreme":  # whole buckets - and with the hubs' graph whole nodes - lose every edge
            assert ((full > 0) & (r0.c == 0)).any()
            if V == 50:
                assert ((full.sum(axis=1) > 0) & (r0.n == 0)).any()
        if name == "zero":
            assert keep.all()
            g2 = g
        else:
            assert V < 50 or not keep.all()
            filtered, first = [], 0
            for a in adjs:
                filtered.append(a[keep[first:first + a.shape[0]]])
                first += a.shape[0]
            g2 = ops.Graph([torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in filtered], V)
        eid2_d, eid2_s = _eids(g2)
        for normalize, mode in COMBOS:
            ns, by_src, by_dst = _dropped(g, normalize, mode, rates_dev, SEED, eid_d, eid_s)
            launches += 1
            what = (name, normalize, mode)
            assert np.isfinite(ns).all() and np.isfinite(by_src).all() and np.isfinite(by_dst).all(), what
            # 1. the pattern, in both edge orders
            assert np.array_equal(by_dst != 0, keep) and np.array_equal(by_src != 0, keep), what
            # 2./3. the values: tfgnn_graph_scales' on the graph of the kept edges (all rates 0: on the graph itself), bit for bit
            ns2, src2, dst2 = _plain_device_scales(g2, normalize, mode)
            src2, dst2 = _by_eid(src2, eid2_s), _by_eid(dst2, eid2_d)
            assert np.array_equal(ns.view(np.uint32), ns2.view(np.uint32)), what
            if normalize or mode != 0:
                assert np.array_equal(by_dst[keep].view(np.uint32), dst2.view(np.uint32)), what
                assert np.array_equal(by_src[keep].view(np.uint32), src2.view(np.uint32)), what
            else:  # a plain sum: no count divides, kept edges carry float32 1 / (1 - rate of their type)
                want = kept_factor[t[keep]]
                assert np.array_equal(by_dst[keep].view(np.uint32), want.view(np.uint32)), what
                assert np.array_equal(by_src[keep].view(np.uint32), want.view(np.uint32)), what
                assert name != "zero" or (np.all(dst2 == 1.0) and np.all(src2 == 1.0))
            # the kept counts, recovered as integers, against the reference's
            if normalize:
                assert np.array_equal(np.rint(1.0 / by_dst[keep].astype(np.float64)).astype(np.int64), r0.c[tgt[keep], t[keep]]), what
            if mode == 1:
                assert np.array_equal(np.rint(1.0 / ns.astype(np.float64)).astype(np.int64), np.maximum(r0.n, 1)), what
            if mode == 0:
                assert np.all(ns == 1.0), what
            assert np.all(ns[r0.n == 0] == 1.0), what
    assert ops.edge_dropout_launch_counts()["edge_dropout_scales"] - before == launches


def test_every_epoch_is_another_draw(dev):
    from tf2_gnn_amd import ops

    V, L = 50, 4
    adjs = _graph_case(V, L)
    per = [a.shape[0] for a in adjs]
    rates = _rate_sets(adjs, V)["paper"]
    g = ops.Graph([torch.from_numpy(a).to(dev) for a in adjs], V)
    eid_d, eid_s = _eids(g)
    rates_dev = torch.tensor(rates, dtype=torch.float32, device=dev)
    old = ops.dropout_epoch()
    patterns = []
    try:
        for k in (3, 1000003):
            ops.dropout_epoch_set(k)
            assert ops.dropout_epoch() == k
            _, by_src, by_dst = _dropped(g, True, 1, rates_dev, SEED, eid_d, eid_s)
            keep = ref.keep_edges(per, rates, SEED, k)
            assert np.array_equal(by_dst != 0, keep) and np.array_equal(by_src != 0, keep), k
            patterns.append(keep)
    finally:
        ops.dropout_epoch_set(old)
    assert ops.dropout_epoch() == old
    assert not np.array_equal(patterns[0], patterns[1])
    # another seed is another draw, the same seed the same one
    _, _, a = _dropped(g, True, 1, rates_dev, SEED, eid_d, eid_s)
    _, _, b = _dropped(g, True, 1, rates_dev, SEED, eid_d, eid_s)
    _, _, c = _dropped(g, True, 1, rates_dev, SEED + 1, eid_d, eid_s)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and not np.array_equal(a != 0, c != 0)


def test_degenerate_graphs_and_refusals(dev):
    from tf2_gnn_amd import _lib, ops

    for V, L in ((1, 3), (5, 2), (0, 2)):
        g = ops.Graph([torch.zeros((0, 2), dtype=torch.int32, device=dev) for _ in range(L)], V)
        rates = torch.full((L,), 0.5, dtype=torch.float32, device=dev)
        for normalize, mode in COMBOS:
            ns, ews, ewd = ops.graph_scales_edge_dropout(g, normalize, mode, rates, 1)
            assert ns.shape == (V,) and ews.shape == (0,) and ewd.shape == (0,)
            assert bool((ns == 1.0).all())
    torch.cuda.synchronize()
    g = ops.Graph([torch.tensor([[0, 1], [2, 3]], dtype=torch.int32, device=dev) for _ in range(2)], 6)
    rates = torch.zeros(2, dtype=torch.float32, device=dev)
    for bad in (lambda: ops.graph_scales_edge_dropout(g, True, 1, torch.zeros(3, device=dev), 0),
                lambda: ops.graph_scales_edge_dropout(g, True, 3, rates, 0)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.graph_scales_edge_dropout(g, True, 1, rates.double(), 0)
    with pytest.raises(RuntimeError):
        ops.graph_scales_edge_dropout(g, True, 1, rates.cpu(), 0)
    lib = _lib.load()
    buf = torch.empty(8, dtype=torch.float32, device=dev)
    p, r = ops._ptr(buf), ops._ptr(rates)
    g.ensure(ops.G_PART_EDGE_MAPS)
    assert lib.tfgnn_graph_scales_edge_dropout(None, 1, 1, r, 0, p, p, p, ops._stream()) == -1
    assert lib.tfgnn_graph_scales_edge_dropout(g._h, 1, 3, r, 0, p, p, p, ops._stream()) == -1
    assert lib.tfgnn_graph_scales_edge_dropout(g._h, 1, 1, None, 0, p, p, p, ops._stream()) == -1
    assert lib.tfgnn_graph_scales_edge_dropout(g._h, 1, 1, r, 0, None, p, p, ops._stream()) == -1
    assert lib.tfgnn_graph_scales_edge_dropout(g._h, 1, 1, r, 0, p, None, p, ops._stream()) == -1
    assert lib.tfgnn_graph_scales_edge_dropout(g._h, 1, 1, r, 0, p, p, None, ops._stream()) == -1
    bare = ops.Graph([torch.tensor([[0, 1]], dtype=torch.int32, device=dev)], 2, parts=ops.G_PART_PLAN_NODE)
    assert lib.tfgnn_graph_scales_edge_dropout(bare._h, 1, 1, r, 0, p, p, p, ops._stream()) == -1
    assert "lacks part" in lib.tfgnn_last_error().decode()
    # the wrapper builds the missing part itself (outside a capture)
    ns, ews, ewd = ops.graph_scales_edge_dropout(bare, False, 1, torch.zeros(1, device=dev), 0)
    assert ns.tolist() == [1.0, 1.0] and ews.tolist() == [1.0] and ewd.tolist() == [1.0]
