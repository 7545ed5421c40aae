"""The numpy reference of the neighbour sampling contract (tests/neighbor_sample_reference.py) on its own: the invariants
of a sample, the exact-hop property - at full fanout a K-layer network gives the seeds the same rows on the subgraph as on
the whole graph - and the uniformity of the keyed positions.  CPU-only; the device sampler is compared with this reference
in tests/test_gpu_neighbor_sample.py."""
import math

import numpy as np
import pytest

from tests import neighbor_sample_reference as ref
from tests.neighbor_sample_cases import HUB, SEED_ORDER, device_test_graph, exact_hop_graph


@pytest.fixture(scope="module")
def graph():
    return device_test_graph()


def test_hashes_and_widths_by_hand():
    assert ref.lowbias32(0) == 0
    x = 1 * 0x7FEB352D & ref.M32
    x ^= x >> 15
    x = x * 0x846CA68B & ref.M32
    assert ref.lowbias32(1) == x ^ (x >> 16)
    assert [ref.feistel_bits(d) for d in (2, 3, 4, 5, 16, 17, 64, 65, 256, 257, 300, 2 ** 31)] == [2, 2, 2, 4, 4, 6, 6, 8, 8, 10, 10, 32]
    s0, s1 = ref.seed_words(0)
    assert (s1 << 32 | s0) == 0xE220A8397B1DCDAF  # splitmix64's first output for the state 0


@pytest.mark.parametrize("d", [2, 3, 4, 5, 16, 17, 64, 65, 256, 257, 300])
def test_positions_are_distinct_and_the_permutation_is_a_bijection(d):
    for k in (0, 1, 0xDEADBEEF, 0xFFFFFFFF):
        assert sorted(ref.permute(k, d, j) for j in range(d)) == list(range(d))
        for c in {1, d // 2, d - 1} - {0}:
            p = ref.positions(k, d, c)
            assert len(p) == c == len(set(p)) and all(0 <= x < d for x in p)
        assert ref.positions(k, d, d) == list(range(d))
    keys = np.array([ref.row_key(3, 4, v, 1) for v in range(50)])
    many = ref.positions_many(keys, d, d - 1)
    assert many.tolist() == [ref.positions(int(k), d, d - 1) for k in keys]


@pytest.mark.parametrize("fanouts", [[3, 2], [0, 5], [-1, -1, -1], [2]])
@pytest.mark.parametrize("S", [1, 7, 64])
def test_sample_invariants(graph, S, fanouts):
    edges, in_ptr, in_src = graph
    seeds = SEED_ORDER[:S]
    s = ref.neighbor_sample(in_ptr, in_src, seeds, fanouts, seed=11)
    K = len(fanouts)
    assert s.status == 0
    assert s.nodes[:S].tolist() == seeds  # seeds first
    assert len(set(s.nodes.tolist())) == len(s.nodes)  # unique
    assert s.hop_ptr.shape == (K + 2,) and s.hop_ptr[0] == 0 and s.hop_ptr[1] == S and s.hop_ptr[-1] == len(s.nodes)
    assert (np.diff(s.hop_ptr) >= 0).all()
    hop_of = np.searchsorted(s.hop_ptr, np.arange(len(s.nodes)), side="right") - 1  # the hop that first reached a row
    for t, adj in enumerate(s.adjacency_lists):
        assert adj.dtype == np.int32 and adj.shape[1] == 2
        if len(adj) == 0:
            continue
        assert adj.min() >= 0 and adj.max() < len(s.nodes)
        assert (hop_of[adj[:, 1]] < K).all()  # every target was a frontier node of an earlier hop ...
        assert (hop_of[adj[:, 0]] <= hop_of[adj[:, 1]] + 1).all()  # ... and its sources were known one hop later at the latest
        assert (np.diff(hop_of[adj[:, 1]]) >= 0).all()  # a type's edges: hop by hop
        # every edge is an edge of the graph
        have = set(map(tuple, edges[t].tolist()))
        assert all((int(s.nodes[a]), int(s.nodes[b])) in have for a, b in adj)
    # every row of a frontier node has exactly min(d, f) edges at distinct positions
    for h in range(1, K + 1):
        f = fanouts[h - 1]
        for v in s.nodes[s.hop_ptr[h - 1]:s.hop_ptr[h]].tolist():
            for t in range(3):
                first, d = int(in_ptr[t][v]), int(in_ptr[t][v + 1] - in_ptr[t][v])
                c = ref.taken(d, f)
                assert c == (d if f < 0 else min(d, f))
                pos = ref.positions(ref.row_key(*ref.seed_words(11), v, t), d, c) if c else []
                assert len(set(pos)) == c
                assert s.drawn[(v, t)] == [int(in_src[t][first + p]) for p in pos]
    if fanouts[0] == 0:
        assert s.hop_ptr.tolist() == [0] + [S] * (K + 1) and all(len(a) == 0 for a in s.adjacency_lists)


def test_same_key_same_sample_another_key_another(graph):
    _, in_ptr, in_src = graph
    a = ref.neighbor_sample(in_ptr, in_src, SEED_ORDER[:7], [3, 2], seed=5)
    b = ref.neighbor_sample(in_ptr, in_src, SEED_ORDER[:7], [3, 2], seed=5)
    c = ref.neighbor_sample(in_ptr, in_src, SEED_ORDER[:7], [3, 2], seed=6)
    assert np.array_equal(a.nodes, b.nodes) and all(np.array_equal(x, y) for x, y in zip(a.adjacency_lists, b.adjacency_lists))
    assert not (np.array_equal(a.nodes, c.nodes) and all(np.array_equal(x, y) for x, y in zip(a.adjacency_lists, c.adjacency_lists)))
    assert ref.neighbor_sample(in_ptr, in_src, [3, 4, 3], [1], seed=0).status == 4


def test_the_draw_of_a_row_does_not_depend_on_the_hop_that_reaches_it(graph):
    """the hub as a seed (drawn at hop 1) and as an in-neighbour of the seed 7 (8 -> 7: drawn at hop 2): the same sources"""
    _, in_ptr, in_src = graph
    as_seed = ref.neighbor_sample(in_ptr, in_src, [HUB], [3], seed=9)
    later = ref.neighbor_sample(in_ptr, in_src, [7], [-1, 3], seed=9)
    at = later.nodes.tolist().index(HUB)
    assert later.hop_ptr[1] <= at < later.hop_ptr[2]  # first reached at hop 1, a frontier node of hop 2
    for t in range(3):
        assert later.drawn[(HUB, t)] == as_seed.drawn[(HUB, t)]
    assert len(as_seed.drawn[(HUB, 0)]) == 3


def _network(features, adjacency_lists, weights, layers):
    """sum aggregation per type, a weight matrix per (layer, type), a clip: float64 on small integers - every sum is exact"""
    h = features
    for l in range(layers):
        out = np.zeros((h.shape[0], weights[l][0].shape[1]))
        for t, adj in enumerate(adjacency_lists):
            m = np.zeros_like(h)
            np.add.at(m, adj[:, 1], h[adj[:, 0]])
            out += m @ weights[l][t]
        h = np.clip(out, -40.0, 40.0)
    return h


def test_exact_hop_property():
    V, K = 300, 3
    edges = exact_hop_graph(V)
    csr = [ref.build_in_csr(e, V) for e in edges]
    rng = np.random.default_rng(3)
    seeds = [5] + rng.choice(np.arange(6, V), size=8, replace=False).tolist()  # the hub and 8 others
    s = ref.neighbor_sample([c[0] for c in csr], [c[1] for c in csr], seeds, [-1] * K, seed=1)
    assert len(s.adjacency_lists[1]) >= 400 and len(s.adjacency_lists[2]) == 0
    feats = rng.integers(-2, 3, size=(V, 6)).astype(np.float64)
    weights = [[rng.integers(-1, 2, size=(6, 6)).astype(np.float64) for _ in range(3)] for _ in range(K)]
    full = _network(feats, edges, weights, K)
    sub = _network(feats[s.nodes], s.adjacency_lists, weights, K)
    assert np.abs(full).max() > 1.0  # not a network of zeros
    assert np.array_equal(sub[:len(seeds)], full[seeds])
    # one hop short: the subgraph is then NOT enough (the test can fail)
    short = ref.neighbor_sample([c[0] for c in csr], [c[1] for c in csr], seeds, [-1] * (K - 1), seed=1)
    assert not np.array_equal(_network(feats[short.nodes], short.adjacency_lists, weights, K)[:len(seeds)], full[seeds])


@pytest.mark.parametrize("d,f", [(5, 2), (9, 4), (17, 16), (37, 5), (65, 10), (257, 25), (300, 10)])
def test_marginal_uniformity(d, f):
    """20 000 row keys: how often each of the d positions is among the f drawn; chi^2 against n f / d per position must stay
    below dof + 6 sqrt(2 dof), dof = d - 1 (draws without replacement are under-dispersed: the cap is conservative)."""
    n = 20000
    s0, s1 = ref.seed_words(2024)
    v = np.arange(n, dtype=np.uint64)
    keys = ref.lowbias32_many((ref.lowbias32_many(v ^ np.uint64(s0)) + np.uint64(3 * ref.GOLDEN)) & np.uint64(ref.M32)) ^ np.uint64(s1)
    assert int(keys[17]) == ref.row_key(s0, s1, 17, 2)
    pos = ref.positions_many(keys, d, f)
    assert (np.sort(pos, axis=1)[:, 1:] != np.sort(pos, axis=1)[:, :-1]).all()  # distinct within a row
    counts = np.bincount(pos.reshape(-1), minlength=d)
    expected = n * f / d
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    dof = d - 1
    cap = dof + 6 * math.sqrt(2 * dof)
    print(f"d={d} f={f}: chi^2 {chi2:.1f}, cap {cap:.1f}")
    assert chi2 < cap
