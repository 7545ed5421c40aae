"""tfgnn_neighbor_sample and tfgnn_gather_node_rows on the device against the numpy reference of the contract
(tests/neighbor_sample_reference.py): nodes, hop_ptr, counts and every adjacency list must be EQUAL.  The graph
(tests/neighbor_sample_cases.py: V = 200, three processed types, one empty, duplicate edges) has rows of in-degree 0, f and
f + 1, rows across the Feistel widths and the wave boundaries (4, 5, 16, 17, 64, 65, 256, 257), a hub of 300 in-edges, and
seeds that are each other's neighbours.  PARITY UNPINNED: the reference has no sampler."""
import numpy as np
import pytest
import torch

from tests import neighbor_sample_reference as ref
from tests.neighbor_sample_cases import HUB, SEED_ORDER, device_test_graph

pytestmark = pytest.mark.gpu

V = 200
GUARD = 0x5A5A5A5A


@pytest.fixture(scope="module")
def graph():
    return device_test_graph(V)


@pytest.fixture(scope="module")
def store(graph):
    from tf2_gnn_amd.data import NeighborStore, PackedFold

    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    edges, in_ptr, in_src = graph
    feats = np.random.default_rng(0).standard_normal((V, 5)).astype(np.float32)
    fold = PackedFold([V], feats, [[len(e)] for e in edges], edges)
    s = NeighborStore(fold, torch.device("cuda", 0))
    for t in range(3):  # the store's in-CSR is the reference's
        assert np.array_equal(s.in_ptr[t].cpu().numpy(), in_ptr[t]) and np.array_equal(s.in_src[t].cpu().numpy(), in_src[t])
    return s


def _seeds(S, dev):
    return torch.tensor(SEED_ORDER[:S], dtype=torch.int32, device=dev)


def _assert_equal(got, want, what):
    assert got.status == want.status, what
    assert got.nodes.cpu().numpy().tolist() == want.nodes.tolist(), what
    assert got.hop_ptr.tolist() == want.hop_ptr.tolist(), what
    for t, (a, b) in enumerate(zip(got.adjacency_lists, want.adjacency_lists)):
        assert a.dtype == torch.int32 and tuple(a.shape) == b.shape, (what, t, tuple(a.shape), b.shape)
        assert np.array_equal(a.cpu().numpy(), b), (what, t)


@pytest.mark.parametrize("fanouts", [[3, 2], [0, 5], [-1, -1, -1], [2], [5, 0, 3]])
@pytest.mark.parametrize("S", [1, 7, 64, 65])
def test_sample_equals_the_reference(dev, graph, store, S, fanouts):
    from tf2_gnn_amd import ops

    _, in_ptr, in_src = graph
    before = ops.sample_launch_counts()
    got = ops.neighbor_sample(store, _seeds(S, dev), fanouts, seed=1234 + S)
    assert ops.sample_launch_counts() == (before[0] + 3 + 6 * len(fanouts), before[1])  # the documented launch count
    want = ref.neighbor_sample(in_ptr, in_src, SEED_ORDER[:S], fanouts, seed=1234 + S)
    _assert_equal(got, want, (S, fanouts))
    assert got.num_seeds == S and got.status == 0
    assert bool((store.local_id_table() == -1).all())
    if S >= 7 and fanouts[0] == 3:  # the rows the case is about were really sampled: the hub and d = 257 gave 3 of their edges
        targets = got.adjacency_lists[0][:, 1].cpu().numpy()
        assert (targets == 0).sum() == 3 and (targets == 1).sum() == 3  # local ids 0 and 1: the hub and node 7


def test_two_calls_back_to_back_on_one_workspace(dev, graph, store):
    """no synchronisation in between; the second call is wrong if the first did not restore the local-id table"""
    from tf2_gnn_amd import _lib, ops

    _, in_ptr, in_src = graph
    lib = _lib.load()
    first_seeds = _seeds(64, dev)
    second_seeds = torch.tensor(SEED_ORDER[30:95][::-1], dtype=torch.int32, device=dev)
    ws = store.workspace(V)
    a = ops.neighbor_sample(store, first_seeds, [-1, 4], seed=1)
    b = ops.neighbor_sample(store, second_seeds, [4, -1], seed=2)
    assert store.workspace(V) is ws  # one workspace
    _assert_equal(a, ref.neighbor_sample(in_ptr, in_src, SEED_ORDER[:64], [-1, 4], seed=1), "first")
    _assert_equal(b, ref.neighbor_sample(in_ptr, in_src, SEED_ORDER[30:95][::-1], [4, -1], seed=2), "second")
    assert bool((store.local_id_table() == -1).all())
    # the same key gives the same sample, another key another
    c = ops.neighbor_sample(store, second_seeds, [4, -1], seed=2)
    d = ops.neighbor_sample(store, second_seeds, [4, -1], seed=3)
    assert torch.equal(b.nodes, c.nodes) and all(torch.equal(x, y) for x, y in zip(b.adjacency_lists, c.adjacency_lists))
    assert not all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(b.adjacency_lists, d.adjacency_lists))
    assert lib.tfgnn_neighbor_sample_workspace_bytes(V, 3, V) == ws.numel() * 4


def _guarded(cap, width, dev):
    buf = torch.full(((cap + 16) * width,), GUARD, dtype=torch.int32, device=dev)
    return buf, (buf[:cap * width].view(cap, width) if width > 1 else buf[:cap])


@pytest.mark.parametrize("node_cap,edge_caps,bits", [(20, [2000, 2000, 0], 1), (V, [10, 700, 0], 2), (12, [9, 3, 0], 3)])
def test_small_capacities_set_the_overflow_bits_and_nothing_is_written_past_them(dev, graph, store, node_cap, edge_caps, bits):
    from tf2_gnn_amd import ops

    _, in_ptr, in_src = graph
    want = ref.neighbor_sample(in_ptr, in_src, SEED_ORDER[:7], [-1, -1], seed=5)
    assert (len(want.nodes) > 20) and len(want.adjacency_lists[0]) > 10 and len(want.adjacency_lists[0]) < 2000
    node_buf, nodes = _guarded(node_cap, 1, dev)
    adj_bufs, adj = zip(*[_guarded(c, 2, dev) for c in edge_caps])
    got = ops.neighbor_sample(store, _seeds(7, dev), [-1, -1], seed=5, out=(nodes, list(adj)))
    assert got.status == bits
    assert got.nodes.shape[0] <= node_cap and all(a.shape[0] <= c for a, c in zip(got.adjacency_lists, edge_caps))
    assert got.nodes[:7].cpu().tolist() == SEED_ORDER[:7]
    assert bool((node_buf[node_cap:] == GUARD).all())
    for buf, c in zip(adj_bufs, edge_caps):
        assert bool((buf[2 * c:] == GUARD).all())
    assert bool((store.local_id_table() == -1).all())  # restored after an overflow too
    # and the next call on the same workspace is right
    _assert_equal(ops.neighbor_sample(store, _seeds(7, dev), [-1, -1], seed=5), want, "after an overflow")


def test_repeated_and_outside_seeds_set_their_status_bits(dev, store):
    from tf2_gnn_amd import _lib, ops

    got = ops.neighbor_sample(store, torch.tensor([3, 4, 3], dtype=torch.int32, device=dev), [2], seed=0)
    assert got.status & _lib.SAMPLE_REPEATED_SEED and not got.status & _lib.SAMPLE_BAD_SEED
    got = ops.neighbor_sample(store, torch.tensor([3, V, -1], dtype=torch.int32, device=dev), [2], seed=0)
    assert got.status & _lib.SAMPLE_BAD_SEED and not got.status & _lib.SAMPLE_REPEATED_SEED
    assert bool((store.local_id_table() == -1).all())
    assert ops.neighbor_sample(store, torch.tensor([3, 4], dtype=torch.int32, device=dev), [2], seed=0).status == 0


def test_the_hub_row_is_the_same_at_hop_one_and_hop_two(dev, store):
    from tf2_gnn_amd import ops

    def hub_sources(sample):
        nodes = sample.nodes.cpu().numpy()
        at = int(np.flatnonzero(nodes == HUB)[0])
        adj = sample.adjacency_lists[0].cpu().numpy()
        return nodes[adj[adj[:, 1] == at, 0]].tolist()

    as_seed = ops.neighbor_sample(store, torch.tensor([HUB], dtype=torch.int32, device=dev), [3], seed=9)
    later = ops.neighbor_sample(store, torch.tensor([7], dtype=torch.int32, device=dev), [-1, 3], seed=9)
    assert len(hub_sources(as_seed)) == 3 and hub_sources(as_seed) == hub_sources(later)


# ---- the row gather ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("F", [1, 3, 4, 121, 128])
def test_gather_node_rows(dev, F, aligned):
    """bit-equal to features[nodes]; a seed_only column is zero below the seed rows; rows behind the outputs stay untouched;
    one launch.  ``aligned`` False: the store arrays start 4 bytes into an allocation, so the scalar path runs at every width."""
    from tf2_gnn_amd import ops

    rng = np.random.default_rng(F)
    store_nodes, n, S = 500, 300, 37  # several tiles at every width (256 rows at most per tile)
    widths = [F, 1, 4]

    def on_device(a):
        flat = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
        view = flat[0 if aligned else 1:][:a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        return view

    host = [rng.standard_normal((store_nodes, w)).astype(np.float32) for w in widths]
    host[0][3, 0] = np.nan  # bits, not values
    feats, weights, extra = (on_device(a) for a in host)
    assert (feats.data_ptr() % 16 == 0) == aligned
    ids = rng.integers(0, store_nodes, size=n).astype(np.int32)
    ids[:4] = [3, 499, 0, 3]
    nodes = torch.from_numpy(ids).to(dev)
    outs = [torch.full((n + 4, w), float("inf"), dtype=torch.float32, device=dev) for w in widths]
    before = ops.sample_launch_counts()
    nf, cols = ops.gather_node_rows(nodes, S, feats, [weights, extra], seed_only=[True, False], out=(outs[0][:n], [outs[1][:n], outs[2][:n]]))
    assert ops.sample_launch_counts() == (before[0], before[1] + 1)
    want = [a[ids] for a in host]
    want[1] = want[1].copy()
    want[1][S:] = 0.0
    for got, w in zip([nf] + cols, want):
        assert np.array_equal(got.cpu().numpy().view(np.int32), w.view(np.int32))
    for o in outs:
        assert bool(torch.isinf(o[n:]).all())
    # a node id outside the store: its row is skipped, the flag is set
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    nodes2 = nodes.clone()
    nodes2[5] = store_nodes
    out0 = torch.full((n, F), 7.0, dtype=torch.float32, device=dev)
    ops.gather_node_rows(nodes2, S, feats, out=(out0, []), bad_flag=bad)
    assert int(bad) == 1 and bool((out0[5] == 7.0).all())
    assert np.array_equal(out0[6:].cpu().numpy().view(np.int32), want[0][6:].view(np.int32))
