"""tfgnn_triples_draw_negatives and tfgnn_triple_tables_build on the device (csrc/negatives.hip): the draw against
tests/negative_sample_reference.py bit for bit, the tables against the host's ops.build_triple_tables exactly - at one key, one
below / at / one above the sort's tile of 8192 keys (the node sort has 2 N keys, the relation sort N), several tiles, every
number of digit passes up to three, a hub node, self triples, empty relations - the launch counts against the header's formula,
and both calls inside a captured graph that redraws at every replay."""
import numpy as np
import pytest
import torch

from tests import negative_sample_reference as nref

pytestmark = pytest.mark.gpu

SENTINEL = -7


def _positives(P, V, T, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, V, P), rng.randint(0, T, P), rng.randint(0, V, P)], axis=1).astype(np.int32)


@pytest.fixture
def epoch_zero_after():
    from tf2_gnn_amd import ops

    yield
    ops.dropout_epoch_set(0)  # every other test draws at epoch 0
    torch.cuda.synchronize()


# ---- the draw ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,K,V", [(1, 1, 2), (257, 3, 50), (1000, 0, 7), (513, 2, 3001), (64, 2, 2 ** 31 - 1)])
def test_draw_equals_the_reference(dev, epoch_zero_after, P, K, V):
    from tf2_gnn_amd import ops

    pos = _positives(P, V, 5, seed=P + K)
    pos[0] = (V - 1, 4, V - 1)
    N, pad = P * (1 + K), 5
    seed = 0xC0FFEE_0000_0000 + P
    for epoch in (0, 5):
        ops.dropout_epoch_set(epoch)
        for use_epoch in (False, True):
            buf = torch.full((N + pad, 3), SENTINEL, dtype=torch.int32, device=dev)
            buf[:P] = torch.from_numpy(pos).to(dev)
            triples = buf[:N]
            before = ops.negatives_launch_counts()
            assert ops.draw_negative_triples(triples, P, V, seed, use_epoch=use_epoch) is triples
            after = ops.negatives_launch_counts()
            assert after["draw_negatives"] - before["draw_negatives"] == (1 if K else 0)  # K = 0 launches nothing
            assert after["triple_tables"] == before["triple_tables"]
            got = buf.cpu().numpy()
            want = nref.triples(pos, K, V, seed, epoch, use_epoch)
            assert np.array_equal(got[:P], pos), "the positives were written"
            assert np.array_equal(got[:N], want), (P, K, V, epoch, use_epoch)
            assert np.all(got[N:] == SENTINEL), "bytes after row N were written"


def test_draw_refusals_through_ops(dev):
    from tf2_gnn_amd import ops

    tr = torch.zeros((6, 3), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="second node"):
        ops.draw_negative_triples(tr, 3, 1, seed=0)
    with pytest.raises(ValueError, match="positives"):
        ops.draw_negative_triples(tr, 4, 5, seed=0)
    with pytest.raises(ValueError, match="contiguous int32"):
        ops.draw_negative_triples(tr[:, :2], 3, 5, seed=0)
    with pytest.raises(TypeError):
        ops.draw_negative_triples(tr.long(), 3, 5, seed=0)


# ---- the tables -------------------------------------------------------------------------------------------------------------
def _triples(N, V, T, seed, hub=None, skip_relation=None):
    rng = np.random.RandomState(seed)
    u, v = rng.randint(0, V, N), rng.randint(0, V, N)
    if hub is not None:  # the hub takes 60 % of all 2 N slots
        u = np.where(rng.rand(N) < 0.6, hub, u)
        v = np.where(rng.rand(N) < 0.6, hub, v)
    t = rng.randint(0, T, N)
    if skip_relation is not None:
        t = np.where(t == skip_relation, (skip_relation + 1) % T, t)
    return np.stack([u, t, v], axis=1).astype(np.int32)


TABLE_CASES = [
    # N, V, T, hub, relation without a triple
    (1, 1, 1, None, None),           # one self triple (0, 0, 0): two entries under node 0
    (4095, 2, 3, None, 1),           # node sort one key below its tile
    (4096, 50, 1, 7, None),          # ... at the tile; a hub of ~4900 entries
    (4097, 512, 3, None, None),      # ... one above; V = 512: the last one-pass size
    (8191, 513, 600, None, 599),     # relation sort one below its tile; V = 513, T = 600: two passes each
    (8192, 1, 3, None, None),        # ... at the tile; every entry lands in node 0, every triple is a self triple
    (8193, 50, 600, 7, 0),           # ... one above
    (2300, 50, 3, 11, 2),            # a hub of >= 2200 entries inside one tile
    (20000, 262145, 600, None, 17),  # several tiles; V = 2^18 + 1: three passes
]


@pytest.mark.parametrize("N,V,T,hub,skip", TABLE_CASES)
def test_tables_equal_the_host_build(dev, N, V, T, hub, skip):
    from tf2_gnn_amd import ops

    host = _triples(N, V, T, seed=N + V, hub=hub, skip_relation=skip if T > 1 else None)
    if V > 2:
        host[N // 2] = (V - 1, T - 1 if skip != T - 1 else 0, V - 1)  # the last node, as a self triple
    want = ops.build_triple_tables(host, V, T)
    if hub is not None:
        assert int(want["node_offsets"][hub + 1]) - int(want["node_offsets"][hub]) >= (2200 if N >= 2300 else 0)
    if skip is not None and T > 1:
        assert want["rel_offsets"][skip] == want["rel_offsets"][skip + 1]
    triples = torch.from_numpy(host).to(dev)
    pv, pt = ops.triple_table_passes(V), ops.triple_table_passes(T)
    assert (pv, pt) == (1 if V <= 512 else 2 if V <= 2 ** 18 else 3, 1 if T <= 512 else 2)

    def launches(fn):
        before = ops.negatives_launch_counts()
        out = fn()
        after = ops.negatives_launch_counts()
        assert after["draw_negatives"] == before["draw_negatives"]
        return out, after["triple_tables"] - before["triple_tables"]

    def same(tabs, names):
        assert sorted(tabs) == sorted(names)
        for name in names:
            assert tabs[name].dtype == torch.int32
            assert np.array_equal(tabs[name].cpu().numpy(), want[name]), (name, N, V, T)

    both, n_both = launches(lambda: ops.build_triple_tables_device(triples, V, T))
    same(both, ops.TRIPLE_TABLE_NAMES)
    assert n_both == (2 * pv + 1) + (2 * pt + 1)  # the header's formula
    again, _ = launches(lambda: ops.build_triple_tables_device(triples, V, T, workspace=ops.triple_tables_workspace(triples, V, T)))
    assert all(torch.equal(both[n], again[n]) for n in ops.TRIPLE_TABLE_NAMES)  # two runs are bit-identical

    # one pair requested: the other pair's buffers are untouched
    sizes = {"node_offsets": V + 1, "node_entries": 2 * N, "rel_offsets": T + 1, "rel_order": N}
    out = {n: torch.full((sizes[n],), SENTINEL, dtype=torch.int32, device=dev) for n in ops.TRIPLE_TABLE_NAMES}
    got, n_node = launches(lambda: ops.build_triple_tables_device(triples, V, T, out=out, rel=False))
    assert n_node == 2 * pv + 1 and got["node_entries"] is out["node_entries"]
    same(got, ("node_offsets", "node_entries"))
    assert bool((out["rel_offsets"] == SENTINEL).all()) and bool((out["rel_order"] == SENTINEL).all())
    out = {n: torch.full((sizes[n],), SENTINEL, dtype=torch.int32, device=dev) for n in ops.TRIPLE_TABLE_NAMES}
    got, n_rel = launches(lambda: ops.build_triple_tables_device(triples, V, T, out=out, node=False))
    assert n_rel == 2 * pt + 1
    same(got, ("rel_offsets", "rel_order"))
    assert bool((out["node_offsets"] == SENTINEL).all()) and bool((out["node_entries"] == SENTINEL).all())
    assert torch.equal(triples.cpu(), torch.from_numpy(host))  # the triples are only read


def test_table_refusals_through_ops(dev):
    from tf2_gnn_amd import ops

    tr = torch.zeros((6, 3), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="neither"):
        ops.build_triple_tables_device(tr, 5, 2, node=False, rel=False)
    with pytest.raises(ValueError, match="node_entries"):
        ops.build_triple_tables_device(tr, 5, 2, out={"node_offsets": torch.zeros(6, dtype=torch.int32, device=dev),
                                                      "node_entries": torch.zeros(11, dtype=torch.int32, device=dev)}, rel=False)
    with pytest.raises(ValueError, match="workspace"):
        ops.build_triple_tables_device(tr, 5, 2, workspace=torch.zeros(64, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="empty batch"):
        ops.build_triple_tables_device(tr[:0], 5, 2)


# ---- capture ----------------------------------------------------------------------------------------------------------------
def test_captured_draw_and_tables_follow_the_epoch(dev, epoch_zero_after):
    """epoch advance, draw, tables as one captured graph: three replays, each equal to the reference for the epoch read back
    and to the host tables of those triples; consecutive replays differ."""
    from tf2_gnn_amd import ops

    P, K, V, T, seed = 300, 3, 40, 5, 0xABCDEF0123
    pos = _positives(P, V, T, seed=1)
    N = P * (1 + K)
    triples = torch.full((N, 3), SENTINEL, dtype=torch.int32, device=dev)
    triples[:P] = torch.from_numpy(pos).to(dev)
    sizes = {"node_offsets": V + 1, "node_entries": 2 * N, "rel_offsets": T + 1, "rel_order": N}
    tables = {n: torch.empty(sizes[n], dtype=torch.int32, device=dev) for n in ops.TRIPLE_TABLE_NAMES}
    workspace = ops.triple_tables_workspace(triples, V, T)
    ops.dropout_epoch_set(10)
    assert ops.dropout_epoch() == 10  # the epoch word exists before the capture

    def work():
        ops.dropout_epoch_advance()
        ops.draw_negative_triples(triples, P, V, seed)
        ops.build_triple_tables_device(triples, V, T, out=tables, workspace=workspace)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        work()
    torch.cuda.synchronize()
    seen = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        epoch = ops.dropout_epoch()
        got = triples.cpu().numpy()
        assert np.array_equal(got, nref.triples(pos, K, V, seed, epoch)), epoch
        want = ops.build_triple_tables(got, V, T)
        for name in ops.TRIPLE_TABLE_NAMES:
            assert np.array_equal(tables[name].cpu().numpy(), want[name]), (name, epoch)
        seen.append((epoch, got))
    assert [e for e, _ in seen] == [seen[0][0] + i for i in range(3)] and seen[0][0] >= 12
    assert not np.array_equal(seen[0][1], seen[1][1]) and not np.array_equal(seen[1][1], seen[2][1])
