"""Batch assembly above the 48 edge types of one tfgnn_batch_assemble call: ``assemble_batch`` makes ceil(L / 48) calls, the
first with the node arrays, the column and types [0, 48), the others with 48 more types each.  A synthetic fold of five
graphs of 3 - 9 nodes, L in {48, 49, 96, 97, 238} types of which ten at most hold edges - at least one in every chunk of 48,
in every graph, so every call has something to launch -, one per-graph column, an epoch of two batches; every output against a
numpy restatement, exactly."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NODE_COUNTS = [3, 9, 5, 7, 4]
ORDER = [3, 1, 0, 4, 2]  # nodes along the order: 7, 9 | 3, 4, 5 -> two batches at max_nodes_per_batch = 16
NONEMPTY = (0, 1, 47, 48, 95, 96, 143, 150, 200, 237)
F = 3


def _fold(L, seed=0):
    from tf2_gnn_amd.data import PackedFold

    rng = np.random.default_rng(seed)
    counts = np.array(NODE_COUNTS, dtype=np.int64)
    feats = rng.standard_normal((int(counts.sum()), F)).astype(np.float32)
    edge_counts, edges = [], []
    for t in range(L):
        c = np.array([1 + (g + t) % 3 if t in NONEMPTY else 0 for g in range(len(counts))], dtype=np.int64)
        edge_counts.append(c)
        edges.append(np.concatenate([rng.integers(0, counts[g], size=(int(c[g]), 2)) for g in range(len(counts))]).astype(np.int32))
    column = rng.standard_normal(len(counts)).astype(np.float32)
    return PackedFold(counts, feats, edge_counts, edges, columns={"target_value": column})


def _restate(fold, order, p0, p1):
    graphs = [order[p] for p in range(p0, p1)]
    offsets = np.concatenate([[0], np.cumsum([fold.node_counts[g] for g in graphs])]).astype(np.int64)
    feats = np.concatenate([fold.features[fold.node_ptr[g]:fold.node_ptr[g + 1]] for g in graphs])
    n2g = np.repeat(np.arange(len(graphs), dtype=np.int32), [fold.node_counts[g] for g in graphs])
    adj = []
    for t in range(fold.num_edge_types):
        parts = [fold.edges[t][fold.edge_ptr[t][g]:fold.edge_ptr[t][g + 1]] + np.int32(offsets[i]) for i, g in enumerate(graphs)]
        adj.append(np.concatenate(parts).astype(np.int32).reshape(-1, 2))
    return feats, n2g, adj, fold.columns["target_value"][graphs]


@pytest.mark.parametrize("L", [48, 49, 96, 97, 238])
def test_every_output_equals_numpy_and_the_calls_are_counted(dev, L):
    from tf2_gnn_amd.data.graph_dataset import EpochPlan, FoldStore, assemble_batch, batch_assemble_launch_counts

    fold = _fold(L, seed=L)
    store = FoldStore(fold, dev)
    plan = EpochPlan(store, ORDER, max_nodes_per_batch=16)
    assert plan.batches == [(0, 2), (2, 5)]
    calls = -(-L // 48)
    assert calls == {48: 1, 49: 2, 96: 2, 97: 3, 238: 5}[L]
    for b, (p0, p1) in enumerate(plan.batches):
        before = batch_assemble_launch_counts()
        features, labels = assemble_batch(plan, p0, p1, bad_flag=plan.bad_flags[b:b + 1])
        assert batch_assemble_launch_counts() - before == calls
        torch.cuda.synchronize()
        feats, n2g, adj, column = _restate(fold, ORDER, p0, p1)
        assert np.array_equal(features["node_features"].cpu().numpy().view(np.int32), feats.view(np.int32))
        assert np.array_equal(features["node_to_graph_map"].cpu().numpy(), n2g)
        assert features["num_graphs_in_batch"] == p1 - p0
        for t in range(L):
            got = features[f"adjacency_list_{t}"]
            assert got.dtype == torch.int32 and tuple(got.shape) == adj[t].shape, t
            assert np.array_equal(got.cpu().numpy(), adj[t]), t
            assert (adj[t].shape[0] > 0) == (t in NONEMPTY)
        assert np.array_equal(labels["target_value"].cpu().numpy().view(np.int32), column.view(np.int32))
    assert plan.bad_flags.tolist() == [0, 0]


@pytest.mark.parametrize("L,bad_type", [(49, 48), (97, 96), (238, 200)])
def test_a_bad_local_node_id_beyond_type_48_sets_its_batch_flag(dev, L, bad_type):
    from tf2_gnn_amd.data.graph_dataset import EpochPlan, FoldStore, assemble_batch

    fold = _fold(L, seed=L + 1)
    g = 4  # graph 4 (4 nodes) is in the second batch
    fold.edges[bad_type][int(fold.edge_ptr[bad_type][g]), 1] = NODE_COUNTS[g]  # one past the graph's last node
    store = FoldStore(fold, dev)
    plan = EpochPlan(store, ORDER, max_nodes_per_batch=16)
    batches = [assemble_batch(plan, p0, p1, bad_flag=plan.bad_flags[b:b + 1]) for b, (p0, p1) in enumerate(plan.batches)]
    torch.cuda.synchronize()
    assert plan.bad_flags.tolist() == [0, 1]
    # the other types of that batch are what they are without the bad id
    _, _, adj, _ = _restate(fold, ORDER, 2, 5)
    for t in range(L):
        if t != bad_type:
            assert np.array_equal(batches[1][0][f"adjacency_list_{t}"].cpu().numpy(), adj[t]), t


def test_featureless_fold_through_the_chunked_route(dev):
    """a fold of width-0 features and 97 types: node_features is a float32 [V, 0], everything else as with features"""
    from tf2_gnn_amd.data import PackedFold
    from tf2_gnn_amd.data.graph_dataset import EpochPlan, FoldStore, assemble_batch

    with_feats = _fold(97, seed=5)
    fold = PackedFold(with_feats.node_counts, np.zeros((int(with_feats.node_counts.sum()), 0), dtype=np.float32),
                      with_feats.edge_counts, with_feats.edges, columns=with_feats.columns)
    plan = EpochPlan(FoldStore(fold, dev), ORDER, max_nodes_per_batch=16)
    features, labels = assemble_batch(plan, 2, 5)
    torch.cuda.synchronize()
    _, n2g, adj, column = _restate(with_feats, ORDER, 2, 5)
    nf = features["node_features"]
    assert nf.dtype == torch.float32 and tuple(nf.shape) == (12, 0) and nf.is_cuda
    assert np.array_equal(features["node_to_graph_map"].cpu().numpy(), n2g)
    assert all(np.array_equal(features[f"adjacency_list_{t}"].cpu().numpy(), adj[t]) for t in range(97))
    assert np.array_equal(labels["target_value"].cpu().numpy(), column) and int(features["_bad_local_index"]) == 0
