"""The mini-batch route of LinkPredictionDataset (``neighbor_fanouts``) on the device: the planted-parity graph of
tests/test_gpu_link_prediction.py at 600 nodes - 150 train edges per relation (P = 450), 3 relations, 7 processed types - where
two hops around a batch's endpoints do not cover the graph.  The batches against tests/triple_batch_reference.py and the host
table builder; scores, loss and gradients of a batch against the sibling's fp64 oracle on the WHOLE graph (two full hops make
the seed rows exact); training through run_one_epoch; a featureless model with a row-sparse table update."""
import math

import numpy as np
import pytest
import torch

from tests import distmult_reference as dref
from tests import test_gpu_link_prediction as lp
from tests import triple_batch_reference as ref
from tests.helpers import assert_close
from tests.test_gpu_tasks import _check_grads

# the library's default mode and bench.py's comparison mode (conftest.py: gemm_modes)
pytestmark = [pytest.mark.gpu, pytest.mark.gemm_modes("f16x2", "bf16x3"), pytest.mark.usefixtures("gemm_mode")]

V_MB, D0_MB, T_MB, P_MB = 600, 8, 3, 450


def _dataset(featureless=False, **over):
    """the sibling's planted structure - an edge u -> v has relation parity(u) + parity(v), the parity is in the features -
    at V = 600: 150 train, 12 validation and 12 test edges per relation, all distinct"""
    from tf2_gnn_amd.data import LinkPredictionDataset

    rng = np.random.default_rng(21)
    parity = np.arange(V_MB) % 2
    feats = (0.1 * rng.standard_normal((V_MB, D0_MB))).astype(np.float32)
    feats[:, 0] += parity
    feats[:, 1] += 1 - parity
    pairs = rng.permutation(V_MB * V_MB)[:20000]
    u, v = pairs // V_MB, pairs % V_MB
    rel = parity[u] + parity[v]
    train, valid, test = [], [], []
    for t in range(T_MB):
        e = np.stack([u[rel == t], v[rel == t]], axis=1)
        train.append(e[:150])
        valid.append(e[150:162])
        test.append(e[162:174])
    params = LinkPredictionDataset.get_default_hyperparameters()
    params.update({"num_negatives_per_positive": 1, "negative_sampling": "device", "negative_sampling_seed": 5})
    params.update(over)
    ds = LinkPredictionDataset(params)
    ds.load_data_from_arrays(None if featureless else feats, train, valid_edges=valid, test_edges=test, num_nodes=V_MB)
    assert ds.num_relations == T_MB and ds.num_edge_types == 2 * T_MB + 1 and ds.num_nodes == V_MB
    return ds


def _np(t):
    return t.cpu().numpy()


def test_batches(dev):
    from tf2_gnn_amd import data, ops
    from tf2_gnn_amd.data import DataFold

    K = 2
    ds = _dataset(neighbor_fanouts=[3, 2], triples_per_batch=100, num_negatives_per_positive=K, sampling_seed=9)
    positives = ds.positive_triples(DataFold.TRAIN)
    assert positives.shape == (P_MB, 3)
    train = ds.get_batches(DataFold.TRAIN, dev)
    epochs = []
    for epoch in range(2):
        np.random.seed(40 + epoch)
        order = np.random.permutation(P_MB)
        np.random.seed(40 + epoch)
        launches = ops.triple_batch_launch_counts()
        seen, negatives, sizes = [], [], []
        for b, (feats, labels) in enumerate(train):  # the triple buffers are reused: look at each batch before the next
            data.check_batch(feats)
            ids = order[100 * b:100 * (b + 1)]
            B, N = len(ids), len(ids) * (1 + K)
            seed = ref.batch_seed(5, 5 * epoch + b)
            assert ds.seed_of_last_batch == seed
            want_triples, want_local, want_seeds, S, status = ref.build(positives, ids, K, V_MB, seed, min(2 * N, V_MB))
            assert status == 0
            assert np.array_equal(_np(labels["global_triples"]), want_triples)
            assert np.array_equal(want_triples[:B], positives[ids])
            node_ids = _np(feats["sampled_node_ids"])
            n = node_ids.shape[0]
            assert feats["num_seed_nodes"] == S and np.array_equal(node_ids[:S], want_seeds)
            assert np.array_equal(node_ids[:S], np.unique(want_triples[:, [0, 2]]))
            local = _np(labels["triples"])
            assert np.array_equal(local, want_local) and np.array_equal(node_ids[local[:, [0, 2]]], want_triples[:, [0, 2]])
            assert S < n < V_MB and np.unique(node_ids).shape[0] == n
            tables = ops.build_triple_tables(local, n, T_MB)
            for name in ops.TRIPLE_TABLE_NAMES:
                assert np.array_equal(_np(labels["triple_tables"][name]), tables[name]), name
            assert labels["triple_labels"].tolist() == [1.0] * B + [0.0] * (B * K) and bool((labels["triple_weights"] == 1).all())
            assert tuple(labels["triple_weights"].shape) == (N,)
            for key in ("triples", "triple_labels", "triple_weights", "triple_tables"):
                assert feats[key] is labels[key]
            for key in ("triple_sampler", "positive_triples", "rank_filters"):
                assert key not in feats and key not in labels
            assert "global_triples" not in feats and labels["global_triples"].dtype == torch.int32
            assert tuple(feats["node_features"].shape) == (n, D0_MB) and feats["num_graphs_in_batch"] == 1
            assert np.array_equal(_np(feats["node_features"]), ds.packed_fold(DataFold.TRAIN).features[node_ids])
            for t in range(ds.num_edge_types):
                adj = _np(feats[f"adjacency_list_{t}"])
                assert adj.shape[0] == 0 or (adj.min() >= 0 and adj.max() < n)
            assert int(feats["hop_ptr"][0]) == 0 and int(feats["hop_ptr"][1]) == S and int(feats["hop_ptr"][-1]) == n
            seen.append(want_triples[:B])
            negatives.append(want_triples[B:])
            sizes.append(B)
        assert sizes == [100, 100, 100, 100, 50]
        assert ops.triple_batch_launch_counts() - launches == 6 * 5
        seen = np.concatenate(seen)
        assert sorted(map(tuple, seen.tolist())) == sorted(map(tuple, positives.tolist()))  # every train triple exactly once
        epochs.append((seen, np.concatenate(negatives)))
    assert not np.array_equal(epochs[0][0], epochs[1][0])  # another order ...
    assert sorted(map(tuple, epochs[0][1].tolist())) != sorted(map(tuple, epochs[1][1].tolist()))  # ... and other negatives

    # VALIDATION (and TEST) stay the single full-graph batch of the full-batch device route
    plain = _dataset(num_negatives_per_positive=K)
    for fold in (DataFold.VALIDATION, DataFold.TEST):
        (f_mb, l_mb), (f_fb, l_fb) = lp._single_batch(ds, fold, dev), lp._single_batch(plain, fold, dev)
        assert sorted(f_mb) == sorted(f_fb) and sorted(l_mb) == sorted(l_fb) and "sampled_node_ids" not in f_mb
        for key in ["node_features", "node_to_graph_map", "triples", "triple_labels", "triple_weights"] + [
                f"adjacency_list_{t}" for t in range(ds.num_edge_types)]:
            assert torch.equal(f_mb[key], f_fb[key]), key
        for name in ops.TRIPLE_TABLE_NAMES:
            assert torch.equal(l_mb["triple_tables"][name], l_fb["triple_tables"][name]), name
        assert torch.equal(l_mb["positive_triples"], l_fb["positive_triples"])
        for side in ("dst", "src"):
            assert all(torch.equal(a, b) for a, b in zip(l_mb["rank_filters"][side], l_fb["rank_filters"][side]))


def test_a_batch_is_exact_against_the_whole_graph(dev):
    """Fanouts [-1, -1] under a 2-layer rgcn: the seed rows of a mini-batch are the whole graph's.  Scores, loss and every
    weight gradient of one batch of 16 positives and 16 negatives against the sibling's fp64 oracle, which runs on the WHOLE
    graph over the batch's ``global_triples``, inside the bounds test_link_prediction_task_loss_and_gradients derives: node
    representations 1e-5; a score by sum_d |R[t, d]| (|h_u[d]| e_v[d] + |h_v[d]| e_u[d]), e = 1e-5 max(1, |h|), 1 % added for
    the second order, plus the kernel's own bound; the loss by the mean of that plus 2e-6 max(1, loss); _check_grads."""
    from tf2_gnn_amd.data import DataFold

    ds = _dataset(neighbor_fanouts=[-1, -1], triples_per_batch=16)
    model, params = lp._task(ds, 3)
    with torch.no_grad():
        model._relation_embeddings.value.mul_(3.0)  # scores away from 0
    np.random.seed(12)
    feats, labels = next(iter(ds.get_batches(DataFold.TRAIN, dev)))
    S, n = feats["num_seed_nodes"], int(feats["sampled_node_ids"].shape[0])
    print(f"mini-batch of 16 positives, K = 1, two full hops: S = {S}, n = {n}, V = {V_MB}")
    assert S < n < V_MB
    out = model(feats, training=False)
    m = model.compute_task_metrics(feats, out, labels)
    step = model._step
    model.backward()

    whole = {"triples": labels["global_triples"], "triple_labels": labels["triple_labels"]}
    h64, R64, loss64, pairs, triples, y = lp._oracle(model, params, ds, whole)
    node_ids = _np(feats["sampled_node_ids"])
    assert_close(step["h"][:S].cpu(), h64.detach()[node_ids[:S]].float(), tol=1e-5, what="the seed rows' representations")
    hn, Rn = h64.detach().numpy(), R64.detach().numpy()
    e = 1e-5 * np.maximum(1.0, np.abs(hn))
    u, r, v = triples[:, 0], triples[:, 1], triples[:, 2]
    ds_stack = 1.01 * (np.abs(Rn[r]) * (np.abs(hn[u]) * e[v] + np.abs(hn[v]) * e[u])).sum(axis=1)
    exact = dref.distmult_ce(hn, Rn, triples, y.numpy())
    ds_total = ds_stack + exact.score_bound
    loss = float(loss64.detach())
    assert abs(exact.loss - loss) <= 1e-12
    bound = 2e-6 * max(1.0, loss) + float(ds_total.mean())
    err = abs(float(m["loss"]) - loss)
    scores = out[0].cpu().numpy().astype(np.float64)
    print(f"mini-batch loss {float(m['loss']):.9g} fp64 on the whole graph {loss:.9g} error / bound {err / bound:.3f}; "
          f"largest score error / bound {float((np.abs(scores - exact.scores) / ds_total).max()):.3f}")
    assert err <= bound
    assert np.all(np.abs(scores - exact.scores) <= ds_total)
    assert int(m["counts"].sum()) == 32
    _check_grads(model, pairs, loss64, "LinkPredictionTask on a mini-batch")


def _validation_loss(model, ds, dev):
    from tf2_gnn_amd.data import DataFold

    feats, labels = lp._single_batch(ds, DataFold.VALIDATION, dev)
    return float(model._run_step(feats, labels, training=False)["loss"])


def test_training_lowers_the_validation_loss_on_planted_structure(dev):
    """The sibling's criterion (finite losses, the last below the first) for the full-batch VALIDATION loss around 4 epochs of
    5 mini-batches at Adam's learning rate 0.001.  Why these: TRAIN positives are edges of the message-passing graph and the
    validation edges are not, so a model trained long enough reads the edge itself and its validation loss RISES.  A float64
    torch restatement of this training on the whole graph (the oracle stack, torch.optim.Adam, the same batches; independent
    of the library) shows it: at 0.01, the sibling's rate, the validation loss falls for two epochs and is at 1.5 after six;
    at 0.001 and 4 epochs it fell from 0.69 to 0.61 - 0.66 for each of 8 initialisations."""
    from tf2_gnn_amd.data import DataFold

    ds = _dataset(neighbor_fanouts=[5, 5], triples_per_batch=100)
    np.random.seed(3)
    model, _ = lp._task(ds, 4, optimizer="Adam", learning_rate=0.001)
    train = ds.get_batches(DataFold.TRAIN, dev)
    losses = [_validation_loss(model, ds, dev)]
    for _ in range(4):
        train_loss, _, results = model.run_one_epoch(train, quiet=True, training=True)
        assert len(results) == 5 and math.isfinite(train_loss)
        losses.append(_validation_loss(model, ds, dev))
    print("LinkPredictionTask, 4 epochs of 5 mini-batches: validation loss " + " -> ".join(f"{l:.4f}" for l in losses))
    assert all(math.isfinite(l) for l in losses) and losses[-1] < losses[0]
    assert model._optimizer.iterations == 20
    metrics = model.evaluate_model(ds.get_batches(DataFold.VALIDATION, dev))
    assert list(metrics) == ["mrr", "hits@1", "hits@3", "hits@10"] and all(0.0 <= x <= 1.0 for x in metrics.values())
    with pytest.raises(ValueError, match="VALIDATION or TEST"):
        model.evaluate_model(train)


def test_featureless_model_updates_only_the_batch_rows(dev):
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import DataFold

    ds = _dataset(featureless=True, neighbor_fanouts=[3, 3], triples_per_batch=32)
    assert ds.node_feature_shape == (0,)
    model, _ = lp._task(ds, 8, optimizer="Adam", learning_rate=0.01, node_embedding_dim=16, node_embedding_update="rows")
    (table,) = [x for x in model.trainable_variables if x.name.endswith("/node_embeddings")]
    assert tuple(table.value.shape) == (V_MB, 16)
    np.random.seed(6)
    feats, labels = next(iter(ds.get_batches(DataFold.TRAIN, dev)))
    assert tuple(feats["node_features"].shape) == (feats["sampled_node_ids"].shape[0], 0)
    before = table.value.clone()
    launches = ops.embedding_launch_count()
    loss = float(model._run_step(feats, labels, training=True)["loss"])
    torch.cuda.synchronize()
    assert math.isfinite(loss) and ops.embedding_launch_count() == launches and int(model.embedding_bad_index) == 0
    inside = torch.zeros(V_MB, dtype=torch.bool, device=dev)
    inside[feats["sampled_node_ids"].long()] = True
    assert 0 < int(inside.sum()) < V_MB
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(table.value[~inside]), bits(before[~inside]))
    changed = (bits(table.value) != bits(before)).any(dim=1)
    assert bool(changed[feats["sampled_node_ids"][:feats["num_seed_nodes"]].long()].all())  # every endpoint's row moved
    assert not bool(changed[~inside].any())
