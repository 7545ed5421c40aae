"""Neighbour-sampled batches of NodeClassificationDataset through NodeClassificationTask on the device.  At full fanout
with as many hops as layers the seed rows of a sampled batch must be what the fp64 oracle computes on the WHOLE graph:
logits within the 1e-5 of assert_close, the loss within 2e-5 * max(1, loss), every gradient through _check_grads with the
oracle's mask set to the seeds - the tolerances tests/test_gpu_node_classification.py uses against the same oracle.  Then
the loops: evaluate_model and run_one_epoch over sampled batches.  PARITY UNPINNED: the reference has no such route."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import assert_close
from tests.test_gpu_node_classification import _oracle_loss_and_pairs
from tests.test_gpu_tasks import _check_grads, _gnn_params

# every test of this module runs in the three GEMM modes (conftest.py: gemm_modes)
pytestmark = [pytest.mark.gpu, pytest.mark.gemm_modes, pytest.mark.usefixtures("gemm_mode")]

V_DS, D0_DS, C_DS, H_DS, LAYERS = 151, 10, 5, 16, 3


def _arrays():
    """one graph of 151 nodes, one forward edge type (self loops + forward + backward = 3 processed types) with a hub of 40
    in-edges, 5 classes, a sixth of the labels unknown, the rest split 50 / 25 / 25"""
    rng = np.random.default_rng(21)
    feats = rng.standard_normal((V_DS, D0_DS)).astype(np.float32)
    labels = rng.integers(0, C_DS, size=V_DS)
    labels[rng.random(V_DS) < 0.16] = -1
    edges = np.concatenate([rng.integers(0, V_DS, size=(110, 2)), np.stack([rng.integers(0, V_DS, size=40), np.full(40, 4)], axis=1)])
    known = rng.permutation(np.flatnonzero(labels >= 0))
    a, b = len(known) // 2, 3 * len(known) // 4
    return feats, labels, [edges], {"train_idx": known[:a], "valid_idx": known[a:b], "test_idx": known[b:]}


def _dataset(**hypers):
    from tf2_gnn_amd.data import NodeClassificationDataset

    params = NodeClassificationDataset.get_default_hyperparameters()
    params.update(hypers)
    ds = NodeClassificationDataset(params)
    feats, labels, edges, idx = _arrays()
    ds.load_data_from_arrays(feats, labels, edges, **idx)
    assert ds.num_edge_types == 3 and ds.num_node_classes == C_DS
    return ds, idx


def _task(ds, seed, **extra):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import NodeClassificationTask

    set_seed(seed)
    params = _gnn_params(NodeClassificationTask, "rgcn", H_DS, LAYERS, extra={"gnn_layer_input_dropout_rate": 0.0, **extra})
    model = NodeClassificationTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    model._bias.value.copy_(torch.randn(C_DS, generator=torch.Generator().manual_seed(1)))
    return model, params


def test_full_fanout_seed_rows_match_the_oracle_on_the_whole_graph(dev):
    from tf2_gnn_amd import data
    from tf2_gnn_amd.data import DataFold

    ds, idx = _dataset(neighbor_fanouts=[-1] * LAYERS, seeds_per_batch=24)
    model, params = _task(ds, 3)
    batches = list(ds.get_batches(DataFold.VALIDATION, dev))
    assert len(batches) == math.ceil(len(idx["valid_idx"]) / 24) >= 2
    feats, labels = batches[0]
    data.check_batch(feats)
    S = feats["num_seed_nodes"]
    n = feats["node_features"].shape[0]
    seeds = idx["valid_idx"][:24]
    assert S == 24 and S < n < V_DS and feats["num_graphs_in_batch"] == 1 and not bool(feats["node_to_graph_map"].any())
    assert feats["sampled_node_ids"].cpu().numpy()[:S].tolist() == seeds.tolist()
    assert feats["hop_ptr"].tolist()[:2] == [0, S] and feats["hop_ptr"][-1] == n and len(feats["hop_ptr"]) == LAYERS + 2
    host = ds.packed_fold(DataFold.VALIDATION)
    ids = feats["sampled_node_ids"].cpu().numpy()
    assert np.array_equal(feats["node_features"].cpu().numpy(), host.features[ids])
    assert np.array_equal(labels["node_labels"].cpu().numpy(), host.node_columns["node_labels"][ids])
    want_w = np.zeros((n, 1), dtype=np.float32)
    want_w[:S] = 1.0  # the fold's weight on the seed rows, 0 below - other validation nodes among the neighbours included
    assert np.array_equal(labels["node_label_weights"].cpu().numpy(), want_w)
    assert (host.node_columns["node_label_weights"][ids][S:] > 0).any()

    out = model(feats, training=False)
    m = model.compute_task_metrics(feats, out, labels)
    model.backward()
    X = torch.from_numpy(host.features)
    all_labels = torch.from_numpy(host.node_columns["node_labels"][:, 0])
    mask = torch.zeros(V_DS)
    mask[torch.from_numpy(seeds)] = 1.0
    logits64, loss64, pairs = _oracle_loss_and_pairs(model, params, X, host.edges, 3, all_labels, mask)
    assert_close(out[0][:S].cpu(), logits64.detach().float()[torch.from_numpy(seeds)], tol=1e-5, what="seed rows of the sampled batch")
    loss = float(loss64.detach())
    print(f"sampled batch loss {float(m['loss']):.9g} fp64 on the whole graph {loss:.9g}")
    assert abs(float(m["loss"]) - loss) <= 2e-5 * max(1.0, loss)
    assert int(m["num_labelled"]) == S
    _check_grads(model, pairs, loss64, "NodeClassificationTask on a sampled batch")


def test_evaluate_model_counts_the_nodes_of_the_full_batch_route(dev):
    from tf2_gnn_amd.data import DataFold

    sampled, idx = _dataset(neighbor_fanouts=[2, 2], eval_neighbor_fanouts=[-1] * LAYERS, seeds_per_batch=16)
    full, _ = _dataset()
    model, _ = _task(full, 4)
    full_batches, sampled_batches = full.get_batches(DataFold.VALIDATION, dev), sampled.get_batches(DataFold.VALIDATION, dev)
    whole = model.predict(full_batches)
    assert tuple(whole.shape) == (V_DS, C_DS)
    valid = idx["valid_idx"]
    counted = []
    for loader in (full_batches, sampled_batches):
        _, _, results = model.run_one_epoch(loader, quiet=True, training=False)
        counted.append(sum(int(r["num_labelled"]) for r in results))
    assert counted == [len(valid), len(valid)]
    at = 0
    for feats, labels in sampled_batches:
        S = feats["num_seed_nodes"]
        assert feats["sampled_node_ids"][:S].cpu().tolist() == valid[at:at + S].tolist()
        logits = model(feats, training=False)[0]
        assert_close(logits[:S].cpu(), whole[torch.from_numpy(valid[at:at + S]).to(dev)].cpu(), tol=1e-5, what="sampled against full-batch logits")
        at += S
    assert at == len(valid)
    metrics_full, metrics_sampled = model.evaluate_model(full_batches), model.evaluate_model(sampled_batches)
    assert list(metrics_sampled) == list(metrics_full) == ["acc", "macro_f1"]
    print(f"acc full-batch {metrics_full['acc']:.6f} sampled {metrics_sampled['acc']:.6f}")
    assert abs(metrics_sampled["acc"] - metrics_full["acc"]) <= 1.0 / len(valid)  # an argmax may sit within the logit tolerance


def test_validation_batches_repeat_and_training_batches_reshuffle(dev):
    from tf2_gnn_amd.data import DataFold

    ds, idx = _dataset(neighbor_fanouts=[3, 2], seeds_per_batch=16, sampling_seed=3)
    valid = ds.get_batches(DataFold.VALIDATION, dev)
    first, second = list(valid), list(valid)
    assert len(first) == len(second) == math.ceil(len(idx["valid_idx"]) / 16)
    for (f1, l1), (f2, l2) in zip(first, second):
        assert f1.keys() == f2.keys() and l1.keys() == l2.keys()
        for k in f1:
            if isinstance(f1[k], torch.Tensor) and not k.startswith("_"):
                assert torch.equal(f1[k], f2[k]), k
        assert np.array_equal(f1["hop_ptr"], f2["hop_ptr"]) and all(torch.equal(l1[k], l2[k]) for k in l1)
    np.random.seed(0)
    train = ds.get_batches(DataFold.TRAIN, dev)
    e1 = [f["sampled_node_ids"][:f["num_seed_nodes"]].cpu().tolist() for f, _ in train]
    e2 = [f["sampled_node_ids"][:f["num_seed_nodes"]].cpu().tolist() for f, _ in train]
    assert e1 != e2 and sorted(sum(e1, [])) == sorted(sum(e2, [])) == sorted(idx["train_idx"].tolist())
    assert [len(c) for c in e1] == [16, 16, 16, 13] and len(idx["train_idx"]) == 61  # the partial chunk is kept


def test_run_one_epoch_over_sampled_training_batches(dev):
    from tf2_gnn_amd.data import DataFold

    ds, idx = _dataset(neighbor_fanouts=[3, 2], seeds_per_batch=16)
    model, _ = _task(ds, 5, optimizer="Adam", learning_rate=0.01)
    np.random.seed(1)
    loss, _, results = model.run_one_epoch(ds.get_batches(DataFold.TRAIN, dev), quiet=True, training=True)
    assert math.isfinite(loss) and all(math.isfinite(float(r["loss"])) for r in results)
    assert len(results) == math.ceil(len(idx["train_idx"]) / 16)
    assert sum(int(r["num_labelled"]) for r in results) == len(idx["train_idx"])
