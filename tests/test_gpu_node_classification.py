"""NodeClassificationTask and NodeClassificationDataset on the device: the task against the fp64 oracle stack with a
float64 ``cross_entropy`` on top, the torch.autograd route, the dataset's batches against its host folds, whole training
steps eager and replayed, a captured evaluation step that follows an in-place change of the fold mask, and
predict / evaluate_model.  The kernel itself: tests/test_gpu_softmax_ce.py.  PARITY UNPINNED: the reference has no such task."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import assert_close
from tests.softmax_ce_reference import softmax_ce
from tests.test_gpu_layers import _gnn_oracle_weights, _to64
from tests.test_gpu_tasks import _batch, _check_grads, _features, _gnn_pairs, _gnn_params, _leaves, _oracle_gnn

# every test of this module runs in the three GEMM modes (conftest.py: gemm_modes)
pytestmark = [pytest.mark.gpu, pytest.mark.gemm_modes, pytest.mark.usefixtures("gemm_mode")]


def _loss64(logits64, labels, weights):
    """sum_v w_v ce_v / sum_v w_v over the nodes with a label, in float64"""
    keep = (labels >= 0) & (weights > 0)
    per_node = torch.nn.functional.cross_entropy(logits64[keep], labels[keep].long(), reduction="none")
    w = weights[keep].double()
    return (w * per_node).sum() / w.sum()


def _oracle_case(dev):
    """the batch of test_node_multiclass_task_loss_and_gradients (three graphs, L = 3, H = 16) with C = 7, a mask over about
    half of the nodes and a few unknown labels"""
    from tf2_gnn_amd.tasks import NodeClassificationTask

    sizes, L, D0, H, C = [30, 45, 12], 3, 10, 16, 7
    X, adjs, n2g = _batch(sizes, L, D0, seed=4)
    params = _gnn_params(NodeClassificationTask, "rgcn", H, 3)
    model = NodeClassificationTask(params, num_edge_types=L, num_node_classes=C)
    feats = _features(X, adjs, n2g, len(sizes), dev)
    model.build({"node_features": (None, D0)})
    model._bias.value.copy_(torch.randn(C, generator=torch.Generator().manual_seed(1)))
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(0, C, (X.shape[0],), generator=g).float()
    labels[::10] = -1.0
    weights = (torch.rand(X.shape[0], generator=g) < 0.5).float()
    assert 30 <= int(weights.sum()) <= 57 and bool(((labels < 0) & (weights > 0)).any())
    return model, params, X, adjs, L, feats, labels, weights


def _oracle_loss_and_pairs(model, params, X, adjs, L, labels, weights):
    w = _gnn_oracle_weights(model._gnn)
    head = {"kernel": model._kernel.value.cpu().clone(), "bias": model._bias.value.cpu().clone()}
    w64, head64 = _to64(w), _to64(head)
    _leaves(w64), _leaves(head64)
    h64, _ = _oracle_gnn(params, w64, X.double(), adjs)
    logits64 = h64 @ head64["kernel"] + head64["bias"]
    pairs = _gnn_pairs(model._gnn, w64, L) + [(model._kernel, head64["kernel"]), (model._bias, head64["bias"])]
    return logits64, _loss64(logits64, labels, weights), pairs


def test_node_classification_task_loss_and_gradients(dev):
    """batch -> logits -> loss / accuracy -> every gradient.  Tolerances of test_node_multiclass_task_loss_and_gradients:
    logits 1e-5, loss 2e-5 * max(1, loss), every gradient through _check_grads; counts from the HIP logits."""
    model, params, X, adjs, L, feats, labels, weights = _oracle_case(dev)
    batch_labels = {"node_labels": labels.view(-1, 1).to(dev), "node_label_weights": weights.view(-1, 1).to(dev)}
    out = model(feats, training=False)
    with pytest.raises(RuntimeError):
        model.backward()  # no loss yet
    m = model.compute_task_metrics(feats, out, batch_labels)
    model.backward()
    assert sorted(m) == ["accuracy", "loss", "num_correct", "num_labelled"]
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in m.values())
    assert m["num_correct"].dtype == m["num_labelled"].dtype == torch.int64

    logits64, loss64, pairs = _oracle_loss_and_pairs(model, params, X, adjs, L, labels, weights)
    assert_close(out[0].cpu(), logits64.detach().float(), tol=1e-5, what="per-node logits")
    loss = float(loss64.detach())
    print(f"NodeClassificationTask loss {float(m['loss']):.9g} fp64 {loss:.9g}")
    assert abs(float(m["loss"]) - loss) <= 2e-5 * max(1.0, loss)
    ref = softmax_ce(out[0].cpu().numpy(), labels.numpy(), weights.numpy())  # counts from the HIP logits
    assert [int(m["num_correct"]), int(m["num_labelled"])] == [ref.correct, ref.counted_nodes]
    assert ref.counted_nodes == int(((labels >= 0) & (weights > 0)).sum())
    assert abs(float(m["accuracy"]) - ref.accuracy) <= 1e-6
    value, text = model.compute_epoch_metrics([m, m])
    assert value == -ref.accuracy and text == f"Accuracy = {ref.accuracy:.3f}"
    _check_grads(model, pairs, loss64, "NodeClassificationTask")

    # without a weight column every node with a label counts
    m_all = model.compute_task_metrics(feats, out, {"node_labels": labels.to(dev)})
    assert int(m_all["num_labelled"]) == int((labels >= 0).sum())


def test_torch_autograd_route_with_cross_entropy(dev):
    """TorchGraphTaskModel + F.cross_entropy(reduction="sum") / W on the device: every weight gradient inside the
    _check_grads bound against the same fp64 loss as the fused route."""
    from tf2_gnn_amd import TorchGraphTaskModel

    model, params, X, adjs, L, feats, labels, weights = _oracle_case(dev)
    module = TorchGraphTaskModel(model).eval()
    logits = module(feats)
    assert logits.requires_grad and tuple(logits.shape) == (X.shape[0], 7)
    masked = torch.where(weights > 0, labels, torch.full_like(labels, -1.0)).long().to(dev)
    W = float(((labels >= 0) & (weights > 0)).sum())
    torch.nn.functional.cross_entropy(logits, masked, ignore_index=-1, reduction="sum").div(W).backward()
    assert all(p.grad is not None for p in module.parameters())
    _, loss64, pairs = _oracle_loss_and_pairs(model, params, X, adjs, L, labels, weights)
    _check_grads(model, pairs, loss64, "TorchGraphTaskModel(NodeClassificationTask)")


# ---- the dataset ------------------------------------------------------------------------------------------------------------
V_DS, D0_DS, C_DS, H_DS = 301, 12, 6, 16


def _dataset():
    """one graph of 301 nodes, two forward edge types (self loops + 2 forward + 2 backward = 5 types), 6 classes, about a
    fifth of the labels unknown, the rest split 60 / 20 / 20"""
    from tf2_gnn_amd.data import NodeClassificationDataset

    rng = np.random.default_rng(11)
    feats = rng.standard_normal((V_DS, D0_DS)).astype(np.float32)
    labels = rng.integers(0, C_DS, size=V_DS)
    labels[rng.random(V_DS) < 0.2] = -1
    edges = [rng.integers(0, V_DS, size=(1200 + 100 * t, 2)) for t in range(2)]
    known = rng.permutation(np.flatnonzero(labels >= 0))
    a, b = int(0.6 * len(known)), int(0.8 * len(known))
    ds = NodeClassificationDataset(NodeClassificationDataset.get_default_hyperparameters())
    ds.load_data_from_arrays(feats, labels, edges, train_idx=known[:a], valid_idx=known[a:b], test_idx=known[b:])
    assert ds.num_edge_types == 5 and ds.num_node_classes == C_DS and ds.node_feature_shape == (D0_DS,)
    return ds


def _task(ds, seed, **extra):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import NodeClassificationTask

    set_seed(seed)
    params = _gnn_params(NodeClassificationTask, "rgcn", H_DS, 2, extra={"gnn_layer_input_dropout_rate": 0.0, **extra})
    model = NodeClassificationTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    return model


def _single_batch(ds, fold, dev):
    batches = list(ds.get_batches(fold, dev))
    assert len(batches) == 1
    return batches[0]


def test_dataset_batches_equal_the_host_folds(dev):
    from tf2_gnn_amd import data
    from tf2_gnn_amd.data import DataFold, batch_assemble_launch_counts

    ds = _dataset()
    weights = {}
    for fold in (DataFold.TRAIN, DataFold.VALIDATION, DataFold.TEST):
        host = ds.packed_fold(fold)
        plan = ds.plan_epoch(fold, dev)
        assert plan.batches == [(0, 1)]
        before = batch_assemble_launch_counts()
        feats, labels = data.assemble_batch(plan, 0, 1)
        assert batch_assemble_launch_counts() - before == 1
        data.check_batch(feats)
        assert feats["num_graphs_in_batch"] == 1 and not bool(feats["node_to_graph_map"].any())
        assert np.array_equal(feats["node_features"].cpu().numpy(), host.features)
        for t in range(5):
            assert np.array_equal(feats[f"adjacency_list_{t}"].cpu().numpy(), host.edges[t]), t
        assert sorted(labels) == ["node_label_weights", "node_labels"]
        for name in labels:
            assert tuple(labels[name].shape) == (V_DS, 1) and labels[name].dtype == torch.float32
            assert np.array_equal(labels[name].cpu().numpy(), host.node_columns[name]), name
        weights[fold] = labels["node_label_weights"].cpu().numpy()
        # get_batches hands out the same single batch
        f2, l2 = _single_batch(ds, fold, dev)
        assert torch.equal(f2["node_features"], feats["node_features"]) and torch.equal(l2["node_labels"], labels["node_labels"])
        assert torch.equal(l2["node_label_weights"], labels["node_label_weights"])
    total = sum(weights.values())
    assert total.max() == 1.0 and int(total.sum()) == int((ds.packed_fold(DataFold.TRAIN).node_columns["node_labels"] >= 0).sum())


def test_training_steps_eager_and_replayed(dev):
    """5 Adam steps on the dataset's single batch through _run_step against a CapturedStep of the same step replayed 5 times
    from the same weights and optimizer state: every loss, every count and the final weights bit for bit (mirrors
    test_training_steps_eager_and_replayed of tests/test_gpu_binary_task.py).  The capture's warm-up steps train the twin, so
    it is put back to the initial state afterwards - in place: a replay reads the buffers the capture saw."""
    from tf2_gnn_amd import CapturedStep, ops
    from tf2_gnn_amd.data import DataFold

    ds = _dataset()
    feats, labels = _single_batch(ds, DataFold.TRAIN, dev)
    train = {"optimizer": "Adam", "learning_rate": 0.01}
    eager, twin = _task(ds, 6, **train), _task(ds, 7, **train)
    for a, b in zip(eager.trainable_variables, twin.trainable_variables):
        b.assign(a.value.clone())
    w0 = [v.value.clone() for v in twin.trainable_variables]

    def step():
        m = twin._run_step(feats, labels, training=True)
        return m["loss"], m["num_correct"], m["num_labelled"]

    try:
        cap = CapturedStep(step)
        cap.capture()
        for v, w in zip(twin.trainable_variables, w0):
            v.assign(w)
            for slot in twin._optimizer.slots(v):
                slot.zero_()
        twin._optimizer.iterations = 0
        ops.dropout_epoch_set(0)
        replayed = []
        for _ in range(5):
            replayed.append(tuple(t.clone() for t in cap.replay()))
        torch.cuda.synchronize()
        assert not cap.guard_tripped()

        ops.dropout_epoch_set(0)
        stepped = []
        for _ in range(5):
            m = eager._run_step(feats, labels, training=True)
            stepped.append((m["loss"].clone(), m["num_correct"].clone(), m["num_labelled"].clone()))
        torch.cuda.synchronize()
    finally:
        ops.dropout_epoch_set(0)  # every other test draws the masks of epoch 0
        torch.cuda.synchronize()
    assert eager._optimizer.iterations == twin._optimizer.iterations == 5
    for e, r in zip(stepped, replayed):
        assert all(torch.equal(a, b) for a, b in zip(e, r)), (stepped, replayed)
    num_train = int(ds.packed_fold(DataFold.TRAIN).node_columns["node_label_weights"].sum())
    assert all(int(n) == num_train for _, _, n in stepped)
    assert all(math.isfinite(float(l)) for l, _, _ in stepped) and float(stepped[-1][0]) < float(stepped[0][0])
    for a, b, w in zip(eager.trainable_variables, twin.trainable_variables, w0):
        assert torch.equal(a.value, b.value) and not torch.equal(a.value, w), a.name


def test_captured_evaluation_follows_an_in_place_mask_swap(dev):
    """A captured forward + metrics step on the training batch; the validation fold's weight column is copied IN PLACE over
    the batch's, and a replay - no re-capture - gives the loss and counts of an eager evaluation of the validation fold, bit
    for bit."""
    from tf2_gnn_amd import CapturedStep
    from tf2_gnn_amd.data import DataFold

    ds = _dataset()
    feats, labels = _single_batch(ds, DataFold.TRAIN, dev)
    valid_feats, valid_labels = _single_batch(ds, DataFold.VALIDATION, dev)
    model = _task(ds, 8)

    def step():
        m = model._run_step(feats, labels, training=False)
        return m["loss"], m["accuracy"], m["num_correct"], m["num_labelled"]

    def eager(f, l):
        m = model._run_step(f, l, training=False)
        return tuple(m[k].clone() for k in ("loss", "accuracy", "num_correct", "num_labelled"))

    cap = CapturedStep(step)
    cap.capture()
    on_train = tuple(t.clone() for t in cap.replay())
    assert not torch.equal(labels["node_label_weights"], valid_labels["node_label_weights"])
    labels["node_label_weights"].copy_(valid_labels["node_label_weights"])
    on_valid = tuple(t.clone() for t in cap.replay())
    torch.cuda.synchronize()
    assert cap.replays == 2 and not cap.guard_tripped()

    want_valid = eager(valid_feats, valid_labels)
    train_feats, train_labels = _single_batch(ds, DataFold.TRAIN, dev)  # a fresh training batch: the first one was overwritten
    want_train = eager(train_feats, train_labels)
    torch.cuda.synchronize()
    for got, want in ((on_train, want_train), (on_valid, want_valid)):
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (got, want)
        assert torch.equal(got[2], want[2]) and torch.equal(got[3], want[3]), (got, want)
    host = {f: int(ds.packed_fold(f).node_columns["node_label_weights"].sum()) for f in (DataFold.TRAIN, DataFold.VALIDATION)}
    assert int(on_train[3]) == host[DataFold.TRAIN] and int(on_valid[3]) == host[DataFold.VALIDATION]
    assert host[DataFold.TRAIN] != host[DataFold.VALIDATION]


def test_predict_and_evaluate_model(dev):
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.utils import eval_metrics

    ds = _dataset()
    model = _task(ds, 9)
    test = ds.get_batches(DataFold.TEST, dev)
    predictions = model.predict(test)
    assert predictions.is_cuda and tuple(predictions.shape) == (V_DS, C_DS) and bool(torch.isfinite(predictions).all())
    _, _, results = model.run_one_epoch(test, quiet=True, training=False)
    correct = sum(int(r["num_correct"]) for r in results)
    counted = sum(int(r["num_labelled"]) for r in results)
    metrics = model.evaluate_model(test)
    assert list(metrics) == ["acc", "macro_f1"]
    assert counted == int(ds.packed_fold(DataFold.TEST).node_columns["node_label_weights"].sum()) > 0
    assert metrics["acc"] == correct / counted
    host = ds.packed_fold(DataFold.TEST)
    want = eval_metrics.multiclass_metrics(host.node_columns["node_labels"], predictions.cpu().numpy().argmax(axis=1), C_DS,
                                           host.node_columns["node_label_weights"])
    assert metrics["macro_f1"] == want["macro_f1"] and 0.0 <= metrics["macro_f1"] <= 1.0
    assert model.compute_epoch_metrics(results) == (-metrics["acc"], f"Accuracy = {metrics['acc']:.3f}")
