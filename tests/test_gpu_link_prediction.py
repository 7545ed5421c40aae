"""LinkPredictionTask and LinkPredictionDataset on the device: a 60-node graph with 3 relations, hidden width 64, a 2-layer
RGCN.  The task against the fp64 oracle stack with a float64 DistMult decoder and binary cross-entropy on top, and against the
op-level calls bit for bit (those are pinned in tests/test_gpu_distmult.py); training lowers the loss on a planted structure;
a CapturedStep replays bit-identically to its eager twin, also after a second ``iter()`` of the TRAIN fold rewrote triples and
tables in place; evaluate_model.  PARITY UNPINNED: the reference has no such task."""
import math

import numpy as np
import pytest
import torch

from tests import distmult_reference as ref
from tests.helpers import assert_close
from tests.test_gpu_layers import _gnn_oracle_weights, _to64
from tests.test_gpu_tasks import _check_grads, _gnn_pairs, _gnn_params, _leaves, _oracle_gnn

# the library's default mode and bench.py's comparison mode (conftest.py: gemm_modes)
pytestmark = [pytest.mark.gpu, pytest.mark.gemm_modes("f16x2", "bf16x3"), pytest.mark.usefixtures("gemm_mode")]

V_DS, D0_DS, H_DS, T_DS = 60, 8, 64, 3


def _dataset(negatives=2):
    """Planted structure: the parity p(v) of a node is in its features, and an edge u -> v has relation p(u) + p(v).  80 train
    edges per relation, 12 validation and 12 test edges per relation, all distinct."""
    from tf2_gnn_amd.data import LinkPredictionDataset

    rng = np.random.default_rng(21)
    parity = np.arange(V_DS) % 2
    feats = (0.1 * rng.standard_normal((V_DS, D0_DS))).astype(np.float32)
    feats[:, 0] += parity
    feats[:, 1] += 1 - parity
    pairs = rng.permutation(V_DS * V_DS)
    u, v = pairs // V_DS, pairs % V_DS
    rel = parity[u] + parity[v]
    train, valid, test = [], [], []
    for t in range(T_DS):
        e = np.stack([u[rel == t], v[rel == t]], axis=1)
        train.append(e[:80])
        valid.append(e[80:92])
        test.append(e[92:104])
    params = LinkPredictionDataset.get_default_hyperparameters()
    params["num_negatives_per_positive"] = negatives
    ds = LinkPredictionDataset(params)
    ds.load_data_from_arrays(feats, train, valid_edges=valid, test_edges=test)
    assert ds.num_relations == T_DS and ds.num_edge_types == 2 * T_DS + 1 and ds.node_feature_shape == (D0_DS,)
    return ds


def _task(ds, seed, **extra):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import LinkPredictionTask

    set_seed(seed)
    params = _gnn_params(LinkPredictionTask, "rgcn", H_DS, 2, extra={"gnn_layer_input_dropout_rate": 0.0, **extra})
    model = LinkPredictionTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    return model, params


def _single_batch(ds, fold, dev):
    batches = list(ds.get_batches(fold, dev))
    assert len(batches) == 1
    return batches[0]


def test_batches_carry_the_host_triples(dev):
    from tf2_gnn_amd import data, ops
    from tf2_gnn_amd.data import DataFold

    ds = _dataset()
    for fold in DataFold:
        feats, labels = _single_batch(ds, fold, dev)
        data.check_batch(feats)
        host = ds.packed_fold(fold)
        assert np.array_equal(feats["node_features"].cpu().numpy(), host.features)
        P = len(ds.positive_triples(fold))
        triples = labels["triples"].cpu().numpy()
        assert triples.shape == (3 * P, 3) and np.array_equal(triples[:P], ds.positive_triples(fold))
        assert labels["triple_labels"].tolist() == [1.0] * P + [0.0] * (2 * P) and bool((labels["triple_weights"] == 1).all())
        want = ops.build_triple_tables(triples, V_DS, T_DS)
        for name in ops.TRIPLE_TABLE_NAMES:
            assert np.array_equal(labels["triple_tables"][name].cpu().numpy(), want[name]), name
        for key in ("triples", "triple_labels", "triple_weights", "triple_tables"):
            assert feats[key] is labels[key]
        assert labels["positive_triples"].cpu().numpy().tolist() == ds.positive_triples(fold).tolist()
        for side in ("dst", "src"):
            for got, host_array in zip(labels["rank_filters"][side], ds.rank_filters(fold)[side]):
                assert got.is_cuda and np.array_equal(got.cpu().numpy(), host_array)


def _oracle(model, params, ds, labels):
    """the stack in float64 on the fold's processed adjacency lists, DistMult and the mean binary cross-entropy on top ->
    (h64, R64, loss64, (variable, float64 leaf) pairs, triples, labels)"""
    from tf2_gnn_amd.data import DataFold

    host = ds.packed_fold(DataFold.TRAIN)
    w64 = _to64(_gnn_oracle_weights(model._gnn))
    R64 = model._relation_embeddings.value.cpu().double().clone()
    _leaves(w64), _leaves(R64)
    h64, _ = _oracle_gnn(params, w64, torch.from_numpy(host.features).double(), host.edges)
    triples = labels["triples"].cpu().numpy()
    t = torch.from_numpy(triples.astype(np.int64))
    s64 = (h64[t[:, 0]] * R64[t[:, 1]] * h64[t[:, 2]]).sum(dim=1)
    y = labels["triple_labels"].cpu().double()
    loss64 = torch.nn.functional.binary_cross_entropy_with_logits(s64, y)
    pairs = _gnn_pairs(model._gnn, w64, ds.num_edge_types) + [(model._relation_embeddings, R64)]
    return h64, R64, loss64, pairs, triples, y


def test_torch_autograd_route_with_bce(dev):
    """TorchGraphTaskModel + F.binary_cross_entropy_with_logits on the device: the backward pass walks the triples and tables
    of the forward pass, and every weight gradient is inside the _check_grads bound against the same fp64 loss as the fused
    route."""
    from tf2_gnn_amd import TorchGraphTaskModel
    from tf2_gnn_amd.data import DataFold

    ds = _dataset()
    model, params = _task(ds, 5)
    feats, labels = _single_batch(ds, DataFold.TRAIN, dev)
    module = TorchGraphTaskModel(model).eval()
    scores = module(feats)
    assert scores.requires_grad and tuple(scores.shape) == (labels["triples"].shape[0],)
    torch.nn.functional.binary_cross_entropy_with_logits(scores, labels["triple_labels"]).backward()
    assert all(p.grad is not None for p in module.parameters())
    _, _, loss64, pairs, _, _ = _oracle(model, params, ds, labels)
    _check_grads(model, pairs, loss64, "TorchGraphTaskModel(LinkPredictionTask)")


def test_link_prediction_task_loss_and_gradients(dev):
    """batch -> scores -> loss / accuracy / counts -> every gradient, against the fp64 oracle stack with the float64 decoder on
    top.  Bounds: node representations 1e-5 (assert_close, as the sibling task tests hold the stack's outputs); a score then
    moves by at most sum_d |R[t, d]| (|h_u[d]| e_v[d] + |h_v[d]| e_u[d]) with e = 1e-5 max(1, |h|) - first order, 1 % added
    for the second - plus the kernel's own bound, and the loss, 1-Lipschitz in every score, by the mean of that plus 2e-6
    max(1, loss); gradients through _check_grads like every task.  And dH / dR of the task path equal the op-level calls on the
    same inputs bit for bit."""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import DataFold

    ds = _dataset()
    model, params = _task(ds, 3)
    with torch.no_grad():
        model._relation_embeddings.value.mul_(3.0)  # scores away from 0
    feats, labels = _single_batch(ds, DataFold.TRAIN, dev)
    before = ops.link_launch_counts()
    out = model(feats, training=False)
    with pytest.raises(RuntimeError):
        model.backward()  # no loss yet
    m = model.compute_task_metrics(feats, out, labels)
    assert ops.link_launch_counts()["distmult_fwd"] - before["distmult_fwd"] == 3  # one fused call for output and metrics
    assert sorted(m) == ["accuracy", "counts", "loss"] and all(isinstance(v, torch.Tensor) and v.is_cuda for v in m.values())
    assert m["counts"].dtype == torch.int64 and tuple(m["counts"].shape) == (4,)
    step = model._step
    d_h, none = model._task_backward()
    assert none is None
    op_dH, op_dR = ops.distmult_backward(step["h"], model._relation_embeddings.value, labels["triples"], step["dloss"],
                                         labels["triple_tables"])
    assert torch.equal(d_h.view(torch.int32), op_dH.view(torch.int32))
    assert torch.equal(model._relation_embeddings.grad.view(torch.int32), op_dR.view(torch.int32))
    model.zero_grad()
    model.backward()
    assert ops.link_launch_counts()["distmult_bwd"] - before["distmult_bwd"] == 3 * 4
    assert torch.equal(model._relation_embeddings.grad.view(torch.int32), op_dR.view(torch.int32))

    h64, R64, loss64, pairs, triples, y = _oracle(model, params, ds, labels)

    assert_close(step["h"].cpu(), h64.detach().float(), tol=1e-5, what="final node representations")
    hn, Rn = h64.detach().numpy(), R64.detach().numpy()
    e = 1e-5 * np.maximum(1.0, np.abs(hn))
    u, r, v = triples[:, 0], triples[:, 1], triples[:, 2]
    ds_stack = 1.01 * (np.abs(Rn[r]) * (np.abs(hn[u]) * e[v] + np.abs(hn[v]) * e[u])).sum(axis=1)
    exact = ref.distmult_ce(hn, Rn, triples, y.numpy())
    ds_total = ds_stack + exact.score_bound
    loss = float(loss64.detach())
    assert abs(exact.loss - loss) <= 1e-12
    bound = 2e-6 * max(1.0, loss) + float(ds_total.mean())
    err = abs(float(m["loss"]) - loss)
    print(f"LinkPredictionTask loss {float(m['loss']):.9g} fp64 {loss:.9g} error / bound {err / bound:.3f}")
    assert err <= bound
    scores = out[0].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(scores - exact.scores) <= ds_total)
    on_hip = ref.distmult_ce(hn, Rn, triples, y.numpy(), scores=scores)  # counts from the HIP scores
    assert [int(x) for x in m["counts"].cpu()] == list(on_hip.counts) and sum(on_hip.counts) == len(triples)
    assert abs(float(m["accuracy"]) - on_hip.accuracy) <= 1e-6
    value, text = model.compute_epoch_metrics([m, m])
    assert value == -on_hip.accuracy and text == f"Accuracy = {on_hip.accuracy:.3f}"
    _check_grads(model, pairs, loss64, "LinkPredictionTask")

    # labels of the caller's own: compute_task_metrics runs the kernel again on the representations of the last forward pass
    flipped = dict(labels, triple_labels=1.0 - labels["triple_labels"])
    m_flipped = model.compute_task_metrics(feats, out, flipped)
    assert [int(x) for x in m_flipped["counts"].cpu()] == [on_hip.counts[i] for i in (1, 0, 3, 2)]


def test_training_lowers_the_loss_on_planted_structure(dev):
    from tf2_gnn_amd.data import DataFold

    ds = _dataset()
    np.random.seed(3)
    feats, labels = _single_batch(ds, DataFold.TRAIN, dev)
    model, _ = _task(ds, 4, optimizer="Adam", learning_rate=0.01)
    losses = [float(model._run_step(feats, labels, training=True)["loss"]) for _ in range(30)]
    print(f"LinkPredictionTask 30 Adam steps: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert all(math.isfinite(l) for l in losses) and losses[-1] < losses[0]


def test_captured_step_equals_eager_also_after_in_place_negatives(dev):
    """3 Adam steps through _run_step against a CapturedStep of the same step replayed 3 times from the same weights and
    optimizer state: every loss, the counts and the final weights bit for bit (mirrors tests/test_gpu_node_classification.py).
    Then a second ``iter()`` of the TRAIN fold draws new negatives and rewrites triples and tables IN PLACE: one more replay -
    no re-capture - equals one more eager step on the new batch."""
    from tf2_gnn_amd import CapturedStep, ops
    from tf2_gnn_amd.data import DataFold

    ds = _dataset()
    np.random.seed(8)
    batches = ds.get_batches(DataFold.TRAIN, dev)
    feats, labels = next(iter(batches))
    train = {"optimizer": "Adam", "learning_rate": 0.01}
    (eager, _), (twin, _) = _task(ds, 6, **train), _task(ds, 7, **train)
    for a, b in zip(eager.trainable_variables, twin.trainable_variables):
        b.assign(a.value.clone())
    w0 = [v.value.clone() for v in twin.trainable_variables]

    def step():
        m = twin._run_step(feats, labels, training=True)
        return m["loss"], m["accuracy"], m["counts"]

    def eager_step():
        m = eager._run_step(feats, labels, training=True)
        return m["loss"].clone(), m["accuracy"].clone(), m["counts"].clone()

    try:
        cap = CapturedStep(step)
        cap.capture()
        for v, w in zip(twin.trainable_variables, w0):
            v.assign(w)
            for slot in twin._optimizer.slots(v):
                slot.zero_()
        twin._optimizer.iterations = 0
        ops.dropout_epoch_set(0)
        replayed = [tuple(t.clone() for t in cap.replay()) for _ in range(3)]
        torch.cuda.synchronize()
        ops.dropout_epoch_set(0)
        stepped = [eager_step() for _ in range(3)]
        torch.cuda.synchronize()

        old = labels["triples"].clone()
        ptrs = [labels["triples"].data_ptr()] + [labels["triple_tables"][n].data_ptr() for n in ops.TRIPLE_TABLE_NAMES]
        feats2, labels2 = next(iter(batches))  # the second epoch: new negatives, same buffers
        assert labels2["triples"] is labels["triples"] and labels2["triple_tables"] is labels["triple_tables"]
        assert ptrs == [labels["triples"].data_ptr()] + [labels["triple_tables"][n].data_ptr() for n in ops.TRIPLE_TABLE_NAMES]
        P = len(ds.positive_triples(DataFold.TRAIN))
        assert torch.equal(labels["triples"][:P], old[:P]) and not torch.equal(labels["triples"][P:], old[P:])
        assert torch.equal(feats2["node_features"], feats["node_features"])
        replayed.append(tuple(t.clone() for t in cap.replay()))
        stepped.append(eager_step())
        torch.cuda.synchronize()
        assert not cap.guard_tripped()
    finally:
        ops.dropout_epoch_set(0)  # every other test draws the masks of epoch 0
        torch.cuda.synchronize()
    assert eager._optimizer.iterations == twin._optimizer.iterations == 4
    for e, r in zip(stepped, replayed):
        assert all(torch.equal(a, b) for a, b in zip(e, r)), (stepped, replayed)
        assert torch.equal(e[0].view(torch.int32), r[0].view(torch.int32))
    assert all(int(c.sum()) == 3 * P for _, _, c in stepped) and all(math.isfinite(float(l)) for l, _, _ in stepped)
    for a, b, w in zip(eager.trainable_variables, twin.trainable_variables, w0):
        assert torch.equal(a.value, b.value) and not torch.equal(a.value, w), a.name


def test_evaluate_model(dev):
    """The four keys on the real model; and with integer-valued node representations and relation embeddings in [-2, 2] (the
    exact family: every fp32 score is exact) the metrics equal ranking_metrics of the float64 reference's filtered counts over
    both sides exactly."""
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.utils import eval_metrics

    ds = _dataset()
    model, _ = _task(ds, 9)
    test = ds.get_batches(DataFold.TEST, dev)
    metrics = model.evaluate_model(test)
    assert list(metrics) == ["mrr", "hits@1", "hits@3", "hits@10"]
    assert all(0.0 <= v <= 1.0 for v in metrics.values()) and metrics["hits@1"] <= metrics["hits@3"] <= metrics["hits@10"]
    predictions = model.predict(test)
    assert predictions.is_cuda and tuple(predictions.shape) == (3 * len(ds.positive_triples(DataFold.TEST)),)

    rng = np.random.default_rng(5)
    H = rng.integers(-2, 3, size=(V_DS, H_DS)).astype(np.float32)
    R = rng.integers(-2, 3, size=(T_DS, H_DS)).astype(np.float32)
    model._relation_embeddings.assign(torch.from_numpy(R).to(dev))
    H_dev = torch.from_numpy(H).to(dev)
    model.compute_final_node_representations = lambda inputs, training: H_dev
    for fold in (DataFold.VALIDATION, DataFold.TEST):
        got = model.evaluate_model(ds.get_batches(fold, dev))
        greater, equal = [], []
        for side in ("dst", "src"):
            g, e, _, _ = ref.distmult_rank(H, R, ds.positive_triples(fold), side, *ds.rank_filters(fold)[side])
            greater.append(g)
            equal.append(e)
        want = eval_metrics.ranking_metrics(np.concatenate(greater), np.concatenate(equal))
        assert got == want, (fold, got, want)
        assert np.concatenate(equal).sum() > 0  # ties occur, and split evenly
