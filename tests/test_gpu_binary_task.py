"""GraphBinaryClassificationTask on the device (tf2_gnn/models/graph_binary_classification_task.py): the fused
cross-entropy / accuracy / gradient kernel against an fp64 restatement of its arithmetic contract (include/tfgnn.h
tfgnn_binary_ce_metrics), the task as "the regression task plus the new head" bit for bit, whole training steps eager and
replayed, the torch.autograd route, predict / evaluate_model and checkpoints.

The fp64 restatements live here (oracle/ holds none for this task): the formulas of the header comment with eps and hi taken
as their float32 values converted to float64.  PARITY UNPINNED like the other float losses: TensorFlow does not run beside
this library."""
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_tasks import _batch, _features, _gnn_params

# every test of this module runs in the three GEMM modes (conftest.py: gemm_modes)
pytestmark = [pytest.mark.gpu, pytest.mark.gemm_modes, pytest.mark.usefixtures("gemm_mode")]

EPS = float(np.float32(1e-7))
HI = float(np.float32(1.0) - np.float32(1e-7))


def _binary_ce_fp64(x: torch.Tensor, y: torch.Tensor):
    """-> loss, accuracy, (tp, fp, tn, fn), probabilities, d loss / d logits; all float64 on the host"""
    x, y = x.double(), y.double()
    G = x.numel()
    p = torch.sigmoid(x)
    pc = p.clamp(EPS, HI)
    bce = -(y * torch.log(pc + EPS) + (1.0 - y) * torch.log(1.0 - pc + EPS))
    pred = torch.round(p)  # half to even
    counts = (int(((pred == 1) & (y == 1)).sum()), int(((pred == 1) & (y == 0)).sum()),
              int(((pred == 0) & (y == 0)).sum()), int(((pred == 0) & (y == 1)).sum()))
    inside = (p >= EPS) & (p <= HI)
    grad = torch.where(inside, (-(y / (pc + EPS)) + (1.0 - y) / (1.0 - pc + EPS)) * p * (1.0 - p) / G, torch.zeros_like(p))
    return float(bce.mean()), float((pred == y).sum()) / G, counts, p, grad


def _kernel_inputs(G):
    """logits 3 * randn clamped to |x| <= 12, every 7th exactly 0 (sigmoid = 0.5 rounds to 0), every 11th +-20 (clipped
    probabilities, alternating sign); labels Bernoulli(0.3).  No logit lies in 12 < |x| < 20: p crosses the clip values near
    |x| = 16, where the gradient jumps between 0 and about 0.5 / G with the last bit of the sigmoid - a property of the
    formula, not an error to measure.  Nothing is excluded from the comparison."""
    g = torch.Generator().manual_seed(G)
    x = (torch.randn(G, generator=g) * 3).clamp(-12.0, 12.0)
    x[::7] = 0.0
    saturated = torch.arange(0, G, 11)
    x[saturated] = 20.0 * (1.0 - 2.0 * (torch.arange(saturated.numel()) % 2))
    y = (torch.rand(G, generator=g) < 0.3).float()
    assert not bool(((x.abs() > 12) & (x.abs() < 20)).any())
    return x, y, saturated


@pytest.mark.parametrize("G", [1, 37, 200000])
def test_binary_ce_metrics_kernel(dev, G):
    """Bounds: counts exact; loss and accuracy 2e-6 * max(1, |ref|), the bound test_sigmoid_ce_metrics_kernel holds its loss
    to; gradient 1e-6 / G + 1e-7 max|ref| (same test); probabilities 1e-6; exactly 0 gradient at the clipped entries; the loss
    bit-identical run to run (fixed-order reduction)."""
    from tf2_gnn_amd import ops

    x, y, saturated = _kernel_inputs(G)
    metrics, counts, prob, grad = ops.binary_ce_metrics(x.to(dev), y.to(dev))
    loss, acc, ref_counts, p64, g64 = _binary_ce_fp64(x, y)
    err_loss, err_acc = abs(float(metrics[0]) - loss), abs(float(metrics[1]) - acc)
    err_grad = float((grad.cpu().double() - g64).abs().max())
    err_prob = float((prob.cpu().double() - p64).abs().max())
    bound_grad = 1e-6 / G + 1e-7 * float(g64.abs().max())
    print(f"binary_ce_metrics G={G}: loss {float(metrics[0]):.9g} ref {loss:.9g} |err| {err_loss:.3g} "
          f"(bound {2e-6 * max(1.0, abs(loss)):.3g}); acc |err| {err_acc:.3g}; dlogits max|err| * G {err_grad * G:.3g} "
          f"(bound * G {bound_grad * G:.3g}); prob max|err| {err_prob:.3g}")
    assert counts.dtype == torch.int64 and counts.cpu().tolist() == list(ref_counts)
    assert sum(ref_counts) == G
    assert err_loss <= 2e-6 * max(1.0, abs(loss))
    assert err_acc <= 2e-6 * max(1.0, abs(acc))
    assert err_grad <= bound_grad
    assert bool((grad.cpu()[saturated] == 0.0).all()) and bool((g64[saturated] == 0.0).all())
    assert bool((grad.cpu()[x == 0.0] != 0.0).all())
    assert err_prob <= 1e-6
    again, counts2, no_prob, no_grad = ops.binary_ce_metrics(x.to(dev), y.to(dev), need_grad=False, want_prob=False)
    assert no_prob is None and no_grad is None
    assert torch.equal(again, metrics) and torch.equal(counts2, counts)


def test_binary_ce_metrics_arguments(dev):
    from tf2_gnn_amd import ops

    with pytest.raises(ValueError, match="empty batch"):
        ops.binary_ce_metrics(torch.zeros(0, device=dev), torch.zeros(0, device=dev))
    with pytest.raises(ValueError, match="differ in shape"):
        ops.binary_ce_metrics(torch.zeros(4, device=dev), torch.zeros(5, device=dev))
    with pytest.raises(TypeError):
        ops.binary_ce_metrics(torch.zeros(4, device=dev, dtype=torch.float64), torch.zeros(4, device=dev))
    # [G, 1] logits and strided labels are flattened
    x = torch.tensor([[-1.0], [0.0], [2.0]], device=dev)
    y = torch.tensor([[0.0, 9.0], [1.0, 9.0], [1.0, 9.0]], device=dev)[:, 0]
    metrics, counts, prob, grad = ops.binary_ce_metrics(x, y)
    assert counts.cpu().tolist() == [1, 0, 1, 1] and prob.shape == (3,) and grad.shape == (3,)
    assert abs(float(metrics[1]) - 2.0 / 3.0) <= 1e-7


# ---------------------------------------------------------------------------------------------------------------
SIZES, L, D0, H = [14, 3, 21, 8, 5], 2, 6, 16
NO_DROPOUT = {"gnn_layer_input_dropout_rate": 0.0, "graph_aggregation_dropout_rate": 0.0, "regression_mlp_dropout": 0.0}


def _params(cls, intermediate=True, **extra):
    return _gnn_params(cls, "rgcn", H, 3, extra={
        "use_intermediate_gnn_results": intermediate, "graph_aggregation_output_size": 8, "graph_aggregation_num_heads": 2,
        "graph_aggregation_layers": [12], "regression_mlp_layers": [10, 6],
        "gnn_dense_every_num_layers": 10000 if intermediate else 2, **NO_DROPOUT, **extra})


def _model(cls, dev, seed, intermediate=True, **extra):
    from tf2_gnn_amd.layers.message_passing import set_seed

    set_seed(seed)
    model = cls(_params(cls, intermediate, **extra), num_edge_types=L)
    model.build({"node_features": (None, D0)})
    return model


def _stripped(model):
    """variable by name without the class prefix of the head's scopes"""
    return {v.name.replace(model.__class__.__name__ + "/", "", 1): v for v in model.trainable_variables}


def _copy_weights(src, dst):
    a, b = _stripped(src), _stripped(dst)
    assert list(a) == list(b)
    for name, v in b.items():
        v.assign(a[name].value.clone())


def _labels(G, seed, dev):
    return {"target_value": (torch.rand(G, generator=torch.Generator().manual_seed(seed)) < 0.4).float().to(dev)}


@pytest.mark.parametrize("intermediate", [True, False])
def test_binary_task_is_the_regression_task_plus_the_head(dev, intermediate):
    """Same hyper-parameters and weights, evaluation mode: the output is the library's sigmoid pass over the regression
    task's output, and every variable gradient is the regression task's when that is fed the kernel's d loss / d logits - bit
    for bit.  The pieces underneath are checked against the fp64 oracle in test_gpu_tasks.py, the kernel above."""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.tasks import GraphBinaryClassificationTask, GraphRegressionTask

    X, adjs, n2g = _batch(SIZES, L, D0, seed=8)
    G = len(SIZES)
    feats = _features(X, adjs, n2g, G, dev)
    reg = _model(GraphRegressionTask, dev, 3, intermediate)
    binary = _model(GraphBinaryClassificationTask, dev, 4, intermediate)
    for b in reg._regression_mlp.biases:
        b.assign(torch.randn(b.shape, generator=torch.Generator().manual_seed(5)) * 0.2)
    _copy_weights(reg, binary)
    labels = _labels(G, 7, dev)

    reg_out = reg(feats, training=False)
    out = binary(feats, training=False)
    assert out.shape == (G,) and torch.equal(out, ops.activation_forward("sigmoid", reg_out))
    assert torch.equal(binary._step["logits"], reg_out) and binary._step["prob"] is out
    with pytest.raises(RuntimeError):
        binary.backward()  # no loss yet

    m = binary.compute_task_metrics(feats, out, labels)
    assert sorted(m) == ["batch_acc", "loss", "num_correct", "num_graphs"]
    assert m["num_graphs"] == float(G) and isinstance(m["num_graphs"], float)
    loss, acc, counts, _, g64 = _binary_ce_fp64(reg_out.cpu(), labels["target_value"].cpu())
    assert int(m["num_correct"]) == counts[0] + counts[2] and m["num_correct"].dtype == torch.int64
    assert abs(float(m["batch_acc"]) - acc) <= 1e-6 and abs(float(m["loss"]) - loss) <= 2e-6 * max(1.0, loss)
    value, text = binary.compute_epoch_metrics([m, m])
    assert value == -acc and text == f"Accuracy = {acc:.3f}"
    dlogits = binary._step["dlogits"]
    assert binary._step["dloss"] is None
    assert float((dlogits.cpu().double() - g64).abs().max()) <= 1e-6 / G + 1e-7 * float(g64.abs().max())
    binary.backward()

    reg.compute_task_metrics(feats, reg_out, labels)
    reg._step["dloss"] = dlogits
    reg.backward()
    torch.cuda.synchronize()
    for (name, v), r in zip(_stripped(binary).items(), _stripped(reg).values()):
        assert v.grad is not None and torch.equal(v.grad, r.grad), name
    fused = [v.grad.clone() for v in binary.trainable_variables]

    # probabilities of the caller's own: the same formula, unfused, gradient with respect to the probabilities
    out = binary(feats, training=False)
    m2 = binary.compute_task_metrics(feats, out.clone(), labels)
    assert int(m2["num_correct"]) == int(m["num_correct"]) and float(m2["batch_acc"]) == float(m["batch_acc"])
    assert abs(float(m2["loss"]) - loss) <= 2e-6 * max(1.0, loss)
    assert binary._step["dloss"] is not None
    binary.backward()
    for v, g in zip(binary.trainable_variables, fused):
        scale = max(float(g.abs().max()), 1e-30)
        assert float((v.grad - g).abs().max()) / scale <= 1e-5, v.name


def test_training_steps_eager_and_replayed(dev):
    """5 Adam steps on a fixed batch through _run_step against a CapturedStep of the same step replayed 5 times from the
    same weights, optimizer state and dropout epoch: every loss and the final weights bit for bit (the contract of
    test_captured_step_with_update_equals_the_eager_steps).  The capture's warm-up steps train the twin, so it is put back to
    the initial state afterwards - in place: a replay reads the buffers the capture saw."""
    from tf2_gnn_amd import CapturedStep, ops
    from tf2_gnn_amd.tasks import GraphBinaryClassificationTask

    X, adjs, n2g = _batch(SIZES, L, D0, seed=9)
    G = len(SIZES)
    feats = _features(X, adjs, n2g, G, dev)
    labels = _labels(G, 11, dev)
    train = {"optimizer": "Adam", "learning_rate": 0.01}
    eager = _model(GraphBinaryClassificationTask, dev, 6, **train)
    twin = _model(GraphBinaryClassificationTask, dev, 7, **train)
    _copy_weights(eager, twin)
    w0 = [v.value.clone() for v in twin.trainable_variables]

    def step():
        out = twin(feats, training=True)
        metrics = twin.compute_task_metrics(feats, out, labels)
        twin._apply_gradients(twin.backward())
        return metrics["loss"], metrics["num_correct"]

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
            loss, num_correct = cap.replay()
            replayed.append((loss.clone(), num_correct.clone()))
        torch.cuda.synchronize()
        assert not cap.guard_tripped()

        ops.dropout_epoch_set(0)
        stepped = []
        for _ in range(5):
            m = eager._run_step(feats, labels, training=True)
            stepped.append((m["loss"].clone(), m["num_correct"].clone()))
        torch.cuda.synchronize()
    finally:
        ops.dropout_epoch_set(0)  # every other test draws the masks of epoch 0
        torch.cuda.synchronize()
    assert eager._optimizer.iterations == twin._optimizer.iterations == 5 and eager._train_step_counter == 5
    for (le, ce), (lr, cr) in zip(stepped, replayed):
        assert torch.equal(le, lr) and torch.equal(ce, cr), (stepped, replayed)
    assert all(math.isfinite(float(l)) for l, _ in stepped) and float(stepped[-1][0]) < float(stepped[0][0])
    for a, b, w in zip(eager.trainable_variables, twin.trainable_variables, w0):
        assert torch.equal(a.value, b.value) and not torch.equal(a.value, w), a.name


def test_torch_autograd_route_agrees_with_the_fused_route(dev):
    """TorchGraphTaskModel hands backward() a gradient with respect to the probabilities; torch's binary_cross_entropy has no
    "+ eps" inside its logs and clamps the logs instead of the probabilities, so the two routes agree to rounding only where
    nothing is clipped: asserted below (|logit| <= 12).  Tolerance: 1e-5 of each gradient's largest entry, as the node
    multiclass check of test_gpu_autograd.py."""
    from tf2_gnn_amd import TorchGraphTaskModel
    from tf2_gnn_amd.tasks import GraphBinaryClassificationTask

    X, adjs, n2g = _batch(SIZES, L, D0, seed=12)
    G = len(SIZES)
    feats = _features(X, adjs, n2g, G, dev)
    labels = _labels(G, 13, dev)
    model = _model(GraphBinaryClassificationTask, dev, 8)
    module = TorchGraphTaskModel(model).eval()
    prob = module(feats)
    assert prob.requires_grad and float(model._step["logits"].abs().max()) <= 12.0
    torch.nn.functional.binary_cross_entropy(prob, labels["target_value"]).backward()
    got = [p.grad.clone() for p in module.parameters()]
    assert model._step["dloss"] is not None

    out = model(feats, training=False)
    assert torch.equal(out, prob.detach())
    model.compute_task_metrics(feats, out, labels)
    for (v, g), mine in zip(model.backward(), got):
        scale = max(float(g.abs().max()), 1e-30)
        assert float((mine.reshape(g.shape) - g).abs().max()) / scale <= 1e-5, v.name


def test_predict_evaluate_model_and_checkpoint(dev, tmp_path):
    """predict = the concatenated evaluation-mode outputs (graph_task_model.py:401-408); evaluate_model = the host metrics
    of those predictions; a saved and restored model predicts the same bits."""
    from tf2_gnn_amd.tasks import GraphBinaryClassificationTask, GraphRegressionTask, NodeMulticlassTask
    from tf2_gnn_amd.utils import eval_metrics, model_utils

    dataset = []
    for k, sizes in enumerate(([14, 3, 21, 8], [5, 9], [7, 7, 2, 30, 11, 4])):
        X, adjs, n2g = _batch(sizes, L, D0, seed=20 + k)
        g = torch.Generator().manual_seed(30 + k)
        target = (torch.rand(len(sizes), generator=g) < 0.5).float()
        dataset.append((_features(X, adjs, n2g, len(sizes), dev), {"target_value": target.to(dev)}))
    num_graphs = sum(f["num_graphs_in_batch"] for f, _ in dataset)
    all_labels = torch.cat([l["target_value"] for _, l in dataset]).cpu().numpy()
    assert 0 < all_labels.sum() < num_graphs

    for cls, metric_fn in ((GraphBinaryClassificationTask, eval_metrics.binary_classification_metrics),
                           (GraphRegressionTask, eval_metrics.regression_metrics)):
        model = _model(cls, dev, 9)
        for b in model._regression_mlp.biases:
            b.assign(torch.randn(b.shape, generator=torch.Generator().manual_seed(5)) * 0.2)
        want = torch.cat([model(f, training=False).clone() for f, _ in dataset], dim=0)
        got = model.predict(dataset)
        assert got.is_cuda and got.shape == (num_graphs,) and torch.equal(got, want)
        metrics = model.evaluate_model(dataset)
        ref = metric_fn(all_labels, want.cpu().numpy())
        assert list(metrics) == list(ref)
        for k in ref:
            assert metrics[k] == ref[k] or (math.isnan(metrics[k]) and math.isnan(ref[k])), (k, metrics[k], ref[k])
        assert all(math.isfinite(v) for v in metrics.values()), metrics

        path = str(tmp_path / f"{cls.__name__}_best.pkl")
        model_utils.save_model(path, model)
        fresh = _model(cls, dev, 10)
        assert not torch.equal(fresh.predict(dataset), want)
        restored = model_utils.load_weights_verbosely(path, fresh)
        assert sorted(restored) == sorted(v.name for v in fresh.variables)
        assert torch.equal(fresh.predict(dataset), want)

    # a 1-tuple output (NodeMulticlassTask) contributes its element
    params = _gnn_params(NodeMulticlassTask, "rgcn", H, 2)
    nodes = NodeMulticlassTask(params, num_edge_types=L, num_node_target_labels=3)
    want = torch.cat([nodes(f, training=False)[0] for f, _ in dataset], dim=0)
    assert torch.equal(nodes.predict(dataset), want) and want.shape[1] == 3
    with pytest.raises(NotImplementedError):
        nodes.evaluate_model(dataset)
