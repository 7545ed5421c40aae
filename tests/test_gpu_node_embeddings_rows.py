"""The hyper-parameter ``node_embedding_update`` end to end, in the sampled setting of tests/test_gpu_node_embeddings.py: node
classification on 200 featureless nodes, one tied forward type and self loops, fanouts [3, 3], 16 seeds per batch, width 32,
rgcn.  ``"rows"`` keeps the table's gradient as an optim.RowGradient and updates the batch's rows only: against a ``"dense"``
twin where the two must agree (Adam's first step, plain SGD), the rows and slots it must leave alone, the documented
difference from the dense step, the full batch that takes the dense route, and the other paths a gradient travels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V_NC, H_NC, C_NC = 200, 32, 4


def _nc_dataset(**over):
    from tf2_gnn_amd.data import NodeClassificationDataset

    rng = np.random.default_rng(8)
    labels = rng.integers(0, C_NC, size=V_NC)
    edges = [rng.integers(0, V_NC, size=(700, 2))]
    order = rng.permutation(V_NC)
    params = NodeClassificationDataset.get_default_hyperparameters()
    params.update({"tie_fwd_bkwd_edges": True, "add_self_loop_edges": True, "neighbor_fanouts": [3, 3], "seeds_per_batch": 16,
                   "sampling_seed": 3})
    params.update(over)
    ds = NodeClassificationDataset(params)
    ds.load_data_from_arrays(None, labels, edges, train_idx=order[:120], valid_idx=order[120:160], test_idx=order[160:])
    return ds


def _nc_task(ds, seed, update, **extra):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import NodeClassificationTask

    set_seed(seed)
    params = NodeClassificationTask.get_default_hyperparameters("rgcn")
    params.update({"gnn_hidden_dim": H_NC, "gnn_num_layers": 2, "gnn_global_exchange_every_num_layers": 10000,
                   "gnn_dense_every_num_layers": 2, "gnn_residual_every_num_layers": 2, "gnn_layer_input_dropout_rate": 0.0,
                   "optimizer": "Adam", "learning_rate": 0.01, "node_embedding_dim": H_NC})
    if update is not None:
        params["node_embedding_update"] = update
    params.update(extra)
    model = NodeClassificationTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    return model


def _table(model):
    (table,) = [v for v in model.trainable_variables if v.name.endswith("/node_embeddings")]
    return table


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _batches(ds, dev, count, seed=2):
    from tf2_gnn_amd.data import DataFold

    np.random.seed(seed)
    it = iter(ds.get_batches(DataFold.TRAIN, dev))
    return [next(it) for _ in range(count)]


def _pair(dev, seed, **extra):
    ds = _nc_dataset()
    rows, dense = _nc_task(ds, seed, "rows", **extra), _nc_task(ds, seed, "dense", **extra)
    for a, b in zip(rows.trainable_variables, dense.trainable_variables):
        assert a.name == b.name and _same(a.value, b.value), a.name
    return ds, rows, dense


def test_adam_first_and_second_step_against_a_dense_twin(dev):
    from tf2_gnn_amd import RowGradient, ops

    ds, rows, dense = _pair(dev, seed=51)
    (feats1, labels1), (feats2, labels2) = _batches(ds, dev, 2)
    ids1, ids2 = (f["sampled_node_ids"].cpu().numpy() for f in (feats1, feats2))
    table, table_d = _table(rows), _table(dense)

    # one step: moments are zero at step 1, so rows without a gradient do not move on either route - the tables are equal
    launches = ops.embedding_launch_count()
    out = rows(feats1, training=True)
    rows.compute_task_metrics(feats1, out, labels1)
    pairs = rows.backward()
    grad = dict((v.name, g) for v, g in pairs)[table.name]
    assert isinstance(grad, RowGradient) and grad.shape == (V_NC, H_NC) and grad.ids is feats1["sampled_node_ids"]
    assert grad.bad_flag is rows.embedding_bad_index and tuple(grad.rows.shape) == (ids1.shape[0], H_NC)
    rows._apply_gradients(pairs)
    torch.cuda.synchronize()
    assert ops.embedding_launch_count() == launches and rows._node_embeddings_grad is None
    dense._run_step(feats1, labels1, training=True)
    torch.cuda.synchronize()
    assert ops.embedding_launch_count() == launches + 2 and tuple(dense._node_embeddings_grad.shape) == (V_NC, H_NC)
    for a, b in zip(rows.trainable_variables, dense.trainable_variables):
        assert _same(a.value, b.value), a.name  # the whole table among them
    assert rows._optimizer.iterations == dense._optimizer.iterations == 1 and int(rows.embedding_bad_index) == 0

    # a second step on another batch: outside its ids the "rows" model keeps the table and both slots bit for bit; the dense
    # twin moves rows that step 1 touched and step 2 did not, along their decaying moments - the documented difference
    after1 = table.value.clone()
    slots1 = [s.clone() for s in rows._optimizer.slots(table)]
    assert len(slots1) == 2
    rows._run_step(feats2, labels2, training=True)
    dense._run_step(feats2, labels2, training=True)
    torch.cuda.synchronize()
    assert rows._node_embeddings_grad is None and ops.embedding_launch_count() == launches + 4
    outside = np.ones(V_NC, dtype=bool)
    outside[ids2] = False
    outside_dev = torch.from_numpy(outside).to(dev)
    assert _same(table.value[outside_dev], after1[outside_dev])
    assert not _same(table.value[~outside_dev], after1[~outside_dev])
    for s, s1 in zip(rows._optimizer.slots(table), slots1):
        assert _same(s.view(V_NC, H_NC)[outside_dev], s1.view(V_NC, H_NC)[outside_dev])
    only_first = np.zeros(V_NC, dtype=bool)
    only_first[ids1] = True
    only_first &= outside
    assert only_first.any()
    moved_d = (_bits(table_d.value) != _bits(after1)).any(dim=1).cpu().numpy()  # after step 1 the two tables were equal
    assert moved_d[only_first].any()
    never = np.ones(V_NC, dtype=bool)
    never[ids1] = False
    never &= outside
    assert not moved_d[never].any()  # zero moments, zero gradient: no row moves there on either route


def test_plain_sgd_equals_the_dense_twin_after_every_step(dev):
    ds, rows, dense = _pair(dev, seed=52, optimizer="SGD", momentum=0.0, learning_rate=0.05, gradient_clip_value=0.01)
    for step, (feats, labels) in enumerate(_batches(ds, dev, 4, seed=5)):
        rows._run_step(feats, labels, training=True)
        dense._run_step(feats, labels, training=True)
        torch.cuda.synchronize()
        for a, b in zip(rows.trainable_variables, dense.trainable_variables):
            assert _same(a.value, b.value), (step, a.name)
    assert rows._optimizer.kind == "sgd" and rows._optimizer.slots(_table(rows)) == [] and rows._optimizer.iterations == 4
    assert rows._node_embeddings_grad is None and dense._node_embeddings_grad is not None


def test_full_batch_takes_the_dense_route_and_stays_capturable(dev):
    from tf2_gnn_amd import CapturedStep, _lib, ops
    from tf2_gnn_amd.data import DataFold

    lib = _lib.load()
    ds = _nc_dataset(neighbor_fanouts=None)
    (feats, labels), = list(ds.get_batches(DataFold.TRAIN, dev))
    assert "sampled_node_ids" not in feats
    counts = {}
    for update in ("rows", "dense"):
        model = _nc_task(ds, 53, update)
        before = (lib.tfgnn_optimizer_launch_count(), ops.embedding_launch_count())
        out = model(feats, training=True)
        model.compute_task_metrics(feats, out, labels)
        pairs = model.backward()
        grad = dict((v.name, g) for v, g in pairs)[_table(model).name]
        assert isinstance(grad, torch.Tensor) and tuple(grad.shape) == (V_NC, H_NC)
        model._apply_gradients(pairs)
        torch.cuda.synchronize()
        counts[update] = (lib.tfgnn_optimizer_launch_count() - before[0], ops.embedding_launch_count() - before[1])
    assert counts["rows"] == counts["dense"] and counts["rows"][1] == 0

    eager, twin = _nc_task(ds, 54, "rows"), _nc_task(ds, 54, "rows")

    def step():
        return twin._run_step(feats, labels, training=True)["loss"]

    cap = CapturedStep(step)  # 4 eager warm-up steps, each with its update
    cap.capture()
    for _ in range(2):
        loss_c = cap.replay()
    torch.cuda.synchronize()
    loss_c = float(loss_c)
    for _ in range(4 + 2):
        loss_e = eager._run_step(feats, labels, training=True)["loss"]
    torch.cuda.synchronize()
    assert float(loss_e) == loss_c and eager._optimizer.iterations == twin._optimizer.iterations == 6
    for a, b in zip(eager.trainable_variables, twin.trainable_variables):
        assert _same(a.value, b.value), a.name


def test_torch_wrapper_checkpoint_and_evaluation(dev, tmp_path):
    from tf2_gnn_amd import RowGradient, TorchGraphTaskModel
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.utils.model_utils import load_weights_verbosely, save_model

    ds = _nc_dataset()
    model = _nc_task(ds, 55, "rows")
    table = _table(model)
    (feats, labels), = _batches(ds, dev, 1, seed=6)
    # torch wrapper: torch optimizers take dense gradients - .grad of the table is the dense scatter of the row gradient
    module = TorchGraphTaskModel(model).eval()
    params = list(module.parameters())
    index = [v.name for v in module._vars].index(table.name)
    assert params[index].data_ptr() == table.value.data_ptr()
    logits = module(feats)
    logits = logits[0] if isinstance(logits, (tuple, list)) else logits
    logits.square().sum().backward()
    wrapped = params[index].grad.clone()
    torch.cuda.synchronize()
    assert isinstance(table.grad, RowGradient)
    ids = feats["sampled_node_ids"].cpu().numpy()
    want = np.zeros((V_NC, H_NC), dtype=np.float32)
    want[ids] = table.grad.rows.cpu().numpy()
    assert tuple(wrapped.shape) == (V_NC, H_NC) and float(np.abs(want).max()) > 0.0
    assert np.array_equal(wrapped.cpu().numpy().view(np.int32), want.view(np.int32))
    assert _same(table.grad.to_dense(), wrapped)
    # a training step, then a checkpoint round trip by name
    model._run_step(feats, labels, training=True)
    path = str(tmp_path / "model.pkl")
    save_model(path, model, ds)
    other = _nc_task(ds, 56, "rows")
    assert not _same(_table(other).value, table.value)
    restored = load_weights_verbosely(path, other)
    assert restored[table.name] == table.name + ":0" and len(restored) == len(model.trainable_variables)
    for a, b in zip(model.trainable_variables, other.trainable_variables):
        assert _same(a.value, b.value), a.name
    # evaluation
    metrics = model.evaluate_model(ds.get_batches(DataFold.VALIDATION, dev))
    assert set(metrics) >= {"acc", "macro_f1"} and 0.0 <= metrics["acc"] <= 1.0 and 0.0 <= metrics["macro_f1"] <= 1.0
