"""Learned node embeddings (the hyper-parameter ``node_embedding_dim``) end to end on featureless datasets.

Link prediction: 60 entities, 30 relations, about 200 training edges, untied backward types and self loops - 61 processed edge
types, so the batch goes through the chunked assembly -, no feature file; LinkPredictionTask on rgcn_basis and rgcn_blockdiag
at width 64 (the width tests/test_gpu_link_prediction.py uses), embeddings of the same width.  The gradients against a twin
that is fed the table's initial values as features; replays of a captured training step against eager steps; evaluation; a
checkpoint round trip; the torch wrapper.

Node classification, neighbour-sampled: 200 nodes, one tied forward type and self loops (2 edge types), fanouts [3, 3], 16
seeds per batch, width 32, no feature file: the rows an Adam step moves, the table gradient against a numpy scatter, the
full-batch route that launches nothing for the lookup, evaluation.  And the three refusals."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

V_LP, T_LP, H_LP = 60, 30, 64
LAYERS = ["rgcn_basis", "rgcn_blockdiag"]


# ---- link prediction --------------------------------------------------------------------------------------------------------
def _lp_edges():
    rng = np.random.default_rng(33)
    pairs = rng.permutation(V_LP * V_LP)[:260]
    u, v = pairs // V_LP, pairs % V_LP
    rel = rng.integers(0, T_LP, size=260)
    split = lambda lo, hi: [np.stack([u[lo:hi][rel[lo:hi] == t], v[lo:hi][rel[lo:hi] == t]], axis=1) for t in range(T_LP)]
    return split(0, 200), split(200, 230), split(230, 260)


def _lp_dataset(features=None, **over):
    from tf2_gnn_amd.data import LinkPredictionDataset

    params = LinkPredictionDataset.get_default_hyperparameters()
    params.update(over)
    ds = LinkPredictionDataset(params)
    train, valid, test = _lp_edges()
    ds.load_data_from_arrays(features, train, valid_edges=valid, test_edges=test, num_nodes=None if features is not None else V_LP)
    return ds


def _lp_task(ds, mp_style, seed, embeddings=True, **extra):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import LinkPredictionTask

    set_seed(seed)
    params = LinkPredictionTask.get_default_hyperparameters(mp_style)
    params.update({"gnn_hidden_dim": H_LP, "gnn_num_layers": 2, "gnn_global_exchange_every_num_layers": 10000,
                   "gnn_dense_every_num_layers": 2, "gnn_residual_every_num_layers": 2, "gnn_layer_input_dropout_rate": 0.0,
                   "optimizer": "Adam", "learning_rate": 0.01})
    if embeddings:
        params["node_embedding_dim"] = H_LP
    params.update(extra)
    model = LinkPredictionTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    return model


def _table(model):
    (table,) = [v for v in model.trainable_variables if v.name.endswith("/node_embeddings")]
    return table


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_featureless_batch_of_61_edge_types(dev):
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.data.graph_dataset import batch_assemble_launch_counts

    ds = _lp_dataset()
    assert ds.num_edge_types == 61 and ds.num_nodes == V_LP and ds.node_feature_shape == (0,)
    before = batch_assemble_launch_counts()
    np.random.seed(0)
    (feats, labels), = list(ds.get_batches(DataFold.TRAIN, dev))
    assert batch_assemble_launch_counts() - before == 2
    nf = feats["node_features"]
    assert nf.dtype == torch.float32 and tuple(nf.shape) == (V_LP, 0) and nf.is_cuda
    train, _, _ = _lp_edges()
    assert feats["adjacency_list_0"].cpu().tolist() == [[i, i] for i in range(V_LP)]
    for t in (0, 17, 29):  # forward type t is processed type 1 + t, its backward type 1 + 30 + t
        assert np.array_equal(feats[f"adjacency_list_{1 + t}"].cpu().numpy(), train[t])
        assert np.array_equal(feats[f"adjacency_list_{31 + t}"].cpu().numpy(), train[t][:, ::-1])
    assert int(feats["_bad_local_index"]) == 0


@pytest.mark.gemm_modes("f16x2", "bf16x3")
@pytest.mark.parametrize("mp_style", LAYERS)
def test_gradients_equal_a_feature_fed_twin(dev, mp_style, gemm_mode):
    from tf2_gnn_amd.data import DataFold

    ds_a = _lp_dataset()
    model_a = _lp_task(ds_a, mp_style, seed=11)
    table = _table(model_a)
    assert table.name == "LinkPredictionTask/node_embeddings" and table.shape == (V_LP, H_LP)
    assert model_a.trainable_variables[-1] is table
    # the twin: no key, the table's initial values as the dataset's features, the same init seed
    ds_b = _lp_dataset(features=table.value.cpu().numpy())
    model_b = _lp_task(ds_b, mp_style, seed=11, embeddings=False)
    shared_a = {v.name: v for v in model_a.trainable_variables if v is not table}
    shared_b = {v.name: v for v in model_b.trainable_variables}
    assert list(shared_a) == list(shared_b) and "LinkPredictionTask/relation_embeddings" in shared_a
    for name in shared_a:
        assert torch.equal(_bits(shared_a[name].value), _bits(shared_b[name].value)), name
    np.random.seed(4)
    feats_a, labels_a = next(iter(ds_a.get_batches(DataFold.TRAIN, dev)))
    np.random.seed(4)
    feats_b, labels_b = next(iter(ds_b.get_batches(DataFold.TRAIN, dev)))
    assert torch.equal(labels_a["triples"], labels_b["triples"])
    assert torch.equal(_bits(feats_b["node_features"]), _bits(table.value))
    out_a = model_a(feats_a, training=True)
    m_a = model_a.compute_task_metrics(feats_a, out_a, labels_a)
    model_a.backward()
    out_b = model_b(feats_b, training=True)
    m_b = model_b.compute_task_metrics(feats_b, out_b, labels_b)
    model_b.backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out_a[0]), _bits(out_b[0])) and torch.equal(_bits(m_a["loss"]), _bits(m_b["loss"]))
    assert torch.equal(m_a["counts"], m_b["counts"])
    for name in shared_a:
        ga, gb = shared_a[name].grad, shared_b[name].grad
        assert ga is not None and gb is not None and torch.equal(_bits(ga), _bits(gb)), name
    # the table's gradient is the stack's input gradient
    grad_final, grad_all = model_b._task_backward()
    d_features = model_b._gnn.backward(grad_final, need_input_grad=True, grad_all_representations=grad_all)
    torch.cuda.synchronize()
    assert tuple(table.grad.shape) == (V_LP, H_LP) and torch.equal(_bits(table.grad), _bits(d_features))
    assert float(table.grad.abs().max()) > 0.0
    # the features of the dataset are not read with the key set: NaN features, the same scores
    nan_feats = dict(feats_b, node_features=torch.full_like(feats_b["node_features"], float("nan")))
    assert torch.equal(_bits(model_a(nan_feats, training=False)[0]), _bits(model_a(feats_a, training=False)[0]))


@pytest.mark.gemm_modes("f16x2", "bf16x3")
@pytest.mark.parametrize("mp_style", LAYERS)
def test_captured_steps_equal_eager_steps(dev, mp_style, gemm_mode):
    """three replays of a captured training step against three eager steps of an identically seeded model.  Both draw their
    negatives on the device: a replay with the captured call's seed at the dropout epoch the replay advanced to, so the eager
    twin's sampler is put on that seed and the epoch word on that epoch before each of its steps."""
    from tf2_gnn_amd import CapturedStep, ops
    from tf2_gnn_amd.data import DataFold

    ds_a, ds_b = (_lp_dataset(negative_sampling="device", negative_sampling_seed=7) for _ in range(2))
    ops.dropout_epoch_set(0)
    feats_a, labels_a = next(iter(ds_a.get_batches(DataFold.TRAIN, dev)))
    feats_b, labels_b = next(iter(ds_b.get_batches(DataFold.TRAIN, dev)))
    model_a, model_b = _lp_task(ds_a, mp_style, seed=21), _lp_task(ds_b, mp_style, seed=21)
    w0 = [v.value.clone() for v in model_a.trainable_variables]
    assert all(torch.equal(a.value, b.value) for a, b in zip(model_a.trainable_variables, model_b.trainable_variables))
    sampler_a, sampler_b = feats_a["triple_sampler"], feats_b["triple_sampler"]

    def step():
        m = model_a._run_step(feats_a, labels_a, training=True)
        return m["loss"], m["counts"]

    try:
        cap = CapturedStep(step)
        cap.capture()
        for v, w in zip(model_a.trainable_variables, w0):  # back to the start: the warm-up steps trained
            v.assign(w)
            for slot in model_a._optimizer.slots(v):
                slot.zero_()
        model_a._optimizer.iterations = 0
        ops.dropout_epoch_set(0)
        replayed, drawn = [], []
        for _ in range(3):
            out = cap.replay()
            replayed.append(tuple(t.clone() for t in out))
            drawn.append(labels_a["triples"].clone())
        torch.cuda.synchronize()
        assert ops.dropout_epoch() == 3 and not cap.guard_tripped()
        stepped = []
        for i in range(3):
            sampler_b.draws = sampler_a.draws - 1  # the captured draw's seed
            ops.dropout_epoch_set(i + 1)
            m = model_b._run_step(feats_b, labels_b, training=True)
            assert sampler_b.seed_of_last_draw == sampler_a.seed_of_last_draw
            assert torch.equal(labels_b["triples"], drawn[i]), f"step {i}: other negatives than replay {i}"
            stepped.append((m["loss"].clone(), m["counts"].clone()))
        torch.cuda.synchronize()
    finally:
        ops.dropout_epoch_set(0)
        torch.cuda.synchronize()
    assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[1], drawn[2])
    assert model_a._optimizer.iterations == model_b._optimizer.iterations == 3
    for (loss_e, counts_e), (loss_r, counts_r) in zip(stepped, replayed):
        assert torch.equal(_bits(loss_e), _bits(loss_r)) and torch.equal(counts_e, counts_r)
    for a, b, w in zip(model_a.trainable_variables, model_b.trainable_variables, w0):
        assert a.name == b.name and torch.equal(_bits(a.value), _bits(b.value)), a.name  # the table among them
        assert not torch.equal(a.value, w), a.name
        slots_a, slots_b = model_a._optimizer.slots(a), model_b._optimizer.slots(b)
        assert len(slots_a) == len(slots_b) == 2  # Adam: m and v
        for sa, sb in zip(slots_a, slots_b):
            assert torch.equal(_bits(sa), _bits(sb)), a.name
    assert _table(model_a) is model_a.trainable_variables[-1]


@pytest.mark.parametrize("mp_style", LAYERS)
def test_evaluation_checkpoint_and_torch_wrapper(dev, mp_style, tmp_path):
    from tf2_gnn_amd import TorchGraphTaskModel
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.utils.model_utils import load_weights_verbosely, save_model

    ds = _lp_dataset()
    model = _lp_task(ds, mp_style, seed=31)
    table = _table(model)
    # evaluation
    metrics = model.evaluate_model(ds.get_batches(DataFold.VALIDATION, dev))
    assert list(metrics) == ["mrr", "hits@1", "hits@3", "hits@10"] and all(0.0 <= v <= 1.0 for v in metrics.values())
    # checkpoint: the table travels under its name
    path = str(tmp_path / "model.pkl")
    save_model(path, model, ds)
    other = _lp_task(ds, mp_style, seed=32)
    assert not torch.equal(_table(other).value, table.value)
    restored = load_weights_verbosely(path, other)
    assert restored["LinkPredictionTask/node_embeddings"] == "LinkPredictionTask/node_embeddings:0"
    assert len(restored) == len(model.trainable_variables)
    for a, b in zip(model.trainable_variables, other.trainable_variables):
        assert torch.equal(_bits(a.value), _bits(b.value)), a.name
    # torch wrapper: the table is a parameter, loss.backward() fills its .grad with the explicit backward's bits
    np.random.seed(6)
    feats, labels = next(iter(ds.get_batches(DataFold.TRAIN, dev)))
    module = TorchGraphTaskModel(model).eval()
    params = list(module.parameters())
    index = [v.name for v in module._vars].index("LinkPredictionTask/node_embeddings")
    assert len(params) == len(model.trainable_variables) and params[index].data_ptr() == table.value.data_ptr()
    scores = module(feats)
    torch.nn.functional.binary_cross_entropy_with_logits(scores, labels["triple_labels"]).backward()
    assert all(p.grad is not None for p in params)
    wrapped = params[index].grad.clone()
    detached = scores.detach().clone().requires_grad_(True)
    torch.nn.functional.binary_cross_entropy_with_logits(detached, labels["triple_labels"]).backward()
    model(feats, training=False)
    model._step["dloss"] = detached.grad.contiguous()
    model.backward()
    torch.cuda.synchronize()
    assert tuple(wrapped.shape) == (V_LP, H_LP) and torch.equal(_bits(wrapped), _bits(table.grad))
    assert float(wrapped.abs().max()) > 0.0


# ---- node classification, neighbour-sampled ----------------------------------------------------------------------------------
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


def _nc_task(ds, seed, **extra):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import NodeClassificationTask

    set_seed(seed)
    params = NodeClassificationTask.get_default_hyperparameters("rgcn")
    params.update({"gnn_hidden_dim": H_NC, "gnn_num_layers": 2, "gnn_global_exchange_every_num_layers": 10000,
                   "gnn_dense_every_num_layers": 2, "gnn_residual_every_num_layers": 2, "gnn_layer_input_dropout_rate": 0.0,
                   "optimizer": "Adam", "learning_rate": 0.01, "node_embedding_dim": H_NC})
    params.update(extra)
    model = NodeClassificationTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    return model


def test_sampled_step_moves_the_sampled_rows_only(dev):
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import DataFold

    ds = _nc_dataset()
    assert ds.num_edge_types == 2 and ds.num_nodes == V_NC and ds.node_feature_shape == (0,)
    model = _nc_task(ds, seed=41)
    table = _table(model)
    assert table.name == "NodeClassificationTask/node_embeddings" and table.shape == (V_NC, H_NC)
    np.random.seed(2)
    feats, labels = next(iter(ds.get_batches(DataFold.TRAIN, dev)))
    ids = feats["sampled_node_ids"].cpu().numpy()
    n = ids.shape[0]
    assert feats["num_seed_nodes"] == 16 and 16 < n < V_NC and np.unique(ids).shape[0] == n
    assert tuple(feats["node_features"].shape) == (n, 0) and feats["node_features"].dtype == torch.float32
    before = table.value.clone()
    launches = ops.embedding_launch_count()
    model._run_step(feats, labels, training=True)
    torch.cuda.synchronize()
    assert ops.embedding_launch_count() - launches == 2  # the fill and the scatter
    moved = (_bits(table.value) != _bits(before)).any(dim=1).cpu().numpy()
    touched = np.zeros(V_NC, dtype=bool)
    touched[ids] = True
    # Adam at step 1 with a zero gradient and zero moments moves nothing: the other rows keep their bits
    assert not moved[~touched].any()
    assert moved[touched].all()
    assert int(model.embedding_bad_index) == 0 and int(feats["_bad_local_index"]) == 0


def test_sampled_table_gradient_is_the_scatter_of_the_input_gradient(dev):
    from tf2_gnn_amd.data import DataFold

    ds = _nc_dataset()
    model = _nc_task(ds, seed=42)
    table = _table(model)
    np.random.seed(3)
    batches = iter(ds.get_batches(DataFold.TRAIN, dev))
    for _ in range(2):  # two batches through the same gradient buffer: the second must not keep rows of the first
        feats, labels = next(batches)
        out = model(feats, training=True)
        model.compute_task_metrics(feats, out, labels)
        model.backward()
        got = table.grad.clone()
        grad_final, grad_all = model._task_backward()
        d_rows = model._gnn.backward(grad_final, need_input_grad=True, grad_all_representations=grad_all)
        torch.cuda.synchronize()
        ids = feats["sampled_node_ids"].cpu().numpy()
        want = np.zeros((V_NC, H_NC), dtype=np.float32)
        want[ids] = d_rows.cpu().numpy()
        assert tuple(d_rows.shape) == (ids.shape[0], H_NC) and float(np.abs(want).max()) > 0.0
        assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


def test_full_batch_takes_the_table_itself(dev):
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import DataFold

    ds = _nc_dataset(neighbor_fanouts=None)
    model = _nc_task(ds, seed=43)
    table = _table(model)
    (feats, labels), = list(ds.get_batches(DataFold.TRAIN, dev))
    assert "sampled_node_ids" not in feats and tuple(feats["node_features"].shape) == (V_NC, 0)
    x0 = model.compute_initial_node_features(feats, training=True)
    assert x0.data_ptr() == table.value.data_ptr() and tuple(x0.shape) == (V_NC, H_NC)
    before_table = table.value.clone()
    scatter, (_, gathers) = ops.embedding_launch_count(), ops.sample_launch_counts()
    m = model._run_step(feats, labels, training=True)
    torch.cuda.synchronize()
    assert ops.embedding_launch_count() == scatter and ops.sample_launch_counts()[1] == gathers  # no launch for the lookup
    assert tuple(table.grad.shape) == (V_NC, H_NC) and bool(torch.isfinite(m["loss"]))
    assert not torch.equal(table.value, before_table)


def test_sampled_evaluation(dev):
    from tf2_gnn_amd.data import DataFold

    ds = _nc_dataset()
    model = _nc_task(ds, seed=44)
    metrics = model.evaluate_model(ds.get_batches(DataFold.VALIDATION, dev))
    assert set(metrics) >= {"acc", "macro_f1"} and 0.0 <= metrics["acc"] <= 1.0 and 0.0 <= metrics["macro_f1"] <= 1.0


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.tasks import NodeClassificationTask

    ds = _nc_dataset()
    params = NodeClassificationTask.get_default_hyperparameters("rgcn")
    with pytest.raises(ValueError, match="node_embedding_dim"):  # a featureless dataset without the key
        NodeClassificationTask(dict(params), dataset=ds)
    with pytest.raises(ValueError, match=r"dataset\.num_nodes.*num_nodes="):  # the key, but nothing that says how many rows
        NodeClassificationTask(dict(params, node_embedding_dim=8), num_edge_types=2, num_node_classes=C_NC)
    model = _nc_task(ds, seed=45)
    np.random.seed(1)
    feats, labels = next(iter(ds.get_batches(DataFold.TRAIN, dev)))
    anonymous = {k: v for k, v in feats.items() if k != "sampled_node_ids"}
    with pytest.raises(ValueError, match="without sampled_node_ids"):  # another row count, and no ids
        model(anonymous, training=False)
