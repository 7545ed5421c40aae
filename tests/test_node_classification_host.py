"""NodeClassificationTask, NodeClassificationDataset and tfgnn_softmax_ce_metrics as far as they go without a device: the C
entry point and its argument checks, the ops wrapper's refusal, hyper-parameters, variable names and checkpoints, epoch
metrics, the registry, the dataset's packing and its errors, and the multiclass evaluation metrics.  CPU-only; the arithmetic
is checked on the GPU (tests/test_gpu_softmax_ce.py, tests/test_gpu_node_classification.py)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tf2_gnn_amd import tasks
from tf2_gnn_amd.data import DataFold, NodeClassificationDataset, compute_number_of_edge_types, get_tied_edge_types
from tf2_gnn_amd.layers.message_passing import set_default_device
from tf2_gnn_amd.utils import eval_metrics, model_utils as mu, task_utils


@pytest.fixture
def cpu_params():
    set_default_device("cpu")
    yield
    set_default_device(None)


# ---- entry point ------------------------------------------------------------------------------------------------------------
def test_softmax_ce_metrics_entry_point_validates_without_gpu():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    for name in ("tfgnn_softmax_ce_metrics", "tfgnn_softmax_ce_workspace_bytes"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5  # new symbols, no signature changed
    ws_bytes = lib.tfgnn_softmax_ce_workspace_bytes()
    assert ws_bytes >= lib.tfgnn_task_metrics_workspace_bytes() >= 40 * 1024  # the older entries keep their requirement
    # never dereferenced: every call below is refused before a launch
    x, y, w, m, ws, d = (ctypes.c_void_p(a) for a in (0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000))

    def call(x=x, ldx=8, y=y, ldy=1, w=None, ldw=0, V=4, C=8, m=m, d=None, ldd=8, ws=ws, nbytes=ws_bytes):
        return lib.tfgnn_softmax_ce_metrics(x, ldx, y, ldy, w, ldw, V, C, m, None, d, ldd, None, ws, nbytes, None)

    for kwargs in ({"V": 0}, {"V": -3}, {"C": 0}, {"C": -1}):
        assert call(**kwargs) == -1
        assert b"empty batch" in lib.tfgnn_last_error()
    assert call(C=2 ** 24 + 1, ldx=2 ** 24 + 1) == -1
    assert b"2^24" in lib.tfgnn_last_error()
    for kwargs in ({"x": None}, {"y": None}, {"m": None}):
        assert call(**kwargs) == -1
        assert b"NULL" in lib.tfgnn_last_error()
    for kwargs in ({"ldx": 7}, {"ldy": 0}, {"w": w, "ldw": 0}, {"d": d, "ldd": 7}):
        assert call(**kwargs) == -1
        assert b"leading dimension" in lib.tfgnn_last_error()
    for kwargs in ({"ws": None}, {"nbytes": ws_bytes - 1}, {"ws": ctypes.c_void_p(0x5004)}):
        assert call(**kwargs) == -1
        assert b"workspace" in lib.tfgnn_last_error()
    with pytest.raises(ValueError, match="empty batch"):
        _lib.check(call(V=0))


def test_ops_wrapper_refuses_cpu_tensors():
    from tf2_gnn_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.softmax_ce_metrics(torch.zeros(3, 4), torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.softmax_ce_metrics(torch.zeros(3, 4), torch.zeros(3, dtype=torch.int64))


# ---- task -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp_style", [None, "rgcn", "rgin"])
def test_default_hyperparameters_are_the_base_models(mp_style):
    assert (tasks.NodeClassificationTask.get_default_hyperparameters(mp_style)
            == tasks.GraphTaskModel.get_default_hyperparameters(mp_style))
    assert issubclass(tasks.NodeClassificationTask, tasks.GraphTaskModel)
    assert tasks.NodeClassificationTask.predict is tasks.GraphTaskModel.predict


def test_construction_needs_the_number_of_classes():
    params = tasks.NodeClassificationTask.get_default_hyperparameters("rgcn")

    class NoClasses:
        num_edge_types = 3

    class Dataset(NoClasses):
        num_node_classes = 40

    with pytest.raises(ValueError, match="num_node_classes"):
        tasks.NodeClassificationTask(params, NoClasses())
    with pytest.raises(ValueError, match="num_node_classes"):
        tasks.NodeClassificationTask(params, num_edge_types=2)
    with pytest.raises(ValueError, match="num_edge_types"):
        tasks.NodeClassificationTask(params, num_node_classes=5)
    model = tasks.NodeClassificationTask(params, Dataset())
    assert model.num_node_classes == 40 and model._num_edge_types == 3 and model.name == "NodeClassificationTask"
    assert tasks.NodeClassificationTask(params, Dataset(), num_node_classes=7).num_node_classes == 7


def _build(**over):
    p = tasks.NodeClassificationTask.get_default_hyperparameters("rgcn")
    p.update(gnn_num_layers=2, gnn_hidden_dim=12)
    p.update(over)
    model = tasks.NodeClassificationTask(p, num_edge_types=2, num_node_classes=7)
    model.build({"node_features": (None, 5)})
    return model


def _randomise(model, seed):
    g = torch.Generator().manual_seed(seed)
    for v in model.variables:
        v.assign(torch.randn(v.value.shape, generator=g))


def test_variable_names_and_checkpoint_round_trip(cpu_params, tmp_path, capsys):
    model = _build()
    names = [v.name for v in model.variables]
    assert len(set(names)) == len(names)
    assert names[-2:] == ["NodeClassificationTask/kernel", "NodeClassificationTask/bias"]
    assert [tuple(v.value.shape) for v in model._task_variables()] == [(12, 7), (7,)]
    assert not any("NodeMulticlassTask" in n for n in names)

    _randomise(model, 1)
    want = {v.name: v.value.clone() for v in model.variables}
    path = str(tmp_path / "node_classification_best.pkl")
    mu.save_model(path, model)
    assert mu.load_pickle(path)["model_class"] is tasks.NodeClassificationTask
    _randomise(model, 2)
    restored = mu.load_weights_verbosely(path, model)
    assert sorted(restored) == sorted(names)
    assert all(torch.equal(v.value, want[v.name]) for v in model.variables)
    assert "freshly initialised" not in capsys.readouterr().out


def test_compute_epoch_metrics():
    """correct predictions over counted nodes across steps of different sizes, not the mean of the steps' accuracies"""
    model = tasks.NodeClassificationTask(tasks.NodeClassificationTask.get_default_hyperparameters("rgcn"), num_edge_types=1,
                                         num_node_classes=3)
    results = [
        {"loss": torch.tensor(0.7), "accuracy": torch.tensor(0.75), "num_correct": torch.tensor(3), "num_labelled": torch.tensor(4)},
        {"loss": torch.tensor(0.2), "accuracy": torch.tensor(1.0), "num_correct": torch.tensor(2), "num_labelled": torch.tensor(2)},
        {"loss": torch.tensor(0.0), "accuracy": torch.tensor(float("nan")), "num_correct": torch.tensor(0), "num_labelled": torch.tensor(0)},
        {"loss": torch.tensor(1.3), "accuracy": torch.tensor(0.1), "num_correct": 1, "num_labelled": 10},
    ]
    value, text = model.compute_epoch_metrics(results)
    assert value == -(6.0 / 16.0) and isinstance(value, float)
    assert text == "Accuracy = 0.375"
    value, _ = model.compute_epoch_metrics(results[2:3])
    assert math.isnan(value)


# ---- registry ---------------------------------------------------------------------------------------------------------------
def test_register_node_classification_task_adds_one_name():
    saved = dict(task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO)
    try:
        before = sorted(task_utils.get_known_tasks())
        assert "NodeClassification" not in before
        with pytest.raises(ValueError, match="Unknown task type"):
            task_utils.task_name_to_model_class("NodeClassification")
        task_utils.register_node_classification_task()
        assert sorted(task_utils.get_known_tasks()) == sorted(before + ["NodeClassification"])
        assert task_utils.task_name_to_dataset_class("nodeclassification") == (NodeClassificationDataset, {})
        assert task_utils.task_name_to_model_class("NodeClassification") == (tasks.NodeClassificationTask, {})
        for name in before:  # the other entries are the objects they were
            assert task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO[name.lower()] is saved[name.lower()]
    finally:
        task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO.clear()
        task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO.update(saved)
    assert sorted(task_utils.get_known_tasks()) == before


# ---- dataset ----------------------------------------------------------------------------------------------------------------
def _arrays(seed=0, two_graphs=True):
    """two graphs of 11 and 7 nodes, two forward edge types; labels in [0, 5) with some unknown"""
    rng = np.random.default_rng(seed)
    sizes = [11, 7] if two_graphs else [18]
    V = sum(sizes)
    feats = rng.standard_normal((V, 4)).astype(np.float32)
    labels = rng.integers(0, 5, size=V)
    labels[[2, 9, 15]] = -1
    labels[5] = 4  # the largest class occurs
    starts = np.cumsum([0] + sizes[:-1])
    edges = []
    for t in range(2):
        parts = [rng.integers(0, n, size=(2 * n + t, 2)) + s for n, s in zip(sizes, starts)]
        e = np.concatenate(parts)
        edges.append(e[rng.permutation(len(e))])  # graphs interleaved in the file
    known = np.flatnonzero(labels >= 0)
    perm = rng.permutation(known)
    idx = {"train_idx": perm[:8], "valid_idx": perm[8:11], "test_idx": perm[11:]}
    graph_id = np.repeat([7, 3], sizes) if two_graphs else None
    return feats, labels, edges, idx, graph_id


def _dataset(**over):
    params = NodeClassificationDataset.get_default_hyperparameters()
    params.update(over)
    return NodeClassificationDataset(params)


def _same_fold(a, b):
    assert np.array_equal(a.node_counts, b.node_counts) and np.array_equal(a.features, b.features)
    assert len(a.edges) == len(b.edges)
    for ea, eb, ca, cb in zip(a.edges, b.edges, a.edge_counts, b.edge_counts):
        assert np.array_equal(ea, eb) and np.array_equal(ca, cb)
    assert list(a.node_columns) == list(b.node_columns) == ["node_labels", "node_label_weights"]
    for k in a.node_columns:
        assert np.array_equal(a.node_columns[k], b.node_columns[k])


@pytest.mark.parametrize("self_loops,tie", [(True, False), (False, True), (True, [1])])
def test_load_data_and_load_data_from_arrays_agree(tmp_path, self_loops, tie):
    feats, labels, edges, idx, graph_id = _arrays()
    np.save(tmp_path / "node_features.npy", feats)
    np.save(tmp_path / "node_labels.npy", labels)
    for t, e in enumerate(edges):
        np.save(tmp_path / f"edges_{t}.npy", e)
    np.save(tmp_path / "node_graph_id.npy", graph_id)
    for name, a in idx.items():
        np.save(tmp_path / f"{name}.npy", a)
    hypers = {"add_self_loop_edges": self_loops, "tie_fwd_bkwd_edges": tie}
    from_files, from_arrays = _dataset(**hypers), _dataset(**hypers)
    with pytest.raises(ValueError, match="loaded"):
        from_files.num_edge_types
    from_files.load_data(tmp_path)
    from_arrays.load_data_from_arrays(feats, labels, edges, node_graph_id=graph_id, **idx)
    with pytest.raises(NotImplementedError):
        from_files.load_data_from_list([])

    tied = get_tied_edge_types(tie, 2)
    L = compute_number_of_edge_types(tied, 2, self_loops)
    assert from_files.num_edge_types == from_arrays.num_edge_types == L
    assert from_files.node_feature_shape == (4,) and from_files.num_node_classes == 5
    folds = [from_files.packed_fold(f) for f in (DataFold.TRAIN, DataFold.VALIDATION, DataFold.TEST)]
    for fold, data_fold in zip(folds, (DataFold.TRAIN, DataFold.VALIDATION, DataFold.TEST)):
        _same_fold(fold, from_arrays.packed_fold(data_fold))
        assert fold.num_edge_types == L and fold.node_counts.tolist() == [11, 7]
    train = folds[0]
    # the folds share the graph and the labels, and differ in the weights
    for other in folds[1:]:
        assert np.shares_memory(other.features, train.features)
        assert all(np.shares_memory(a, b) for a, b in zip(other.edges, train.edges))
        assert np.array_equal(other.node_columns["node_labels"], train.node_columns["node_labels"])
    for fold, name in zip(folds, ("train_idx", "valid_idx", "test_idx")):
        want = np.zeros((18, 1), dtype=np.float32)
        want[idx[name]] = 1.0
        assert np.array_equal(fold.node_columns["node_label_weights"], want)
    assert np.array_equal(train.node_columns["node_labels"][:, 0], labels.astype(np.float32))
    assert sum(f.node_columns["node_label_weights"] for f in folds).max() == 1.0  # disjoint

    # edge types: self loops first, then the forward types (a tied one followed by its flipped edges per graph), then the
    # backward types of the untied ones
    t0 = 1 if self_loops else 0
    if self_loops:
        assert train.edges[0].tolist() == [[i, i] for i in range(11)] + [[i, i] for i in range(7)]
    g0 = [e[(e[:, 0] < 11)] for e in edges]
    g1 = [e[(e[:, 0] >= 11)] - 11 for e in edges]
    untied = [t for t in range(2) if t not in tied]
    for t in range(2):
        got = train.edges[t0 + t]
        if t in tied:
            want = np.concatenate([g0[t], g0[t][:, ::-1], g1[t], g1[t][:, ::-1]])
        else:
            want = np.concatenate([g0[t], g1[t]])
            assert np.array_equal(train.edges[t0 + 2 + untied.index(t)], want[:, ::-1])
        assert np.array_equal(got, want)


def test_single_graph_from_edges_file_and_default_batching(tmp_path):
    from tf2_gnn_amd.data import plan_batches

    feats, labels, edges, idx, _ = _arrays(seed=1, two_graphs=False)
    np.save(tmp_path / "node_features.npy", feats)
    np.save(tmp_path / "node_labels.npy", labels.astype(np.int32))
    np.save(tmp_path / "edges.npy", edges[0])
    for name, a in idx.items():
        np.save(tmp_path / f"{name}.npy", a)
    ds = _dataset(num_node_classes=9)
    ds.load_data(tmp_path, folds_to_load={DataFold.TRAIN, DataFold.TEST})
    assert ds.num_node_classes == 9 and ds.num_edge_types == 3
    assert sorted(ds._loaded_data, key=lambda f: f.value) == [DataFold.TRAIN, DataFold.TEST]
    fold = ds.packed_fold(DataFold.TRAIN)
    assert fold.node_counts.tolist() == [18] and np.array_equal(fold.edges[1], edges[0])
    assert np.array_equal(fold.edges[2], edges[0][:, ::-1])
    # the default limit makes the largest graph int32 node ids admit one batch, with no empty batch in front
    limit = ds.params["max_nodes_per_batch"]
    assert plan_batches(np.array([2 ** 31 - 1]), limit) == [(0, 1)]
    assert plan_batches(np.array([11, 7]), limit) == [(0, 2)]


def test_dataset_errors():
    feats, labels, edges, idx, graph_id = _arrays()

    def load(feats=feats, labels=labels, edges=edges, graph_id=graph_id, hypers=(), **over):
        _dataset(**dict(hypers)).load_data_from_arrays(feats, labels, edges, node_graph_id=graph_id, **{**idx, **over})

    load()
    with pytest.raises(ValueError, match="outside the 18 nodes"):
        load(valid_idx=np.array([3, 18]))
    with pytest.raises(ValueError, match="outside the 18 nodes"):
        load(test_idx=np.array([-1]))
    with pytest.raises(ValueError, match="has label 4, the dataset has 4 classes"):
        load(hypers={"num_node_classes": 4})
    with pytest.raises(ValueError, match="TRAIN index 9 names a node without a label"):
        load(train_idx=np.array([0, 9]))
    with pytest.raises(ValueError, match="not contiguous"):
        load(graph_id=np.array([7] * 5 + [3] * 7 + [7] * 6))
    crossing = [edges[0], np.concatenate([edges[1], [[3, 12]]])]
    with pytest.raises(ValueError, match=r"edge \d+ of type 1 \(3 -> 12\) joins graph 7 and graph 3"):
        load(edges=crossing)
    with pytest.raises(ValueError, match="names a node outside"):
        load(edges=[np.array([[0, 18]]), edges[1]])
    with pytest.raises(ValueError, match="do not describe the same nodes"):
        load(feats=feats[:-1])
    with pytest.raises(ValueError, match="must be integers"):
        load(labels=labels + 0.5)
    with pytest.raises(ValueError, match="-1 stands for unknown"):
        load(labels=np.where(labels < 0, -2, labels))


# ---- metrics ----------------------------------------------------------------------------------------------------------------
def test_multiclass_metrics_by_hand():
    labels = [0, 0, 1, 1, 1, 3, -1, 2]
    preds_ = [0, 1, 1, 1, 3, 3, 0, 4]
    weights = [1, 1, 1, 1, 1, 1, 1, 0]
    m = eval_metrics.multiclass_metrics(labels, preds_, 5, weights)
    # counted: the first six.  class 0: tp 1 fp 0 fn 1 -> 2/3; class 1: tp 2 fp 1 fn 1 -> 4/6; class 3: tp 1 fp 1 fn 0 -> 2/3;
    # classes 2 and 4 occur only at uncounted samples and are left out
    assert list(m) == ["acc", "macro_f1"]
    assert m["acc"] == 4 / 6
    assert m["macro_f1"] == pytest.approx((2 / 3 + 4 / 6 + 2 / 3) / 3, rel=1e-15)
    # without weights the last sample counts too: classes 2 (fn only) and 4 (fp only) enter with F1 = 0
    m = eval_metrics.multiclass_metrics(labels, preds_, 5)
    assert m["acc"] == 4 / 7
    assert m["macro_f1"] == pytest.approx((2 / 3 + 4 / 6 + 2 / 3 + 0 + 0) / 5, rel=1e-15)
    perfect = eval_metrics.multiclass_metrics([2, 0, 2], [2, 0, 2], 3)
    assert perfect == {"acc": 1.0, "macro_f1": 1.0}
    nothing = eval_metrics.multiclass_metrics([-1, 7, 1], [0, 0, 0], 3, [1, 1, 0])
    assert math.isnan(nothing["acc"]) and math.isnan(nothing["macro_f1"])
    with pytest.raises(ValueError, match="differ in length"):
        eval_metrics.multiclass_metrics([0, 1], [0], 2)
