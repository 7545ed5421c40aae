"""GraphBinaryClassificationTask, predict / evaluate_model and tfgnn_binary_ce_metrics, as far as they go without a device
(tf2_gnn/models/graph_binary_classification_task.py, graph_task_model.py:401-420): the C entry point and its argument
checks, hyper-parameters, epoch metrics, variable names and checkpoints.  CPU-only; the arithmetic is checked on the GPU
(tests/test_gpu_binary_task.py)."""
import pytest
import torch

from tf2_gnn_amd import tasks
from tf2_gnn_amd.layers.message_passing import set_default_device
from tf2_gnn_amd.utils import model_utils as mu


@pytest.fixture
def cpu_params():
    set_default_device("cpu")
    yield
    set_default_device(None)


def test_binary_ce_metrics_entry_point_validates_without_gpu():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    assert "tfgnn_binary_ce_metrics" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "tfgnn_binary_ce_metrics")
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5  # a new symbol, no signature changed
    ws_bytes = lib.tfgnn_task_metrics_workspace_bytes()
    assert ws_bytes >= 40 * 1024  # what the two older entries were sized for
    # never dereferenced: every call below is refused before a launch
    x, y, m, ws = (ctypes_ptr(a) for a in (0x1000, 0x2000, 0x3000, 0x4000))
    for G in (0, -3):
        assert lib.tfgnn_binary_ce_metrics(x, y, G, None, m, None, None, ws, ws_bytes, None) == -1
        msg = lib.tfgnn_last_error()
        assert b"empty batch" in msg and b"nan" in msg
    for args in ((None, y, 4, None, m), (x, None, 4, None, m), (x, y, 4, None, None)):
        assert lib.tfgnn_binary_ce_metrics(*args, None, None, ws, ws_bytes, None) == -1
        assert b"NULL" in lib.tfgnn_last_error()
    assert lib.tfgnn_binary_ce_metrics(x, y, 4, None, m, None, None, None, ws_bytes, None) == -1
    assert b"workspace" in lib.tfgnn_last_error()
    assert lib.tfgnn_binary_ce_metrics(x, y, 4, None, m, None, None, ws, ws_bytes - 1, None) == -1
    assert b"workspace" in lib.tfgnn_last_error()
    with pytest.raises(ValueError, match="empty batch"):
        _lib.check(lib.tfgnn_binary_ce_metrics(x, y, 0, None, m, None, None, ws, ws_bytes, None))


def ctypes_ptr(address):
    import ctypes

    return ctypes.c_void_p(address)


def test_ops_wrapper_refuses_cpu_tensors():
    from tf2_gnn_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.binary_ce_metrics(torch.zeros(3), torch.zeros(3))


@pytest.mark.parametrize("mp_style", [None, "rgcn", "ggnn"])
def test_default_hyperparameters_are_the_regression_tasks(mp_style):
    """graph_binary_classification_task.py:12-19: the parent's, nothing added"""
    assert (tasks.GraphBinaryClassificationTask.get_default_hyperparameters(mp_style)
            == tasks.GraphRegressionTask.get_default_hyperparameters(mp_style))
    assert issubclass(tasks.GraphBinaryClassificationTask, tasks.GraphRegressionTask)


def test_construction_needs_the_number_of_edge_types_like_the_parent():
    for cls in (tasks.GraphRegressionTask, tasks.GraphBinaryClassificationTask):
        with pytest.raises(ValueError, match="num_edge_types"):
            cls(cls.get_default_hyperparameters("rgcn"))

    class Dataset:
        num_edge_types = 3

    model = tasks.GraphBinaryClassificationTask(tasks.GraphBinaryClassificationTask.get_default_hyperparameters("rgcn"), Dataset())
    assert model._num_edge_types == 3 and model.name == "GraphBinaryClassificationTask"


def test_compute_epoch_metrics():
    """:60-68: correct predictions over graphs, across batches of different sizes; the smaller the better, so -accuracy"""
    model = tasks.GraphBinaryClassificationTask(tasks.GraphBinaryClassificationTask.get_default_hyperparameters("rgcn"),
                                                num_edge_types=1)
    results = [
        {"loss": torch.tensor(0.7), "batch_acc": torch.tensor(0.75), "num_correct": torch.tensor(3), "num_graphs": 4.0},
        {"loss": torch.tensor(0.2), "batch_acc": torch.tensor(1.0), "num_correct": torch.tensor(2), "num_graphs": 2.0},
        {"loss": torch.tensor(1.3), "batch_acc": torch.tensor(0.1), "num_correct": 1, "num_graphs": 10.0},
    ]
    value, text = model.compute_epoch_metrics(results)
    assert value == -(6.0 / 16.0) and isinstance(value, float)
    assert text == "Accuracy = 0.375"


def test_evaluate_model_of_the_base_class_is_not_implemented():
    model = tasks.GraphTaskModel(tasks.GraphTaskModel.get_default_hyperparameters("rgcn"), num_edge_types=2)
    with pytest.raises(NotImplementedError):
        model.evaluate_model([])
    for cls in (tasks.GraphRegressionTask, tasks.GraphBinaryClassificationTask):
        assert cls.evaluate_model is not tasks.GraphTaskModel.evaluate_model
    for cls in (tasks.NodeMulticlassTask, tasks.QM9RegressionTask, tasks.GraphRegressionTask, tasks.GraphBinaryClassificationTask):
        assert cls.predict is tasks.GraphTaskModel.predict


def _build(cls, **over):
    p = cls.get_default_hyperparameters("rgcn")
    p.update(gnn_num_layers=2, gnn_hidden_dim=12, graph_aggregation_output_size=8, graph_aggregation_num_heads=2,
             graph_aggregation_layers=[6], regression_mlp_layers=[10, 6])
    p.update(over)
    model = cls(p, num_edge_types=2)
    model.build({"node_features": (None, 5)})
    return model


def _randomise(model, seed):
    g = torch.Generator().manual_seed(seed)
    for v in model.variables:
        v.assign(torch.randn(v.value.shape, generator=g))


def test_variable_names_and_checkpoint_round_trip(cpu_params, tmp_path, capsys):
    """The head's variables carry the class name, as in the reference's checkpoints (name scopes of
    graph_regression_task.py:91-106 under the subclass), and differ from the regression task's in that prefix only."""
    model = _build(tasks.GraphBinaryClassificationTask)
    reg = _build(tasks.GraphRegressionTask)
    names = [v.name for v in model.variables]
    assert len(set(names)) == len(names)
    head = [n for n in names if n.startswith("GraphBinaryClassificationTask/")]
    assert len(head) == len(model._task_variables()) and not any("GraphRegressionTask" in n for n in names)
    assert [n.replace("GraphBinaryClassificationTask/", "GraphRegressionTask/") for n in names] == [v.name for v in reg.variables]

    _randomise(model, 1)
    want = {v.name: v.value.clone() for v in model.variables}
    path = str(tmp_path / "binary_best.pkl")
    mu.save_model(path, model)
    assert mu.load_pickle(path)["model_class"] is tasks.GraphBinaryClassificationTask
    _randomise(model, 2)
    restored = mu.load_weights_verbosely(path, model)
    assert sorted(restored) == sorted(names)
    assert all(torch.equal(v.value, want[v.name]) for v in model.variables)
    assert "freshly initialised" not in capsys.readouterr().out


def test_regression_checkpoint_into_the_binary_task(cpu_params, tmp_path, capsys):
    """A GraphRegressionTask pickle loaded into the binary task.  The relaxed-name path of load_weights_verbosely drops
    auto-generated layer names and an MLP's wrapper scope; it does NOT drop or rewrite a class prefix, and it is not widened
    for this: the stack's weights (no class prefix) are restored, the head's stay as initialised and are reported, the saved
    head weights are reported as unused.  The renaming hook the loader already has carries the head over."""
    reg = _build(tasks.GraphRegressionTask)
    _randomise(reg, 3)
    path = str(tmp_path / "regression_best.pkl")
    mu.save_model(path, reg)

    model = _build(tasks.GraphBinaryClassificationTask)
    _randomise(model, 4)
    before = {v.name: v.value.clone() for v in model.variables}
    restored = mu.load_weights_verbosely(path, model)
    out = capsys.readouterr().out
    head = {v.name for v in model._task_variables()}
    assert head and not (set(restored) & head)
    assert sorted(restored) == sorted(v.name for v in model.variables if v.name not in head)
    for v, r in zip(model.variables, reg.variables):
        if v.name in head:
            assert torch.equal(v.value, before[v.name])
            assert f"Weights for {v.name} freshly initialised" in out
            assert f"Model does not use saved weights for {r.name}" in out
        else:
            assert v.name == r.name and torch.equal(v.value, r.value)

    def rename(saved_name):
        return mu.backward_compat_weight_renaming_fn(saved_name).replace("GraphRegressionTask/", "GraphBinaryClassificationTask/")

    restored = mu.load_weights_verbosely(path, model, weight_name_to_var_name=rename)
    assert sorted(restored) == sorted(v.name for v in model.variables)
    assert all(torch.equal(v.value, r.value) for v, r in zip(model.variables, reg.variables))
