"""PPIDataset, QM9Dataset, node columns and the task registry - the part that needs no GPU.

The yardstick is tests/golden/reference_ppi_qm9_batches.json: the reference's own PPIDataset and QM9Dataset run on two small
synthetic directories (make_reference_ppi_qm9_batches.py).  The raw inputs in the fixture are written back to files, loaded
here, and every graph of the packed fold has to equal the reference's processed sample: adjacency lists, in-degree tables,
features and labels.  Everything is a copy or integer arithmetic: all comparisons are exact."""
import ctypes
import gzip
import json
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def fixture():
    return json.loads((ROOT / "tests" / "golden" / "reference_ppi_qm9_batches.json").read_text())


def write_ppi_dir(path, raw, names=("valid",)):
    path.mkdir(exist_ok=True)
    for name in names:
        (path / f"{name}_graph.json").write_text(json.dumps({"directed": False, "links": raw["links"], "nodes": "never read"}))
        np.save(path / f"{name}_feats.npy", np.array(raw["feats"], dtype=np.float64))
        np.save(path / f"{name}_labels.npy", np.array(raw["labels"], dtype=np.int64))
        np.save(path / f"{name}_graph_id.npy", np.array(raw["graph_id"], dtype=np.int64))
    return path


def write_qm9_dir(path, lines, names=("valid",)):
    path.mkdir(exist_ok=True)
    for name in names:
        with gzip.open(path / f"{name}.jsonl.gz", "wt", encoding="utf-8") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return path


def _dataset(cls, cfg):
    params = cls.get_default_hyperparameters()
    params.update(cfg["params"])
    return cls(params)


# ---- hyper-parameters and shapes ---------------------------------------------------------------------------------------------
def test_hyperparameters_and_edge_type_counts_equal_the_reference(fixture):
    from tf2_gnn_amd.data import PPIDataset, QM9Dataset

    assert PPIDataset.get_default_hyperparameters() == fixture["ppi"]["default_hyperparameters"]
    assert QM9Dataset.get_default_hyperparameters() == fixture["qm9"]["default_hyperparameters"]
    assert PPIDataset.get_default_hyperparameters() == {"max_nodes_per_batch": 10000, "add_self_loop_edges": True,
                                                        "tie_fwd_bkwd_edges": False}
    assert QM9Dataset.get_default_hyperparameters()["task_id"] == 0 and QM9Dataset.get_default_hyperparameters()["tie_fwd_bkwd_edges"]
    assert PPIDataset.default_data_path() == "data/ppi"
    for key, cls in (("ppi", PPIDataset), ("qm9", QM9Dataset)):
        assert len(fixture[key]["configs"]) == 2
        for cfg in fixture[key]["configs"]:
            ds = _dataset(cls, cfg)
            assert ds.num_edge_types == cfg["num_edge_types"], (key, cfg["params"])
            if key == "ppi":
                assert ds.num_node_target_labels == cfg["num_node_target_labels"] == 121
    assert [c["num_edge_types"] for c in fixture["ppi"]["configs"]] == [3, 1]
    assert [c["num_edge_types"] for c in fixture["qm9"]["configs"]] == [5, 8]


def _assert_sample_equals(sample, ref, what):
    assert len(sample.adjacency_lists) == len(ref["adjacency_lists"]), what
    for t, (got, exp) in enumerate(zip(sample.adjacency_lists, ref["adjacency_lists"])):
        assert got.dtype == np.int32 and np.array_equal(got, np.array(exp, dtype=np.int32).reshape(-1, 2)), (what, t)
    assert np.array_equal(np.asarray(sample.type_to_node_to_num_inedges), np.array(ref["type_to_node_to_num_inedges"])), what
    feats = np.asarray(sample.node_features)
    assert feats.dtype == np.float32 and np.array_equal(feats, np.array(ref["node_features"], dtype=np.float32)), what


@pytest.mark.parametrize("cfg_idx", [0, 1])
def test_ppi_fold_equals_the_reference_samples(fixture, tmp_path, cfg_idx):
    from tf2_gnn_amd.data import DataFold, PPIDataset, PPIGraphSample

    cfg = fixture["ppi"]["configs"][cfg_idx]
    ds = _dataset(PPIDataset, cfg)
    ds.load_data(str(write_ppi_dir(tmp_path / "ppi", fixture["ppi"]["raw"])), folds_to_load={DataFold.VALIDATION})  # a str path
    fold = ds.packed_fold(DataFold.VALIDATION)
    assert fold.num_graphs == len(cfg["samples"]) == 5 and 1 in fold.node_counts.tolist()
    assert ds.node_feature_shape == tuple(cfg["node_feature_shape"]) == (10,)
    assert list(fold.node_columns) == ["node_labels"] and fold.columns == {}
    labels = fold.node_columns["node_labels"]
    assert labels.dtype == np.float32 and labels.shape == (40, 121)
    for i, ref in enumerate(cfg["samples"]):
        _assert_sample_equals(fold.sample(i), ref, ("ppi", cfg_idx, i))
        assert np.array_equal(labels[fold.node_ptr[i]:fold.node_ptr[i + 1]], np.array(ref["node_labels"], dtype=np.float32)), i
    # the host route hands out the reference's sample class, in file order
    samples = list(ds._graph_iterator(DataFold.VALIDATION))
    assert len(samples) == 5 and all(isinstance(s, PPIGraphSample) for s in samples)
    for i, (s, ref) in enumerate(zip(samples, cfg["samples"])):
        _assert_sample_equals(s, ref, ("ppi iterator", cfg_idx, i))
        assert np.array_equal(s.node_labels, np.array(ref["node_labels"], dtype=np.float32))
    s = PPIGraphSample(adjacency_lists=[], type_to_node_to_num_inedges=None, node_features=None, node_labels="labels")
    assert s.node_labels == "labels"


@pytest.mark.parametrize("cfg_idx", [0, 1])
def test_qm9_fold_equals_the_reference_samples(fixture, tmp_path, cfg_idx):
    from tf2_gnn_amd.data import DataFold, QM9Dataset, QM9GraphSample

    cfg = fixture["qm9"]["configs"][cfg_idx]
    ds = _dataset(QM9Dataset, cfg)
    ds.load_data(write_qm9_dir(tmp_path / "qm9", fixture["qm9"]["raw"]), folds_to_load={DataFold.VALIDATION})  # a Path
    fold = ds.packed_fold(DataFold.VALIDATION)
    assert fold.num_graphs == len(cfg["samples"]) == 8
    assert ds.node_feature_shape == tuple(cfg["node_feature_shape"]) == (6,)
    assert list(fold.columns) == ["target_value"] and fold.node_columns == {}
    for i, ref in enumerate(cfg["samples"]):
        _assert_sample_equals(fold.sample(i), ref, ("qm9", cfg_idx, i))
    assert np.array_equal(fold.columns["target_value"], np.array([s["target_value"] for s in cfg["samples"]], dtype=np.float32))
    if cfg_idx == 1:  # task_id 1 reads the other target
        assert cfg["params"]["task_id"] == 1
        assert fold.columns["target_value"].tolist() == [line["targets"][1][0] for line in fixture["qm9"]["raw"]]
    samples = list(ds._graph_iterator(DataFold.VALIDATION))
    assert all(isinstance(s, QM9GraphSample) for s in samples)
    assert [s.target_value for s in samples] == [s["target_value"] for s in cfg["samples"]]
    for i, (s, ref) in enumerate(zip(samples, cfg["samples"])):
        _assert_sample_equals(s, ref, ("qm9 iterator", cfg_idx, i))


# ---- inputs the reference would mangle -------------------------------------------------------------------------------------
def test_bad_ppi_inputs_raise_value_errors_that_name_the_offender(fixture, tmp_path):
    from tf2_gnn_amd.data import DataFold, PPIDataset

    raw = fixture["ppi"]["raw"]
    ds = PPIDataset(PPIDataset.get_default_hyperparameters())

    def load(**over):
        ds.load_data(write_ppi_dir(tmp_path / "bad", dict(raw, **over)), folds_to_load={DataFold.VALIDATION})

    ids = list(raw["graph_id"])
    ids[-1] = ids[0]  # graph 7 comes back behind the others
    with pytest.raises(ValueError, match="graph 7 are not contiguous"):
        load(graph_id=ids)
    crossing = raw["links"] + [{"source": 0, "target": 39}]
    with pytest.raises(ValueError, match=r"edge %d \(0 -> 39\) joins graph 7 and graph 5" % len(raw["links"])):
        load(links=crossing)
    with pytest.raises(ValueError, match="width 120"):
        load(labels=[row[:120] for row in raw["labels"]])
    with pytest.raises(ValueError, match="outside the 40 nodes"):
        load(links=raw["links"] + [{"source": 3, "target": 40}])
    with pytest.raises(ValueError, match="same nodes"):
        load(feats=raw["feats"][:-1])
    load()  # and the untouched input still loads
    assert ds.packed_fold(DataFold.VALIDATION).num_graphs == 5


@pytest.mark.parametrize("bad_type", [0, 5])
def test_qm9_edge_types_outside_1_to_4_raise(fixture, tmp_path, bad_type):
    from tf2_gnn_amd.data import DataFold, QM9Dataset

    lines = json.loads(json.dumps(fixture["qm9"]["raw"]))
    lines[2]["graph"].append([0, bad_type, 1])
    ds = QM9Dataset(QM9Dataset.get_default_hyperparameters())
    with pytest.raises(ValueError, match=f"graph 2: .* type {bad_type}"):
        ds.load_data(write_qm9_dir(tmp_path / "qm9", lines), folds_to_load={DataFold.VALIDATION})


def test_load_data_from_list_is_not_implemented_and_qm9_has_no_default_directory(fixture):
    from tf2_gnn_amd.data import PPIDataset, QM9Dataset

    for cls in (PPIDataset, QM9Dataset):
        with pytest.raises(NotImplementedError):
            cls(cls.get_default_hyperparameters()).load_data_from_list([])
    with pytest.raises(ValueError, match="no data ships"):
        QM9Dataset(QM9Dataset.get_default_hyperparameters()).load_data(None)


# ---- node columns in the packed fold ---------------------------------------------------------------------------------------
def _small_fold(node_counts, seed, **kw):
    from tf2_gnn_amd.data import PackedFold

    rng = np.random.default_rng(seed)
    V = int(sum(node_counts))
    edges = np.zeros((0, 2), dtype=np.int32)
    return PackedFold(node_counts, rng.standard_normal((V, 3)), [np.zeros(len(node_counts), dtype=np.int64)], [edges], **kw), rng


def test_packed_fold_keeps_and_checks_node_columns():
    from tf2_gnn_amd.data import GraphSample, PackedFold

    a, rng = _small_fold([2, 0, 3], 1, columns={"y": [1.0, 2.0, 3.0]},
                         node_columns={"labels": np.arange(10.0).reshape(5, 2), "w": np.arange(5.0)})
    assert a.node_columns["labels"].dtype == np.float32 and a.node_columns["w"].shape == (5, 1)
    b, _ = _small_fold([4], 2, columns={"y": [4.0]}, node_columns={"labels": np.ones((4, 2)), "w": np.zeros((4, 1))})
    both = PackedFold.concatenate([a, b])
    assert list(both.node_columns) == ["labels", "w"]
    assert np.array_equal(both.node_columns["labels"], np.concatenate([a.node_columns["labels"], b.node_columns["labels"]]))
    assert np.array_equal(both.node_columns["w"], np.concatenate([a.node_columns["w"], b.node_columns["w"]]))
    assert both.features.shape[0] == 9 and both.columns["y"].tolist() == [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(ValueError, match="one row per node"):
        _small_fold([2, 0, 3], 1, node_columns={"labels": np.zeros((4, 2))})
    with pytest.raises(ValueError, match="one row per node"):
        _small_fold([2, 0, 3], 1, node_columns={"labels": np.zeros((5, 2, 2))})
    with pytest.raises(ValueError, match="width"):
        _small_fold([2, 0, 3], 1, node_columns={"labels": np.zeros((5, 0))})
    with pytest.raises(ValueError, match="both a per-graph column and a node column"):
        _small_fold([2, 0, 3], 1, columns={"y": [1.0, 2.0, 3.0]}, node_columns={"y": np.zeros((5, 1))})
    c, _ = _small_fold([4], 2, columns={"y": [4.0]}, node_columns={"labels": np.ones((4, 3)), "w": np.zeros((4, 1))})
    with pytest.raises(ValueError, match="node columns"):
        PackedFold.concatenate([a, c])
    no_columns, _ = _small_fold([4], 2, columns={"y": [4.0]})
    with pytest.raises(ValueError, match="node columns"):
        PackedFold.concatenate([a, no_columns])
    # from_samples and from_raw_graphs take them for the whole fold
    samples = [GraphSample([np.zeros((0, 2), dtype=np.int32)], None, np.ones((n, 3), dtype=np.float32)) for n in (2, 3)]
    packed = PackedFold.from_samples(samples, 1, node_columns={"labels": np.arange(5.0)})
    assert packed.node_columns["labels"].reshape(-1).tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    raw = PackedFold.from_raw_graphs([np.ones((2, 3)), np.ones((3, 3))], [[[(0, 1)]], [[(1, 2)]]], 1, True, set(),
                                     node_columns={"labels": np.arange(10.0).reshape(5, 2)})
    assert raw.node_columns["labels"].shape == (5, 2) and raw.num_edge_types == 3
    with pytest.raises(ValueError, match="one row per node"):
        PackedFold.from_samples(samples, 1, node_columns={"labels": np.arange(6.0)})


def test_graph_dataset_has_a_node_column_hook_next_to_the_graph_column_hook():
    from tf2_gnn_amd.data import DataFold, JsonLGraphPropertyDataset

    class WithNodeLabels(JsonLGraphPropertyDataset):
        def _extra_node_columns(self, datapoints):
            return {"node_labels": np.concatenate([np.asarray(d["node_labels"], dtype=np.float32) for d in datapoints])}

    class Clash(WithNodeLabels):
        def _extra_node_columns(self, datapoints):
            return {"target_value": super()._extra_node_columns(datapoints)["node_labels"]}

    params = JsonLGraphPropertyDataset.get_default_hyperparameters()
    params["num_fwd_edge_types"] = 1
    points = [{"graph": {"node_features": [[1.0], [2.0]], "adjacency_lists": [[[0, 1]]]}, "Property": 1.5, "node_labels": [[1, 0], [0, 1]]},
              {"graph": {"node_features": [[3.0]], "adjacency_lists": [[]]}, "Property": 2.5, "node_labels": [[1, 1]]}]
    assert JsonLGraphPropertyDataset(params)._extra_node_columns(points) == {}
    ds = WithNodeLabels(params)
    ds.load_data_from_list(points, target_fold=DataFold.TEST)
    ds.load_data_from_list(points[:1], target_fold=DataFold.TEST)
    fold = ds.packed_fold(DataFold.TEST)
    assert fold.node_columns["node_labels"].tolist() == [[1, 0], [0, 1], [1, 1], [1, 0], [0, 1]]
    assert fold.columns["target_value"].tolist() == [1.5, 2.5, 1.5]
    with pytest.raises(ValueError, match="both a per-graph column and a node column"):
        Clash(params).load_data_from_list(points)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_header_struct_and_binding_agree_on_the_node_column_fields():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"#define TFGNN_BATCH_MAX_NODE_COLUMNS (\d+)", header)
    assert m and int(m.group(1)) == _lib.BATCH_MAX_NODE_COLUMNS == 4
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in text
    body = re.search(r"typedef struct tfgnn_batch_assemble_args \{(.*?)\} tfgnn_batch_assemble_args;", header, flags=re.S).group(1)
    declared = []
    for decl in body.split(";"):
        declared += re.findall(r"(\w+)\s*(?:,|$)", decl.strip())
    fields = [f[0] for f in _lib.BatchAssembleArgs._fields_]
    assert declared == fields
    # appended behind bad_flag, in this order: no earlier field offset moved
    assert fields[-5:] == ["bad_flag", "num_node_columns", "node_column_widths", "node_columns", "node_column_out"]
    assert _lib.BatchAssembleArgs.bad_flag.offset == 176 and _lib.BatchAssembleArgs.num_node_columns.offset == 184
    assert ctypes.sizeof(_lib.BatchAssembleArgs) == 216


def _args(L=2, C=1, NC=2, **over):
    """A well-formed argument struct whose device pointers are made-up addresses: the host-side checks never read them."""
    from tf2_gnn_amd import _lib

    a = _lib.BatchAssembleArgs()
    a.struct_size = ctypes.sizeof(_lib.BatchAssembleArgs)
    a.num_edge_types, a.num_columns, a.num_node_columns = L, C, NC
    a.num_graphs, a.store_nodes, a.feature_dim = 10, 200, 35
    a.order_len, a.p0, a.p1, a.num_nodes = 10, 2, 5, 60
    keep = {
        "edge_ptr": (ctypes.c_void_p * 4)(0x1000, 0x2000, 0x3000, 0x4000),
        "edges": (ctypes.c_void_p * 4)(0x5000, 0x6000, 0x7000, 0x8000),
        "pos_edge_ptr": (ctypes.c_void_p * 4)(0x9000, 0xA000, 0xB000, 0xC000),
        "adjacency_lists": (ctypes.c_void_p * 4)(0xD000, 0xE000, 0xF000, 0x10000),
        "columns": (ctypes.c_void_p * 2)(0x11000, 0x12000),
        "column_out": (ctypes.c_void_p * 2)(0x13000, 0x14000),
        "num_edges": (ctypes.c_int64 * 4)(7, 0, 3, 1),
        "node_column_widths": (ctypes.c_int64 * 5)(121, 1, 4, 8, 8),
        "node_columns": (ctypes.c_void_p * 5)(0x15000, 0x16000, 0x17000, 0x18000, 0x19000),
        "node_column_out": (ctypes.c_void_p * 5)(0x1A000, 0x1B000, 0x1C000, 0x1D000, 0x1E000),
    }
    for k, v in keep.items():
        setattr(a, k, ctypes.addressof(v))
    for k in ("node_ptr", "features", "order", "pos_node_ptr", "node_features", "node_to_graph_map", "bad_flag"):
        setattr(a, k, 0x20000)
    for k, v in over.items():
        if isinstance(v, ctypes.Array):
            keep[k] = v
            v = ctypes.addressof(v)
        setattr(a, k, v)
    return a, keep


@pytest.mark.parametrize("over, word", [
    (dict(num_node_columns=-1), b"negative"),
    (dict(node_column_widths=0), b"NULL pointer table"),
    (dict(node_columns=0), b"NULL pointer table"),
    (dict(node_column_out=0), b"NULL pointer table"),
    (dict(node_column_widths=(ctypes.c_int64 * 2)(121, 0)), b"node column width"),
    (dict(node_column_widths=(ctypes.c_int64 * 2)(-3, 4)), b"node column width"),
    (dict(node_column_widths=(ctypes.c_int64 * 2)(121, 2 ** 31)), b"node column width"),
    (dict(node_columns=(ctypes.c_void_p * 2)(0x15000, 0)), b"NULL pointer"),
    (dict(node_column_out=(ctypes.c_void_p * 2)(0, 0x1B000)), b"NULL pointer"),
    # the checks of the batch itself come before anything is read through the node column tables
    (dict(p0=5, p1=5, num_nodes=3, num_edges=(ctypes.c_int64 * 4)(0, 0, 0, 0)), b"empty batch"),
])
def test_node_column_rejections_need_no_device(over, word):
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    a, keep = _args(**over)
    assert lib.tfgnn_batch_assemble(ctypes.byref(a), None) == -1, over
    assert word in lib.tfgnn_last_error(), (over, lib.tfgnn_last_error())
    with pytest.raises(ValueError):
        _lib.check(lib.tfgnn_batch_assemble(ctypes.byref(a), None))


def test_too_many_node_columns_are_unsupported_and_a_zeroed_tail_is_accepted():
    from tf2_gnn_amd import _lib
    from tf2_gnn_amd.data import batch_assemble_launch_counts

    lib = _lib.load()
    a, keep = _args(NC=_lib.BATCH_MAX_NODE_COLUMNS + 1)
    assert lib.tfgnn_batch_assemble(ctypes.byref(a), None) == -4 and b"node columns" in lib.tfgnn_last_error()
    before = batch_assemble_launch_counts()
    empty = dict(p0=5, p1=5, num_nodes=0, num_edges=(ctypes.c_int64 * 4)(0, 0, 0, 0))
    a, keep = _args(NC=_lib.BATCH_MAX_NODE_COLUMNS, **empty)  # the limit itself is accepted
    assert lib.tfgnn_batch_assemble(ctypes.byref(a), None) == 0
    # a caller that knows nothing of node columns leaves the tail zeroed: accepted as before
    a, keep = _args(NC=0, node_column_widths=0, node_columns=0, node_column_out=0, **empty)
    assert lib.tfgnn_batch_assemble(ctypes.byref(a), None) == 0
    # a NULL node column is only an error when there are rows to copy
    a, keep = _args(node_columns=(ctypes.c_void_p * 2)(0, 0), **empty)
    assert lib.tfgnn_batch_assemble(ctypes.byref(a), None) == 0
    assert batch_assemble_launch_counts() == before
    # the struct without the tail is another struct_size
    a, keep = _args(NC=0, **empty)
    a.struct_size = _lib.BatchAssembleArgs.num_node_columns.offset
    assert lib.tfgnn_batch_assemble(ctypes.byref(a), None) == -1 and b"struct_size" in lib.tfgnn_last_error()


def test_fold_store_limit_on_node_columns_is_checked_before_the_device():
    from tf2_gnn_amd import _lib

    cols = {f"c{i}": np.zeros((5, 1)) for i in range(_lib.BATCH_MAX_NODE_COLUMNS + 1)}
    fold, _ = _small_fold([2, 0, 3], 1, node_columns=cols)
    with pytest.raises(ValueError, match="at most 4 node columns"):
        fold.to("cpu")


# ---- the registry ------------------------------------------------------------------------------------------------------------
def test_task_registry_resolves_the_four_default_tasks():
    from tf2_gnn_amd import data, tasks, utils
    from tf2_gnn_amd.utils import task_utils

    assert list(utils.get_known_tasks()) == ["PPI", "QM9", "GraphRegression", "GraphBinaryClassification"]
    expected = {
        "PPI": (data.PPIDataset, {}, tasks.NodeMulticlassTask),
        "QM9": (data.QM9Dataset, {}, tasks.QM9RegressionTask),
        "GraphRegression": (data.JsonLGraphPropertyDataset, {"threshold_for_classification": None}, tasks.GraphRegressionTask),
        "GraphBinaryClassification": (data.JsonLGraphPropertyDataset, {"threshold_for_classification": 23.0},
                                      tasks.GraphBinaryClassificationTask),
    }
    for name, (dataset_class, dataset_hypers, model_class) in expected.items():
        for spelled in (name, name.lower(), name.upper()):
            assert utils.task_name_to_dataset_class(spelled) == (dataset_class, dataset_hypers)
            assert utils.task_name_to_model_class(spelled) == (model_class, {})
    for fn in (utils.task_name_to_dataset_class, utils.task_name_to_model_class):
        with pytest.raises(ValueError, match="Unknown task type 'ppi2'"):
            fn("ppi2")
    # register_task / clear_known_tasks work on the same table
    saved = dict(task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO)
    try:
        utils.clear_known_tasks()
        assert list(utils.get_known_tasks()) == []
        with pytest.raises(ValueError):
            utils.task_name_to_model_class("PPI")
        utils.register_task("Mine", data.QM9Dataset, {"task_id": 3}, tasks.QM9RegressionTask, {"gnn_hidden_dim": 8})
        info = task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO["mine"]
        assert isinstance(info, utils.TaskInfo) and info.name == "Mine" and info.dataset_default_hypers == {"task_id": 3}
        assert utils.task_name_to_model_class("mine") == (tasks.QM9RegressionTask, {"gnn_hidden_dim": 8})
    finally:
        task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO.clear()
        task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO.update(saved)
    assert list(utils.get_known_tasks()) == list(expected)
