"""Learned node embeddings and featureless datasets as far as they go without a device: the new symbols, the host-side
checks of tfgnn_embedding_scatter_rows through the loaded library (refused before any HIP call), featureless loading of the
two transductive datasets, the validation of ``node_embedding_dim``, and the edge-type limit that batch assembly lost and the
sampler kept.  On the device: tests/test_gpu_embedding_scatter.py, test_gpu_many_edge_types.py, test_gpu_node_embeddings.py."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = ("tfgnn_embedding_scatter_rows", "tfgnn_embedding_launch_count")


# ---- the C entry ----------------------------------------------------------------------------------------------------------------
def test_symbols_and_abi():
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in text
    assert "#define TFGNN_BATCH_MAX_EDGE_TYPES 48" in text and _lib.BATCH_MAX_EDGE_TYPES == 48  # the macro stays
    assert list(inspect.signature(ops.embedding_scatter_rows).parameters) == ["rows", "ids", "num_rows", "out", "bad_flag"]
    assert isinstance(ops.embedding_launch_count(), int)


def test_scatter_rejections_before_any_hip_call():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    ROWS, IDS, GRAD, FLAG = 0x10000, 0x20000, 0x30000, 0x40000  # made-up device addresses: the checks never read them
    good = dict(rows=ROWS, ld_rows=8, ids=IDS, n=5, D=8, grad=GRAD, ld_grad=8, N=10, flag=FLAG)

    def call(**over):
        a = dict(good, **over)
        return lib.tfgnn_embedding_scatter_rows(a["rows"], a["ld_rows"], a["ids"], a["n"], a["D"], a["grad"], a["ld_grad"], a["N"],
                                                a["flag"], None)

    before = lib.tfgnn_embedding_launch_count()

    def refused(match, **over):
        assert call(**over) == -1, over
        assert match in lib.tfgnn_last_error(), (over, lib.tfgnn_last_error())

    refused(b"negative size", n=-1)
    refused(b"negative size", N=-1, n=0)
    refused(b"negative size", ld_rows=-8)
    refused(b"negative size", ld_grad=-8)
    for D in (0, -3, 2 ** 31):
        refused(b"D must be in [1, 2^31)", D=D, ld_rows=2 ** 32, ld_grad=2 ** 32)
    refused(b"pitch below D", ld_rows=7)
    refused(b"pitch below D", ld_grad=7)
    refused(b"2^31 or more table rows", N=2 ** 31)
    refused(b"more rows than the table", n=11)
    refused(b"NULL table_grad", grad=None)
    refused(b"NULL rows or ids", rows=None)
    refused(b"NULL rows or ids", ids=None)
    # an empty table takes no pointers and launches nothing; the flag is nullable (checked on the device side only)
    assert call(N=0, n=0, rows=None, ids=None, grad=None, flag=None) == 0
    assert lib.tfgnn_embedding_launch_count() == before


# ---- featureless datasets -------------------------------------------------------------------------------------------------------
def _link_dataset(**over):
    from tf2_gnn_amd.data import LinkPredictionDataset

    params = LinkPredictionDataset.get_default_hyperparameters()
    params.update(over)
    return LinkPredictionDataset(params)


def _node_dataset(**over):
    from tf2_gnn_amd.data import NodeClassificationDataset

    params = NodeClassificationDataset.get_default_hyperparameters()
    params.update(over)
    return NodeClassificationDataset(params)


def _link_edges():
    train = [np.array([[0, 1], [2, 3], [4, 5]]), np.array([[1, 2], [6, 0]])]
    valid = [np.array([[8, 2]]), np.zeros((0, 2), dtype=np.int64)]  # node 8 appears in a validation file only
    test = [np.zeros((0, 2), dtype=np.int64), np.array([[3, 4]])]
    return train, valid, test


def test_featureless_link_prediction_from_arrays():
    from tf2_gnn_amd.data import DataFold

    train, valid, test = _link_edges()
    ds = _link_dataset()
    ds.load_data_from_arrays(None, train, valid_edges=valid, test_edges=test)
    assert ds.num_nodes == 9  # the largest id of ANY edge array, plus one
    assert ds.node_feature_shape == (0,) and ds.num_relations == 2 and ds.num_edge_types == 5
    fold = ds.packed_fold(DataFold.TRAIN)
    assert fold.features.shape == (9, 0) and fold.features.dtype == np.float32 and fold.edges[0].shape == (9, 2)  # self loops
    ds = _link_dataset()
    ds.load_data_from_arrays(None, train, valid_edges=valid, test_edges=test, num_nodes=20)  # isolated entities at the end
    assert ds.num_nodes == 20 and ds.node_feature_shape == (0,) and ds.packed_fold(DataFold.TEST).features.shape == (20, 0)
    with pytest.raises(ValueError, match="outside the 7 nodes"):
        _link_dataset().load_data_from_arrays(None, train, valid_edges=valid, num_nodes=7)
    for bad in (0, -4, 2.5, [3, 4]):
        with pytest.raises(ValueError, match="num_nodes must be one integer"):
            _link_dataset().load_data_from_arrays(None, train, num_nodes=bad)
    with pytest.raises(ValueError, match="num_nodes = 12"):
        _link_dataset().load_data_from_arrays(np.zeros((9, 4), dtype=np.float32), train, num_nodes=12)
    # with features nothing changed
    ds = _link_dataset()
    ds.load_data_from_arrays(np.ones((9, 4), dtype=np.float32), train, valid_edges=valid, test_edges=test)
    assert ds.num_nodes == 9 and ds.node_feature_shape == (4,)


def test_featureless_link_prediction_from_a_directory(tmp_path):
    from tf2_gnn_amd.data import DataFold

    train, valid, test = _link_edges()
    for t in range(2):
        np.save(tmp_path / f"edges_{t}.npy", train[t])
        np.save(tmp_path / f"valid_edges_{t}.npy", valid[t])
        np.save(tmp_path / f"test_edges_{t}.npy", test[t])
    ds = _link_dataset()
    ds.load_data(tmp_path)
    assert ds.num_nodes == 9 and ds.node_feature_shape == (0,)
    ds = _link_dataset()
    ds.load_data(tmp_path, folds_to_load={DataFold.TRAIN, DataFold.TEST})  # the validation file with node 8 is not read
    assert ds.num_nodes == 7
    np.save(tmp_path / "num_nodes.npy", np.array(31))
    ds = _link_dataset()
    ds.load_data(tmp_path)
    assert ds.num_nodes == 31 and ds.node_feature_shape == (0,)  # num_nodes.npy wins over the largest id
    assert ds.positive_triples(DataFold.VALIDATION).tolist() == [[8, 0, 2]]


def _node_arrays(V=12):
    labels = np.arange(V) % 3
    labels[5] = -1
    edges = [np.array([[0, 1], [1, 2], [7, 3]]), np.array([[4, 4], [9, 11]])]
    idx = {"train_idx": np.array([0, 1, 2, 3]), "valid_idx": np.array([4, 6]), "test_idx": np.array([7, 8])}
    return labels, edges, idx


def test_featureless_node_classification(tmp_path):
    from tf2_gnn_amd.data import DataFold

    labels, edges, idx = _node_arrays()
    ds = _node_dataset()
    ds.load_data_from_arrays(None, labels, edges, **idx)
    assert ds.num_nodes == 12 and ds.node_feature_shape == (0,) and ds.num_node_classes == 3 and ds.num_edge_types == 5
    fold = ds.packed_fold(DataFold.VALIDATION)
    assert fold.features.shape == (12, 0) and fold.node_columns["node_label_weights"].reshape(-1).tolist() == [
        0, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0]
    np.save(tmp_path / "node_labels.npy", labels)
    for t, e in enumerate(edges):
        np.save(tmp_path / f"edges_{t}.npy", e)
    for name, i in idx.items():
        np.save(tmp_path / f"{name}.npy", i)
    ds = _node_dataset(neighbor_fanouts=[2, 2])
    ds.load_data(tmp_path)
    assert ds.num_nodes == 12 and ds.node_feature_shape == (0,) and ds.sampled
    # with features: num_nodes is there as well, nothing else changed
    ds = _node_dataset()
    ds.load_data_from_arrays(np.ones((12, 6), dtype=np.float32), labels, edges, **idx)
    assert ds.num_nodes == 12 and ds.node_feature_shape == (6,)
    with pytest.raises(ValueError, match="known once data has been loaded"):
        _node_dataset().num_nodes


# ---- node_embedding_dim ---------------------------------------------------------------------------------------------------------
def _task_params(task_cls, **over):
    params = task_cls.get_default_hyperparameters("rgcn")
    params.update({"gnn_hidden_dim": 8, "gnn_num_layers": 2})
    params.update(over)
    return params


def test_node_embedding_dim_validation_and_variables():
    import torch

    from tf2_gnn_amd.layers.message_passing.message_passing import set_default_device
    from tf2_gnn_amd.tasks import GraphTaskModel, LinkPredictionTask, NodeClassificationTask

    assert "node_embedding_dim" not in GraphTaskModel.get_default_hyperparameters()
    assert "node_embedding_dim" not in LinkPredictionTask.get_default_hyperparameters("rgcn_basis")
    kw = dict(num_edge_types=3, num_relations=2)
    for bad in (0, -1, 2.5, True, "8"):
        with pytest.raises(ValueError, match="node_embedding_dim must be an integer >= 1"):
            LinkPredictionTask(_task_params(LinkPredictionTask, node_embedding_dim=bad), num_nodes=10, **kw)
    with pytest.raises(ValueError, match=r"dataset\.num_nodes.*num_nodes="):
        LinkPredictionTask(_task_params(LinkPredictionTask, node_embedding_dim=4), **kw)
    set_default_device("cpu")
    try:
        names = {}
        for dim in ("absent", None, 4, np.int64(4)):
            over = {} if dim == "absent" else {"node_embedding_dim": dim}
            model = LinkPredictionTask(_task_params(LinkPredictionTask, **over), num_nodes=10, **kw)
            model.build({"node_features": (None, 4)})
            names[f"{type(dim).__name__} {dim}" if dim is not None and dim != "absent" else str(dim)] = [
                (v.name, v.shape) for v in model.trainable_variables]
            assert [v.name for v in model.variables] == [v.name for v in model.trainable_variables]
        assert names["absent"] == names["None"] and names.pop("int64 4") == names["int 4"]
        names["4"] = names["int 4"]
        assert all("node_embeddings" not in n for n, _ in names["absent"])
        assert names["4"] == names["absent"] + [("LinkPredictionTask/node_embeddings", (10, 4))]
        model = NodeClassificationTask(_task_params(NodeClassificationTask, node_embedding_dim=6), num_edge_types=2,
                                       num_node_classes=3, num_nodes=7)
        assert model.get_initial_node_feature_shape({"node_features": (None, 0)}) == (None, 6)
        model.build({"node_features": (None, 0)})
        table = model.trainable_variables[-1]
        assert table.name == "NodeClassificationTask/node_embeddings" and table.shape == (7, 6)
        assert table.value.dtype == torch.float32 and float(table.value.abs().max()) <= (6.0 / 13.0) ** 0.5  # glorot_uniform
        assert model._gnn._initial_projection_layer.shape == (6, 8)
        batch = {"node_to_graph_map": torch.zeros(5, dtype=torch.int32)}
        with pytest.raises(ValueError, match="5 nodes without sampled_node_ids"):
            model.compute_initial_node_features(batch, training=False)
        full = model.compute_initial_node_features({"node_to_graph_map": torch.zeros(7, dtype=torch.int32)}, training=False)
        assert full.data_ptr() == table.value.data_ptr() and full.shape == (7, 6)  # the table itself
    finally:
        set_default_device(None)


def test_featureless_dataset_needs_the_hyperparameter():
    from tf2_gnn_amd.tasks import LinkPredictionTask, NodeClassificationTask

    train, valid, test = _link_edges()
    ds = _link_dataset()
    ds.load_data_from_arrays(None, train, valid_edges=valid, test_edges=test)
    with pytest.raises(ValueError, match="node_embedding_dim"):
        LinkPredictionTask(_task_params(LinkPredictionTask), ds)
    assert LinkPredictionTask(_task_params(LinkPredictionTask, node_embedding_dim=8), ds)._num_nodes == 9
    labels, edges, idx = _node_arrays()
    nds = _node_dataset()
    nds.load_data_from_arrays(None, labels, edges, **idx)
    with pytest.raises(ValueError, match="node_embedding_dim"):
        NodeClassificationTask(_task_params(NodeClassificationTask), nds)
    assert NodeClassificationTask(_task_params(NodeClassificationTask, node_embedding_dim=8), nds)._num_nodes == 12
    # a batch of width 0 handed to a model without the key, whatever dataset it was built on
    model = NodeClassificationTask(_task_params(NodeClassificationTask), num_edge_types=2, num_node_classes=3)
    with pytest.raises(ValueError, match="node_embedding_dim"):
        model.get_initial_node_feature_shape({"node_features": (5, 0)})


# ---- the edge-type limit --------------------------------------------------------------------------------------------------------
def _fold_with_types(L, graphs=1):
    from tf2_gnn_amd.data import PackedFold

    node_counts = np.full(graphs, 4, dtype=np.int64)
    edge_counts = [np.full(graphs, 1 if t % 7 == 0 else 0, dtype=np.int64) for t in range(L)]
    edges = [np.tile(np.array([[0, 1]], dtype=np.int32), (int(c.sum()), 1)) for c in edge_counts]
    return PackedFold(node_counts, np.ones((4 * graphs, 3), dtype=np.float32), edge_counts, edges,
                      columns={"target_value": np.zeros(graphs, dtype=np.float32)})


def test_plain_fold_above_48_types_plans_and_the_sampler_still_refuses():
    from tf2_gnn_amd.data import NeighborStore
    from tf2_gnn_amd.data.graph_dataset import EpochPlan, FoldStore

    fold = _fold_with_types(49, graphs=3)
    store = FoldStore(fold, "cpu")  # raised "at most 48 edge types ..." before
    plan = EpochPlan(store, [2, 0, 1], max_nodes_per_batch=8)
    assert store.num_edge_types == 49 and plan.batches == [(0, 2), (2, 3)] and plan.device_arrays.shape == (51, 4)
    assert plan.sizes(0, 2) == (8, [2 if t % 7 == 0 else 0 for t in range(49)])
    with pytest.raises(ValueError, match="at most 8 per-graph columns"):  # the column limit stays
        FoldStore(type(fold)(fold.node_counts, fold.features, fold.edge_counts, fold.edges,
                             columns={f"c{i}": np.zeros(3, dtype=np.float32) for i in range(9)}), "cpu")
    with pytest.raises(ValueError, match="^at most 48 edge types and 4 node columns$"):
        NeighborStore(_fold_with_types(49), "cpu")
    assert NeighborStore(_fold_with_types(48), "cpu").num_edge_types == 48
    featureless = _fold_with_types(2)
    featureless = type(featureless)(featureless.node_counts, np.zeros((4, 0), dtype=np.float32), featureless.edge_counts,
                                    featureless.edges)
    assert FoldStore(featureless, "cpu").featureless and FoldStore(featureless, "cpu").feature_dim == 1  # the placeholder column
    assert NeighborStore(featureless, "cpu").features.shape == (4, 1)
