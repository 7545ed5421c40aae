"""LinkPredictionTask, LinkPredictionDataset and the tfgnn_distmult_* entry points as far as they go without a device: header,
symbols and binding, the argument checks of the three calls (all before any launch), the ops wrappers' refusals, the task's
variable and checkpoint, epoch metrics, the registry, the dataset - folds, filter lists, negatives, in-place buffer reuse,
every ValueError - and the ranking metrics.  CPU-only; the arithmetic is checked on the GPU (tests/test_gpu_distmult.py,
tests/test_gpu_link_prediction.py)."""
import ctypes
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tf2_gnn_amd import tasks
from tf2_gnn_amd.data import DataFold, LinkPredictionDataset
from tf2_gnn_amd.layers.message_passing import set_default_device
from tf2_gnn_amd.utils import eval_metrics, model_utils as mu, task_utils

ROOT = Path(__file__).resolve().parent.parent
NEW = ["tfgnn_distmult_ce_workspace_bytes", "tfgnn_distmult_ce_metrics", "tfgnn_distmult_backward_workspace_bytes",
       "tfgnn_distmult_backward", "tfgnn_distmult_rank_workspace_bytes", "tfgnn_distmult_rank", "tfgnn_link_launch_counts"]


@pytest.fixture
def cpu_params():
    set_default_device("cpu")
    yield
    set_default_device(None)


# ---- entry points -----------------------------------------------------------------------------------------------------------
def _link_counts(lib):
    buf = (ctypes.c_int64 * 4)()
    assert lib.tfgnn_link_launch_counts(buf, 4) == 0
    assert buf[3] == 0
    return list(buf)[:3]


def test_header_symbols_and_binding_agree():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tfgnn.h").read_text(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in header
    assert lib.tfgnn_distmult_ce_workspace_bytes() >= 8
    # one wave ("item") per 128 list positions, 2 N node entries and N relation positions, D floats each
    assert lib.tfgnn_distmult_backward_workspace_bytes(257, 3) == (5 + 3) * 3 * 4
    assert lib.tfgnn_distmult_backward_workspace_bytes(1, 1024) == 2 * 1024 * 4
    assert lib.tfgnn_distmult_backward_workspace_bytes(0, 8) == 0 and lib.tfgnn_distmult_backward_workspace_bytes(8, 1025) == 0
    assert lib.tfgnn_distmult_rank_workspace_bytes(17) == 68 and lib.tfgnn_distmult_rank_workspace_bytes(0) == 0
    assert _lib.LINK_CHUNK == 256
    assert lib.tfgnn_link_launch_counts(None, 1) == -1


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    before = _link_counts(lib)
    # never dereferenced: every call below is refused before a launch
    P = lambda a: ctypes.c_void_p(a)
    H, R, tr, y, w, m, ws, g, dH, dR, t0, t1, t2, t3 = (P(0x1000 * (i + 1)) for i in range(14))
    big = 1 << 20

    def ce(H=H, ldh=8, R=R, tr=tr, y=y, ldy=1, w=None, ldw=0, V=5, T=2, N=4, D=8, m=m, ws=ws, nbytes=big):
        return lib.tfgnn_distmult_ce_metrics(H, ldh, R, tr, y, ldy, w, ldw, V, T, N, D, m, None, None, None, ws, nbytes, None)

    def bwd(H=H, ldh=8, R=R, tr=tr, g=g, t0=t0, t1=t1, t2=t2, t3=t3, V=5, T=2, N=4, D=8, dH=dH, ldd=8, dR=dR, ws=ws, nbytes=big):
        return lib.tfgnn_distmult_backward(H, ldh, R, tr, g, t0, t1, t2, t3, V, T, N, D, dH, ldd, 0, dR, ws, nbytes, None)

    def rank(H=H, ldh=8, R=R, q=tr, Q=4, side=0, fo=None, fi=None, V=5, T=2, D=8, gt=dH, eq=dR, ws=ws, nbytes=big):
        return lib.tfgnn_distmult_rank(H, ldh, R, q, Q, side, fo, fi, V, T, D, gt, eq, ws, nbytes, None)

    def refused(status, text):
        assert status == -1
        assert text in lib.tfgnn_last_error(), lib.tfgnn_last_error()

    for call in (ce, bwd):
        refused(call(N=0), b"empty batch")
        refused(call(N=-2), b"empty batch")
        refused(call(N=2 ** 30 + 1), b"2^30")
    refused(rank(Q=0), b"empty batch")
    refused(rank(Q=2 ** 30 + 1), b"2^30")
    for call in (ce, bwd, rank):
        refused(call(D=0), b"width D")
        refused(call(D=1025, ldh=2048), b"width D")
        refused(call(V=0), b"V and T")
        refused(call(T=0), b"V and T")
        refused(call(V=2 ** 31), b"V and T")
        refused(call(ldh=7), b"leading dimension of H")
        refused(call(H=None), b"NULL")
        refused(call(R=None), b"NULL")
        refused(call(ws=None), b"workspace")
        refused(call(nbytes=3), b"workspace")
    refused(ce(tr=None), b"NULL")
    refused(ce(y=None), b"NULL")
    refused(ce(m=None), b"NULL")
    refused(ce(ldy=0), b"stride")
    refused(ce(w=w, ldw=0), b"stride")
    refused(ce(ws=P(0x9004)), b"workspace")
    refused(bwd(g=None), b"NULL")
    refused(bwd(dH=None, dR=None), b"NULL")
    refused(bwd(t1=None), b"tables")
    refused(bwd(t2=None), b"tables")
    refused(bwd(ldd=7), b"leading dimension of dH")
    refused(bwd(ws=P(0x9002)), b"workspace")
    refused(rank(side=2), b"side")
    refused(rank(gt=None), b"NULL")
    refused(rank(fo=t0), b"filter")
    refused(rank(fi=t0), b"filter")
    assert _link_counts(lib) == before  # nothing was launched
    with pytest.raises(ValueError, match="empty batch"):
        _lib.check(ce(N=0))


def test_ops_wrappers_refuse_cpu_tensors_and_bad_triples():
    from tf2_gnn_amd import ops

    H, R = torch.zeros(5, 4), torch.zeros(2, 4)
    tr = np.array([[0, 1, 4]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.distmult_ce_metrics(H, R, tr, torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.distmult_backward(H, R, tr, torch.zeros(1), {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.distmult_rank(H, R, tr)
    with pytest.raises(ValueError, match="corrupt"):
        ops.distmult_rank(H, R, tr, corrupt="both")
    with pytest.raises(ValueError, match="outside 5 nodes / 2 relations"):
        ops.check_triples([[0, 2, 1]], 5, 2)
    with pytest.raises(ValueError, match="outside 5 nodes / 2 relations"):
        ops.check_triples([[5, 0, 1]], 5, 2)
    assert ops.check_triples(np.array([[4, 1, 0]], dtype=np.int64), 5, 2).dtype == np.int32
    off, ids = ops.check_rank_filter([0, 2, 2, 3], [1, 4, 0], 3, 5)
    assert off.dtype == ids.dtype == np.int32 and off.tolist() == [0, 2, 2, 3]
    for bad_off, bad_ids in (([0, 2, 3], [1, 4, 0]), ([0, 2, 2, 3], [4, 1, 0]), ([0, 2, 2, 3], [1, 1, 0]),
                             ([0, 2, 2, 3], [1, 5, 0]), ([0, 3, 2, 3], [1, 4, 0]), ([1, 2, 2, 3], [1, 4, 0])):
        with pytest.raises(ValueError):
            ops.check_rank_filter(bad_off, bad_ids, 3, 5)


# ---- task -------------------------------------------------------------------------------------------------------------------
def test_construction_and_hyperparameters():
    params = tasks.LinkPredictionTask.get_default_hyperparameters("rgcn")
    assert params == tasks.GraphTaskModel.get_default_hyperparameters("rgcn")

    class NoRelations:
        num_edge_types = 7

    class Dataset(NoRelations):
        num_relations = 3

    with pytest.raises(ValueError, match="num_relations"):
        tasks.LinkPredictionTask(params, NoRelations())
    with pytest.raises(ValueError, match="num_edge_types"):
        tasks.LinkPredictionTask(params, num_relations=3)
    with pytest.raises(ValueError, match="at least one relation"):
        tasks.LinkPredictionTask(params, num_edge_types=1, num_relations=0)
    model = tasks.LinkPredictionTask(params, Dataset())
    assert model.num_relations == 3 and model._num_edge_types == 7 and model.name == "LinkPredictionTask"


def test_relation_embeddings_variable_and_checkpoint(cpu_params, tmp_path):
    p = tasks.LinkPredictionTask.get_default_hyperparameters("rgcn")
    p.update(gnn_num_layers=2, gnn_hidden_dim=12)
    model = tasks.LinkPredictionTask(p, num_edge_types=3, num_relations=5)
    model.build({"node_features": (None, 6)})
    names = [v.name for v in model.variables]
    assert len(set(names)) == len(names) and names[-1] == "LinkPredictionTask/relation_embeddings"
    (rel,) = model._task_variables()
    assert tuple(rel.value.shape) == (5, 12) and rel in model.trainable_variables
    limit = math.sqrt(6.0 / (5 + 12))  # glorot-uniform
    assert float(rel.value.abs().max()) <= limit and float(rel.value.std()) > 0.2 * limit
    want = {v.name: v.value.clone() for v in model.variables}
    path = str(tmp_path / "link_best.pkl")
    mu.save_model(path, model)
    assert mu.load_pickle(path)["model_class"] is tasks.LinkPredictionTask
    for v in model.variables:
        v.assign(torch.zeros_like(v.value))
    assert sorted(mu.load_weights_verbosely(path, model)) == sorted(names)
    assert all(torch.equal(v.value, want[v.name]) for v in model.variables)


def test_compute_epoch_metrics():
    model = tasks.LinkPredictionTask(tasks.LinkPredictionTask.get_default_hyperparameters("rgcn"), num_edge_types=1, num_relations=1)
    results = [{"loss": torch.tensor(0.7), "counts": torch.tensor([3, 1, 2, 0])}, {"loss": torch.tensor(0.1), "counts": torch.tensor([0, 4, 1, 5])}]
    value, text = model.compute_epoch_metrics(results)
    assert value == -(6.0 / 16.0) and text == "Accuracy = 0.375"
    assert math.isnan(model.compute_epoch_metrics([{"counts": torch.zeros(4, dtype=torch.int64)}])[0])


def test_register_link_prediction_task_adds_one_name():
    saved = dict(task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO)
    try:
        before = sorted(task_utils.get_known_tasks())
        assert "LinkPrediction" not in before
        task_utils.register_link_prediction_task()
        assert sorted(task_utils.get_known_tasks()) == sorted(before + ["LinkPrediction"])
        assert task_utils.task_name_to_dataset_class("linkprediction") == (LinkPredictionDataset, {})
        assert task_utils.task_name_to_model_class("LinkPrediction") == (tasks.LinkPredictionTask, {})
    finally:
        task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO.clear()
        task_utils.TASK_NAME_TO_DATASET_AND_MODEL_INFO.update(saved)
    assert sorted(task_utils.get_known_tasks()) == before


# ---- dataset ----------------------------------------------------------------------------------------------------------------
V_TINY = 9


def _tiny():
    """9 nodes, 2 relations.  (0, r0, 1) is a training edge, (0, r0, 2) a validation edge, (0, r0, 3) a test edge, so the
    target filter of each of them is {1, 2, 3}"""
    feats = np.arange(V_TINY * 3, dtype=np.float32).reshape(V_TINY, 3)
    edges = [np.array([[0, 1], [4, 5], [5, 6], [6, 4], [2, 2]]), np.array([[7, 8], [8, 7], [1, 0]])]
    valid = [np.array([[0, 2], [4, 6]]), np.zeros((0, 2), dtype=np.int64)]
    test = [np.array([[0, 3]]), np.array([[7, 7]])]
    return feats, edges, valid, test


def _dataset(**over):
    params = LinkPredictionDataset.get_default_hyperparameters()
    params.update(over)
    return LinkPredictionDataset(params)


def _loaded(**over):
    ds = _dataset(**over)
    feats, edges, valid, test = _tiny()
    ds.load_data_from_arrays(feats, edges, valid_edges=valid, test_edges=test)
    return ds


def test_folds_and_filter_lists(tmp_path):
    feats, edges, valid, test = _tiny()
    ds = _loaded()
    assert ds.num_relations == 2 and ds.num_edge_types == 5 and ds.node_feature_shape == (3,) and ds.num_nodes == V_TINY
    assert ds.params["num_negatives_per_positive"] == 1
    assert ds.positive_triples(DataFold.TRAIN).tolist() == [[0, 0, 1], [4, 0, 5], [5, 0, 6], [6, 0, 4], [2, 0, 2], [7, 1, 8], [8, 1, 7], [1, 1, 0]]
    assert ds.positive_triples(DataFold.VALIDATION).tolist() == [[0, 0, 2], [4, 0, 6]]
    assert ds.positive_triples(DataFold.TEST).tolist() == [[0, 0, 3], [7, 1, 7]]
    # every fold is the message-passing graph of the TRAIN edges: self loops, two forward types, their two backward types
    folds = [ds.packed_fold(f) for f in DataFold]
    assert all(f is folds[0] for f in folds) and folds[0].node_counts.tolist() == [V_TINY]
    assert np.array_equal(folds[0].edges[1], edges[0]) and np.array_equal(folds[0].edges[4], edges[1][:, ::-1])

    def lists(fold, side):
        off, ids = ds.rank_filters(fold)[side]
        assert off.dtype == ids.dtype == np.int32
        return [ids[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]

    # known = the true triples of all three folds
    assert lists(DataFold.VALIDATION, "dst") == [[1, 2, 3], [5, 6]]
    assert lists(DataFold.VALIDATION, "src") == [[0, 2], [4, 5]]
    assert lists(DataFold.TEST, "dst") == [[1, 2, 3], [7, 8]]
    assert lists(DataFold.TEST, "src") == [[0], [7, 8]]
    assert lists(DataFold.TRAIN, "dst")[0] == [1, 2, 3] and lists(DataFold.TRAIN, "src")[4] == [0, 2]

    # the same through files; with one fold left out the filter shrinks to the loaded folds
    np.save(tmp_path / "node_features.npy", feats)
    for t in range(2):
        np.save(tmp_path / f"edges_{t}.npy", edges[t])
        np.save(tmp_path / f"test_edges_{t}.npy", test[t])
    np.save(tmp_path / "valid_edges_0.npy", valid[0])  # no file for type 1: no validation edge of that type
    from_files = _dataset()
    from_files.load_data(tmp_path)
    for fold in DataFold:
        assert np.array_equal(from_files.positive_triples(fold), ds.positive_triples(fold))
        for side in ("dst", "src"):
            assert all(np.array_equal(a, b) for a, b in zip(from_files.rank_filters(fold)[side], ds.rank_filters(fold)[side]))
    partial = _dataset()
    partial.load_data(tmp_path, folds_to_load={DataFold.TRAIN, DataFold.TEST})
    assert sorted(partial._loaded_data, key=lambda f: f.value) == [DataFold.TRAIN, DataFold.TEST]
    off, ids = partial.rank_filters(DataFold.TEST)["dst"]
    assert ids[off[0]:off[1]].tolist() == [1, 3]
    with pytest.raises(NotImplementedError):
        ds.load_data_from_list([])


def test_single_type_files(tmp_path):
    feats, edges, valid, test = _tiny()
    np.save(tmp_path / "node_features.npy", feats)
    np.save(tmp_path / "edges.npy", edges[0])
    np.save(tmp_path / "valid_edges.npy", valid[0])
    np.save(tmp_path / "test_edges.npy", test[0])
    ds = _dataset(add_self_loop_edges=False, tie_fwd_bkwd_edges=True)
    ds.load_data(tmp_path)
    assert ds.num_relations == 1 and ds.num_edge_types == 1
    assert ds.positive_triples(DataFold.TEST).tolist() == [[0, 0, 3]]


@pytest.mark.parametrize("K", [1, 3])
def test_negatives_differ_in_exactly_one_slot(K):
    ds = _loaded(num_negatives_per_positive=K)
    np.random.seed(5)
    for fold in DataFold:
        pos = ds.positive_triples(fold)
        P = len(pos)
        coins = []
        for _ in range(40):
            triples = ds.draw_triples(fold)
            assert triples.dtype == np.int32 and triples.shape == (P * (1 + K), 3)
            assert np.array_equal(triples[:P], pos)
            neg, of = triples[P:], np.repeat(pos, K, axis=0)
            assert np.array_equal(neg[:, 1], of[:, 1])  # the relation stays
            same = neg == of
            assert np.all(same[:, 0] != same[:, 2])  # exactly one end replaced, by another node
            assert neg.min() >= 0 and neg[:, [0, 2]].max() < V_TINY
            coins.append((~same[:, 0]).sum() - (~same[:, 2]).sum())
        if fold == DataFold.TRAIN:
            assert len(set(np.asarray(coins).tolist())) > 1  # drawn anew, and both sides occur
    b = ds.triple_batch(DataFold.TRAIN, "cpu")
    P = len(ds.positive_triples(DataFold.TRAIN))
    assert b["triple_labels"].tolist() == [1.0] * P + [0.0] * (P * K) and b["triple_weights"].tolist() == [1.0] * (P * (1 + K))


def test_train_buffers_are_rewritten_in_place_and_eval_folds_are_fixed():
    from tf2_gnn_amd import ops

    ds = _loaded(num_negatives_per_positive=2)
    np.random.seed(11)
    first = ds.triple_batch(DataFold.TRAIN, "cpu")
    tensors = lambda b: [b["triples"], b["triple_labels"], b["triple_weights"]] + [b["triple_tables"][n] for n in ops.TRIPLE_TABLE_NAMES]
    ptrs = [t.data_ptr() for t in tensors(first)]
    old = first["triples"].clone()
    second = ds.triple_batch(DataFold.TRAIN, "cpu")
    assert second is first and [t.data_ptr() for t in tensors(second)] == ptrs
    assert not torch.equal(second["triples"], old) and torch.equal(second["triples"][:8], old[:8])
    want = ops.build_triple_tables(second["triples"].numpy(), V_TINY, 2)
    for name in ops.TRIPLE_TABLE_NAMES:
        assert second["triple_tables"][name].dtype == torch.int32
        assert np.array_equal(second["triple_tables"][name].numpy(), want[name]), name
    assert sorted(second) == ["positive_triples", "rank_filters", "triple_labels", "triple_tables", "triple_weights", "triples"]
    assert second["positive_triples"].tolist() == ds.positive_triples(DataFold.TRAIN).tolist()
    # np.random.seed seeds the TRAIN draw
    np.random.seed(11)
    again = _loaded(num_negatives_per_positive=2).triple_batch(DataFold.TRAIN, "cpu")["triples"]
    assert torch.equal(again, old)
    # VALIDATION: one draw from a fixed seed, whatever the global generator holds
    np.random.seed(1)
    v1 = ds.triple_batch(DataFold.VALIDATION, "cpu")["triples"].clone()
    np.random.seed(2)
    v2 = ds.triple_batch(DataFold.VALIDATION, "cpu")["triples"]
    v3 = _loaded(num_negatives_per_positive=2).triple_batch(DataFold.VALIDATION, "cpu")["triples"]
    assert torch.equal(v1, v2) and torch.equal(v1, v3)
    assert ds.triple_batch(DataFold.VALIDATION, "cpu") is not ds.triple_batch(DataFold.TEST, "cpu")


def test_dataset_errors():
    feats, edges, valid, test = _tiny()

    def load(feats=feats, edges=edges, valid=valid, test=test, **hypers):
        _dataset(**hypers).load_data_from_arrays(feats, edges, valid_edges=valid, test_edges=test)

    load()
    with pytest.raises(ValueError, match="loaded"):
        _dataset().num_relations
    with pytest.raises(ValueError, match="loaded"):
        _dataset().triple_batch(DataFold.TRAIN, "cpu")
    with pytest.raises(ValueError, match="would cut the graph of 9 nodes"):
        load(max_nodes_per_batch=8)
    load(max_nodes_per_batch=9)
    with pytest.raises(ValueError, match="num_negatives_per_positive"):
        load(num_negatives_per_positive=-1)
    with pytest.raises(ValueError, match="num_negatives_per_positive"):
        load(num_negatives_per_positive=1.5)
    with pytest.raises(ValueError, match="names a node outside the 9 nodes"):
        load(edges=[np.array([[0, 9]]), edges[1]])
    with pytest.raises(ValueError, match=r"\(valid\): edge 1 of type 0 \(-1 -> 2\) names a node outside"):
        load(valid=[np.array([[0, 2], [-1, 2]]), valid[1]])
    with pytest.raises(ValueError, match="1 edge lists for 2 forward edge types"):
        load(test=[test[0]])
    with pytest.raises(ValueError, match="must be an integer"):
        load(edges=[edges[0].astype(np.float32), edges[1]])
    with pytest.raises(ValueError, match="must be an integer"):
        load(edges=[edges[0][:, :1], edges[1]])
    with pytest.raises(ValueError, match="VALIDATION fold has no edge"):
        load(valid=[np.zeros((0, 2), dtype=np.int64)] * 2)
    with pytest.raises(ValueError, match="node features"):
        load(feats=feats.reshape(-1))
    with pytest.raises(ValueError, match="no edge type"):
        load(edges=[])
    with pytest.raises(ValueError, match="at least two nodes"):
        _dataset().load_data_from_arrays(feats[:1], [np.array([[0, 0]])])


def test_load_data_errors(tmp_path):
    feats, edges, valid, test = _tiny()
    np.save(tmp_path / "node_features.npy", feats)
    with pytest.raises(ValueError, match="neither edges.npy nor edges_0.npy"):
        _dataset().load_data(tmp_path)
    np.save(tmp_path / "edges_0.npy", edges[0])
    with pytest.raises(ValueError, match="no valid_edges file"):
        _dataset().load_data(tmp_path)
    ds = _dataset()
    ds.load_data(tmp_path, folds_to_load={DataFold.TRAIN})
    assert list(ds._loaded_data) == [DataFold.TRAIN]


# ---- metrics ----------------------------------------------------------------------------------------------------------------
def test_ranking_metrics_by_hand():
    # ranks 1, 2, 3.5 (two ties: 1 + 2 + 3 / 2), 11, 1.5 (one tie)
    m = eval_metrics.ranking_metrics([0, 1, 1, 10, 0], [0, 0, 3, 0, 1])
    assert list(m) == ["mrr", "hits@1", "hits@3", "hits@10"]
    assert m["mrr"] == pytest.approx((1 + 1 / 2 + 1 / 3.5 + 1 / 11 + 1 / 1.5) / 5, rel=1e-15)
    assert m["hits@1"] == 1 / 5 and m["hits@3"] == 3 / 5 and m["hits@10"] == 4 / 5
    # everything tied among 9 other candidates: rank 5.5, not 1
    assert eval_metrics.ranking_metrics([0], [9]) == {"mrr": 1 / 5.5, "hits@1": 0.0, "hits@3": 0.0, "hits@10": 1.0}
    assert eval_metrics.ranking_metrics(np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32))["mrr"] == 1.0
    assert all(math.isnan(v) for v in eval_metrics.ranking_metrics([], []).values())
    with pytest.raises(ValueError, match="differ in length"):
        eval_metrics.ranking_metrics([0, 1], [0])
    with pytest.raises(ValueError, match="negative"):
        eval_metrics.ranking_metrics([0, -1], [0, 0])
