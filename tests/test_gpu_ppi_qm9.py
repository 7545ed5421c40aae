"""PPIDataset, QM9Dataset and per-node label columns on the GPU (tf2_gnn_amd.data, csrc/batch.hip tfgnn_batch_assemble):
  * the VALIDATION batches of both datasets, in both fixture configurations, equal the REFERENCE's batches key by key -
    node_labels as [V, 121] and target_value included (tests/golden/reference_ppi_qm9_batches.json);
  * the node column part of the kernel on a hand-built fold against a numpy gather: widths 1, 4, 121, 128 and 8200 (one row
    longer than a tile), features of width 50 that cut other tiles than the columns do (163 rows a tile against 67 at width
    121), two node columns and a per-graph column at once, a graph without nodes in mid-batch, p0 > 0, an order with repeated
    ids, an output 4 bytes off the 16-byte grid (the scalar path at W % 4 == 0), NaN-filled outputs with guard rows behind
    each, and a graph id outside the fold, which sets the flag and leaves its rows alone;
  * one launch per batch with node columns present;
  * from the fixture directories to trained and evaluated NodeMulticlassTask / QM9RegressionTask models, whose metrics on an
    assembled batch are bit-identical to those on the same batch built on the host through the per-batch route.
    NodeMulticlassTask has no evaluate_model (the reference's has none, and test_gpu_binary_task.py pins that it raises): it is
    evaluated through run_one_epoch(training=False) and compute_epoch_metrics.
Everything compared is a copy or integer arithmetic: all comparisons are exact."""
import gzip
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GUARD_ROWS = 3


@pytest.fixture(scope="module")
def fixture():
    return json.loads((ROOT / "tests" / "golden" / "reference_ppi_qm9_batches.json").read_text())


def _write_ppi_dir(path, raw, names=("train", "valid", "test")):
    path.mkdir(exist_ok=True)
    for name in names:
        (path / f"{name}_graph.json").write_text(json.dumps({"links": raw["links"]}))
        np.save(path / f"{name}_feats.npy", np.array(raw["feats"], dtype=np.float64))
        np.save(path / f"{name}_labels.npy", np.array(raw["labels"], dtype=np.int64))
        np.save(path / f"{name}_graph_id.npy", np.array(raw["graph_id"], dtype=np.int64))
    return path


def _write_qm9_dir(path, lines, names=("train", "valid", "test")):
    path.mkdir(exist_ok=True)
    for name in names:
        with gzip.open(path / f"{name}.jsonl.gz", "wt", encoding="utf-8") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return path


def _load(key, fixture, tmp_path, cfg_idx, names=("valid",)):
    from tf2_gnn_amd.data import DataFold, PPIDataset, QM9Dataset

    cls, write = {"ppi": (PPIDataset, _write_ppi_dir), "qm9": (QM9Dataset, _write_qm9_dir)}[key]
    params = cls.get_default_hyperparameters()
    params.update(fixture[key]["configs"][cfg_idx]["params"])
    ds = cls(params)
    folds = {"train": DataFold.TRAIN, "valid": DataFold.VALIDATION, "test": DataFold.TEST}
    ds.load_data(write(tmp_path / key, fixture[key]["raw"], names), folds_to_load={folds[n] for n in names})
    return ds


# ---- the reference's batches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_idx", [0, 1])
@pytest.mark.parametrize("key", ["ppi", "qm9"])
def test_validation_batches_reproduce_the_reference(dev, fixture, tmp_path, key, cfg_idx):
    from tf2_gnn_amd import data
    from tf2_gnn_amd.data import DataFold

    cfg = fixture[key]["configs"][cfg_idx]
    L = cfg["num_edge_types"]
    ds = _load(key, fixture, tmp_path, cfg_idx)
    assert ds.num_edge_types == L
    label, label_width = {"ppi": ("node_labels", 121), "qm9": ("target_value", None)}[key]
    batches = ds.get_batches(DataFold.VALIDATION, dev)
    assert len(cfg["batches"]) == (1 if cfg_idx == 0 else 4)
    for _ in range(2):  # re-iterable: the second pass gives the same batches
        got_all = list(batches)
        assert len(got_all) == len(cfg["batches"])
        for (got, labels), exp in zip(got_all, cfg["batches"]):
            data.check_batch(got)
            assert sorted(got) == sorted(["node_features", "node_to_graph_map", "num_graphs_in_batch", "_bad_local_index"]
                                         + [f"adjacency_list_{t}" for t in range(L)])
            assert got["num_graphs_in_batch"] == exp["num_graphs_in_batch"] and isinstance(got["num_graphs_in_batch"], int)
            assert got["node_to_graph_map"].dtype == torch.int32
            assert np.array_equal(got["node_to_graph_map"].cpu().numpy(), np.array(exp["node_to_graph_map"], dtype=np.int32))
            assert got["node_features"].dtype == torch.float32
            assert np.array_equal(got["node_features"].cpu().numpy(), np.array(exp["node_features"], dtype=np.float32))
            for t in range(L):
                a = got[f"adjacency_list_{t}"]
                assert a.dtype == torch.int32 and tuple(a.shape)[1:] == (2,) and a.is_contiguous()
                assert np.array_equal(a.cpu().numpy(), np.array(exp["adjacency_lists"][t], dtype=np.int32).reshape(-1, 2))
            assert list(labels) == [label] and labels[label].dtype == torch.float32 and labels[label].is_contiguous()
            want = np.array(exp[label], dtype=np.float32)
            if label_width is not None:
                assert tuple(labels[label].shape) == (len(exp["node_to_graph_map"]), label_width)
            assert np.array_equal(labels[label].cpu().numpy(), want)


# ---- the node column tiles against a numpy gather ---------------------------------------------------------------------------
F = 50
NODE_COUNTS = [40, 0, 37, 1, 33, 12, 25]
ORDER = [5, 4, 0, 1, 2, 4, 3, 6]  # graph 4 twice, the graph without nodes (1) in the middle
P0, P1 = 1, 7  # positions 1..6: 33 + 40 + 0 + 37 + 33 + 1 = 144 nodes
_FOLDS = {}


def _hand_built_fold(widths):
    """7 graphs (148 nodes in the store), features [148, 50], one edge type, the per-graph column ``y`` and the node columns
    ``a`` and ``b`` of the given widths.  Built once per pair of widths and never modified."""
    if widths not in _FOLDS:
        from tf2_gnn_amd.data import PackedFold

        rng = np.random.default_rng(7 + sum(widths))
        V = sum(NODE_COUNTS)
        edge_counts = np.array([2 * n for n in NODE_COUNTS], dtype=np.int64)
        edges = np.concatenate([rng.integers(0, n, size=(2 * n, 2)) for n in NODE_COUNTS if n]).astype(np.int32)
        _FOLDS[widths] = PackedFold(
            NODE_COUNTS, rng.standard_normal((V, F)).astype(np.float32), [edge_counts], [edges],
            columns={"y": rng.standard_normal(len(NODE_COUNTS)).astype(np.float32)},
            node_columns={"a": rng.standard_normal((V, widths[0])).astype(np.float32),
                          "b": rng.standard_normal((V, widths[1])).astype(np.float32)})
    return _FOLDS[widths]


def _source_rows(fold, ids):
    """the store rows of the batch's nodes, and the batch's node_to_graph_map"""
    rows = [np.arange(fold.node_ptr[g], fold.node_ptr[g + 1]) for g in ids]
    return np.concatenate(rows), np.repeat(np.arange(len(ids)), [len(r) for r in rows]).astype(np.int32)


def _guarded_outputs(plan, widths, offset_floats, dev):
    """every output NaN-filled (integers: a sentinel), with GUARD_ROWS rows behind it; the node columns start
    ``offset_floats`` floats into their buffers"""
    V, (E,) = plan.sizes(P0, P1)
    bufs, out, rows = {}, {}, {}

    def floats(name, n, width, offset=0):
        bufs[name] = torch.full(((n + GUARD_ROWS) * width + offset,), float("nan"), dtype=torch.float32, device=dev)
        out[name] = bufs[name][offset:offset + n * width].view(n, width)
        rows[name] = offset + n * width

    floats("node_features", V, F)
    floats("a", V, widths[0], offset_floats)
    floats("b", V, widths[1], offset_floats)
    floats("y", P1 - P0, 1)
    out["y"] = out["y"].view(-1)
    bufs["node_to_graph_map"] = torch.full((V + GUARD_ROWS,), -7, dtype=torch.int32, device=dev)
    out["node_to_graph_map"], rows["node_to_graph_map"] = bufs["node_to_graph_map"][:V], V
    bufs["adjacency_list_0"] = torch.full((E + GUARD_ROWS, 2), -7, dtype=torch.int32, device=dev)
    out["adjacency_list_0"], rows["adjacency_list_0"] = bufs["adjacency_list_0"][:E], E
    return bufs, out, rows


def _assert_guards_untouched(bufs, rows):
    for name, buf in bufs.items():
        tail = buf.reshape(-1)[rows[name] * (2 if name == "adjacency_list_0" else 1):]
        assert tail.numel() and bool((torch.isnan(tail) if buf.dtype == torch.float32 else tail == -7).all()), name


@pytest.mark.parametrize("widths, offset_floats", [
    ((1, 121), 0),   # the narrowest column; 121: 67 rows a tile, three tiles where the features have one
    ((4, 128), 0),   # float4 copies
    ((4, 128), 1),   # the same widths with outputs 4 bytes off the 16-byte grid: the scalar path at W % 4 == 0
    ((8200, 4), 0),  # a row longer than a tile: one row per workgroup
])
def test_node_columns_equal_a_numpy_gather(dev, widths, offset_floats):
    from tf2_gnn_amd import data
    from tf2_gnn_amd.data import batch_assemble_launch_counts

    fold = _hand_built_fold(widths)
    store = fold.to(dev)
    assert store.node_column_names == ["a", "b"] and store.node_column_widths == list(widths)
    plan = data.EpochPlan(store, ORDER, 10 ** 6)
    V, (E,) = plan.sizes(P0, P1)
    assert V == 144 and 8192 // F == 163 and 8192 // 121 == 67  # one feature tile; the 121-wide column cuts three
    bufs, out, rows = _guarded_outputs(plan, widths, offset_floats, dev)
    assert out["a"].data_ptr() % 16 == 4 * offset_floats and out["a"].is_contiguous()
    before = batch_assemble_launch_counts()
    got, labels = data.assemble_batch(plan, P0, P1, out=out)
    assert batch_assemble_launch_counts() - before == 1
    data.check_batch(got)
    ids = ORDER[P0:P1]
    src, n2g = _source_rows(fold, ids)
    assert list(labels) == ["y", "a", "b"]
    for name in ("a", "b"):
        assert labels[name].data_ptr() == out[name].data_ptr()  # written in place
        result = labels[name].cpu().numpy()
        assert not np.isnan(result).any(), name  # every row was written
        assert np.array_equal(result, fold.node_columns[name][src]), name
    assert np.array_equal(got["node_features"].cpu().numpy(), fold.features[src])
    assert np.array_equal(got["node_to_graph_map"].cpu().numpy(), n2g)
    assert np.array_equal(labels["y"].cpu().numpy(), fold.columns["y"][ids])
    offsets = np.concatenate([[0], np.cumsum([NODE_COUNTS[g] for g in ids])])
    want_edges = np.concatenate([fold.edges[0][fold.edge_ptr[0][g]:fold.edge_ptr[0][g + 1]] + offsets[k] for k, g in enumerate(ids)])
    assert np.array_equal(got["adjacency_list_0"].cpu().numpy(), want_edges)
    _assert_guards_untouched(bufs, rows)
    # without ``out`` the node columns are carved from the batch's float allocation, [V, W] each
    got2, labels2 = data.assemble_batch(plan, P0, P1)
    for name, w in zip(("a", "b"), widths):
        assert tuple(labels2[name].shape) == (V, w) and labels2[name].is_contiguous() and labels2[name].data_ptr() % 256 == 0
        assert torch.equal(labels2[name], labels[name])
    assert torch.equal(got2["node_features"], got["node_features"])


def test_node_column_outputs_are_validated(dev):
    from tf2_gnn_amd import data

    widths = (4, 128)
    store = _hand_built_fold(widths).to(dev)
    plan = data.EpochPlan(store, ORDER, 10 ** 6)
    bufs, out, rows = _guarded_outputs(plan, widths, 0, dev)
    for bad in (out["b"][:-1], out["b"].to(torch.float64), out["b"].t().contiguous().t(), out["b"].reshape(-1)):
        with pytest.raises(ValueError, match="the b output must be a contiguous float32"):
            data.assemble_batch(plan, P0, P1, out=dict(out, b=bad))
    with pytest.raises(KeyError):
        data.assemble_batch(plan, P0, P1, out={k: v for k, v in out.items() if k != "a"})


def test_a_graph_id_outside_the_fold_sets_the_flag_and_skips_its_rows(dev):
    from tf2_gnn_amd import data

    widths = (1, 121)
    fold = _hand_built_fold(widths)
    store = fold.to(dev)
    plan = data.EpochPlan(store, ORDER, 10 ** 6)
    # the host plans with valid ids; the device's copy of the order then names a graph the fold does not have at position 2
    # (graph 0, 40 nodes: batch rows 33..72)
    assert ORDER[2] == 0 and NODE_COUNTS[ORDER[1]] == 33
    plan.device_arrays[0, 2] = len(NODE_COUNTS) + 2
    bufs, out, rows = _guarded_outputs(plan, widths, 0, dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    got, labels = data.assemble_batch(plan, P0, P1, out=out, bad_flag=flag)
    assert int(flag.item()) == 1
    with pytest.raises(ValueError):
        data.check_batch(got)
    src, _ = _source_rows(fold, ORDER[P0:P1])
    skipped = np.zeros(144, dtype=bool)
    skipped[33:73] = True
    for name, result, want in (("a", labels["a"], fold.node_columns["a"]), ("b", labels["b"], fold.node_columns["b"]),
                               ("node_features", got["node_features"], fold.features)):
        result = result.cpu().numpy()
        assert np.isnan(result[skipped]).all(), name  # the rows keep the sentinel
        assert np.array_equal(result[~skipped], want[src][~skipped]), name
    assert bool((got["node_to_graph_map"][33:73] == -7).all())
    _assert_guards_untouched(bufs, rows)


# ---- launches ---------------------------------------------------------------------------------------------------------------
def test_a_batch_with_node_columns_is_one_launch(dev, fixture, tmp_path):
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import DataFold, assemble_batch, batch_assemble_launch_counts

    ds = _load("ppi", fixture, tmp_path, 1)
    plan = ds.plan_epoch(DataFold.VALIDATION, dev)  # packing, the upload and the plan are per fold and per epoch
    assert len(plan.batches) == 4 and plan.store.node_column_names == ["node_labels"]
    other_before = ops.launch_counts()
    for p0, p1 in plan.batches:
        before = batch_assemble_launch_counts()
        _, labels = assemble_batch(plan, p0, p1)
        assert batch_assemble_launch_counts() - before == 1
        assert labels["node_labels"].shape[1] == 121
    assert ops.launch_counts() == other_before  # and no other library kernel


# ---- from the directories to trained models -----------------------------------------------------------------------------------
def _host_batches(ds, fold, dev, label):
    """the fold's batches built on the host from ``fold.sample(i)`` through the per-batch route, labels uploaded next to them"""
    from tf2_gnn_amd import data

    samples = [fold.sample(i) for i in range(fold.num_graphs)]
    features = list(data.graph_batch_iterator_from_graph_iterator(iter(samples), ds.num_edge_types, ds.params["max_nodes_per_batch"], dev))
    out, g = [], 0
    for f in features:
        G = f["num_graphs_in_batch"]
        if label == "node_labels":
            rows = fold.node_columns[label][fold.node_ptr[g]:fold.node_ptr[g + G]]
        else:
            rows = fold.columns[label][g:g + G]
        out.append((f, {label: torch.from_numpy(np.ascontiguousarray(rows)).to(dev)}))
        g += G
    assert g == fold.num_graphs
    return out


@pytest.mark.parametrize("key", ["ppi", "qm9"])
def test_directory_to_trained_and_evaluated_model(dev, fixture, tmp_path, key):
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.utils import task_name_to_dataset_class, task_name_to_model_class

    ds = _load(key, fixture, tmp_path, 1, names=("train", "valid", "test"))  # batches of at most 14 / 12 nodes: four per epoch
    model_class, _ = task_name_to_model_class(key)
    assert task_name_to_dataset_class(key)[0] is type(ds)
    label = {"ppi": "node_labels", "qm9": "target_value"}[key]
    params = model_class.get_default_hyperparameters("rgcn")
    params.update({"gnn_hidden_dim": 32, "gnn_num_layers": 2, "gnn_global_exchange_every_num_layers": 10000})
    model = model_class(params, dataset=ds)  # num_edge_types, num_node_target_labels / task_id come from the dataset
    np.random.seed(5)
    torch.manual_seed(5)
    for _ in range(2):
        loss, speed, results = model.run_one_epoch(ds.get_batches(DataFold.TRAIN), quiet=True)
        assert math.isfinite(loss) and speed > 0 and len(results) >= 3
    valid = ds.get_batches(DataFold.VALIDATION)
    loss, _, results = model.run_one_epoch(valid, quiet=True, training=False)
    value, text = model.compute_epoch_metrics(results)
    assert math.isfinite(loss) and math.isfinite(value) and len(results) == 4, text
    predictions = model.predict(valid)
    assert bool(torch.isfinite(predictions).all())
    if key == "ppi":
        assert tuple(predictions.shape) == (40, 121)
    else:
        assert tuple(predictions.shape) == (8,) and model._task_id == 1
        metrics = model.evaluate_model(valid)
        assert sorted(metrics) == ["expl_var", "mae", "max_err", "mse", "r2_score"]
        assert all(math.isfinite(v) for v in metrics.values()), metrics

    # an assembled batch against the same batch built on the host
    host = _host_batches(ds, ds.packed_fold(DataFold.VALIDATION), dev, label)
    assembled = list(valid)
    assert len(host) == len(assembled) == 4
    for (f_new, l_new), (f_old, l_old) in zip(assembled, host):
        assert torch.equal(f_new["node_features"], f_old["node_features"]) and torch.equal(l_new[label], l_old[label])
        m_new = model.compute_task_metrics(f_new, model(f_new, training=False), l_new)
        m_new = {k: v.clone() if isinstance(v, torch.Tensor) else v for k, v in m_new.items()}
        m_old = model.compute_task_metrics(f_old, model(f_old, training=False), l_old)
        assert list(m_new) == list(m_old)
        for k in m_new:
            if isinstance(m_new[k], torch.Tensor):
                assert torch.equal(m_new[k], m_old[k]), k  # bit for bit
            else:
                assert m_new[k] == m_old[k], k
        assert bool(torch.isfinite(m_new["loss"]).all())
