"""Device-resident graph datasets on the GPU (tf2_gnn_amd.data.graph_dataset, csrc/batch.hip tfgnn_batch_assemble):
  * a fold loaded from the golden fixture's raw graphs reproduces the REFERENCE's processed samples and batches bit for bit;
  * on a synthetic fold with empty graphs, empty edge types and several feature widths, every batch equals what the per-batch
    route (graph_batch_iterator_from_graph_iterator) gives for the same sample order, at batch limits that cut the fold
    into one, several and single-graph batches (with the reference's empty first batch).  The per-batch route cannot take a
    graph WITHOUT nodes (its ``reshape(0, -1)`` of the features raises), so it is the yardstick for the order with those
    graphs left out, and for the full order the yardstick is ``_host_batches``: the reference's _add_graph_to_batch /
    _finalise_batch restated in numpy, itself held against the per-batch route on the orders that route accepts;
  * guard rows behind every output stay untouched; orders from both ends of the store and with repeats; the bad-index flag;
  * one library launch per batch; a JSONL directory to a trained and evaluated task model.
Integer outputs and copies are compared for equality."""
import gzip
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
LAUNCHES_PER_BATCH = 1  # include/tfgnn.h: tfgnn_batch_assemble is ONE launch (none for an empty batch)
SENTINEL = -0x21524111  # int32 pattern of the guard rows (as float32: a negative number no output holds)
GUARD_ROWS = 3


@pytest.fixture(scope="module")
def fixture():
    """The golden file, its raw graphs put back into the JSONL line format they were read from"""
    f = json.loads((ROOT / "tests" / "golden" / "reference_molecule_batch.json").read_text())
    f["lines"] = [{"graph": {"node_features": g["node_features"], "adjacency_lists": g["adjacency_lists"]}, "Property": g["Property"]}
                  for g in f["graphs"]]
    return f


def _params(cfg, **over):
    from tf2_gnn_amd.data import JsonLGraphPropertyDataset

    p = JsonLGraphPropertyDataset.get_default_hyperparameters()
    p.update(cfg["params"])
    p.update(over)
    return p


def _write_dir(path, lines, names=("train", "valid", "test")):
    for name in names:
        with gzip.open(path / f"{name}.jsonl.gz", "wt", encoding="utf-8") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
    return path


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _assert_same_batch(got, exp, L, what):
    """two batch_features dictionaries (device tensors or numpy arrays), bit for bit"""
    assert got["num_graphs_in_batch"] == exp["num_graphs_in_batch"] and isinstance(got["num_graphs_in_batch"], int), what
    n2g, feats = _np(got["node_to_graph_map"]), _np(got["node_features"])
    assert n2g.dtype == np.int32 and feats.dtype == np.float32
    assert np.array_equal(n2g, _np(exp["node_to_graph_map"])), what
    assert feats.shape[0] == _np(exp["node_features"]).shape[0], what
    if feats.size or _np(exp["node_features"]).size:
        assert np.array_equal(feats, _np(exp["node_features"])), what
    for t in range(L):
        a = _np(got[f"adjacency_list_{t}"])
        assert a.dtype == np.int32 and a.ndim == 2 and a.shape[1] == 2, what
        assert np.array_equal(a, _np(exp[f"adjacency_list_{t}"])), (what, t)


# ---- the reference's batches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_idx", [0, 1])
def test_validation_batches_reproduce_the_reference(dev, fixture, tmp_path, cfg_idx):
    from tf2_gnn_amd import data
    from tf2_gnn_amd.data import DataFold, JsonLGraphPropertyDataset

    cfg = fixture["configs"][cfg_idx]
    L = cfg["num_edge_types"]
    ds = JsonLGraphPropertyDataset(_params(cfg))
    ds.load_data(_write_dir(tmp_path, fixture["lines"], names=("valid",)), folds_to_load={DataFold.VALIDATION})
    assert ds.num_edge_types == L and ds.node_feature_shape == (35,)

    store = ds.fold_store(DataFold.VALIDATION, dev)
    assert store.num_graphs == 10 and store.num_edge_types == L
    for i, (g, ref) in enumerate(zip(fixture["graphs"], cfg["samples"])):
        s = store.sample(i)
        assert np.array_equal(s.node_features, np.array(g["node_features"], dtype=np.float32))
        for got, exp in zip(s.adjacency_lists, ref["adjacency_lists"]):
            assert got.dtype == np.int32 and np.array_equal(got, np.array(exp, dtype=np.int32).reshape(-1, 2)), i
    assert np.array_equal(store.columns[0].cpu().numpy(), np.array([s["target_value"] for s in cfg["samples"]], dtype=np.float32))

    batches = ds.get_batches(DataFold.VALIDATION, dev)
    for _ in range(2):  # re-iterable: the second pass gives the same batches
        got_all = list(batches)
        assert len(got_all) == len(cfg["batches"])
        for (got, labels), exp in zip(got_all, cfg["batches"]):
            data.check_batch(got)
            assert got["num_graphs_in_batch"] == exp["num_graphs_in_batch"] and isinstance(got["num_graphs_in_batch"], int)
            assert got["node_to_graph_map"].dtype == torch.int32
            assert np.array_equal(got["node_to_graph_map"].cpu().numpy(), np.array(exp["node_to_graph_map"], dtype=np.int32))
            assert got["node_features"].dtype == torch.float32
            assert np.array_equal(got["node_features"].cpu().numpy(), np.array(exp["node_features"], dtype=np.float32))
            for t in range(L):
                a = got[f"adjacency_list_{t}"]
                assert a.dtype == torch.int32 and tuple(a.shape)[1:] == (2,) and a.is_contiguous()
                assert np.array_equal(a.cpu().numpy(), np.array(exp["adjacency_lists"][t], dtype=np.int32).reshape(-1, 2))
            assert list(labels) == ["target_value"] and labels["target_value"].dtype == torch.float32
            assert np.array_equal(labels["target_value"].cpu().numpy(), np.array(exp["target_value"], dtype=np.float32))
    assert [f["num_graphs_in_batch"] for f, _ in ds.graph_batch_iterator(DataFold.VALIDATION)] == \
        [b["num_graphs_in_batch"] for b in cfg["batches"]]


# ---- a synthetic fold against the per-batch route -----------------------------------------------------------------------------
NUM_TYPES = 4
_SAMPLES = {}


def _synthetic_samples(F):
    """64 graphs with node counts from {0, 1, 2, 17, 300} (graph 0 has 300, so that it exceeds the small limits); type 0
    has edges wherever there are nodes, type 1 is empty in about half of the graphs, type 2 in all of them, type 3 is sparse.
    Built once per feature width and never modified."""
    if F not in _SAMPLES:
        from tf2_gnn_amd.data import GraphSample

        rng = np.random.default_rng(1000 + F)
        counts = rng.choice([0, 1, 2, 17, 300], size=64)
        counts[0], counts[1], counts[63] = 300, 0, 17
        assert set(counts.tolist()) == {0, 1, 2, 17, 300}
        samples = []
        for g, n in enumerate(counts.tolist()):
            def edges(k):
                return rng.integers(0, n, size=(k, 2)).astype(np.int32) if n and k else np.zeros((0, 2), dtype=np.int32)

            adj = [edges(3 * n + 1), edges(0 if g % 2 else 2 * n), edges(0), edges(int(rng.integers(0, 3)))]
            samples.append(GraphSample(adj, None, rng.standard_normal((n, F)).astype(np.float32)))
        target = rng.standard_normal(64).astype(np.float32)
        _SAMPLES[F] = (samples, target)
    return _SAMPLES[F]


def _old_route(samples, order, limit, dev):
    from tf2_gnn_amd import data

    return list(data.graph_batch_iterator_from_graph_iterator(iter([samples[i] for i in order]), NUM_TYPES, limit, dev))


def _host_batches(samples, order, limit, F):
    """GraphDataset.graph_batch_iterator_from_graph_iterator with _add_graph_to_batch / _finalise_batch, in numpy: a graph
    that would push the node count over the limit closes the batch; node ids shift by the nodes already in the batch."""
    def finalise(graphs):
        feats, n2g, adj, nodes = [], [], [[] for _ in range(NUM_TYPES)], 0
        for k, g in enumerate(graphs):
            n = len(g.node_features)
            feats.append(np.asarray(g.node_features, dtype=np.float32).reshape(n, F))
            n2g.append(np.full(n, k, dtype=np.int32))
            for t in range(NUM_TYPES):
                adj[t].append(g.adjacency_lists[t].reshape(-1, 2) + nodes)
            nodes += n
        batch = {"node_features": np.concatenate(feats) if feats else np.zeros((0, F), dtype=np.float32),
                 "node_to_graph_map": np.concatenate(n2g) if n2g else np.zeros(0, dtype=np.int32), "num_graphs_in_batch": len(graphs)}
        for t in range(NUM_TYPES):
            batch[f"adjacency_list_{t}"] = np.concatenate(adj[t]).astype(np.int32) if adj[t] else np.zeros((0, 2), dtype=np.int32)
        return batch

    out, cur, nodes = [], [], 0
    for i in order:
        n = len(samples[i].node_features)
        if nodes + n > limit:
            out.append(finalise(cur))
            cur, nodes = [], 0
        cur.append(samples[i])
        nodes += n
    out.append(finalise(cur))
    return out


def _store(F, dev):
    from tf2_gnn_amd.data import PackedFold

    samples, target = _synthetic_samples(F)
    return PackedFold.from_samples(samples, NUM_TYPES, columns={"target_value": target, "weight": 2 * target}, feature_dim=F).to(dev)


@pytest.mark.parametrize("limit", [1, 60, 10 ** 6])
@pytest.mark.parametrize("F", [1, 4, 35, 128])
def test_batches_equal_the_per_batch_route(dev, F, limit):
    from tf2_gnn_amd import data

    samples, target = _synthetic_samples(F)
    store = _store(F, dev)
    order = np.random.default_rng(F + limit).permutation(64)
    order[order == 0], order[0] = order[0], 0  # the 300-node graph first
    # the per-batch route on the graphs it accepts, against the new route and against the numpy restatement
    with_nodes = np.array([i for i in order if len(samples[i].node_features)], dtype=np.int64)
    assert 0 < len(with_nodes) < 64
    old_all = _old_route(samples, with_nodes, limit, dev)
    plan = data.EpochPlan(store, with_nodes, limit)
    assert len(plan) == len(old_all)
    for (p0, p1), old, host in zip(plan.batches, old_all, _host_batches(samples, with_nodes, limit, F)):
        got, _ = data.assemble_batch(plan, p0, p1)
        _assert_same_batch(got, old, NUM_TYPES, ("per-batch route", F, limit, p0, p1))
        _assert_same_batch(host, old, NUM_TYPES, ("restatement", F, limit, p0, p1))
    # the full order, graphs without nodes included
    exp_all = _host_batches(samples, order, limit, F)
    plan = data.EpochPlan(store, order, limit)
    assert len(plan) == len(exp_all)
    if limit < 300:
        assert plan.batches[0] == (0, 0) and exp_all[0]["num_graphs_in_batch"] == 0  # the reference's empty first batch
    else:
        assert len(plan) == 1
    seen = 0
    for (p0, p1), exp in zip(plan.batches, exp_all):
        got, labels = data.assemble_batch(plan, p0, p1)
        data.check_batch(got)
        _assert_same_batch(got, exp, NUM_TYPES, (F, limit, p0, p1))
        assert got["adjacency_list_2"].shape == (0, 2)
        ids = order[p0:p1]
        assert list(labels) == ["target_value", "weight"]
        assert np.array_equal(labels["target_value"].cpu().numpy(), target[ids])
        assert np.array_equal(labels["weight"].cpu().numpy(), 2 * target[ids])
        seen += p1 - p0
    assert seen == 64


@pytest.mark.parametrize("F", [1, 35, 128])
def test_guard_rows_behind_every_output_stay_untouched(dev, F):
    from tf2_gnn_amd import data

    samples, target = _synthetic_samples(F)
    store = _store(F, dev)
    order = np.arange(64)
    exp_all = _host_batches(samples, order, 320, F)
    plan = data.EpochPlan(store, order, 320)
    assert len(plan) == len(exp_all) > 3

    def guarded(rows, width, dtype):
        buf = torch.full((rows + GUARD_ROWS, width), SENTINEL, dtype=torch.int32, device=dev)
        return buf, buf.view(dtype)[:rows]

    for (p0, p1), exp in zip(plan.batches, exp_all):
        V, E = plan.sizes(p0, p1)
        G = p1 - p0
        bufs, out = {}, {}
        bufs["node_features"], out["node_features"] = guarded(V, F, torch.float32)
        bufs["node_to_graph_map"], n2g = guarded(V, 1, torch.int32)
        out["node_to_graph_map"] = n2g.view(-1)
        for t in range(NUM_TYPES):
            bufs[f"adjacency_list_{t}"], out[f"adjacency_list_{t}"] = guarded(E[t], 2, torch.int32)
        for name in ("target_value", "weight"):
            bufs[name], col = guarded(G, 1, torch.float32)
            out[name] = col.view(-1)
        rows = {"node_features": V, "node_to_graph_map": V, "target_value": G, "weight": G}
        rows.update({f"adjacency_list_{t}": E[t] for t in range(NUM_TYPES)})
        got, labels = data.assemble_batch(plan, p0, p1, out=out)
        data.check_batch(got)
        _assert_same_batch(got, exp, NUM_TYPES, (F, p0, p1))
        assert np.array_equal(labels["target_value"].cpu().numpy(), target[p0:p1])
        for name, buf in bufs.items():
            if rows[name]:
                assert got.get(name, labels.get(name)).data_ptr() == buf.data_ptr(), name  # written in place
            assert bool((buf[rows[name]:] == SENTINEL).all()), (name, p0, p1)


def test_orders_from_both_ends_and_with_repeated_ids(dev):
    from tf2_gnn_amd import data

    F = 35
    samples, target = _synthetic_samples(F)
    store = _store(F, dev)
    for order in ([63, 0, 62, 1, 61, 2, 33], [63, 0, 62, 2, 0, 63, 63, 33, 5], [5, 63, 5, 5, 0, 63, 0, 7, 7], [63], [1], []):
        order = np.array(order, dtype=np.int64)
        for limit in (60, 10 ** 6):
            exp_all = _host_batches(samples, order, limit, F)
            if all(len(samples[i].node_features) for i in order):
                for old, host in zip(_old_route(samples, order, limit, dev), exp_all):
                    _assert_same_batch(host, old, NUM_TYPES, ("restatement", order.tolist(), limit))
            plan = data.EpochPlan(store, order, limit)
            assert len(plan) == len(exp_all)
            for (p0, p1), exp in zip(plan.batches, exp_all):
                got, labels = data.assemble_batch(plan, p0, p1)
                data.check_batch(got)
                _assert_same_batch(got, exp, NUM_TYPES, (order.tolist(), limit, p0, p1))
                assert np.array_equal(labels["target_value"].cpu().numpy(), target[order[p0:p1]])
    with pytest.raises(ValueError, match="outside the fold"):
        data.EpochPlan(store, [0, 64], 60)


def test_a_local_index_outside_its_graph_sets_the_flag(dev):
    from tf2_gnn_amd import data
    from tf2_gnn_amd.data import GraphSample, PackedFold

    good = GraphSample([np.array([[0, 1], [1, 2]], dtype=np.int32)], None, np.zeros((3, 4), dtype=np.float32))
    bad = GraphSample([np.array([[0, 3]], dtype=np.int32)], None, np.ones((3, 4), dtype=np.float32))  # node 3 of 3
    neg = GraphSample([np.array([[-1, 0]], dtype=np.int32)], None, np.ones((2, 4), dtype=np.float32))
    store = PackedFold.from_samples([good, bad, good, neg], 1).to(dev)
    plan = data.EpochPlan(store, [0, 1, 2, 0, 3, 0], 6)
    assert plan.batches == [(0, 2), (2, 4), (4, 6)]
    flags = []
    for b, (p0, p1) in enumerate(plan.batches):
        feats, _ = data.assemble_batch(plan, p0, p1, bad_flag=plan.bad_flags[b:b + 1])
        try:
            data.check_batch(feats)
            flags.append(False)
        except ValueError:
            flags.append(True)
    assert flags == [True, False, True]
    # the values are still the shifted ones, as tfgnn_batch_offset_edges writes them
    (exp,) = list(data.graph_batch_iterator_from_graph_iterator(iter([good, bad]), 1, 6, dev))
    got, _ = data.assemble_batch(plan, 0, 2)
    assert torch.equal(got["adjacency_list_0"], exp["adjacency_list_0"])
    with pytest.raises(ValueError):
        data.check_batch(got)


# ---- launches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_idx", [0, 1])
def test_one_library_launch_per_batch(dev, fixture, cfg_idx):
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import DataFold, JsonLGraphPropertyDataset, batch_assemble_launch_counts

    cfg = fixture["configs"][cfg_idx]
    ds = JsonLGraphPropertyDataset(_params(cfg))
    ds.load_data_from_list(fixture["lines"], target_fold=DataFold.TRAIN)
    ds.fold_store(DataFold.TRAIN, dev)  # packing and the upload are per fold, not per epoch
    other_before = ops.launch_counts()
    before = batch_assemble_launch_counts()
    num_batches = sum(1 for _ in ds.get_batches(DataFold.TRAIN, dev))
    launches = batch_assemble_launch_counts() - before
    assert num_batches >= len(cfg["batches"]) - 1
    assert 0 < launches <= LAUNCHES_PER_BATCH * num_batches
    assert ops.launch_counts() == other_before  # and no other library kernel


# ---- from a JSONL directory to a trained model ---------------------------------------------------------------------------------
def test_jsonl_directory_to_trained_and_evaluated_models(dev, fixture, tmp_path):
    from tf2_gnn_amd.data import DataFold, JsonLGraphPropertyDataset
    from tf2_gnn_amd.tasks import GraphBinaryClassificationTask, GraphRegressionTask
    from tf2_gnn_amd.utils import eval_metrics

    _write_dir(tmp_path, fixture["lines"])
    cfg = fixture["configs"][1]  # 8 edge types, batches of at most 60 nodes: four batches per epoch
    for cls, threshold, metric_fn in ((GraphRegressionTask, None, eval_metrics.regression_metrics),
                                      (GraphBinaryClassificationTask, 20.0, eval_metrics.binary_classification_metrics)):
        ds = JsonLGraphPropertyDataset(_params(cfg, threshold_for_classification=threshold))
        ds.load_data(tmp_path)
        params = cls.get_default_hyperparameters("rgcn")
        params.update({"gnn_hidden_dim": 32, "gnn_num_layers": 2, "gnn_global_exchange_every_num_layers": 10000})
        model = cls(params, dataset=ds)
        np.random.seed(3)
        torch.manual_seed(3)
        for _ in range(2):
            loss, speed, results = model.run_one_epoch(ds.get_batches(DataFold.TRAIN), quiet=True)
            assert math.isfinite(loss) and speed > 0 and len(results) >= 3
        valid = ds.get_batches(DataFold.VALIDATION)
        predictions = model.predict(valid)
        assert predictions.shape == (10,) and bool(torch.isfinite(predictions).all())
        # one row per graph, in file order: the rows are the batches' outputs end to end, and the batches' labels end to end
        # are the file's properties (the graphs themselves: test_validation_batches_reproduce_the_reference)
        assert torch.equal(predictions, torch.cat([model(f, training=False).clone() for f, _ in valid]))
        labels = torch.cat([l["target_value"] for _, l in valid])
        targets = np.array([float(line["Property"]) for line in fixture["lines"]], dtype=np.float32)
        if threshold is not None:
            targets = (targets > threshold).astype(np.float32)
            assert 0 < targets.sum() < 10
        assert np.array_equal(labels.cpu().numpy(), targets)
        metrics = model.evaluate_model(valid)
        assert list(metrics) == list(metric_fn(targets, predictions.cpu().numpy()))
        assert all(math.isfinite(v) for v in metrics.values()), metrics
