"""Generate tests/golden/reference_ppi_qm9_batches.json by EXECUTING the reference's own PPIDataset and QM9Dataset
(tf2_gnn/data/ppi_dataset.py, tf2_gnn/data/qm9_dataset.py) on two small synthetic data directories.

Run where the reference checkout is available:  python tests/golden/make_reference_ppi_qm9_batches.py

As in make_reference_molecule_batch.py, TensorFlow and dpu_utils are replaced by inert stand-ins in sys.modules - the
loading and batching code is pure python + numpy - and the reference classes run unmodified.  Where the reference expects
a dpu_utils RichPath, it gets ``_Path``: join() and read_by_file_suffix() for .json, .npy and .jsonl.gz, nothing else.

The directories are synthesised from a fixed seed:
  * PPI: 5 graphs of 9, 1, 12, 7 and 11 nodes (40 in all), 10 features and 121 labels per node; the graph ids are
    7, 3, 20, 11, 5 and the links are shuffled, so they are not grouped by graph;
  * QM9: 8 molecules, bond types 1..4 all present, one molecule without bonds, 2 targets per molecule.
Feature values are multiples of 1/8, exactly representable in fp32.  Both are loaded as the VALIDATION fold, in file order,
in two configurations each: the defaults, and flipped tie_fwd_bkwd_edges / add_self_loop_edges with a max_nodes_per_batch
small enough for several batches (QM9: also task_id 1).  The fixture holds the raw inputs, the reference's default
hyper-parameters, num_edge_types, the per-graph processed samples and the batches."""
import gzip
import json
import sys
import tempfile
import types
from pathlib import Path
from unittest import mock

import numpy as np

REF = Path("/root/reference")
OUT = Path(__file__).resolve().parent / "reference_ppi_qm9_batches.json"
SEED = 20240521


class _Path:
    """What the reference uses of dpu_utils' RichPath"""

    def __init__(self, path):
        self._path = Path(path)

    def join(self, name):
        return _Path(self._path / name)

    def read_by_file_suffix(self):
        name = self._path.name
        if name.endswith(".jsonl.gz"):
            with gzip.open(self._path, "rt", encoding="utf-8") as f:
                return [json.loads(line) for line in f if line.strip()]
        if name.endswith(".json"):
            return json.loads(self._path.read_text())
        if name.endswith(".npy"):
            return np.load(self._path)
        raise ValueError(f"unsupported file suffix: {name}")

    def __str__(self):
        return str(self._path)


def _install_stand_ins():
    for name in ("tensorflow", "dpu_utils", "dpu_utils.utils", "dpu_utils.tf2utils", "docopt", "h5py"):
        m = mock.MagicMock(name=name)
        m.__path__ = []  # behaves as a package for "from x.y import z"
        sys.modules[name] = m
    sys.path.insert(0, str(REF))
    # import the data sub-package only (tf2_gnn/__init__ pulls in the Keras layers)
    pkg = types.ModuleType("tf2_gnn")
    pkg.__path__ = [str(REF / "tf2_gnn")]
    sys.modules["tf2_gnn"] = pkg
    data_pkg = types.ModuleType("tf2_gnn.data")
    data_pkg.__path__ = [str(REF / "tf2_gnn" / "data")]
    sys.modules["tf2_gnn.data"] = data_pkg


def _eighths(rng, shape, lo=-16, hi=17):
    return rng.integers(lo, hi, size=shape) / 8.0


def synthesise_ppi(rng):
    node_counts, graph_ids = [9, 1, 12, 7, 11], [7, 3, 20, 11, 5]
    V = sum(node_counts)
    node_to_graph_id = np.repeat(graph_ids, node_counts).astype(np.int64)
    starts = np.concatenate([[0], np.cumsum(node_counts)[:-1]])
    links = []
    for start, n in zip(starts, node_counts):
        if n > 1:
            for _ in range(2 * n):
                s, t = rng.integers(0, n, size=2)
                links.append({"source": int(start + s), "target": int(start + t)})
    links = [links[i] for i in rng.permutation(len(links))]
    return {
        "links": links,
        "feats": _eighths(rng, (V, 10)).tolist(),
        "labels": rng.integers(0, 2, size=(V, 121)).tolist(),
        "graph_id": node_to_graph_id.tolist(),
    }


def write_ppi_dir(path, raw, name="valid"):
    (path / f"{name}_graph.json").write_text(json.dumps({"directed": False, "multigraph": False, "links": raw["links"]}))
    np.save(path / f"{name}_feats.npy", np.array(raw["feats"], dtype=np.float64))
    np.save(path / f"{name}_labels.npy", np.array(raw["labels"], dtype=np.int64))
    np.save(path / f"{name}_graph_id.npy", np.array(raw["graph_id"], dtype=np.int64))


def synthesise_qm9(rng):
    lines = []
    for m, n in enumerate([5, 3, 7, 4, 6, 2, 5, 4]):
        graph = []
        if m != 3:  # molecule 3 has no bonds
            for k in range(n + 1):
                s, t = rng.integers(0, n, size=2)
                graph.append([int(s), 1 + (m + k) % 4, int(t)])
        feats = np.zeros((n, 6))
        feats[np.arange(n), rng.integers(0, 4, size=n)] = 1.0
        feats[:, 4:] = _eighths(rng, (n, 2))
        lines.append({"targets": [[float(v)] for v in _eighths(rng, 2, -40, 41)], "graph": graph, "node_features": feats.tolist()})
    assert {e[1] for line in lines for e in line["graph"]} == {1, 2, 3, 4}
    return lines


def write_qm9_dir(path, lines, name="valid"):
    with gzip.open(path / f"{name}.jsonl.gz", "wt", encoding="utf-8") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


def _run(cls, fold, path, over, label_of_sample, labels_of_batch):
    params = cls.get_default_hyperparameters()
    params.update(over)
    ds = cls(params)
    ds.load_data(_Path(path), folds_to_load={fold})
    samples = ds._loaded_data[fold]
    batches = []
    for feats, labels in ds.graph_batch_iterator_from_graph_iterator(iter(samples)):
        batch = {
            "node_features": np.asarray(feats["node_features"]).tolist(),
            "node_to_graph_map": feats["node_to_graph_map"].tolist(),
            "num_graphs_in_batch": int(feats["num_graphs_in_batch"]),
            "adjacency_lists": [np.asarray(feats[f"adjacency_list_{i}"]).astype(np.int64).reshape(-1, 2).tolist()
                                for i in range(ds.num_edge_types)],
        }
        batch.update(labels_of_batch(labels))
        batches.append(batch)
    out_samples = []
    for s in samples:
        sample = {"adjacency_lists": [np.asarray(a).astype(np.int64).reshape(-1, 2).tolist() for a in s.adjacency_lists],
                  "type_to_node_to_num_inedges": np.asarray(s.type_to_node_to_num_inedges).astype(np.int64).tolist(),
                  "node_features": np.asarray(s.node_features).tolist()}
        sample.update(label_of_sample(s))
        out_samples.append(sample)
    return {"params": dict(over), "num_edge_types": ds.num_edge_types, "samples": out_samples, "batches": batches}, ds


def main():
    _install_stand_ins()
    from tf2_gnn.data.graph_dataset import DataFold  # noqa: E402
    from tf2_gnn.data.ppi_dataset import PPIDataset  # noqa: E402
    from tf2_gnn.data.qm9_dataset import QM9Dataset  # noqa: E402

    rng = np.random.default_rng(SEED)
    ppi_raw, qm9_lines = synthesise_ppi(rng), synthesise_qm9(rng)
    out = {"source": "synthetic PPI and QM9 directories (seed %d) run through the reference's PPIDataset and QM9Dataset "
                     "(TensorFlow / dpu_utils replaced by inert stand-ins)" % SEED}
    with tempfile.TemporaryDirectory() as tmp:
        ppi_dir, qm9_dir = Path(tmp) / "ppi", Path(tmp) / "qm9"
        ppi_dir.mkdir()
        qm9_dir.mkdir()
        write_ppi_dir(ppi_dir, ppi_raw)
        write_qm9_dir(qm9_dir, qm9_lines)

        configs = []
        for over in ({}, {"tie_fwd_bkwd_edges": True, "add_self_loop_edges": False, "max_nodes_per_batch": 14}):
            cfg, ds = _run(PPIDataset, DataFold.VALIDATION, ppi_dir, over,
                           lambda s: {"node_labels": np.asarray(s.node_labels).astype(np.int64).tolist()},
                           lambda labels: {"node_labels": np.asarray(labels["node_labels"]).astype(np.int64).tolist()})
            cfg["num_node_target_labels"] = ds.num_node_target_labels
            cfg["node_feature_shape"] = list(ds.node_feature_shape)
            configs.append(cfg)
        out["ppi"] = {"raw": ppi_raw, "default_hyperparameters": PPIDataset.get_default_hyperparameters(), "configs": configs}

        configs = []
        for over in ({}, {"tie_fwd_bkwd_edges": False, "add_self_loop_edges": False, "max_nodes_per_batch": 12, "task_id": 1}):
            cfg, ds = _run(QM9Dataset, DataFold.VALIDATION, qm9_dir, over,
                           lambda s: {"target_value": float(s.target_value)},
                           lambda labels: {"target_value": [float(v) for v in labels["target_value"]]})
            cfg["node_feature_shape"] = list(ds.node_feature_shape)
            configs.append(cfg)
        out["qm9"] = {"raw": qm9_lines, "default_hyperparameters": QM9Dataset.get_default_hyperparameters(), "configs": configs}

    OUT.write_text(json.dumps(out, separators=(",", ":")))
    print("wrote", OUT, OUT.stat().st_size, "bytes;",
          {k: [(c["num_edge_types"], len(c["batches"])) for c in out[k]["configs"]] for k in ("ppi", "qm9")})


if __name__ == "__main__":
    main()
