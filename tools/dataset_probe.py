"""Batch production, per-batch route against the fold store: one epoch of batches of a QM9-shaped and a PPI-shaped fold
through ``graph_batch_iterator_from_graph_iterator`` (host concatenation, L + 2 copies and L + 1 launches per batch) and through
``GraphDataset.get_batches`` (fold packed on the device once; per epoch one plan upload, per batch one tfgnn_batch_assemble).

Reported per route: host time per batch (the time the host spends inside the iterator for one batch, no synchronisation) and
wall time per epoch (first ``next()`` to the end of a final device synchronisation; the new route's epoch includes drawing the
order, planning and the upload).  Both routes shuffle per epoch.  ``--warmup`` epochs are discarded, ``--epochs`` are
measured; median, minimum and maximum over the measured epochs are printed, and the verdict line compares the medians with
the per-batch route's own epoch-to-epoch spread.  Packing and uploading the fold is timed once and reported apart.

``--node-column-width W`` gives every node of the PPI-shaped fold W float32 labels (PPI has 121): the fold store carries them as
the node column ``node_labels`` and assembles them in the same launch; the per-batch route concatenates the batch's label rows
on the host and uploads them, one more copy per batch - what the reference's _finalise_batch plus a transfer would do.

    python tools/dataset_probe.py [--epochs 9] [--warmup 3] [--node-column-width 121] [--out profiles/dataset_probe.txt]
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tf2_gnn_amd import data  # noqa: E402
from tf2_gnn_amd.data import DataFold, GraphDataset, GraphSample, PackedFold  # noqa: E402


def _split(feats, adjs, offs):
    """one disjoint-union batch -> per-graph samples with local node ids (each type's edges keep their order within a graph)"""
    offs = np.asarray(offs, dtype=np.int64)
    G = len(offs) - 1
    per_type = []
    for a in adjs:
        g = np.searchsorted(offs, a[:, 0], side="right") - 1
        idx = np.argsort(g, kind="stable")
        local = (a[idx] - offs[g[idx]][:, None]).astype(np.int32)
        per_type.append(np.split(local, np.cumsum(np.bincount(g, minlength=G))[:-1]))
    return [GraphSample([t[i] for t in per_type], None, feats[offs[i]:offs[i + 1]]) for i in range(G)]


def qm9_fold(num_graphs, seed=0):
    feats, adjs, _, offs = data.make_qm9_shaped_batch(num_graphs, seed=seed, feature_dim=15)  # 15: QM9's atom features
    return _split(feats, adjs, offs), len(adjs)


def ppi_fold(num_graphs, seed=0):
    """self loops, forward and backward edges as three types (what process_adjacency_lists makes of PPI's one forward type)"""
    nodes = 2370
    feats, fwd, _, _ = data.make_ppi_shaped_batch(num_graphs=num_graphs, nodes_per_graph=nodes, seed=seed)
    loops = np.stack([np.arange(len(feats)), np.arange(len(feats))], axis=1).astype(np.int32)
    return _split(feats, [loops, fwd, np.ascontiguousarray(fwd[:, ::-1])], np.arange(num_graphs + 1) * nodes), 3


class _SampleDataset(GraphDataset):
    """a GraphDataset over processed samples: all the probe needs"""

    def __init__(self, params, samples, num_edge_types, node_columns=None):
        super().__init__(params)
        self._num_edge_types = num_edge_types
        self._set_fold(DataFold.TRAIN, PackedFold.from_samples(samples, num_edge_types, node_columns=node_columns))

    @property
    def num_edge_types(self):
        return self._num_edge_types

    @property
    def node_feature_shape(self):
        return (int(self.packed_fold(DataFold.TRAIN).features.shape[1]),)

    def load_data(self, path, folds_to_load=None):
        raise NotImplementedError

    def load_data_from_list(self, datapoints, target_fold=DataFold.TEST):
        raise NotImplementedError


def _epoch(make_iterator):
    """-> (wall seconds, host seconds per batch, batches)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    it = make_iterator()
    host, n, keep = 0.0, 0, None
    while True:
        a = time.perf_counter()
        try:
            keep = next(it)  # the previous batch is released here, as in a training loop
        except StopIteration:
            host += time.perf_counter() - a
            break
        host += time.perf_counter() - a
        n += 1
    torch.cuda.synchronize()
    return time.perf_counter() - t0, host / max(n, 1), n


def _measure(make_iterator, warmup, epochs):
    for _ in range(warmup):
        _epoch(make_iterator)
    runs = [_epoch(make_iterator) for _ in range(epochs)]
    return [r[0] for r in runs], [r[1] for r in runs], runs[0][2]


def _fmt(xs, scale, unit):
    return f"median {statistics.median(xs) * scale:9.3f} {unit}  min {min(xs) * scale:9.3f}  max {max(xs) * scale:9.3f}"


def _with_node_labels(batches, labels, width, dev):
    """the per-batch route's batches with the label rows of their graphs, concatenated on the host and uploaded"""
    g = 0
    for features in batches:
        G = features["num_graphs_in_batch"]
        rows = np.concatenate(labels[g:g + G]) if G else np.zeros((0, width), dtype=np.float32)
        g += G
        yield features, {"node_labels": torch.from_numpy(rows).to(dev)}


def probe(name, samples, num_edge_types, max_nodes, warmup, epochs, dev, out, node_column_width=0):
    samples = list(samples)
    node_labels = None
    if node_column_width:
        rng = np.random.default_rng(0)
        node_labels = [rng.integers(0, 2, size=(len(s.node_features), node_column_width)).astype(np.float32) for s in samples]

    def old_route():
        if node_labels is None:
            np.random.shuffle(samples)
            return data.graph_batch_iterator_from_graph_iterator(iter(samples), num_edge_types, max_nodes, dev)
        order = np.random.permutation(len(samples))
        batches = data.graph_batch_iterator_from_graph_iterator(iter([samples[i] for i in order]), num_edge_types, max_nodes, dev)
        return _with_node_labels(batches, [node_labels[i] for i in order], node_column_width, dev)

    t0 = time.perf_counter()
    ds = _SampleDataset({"max_nodes_per_batch": max_nodes}, samples, num_edge_types,
                        None if node_labels is None else {"node_labels": np.concatenate(node_labels)})
    ds.fold_store(DataFold.TRAIN, dev)
    torch.cuda.synchronize()
    pack = time.perf_counter() - t0
    batches = ds.get_batches(DataFold.TRAIN, dev)

    old_wall, old_host, nb_old = _measure(old_route, warmup, epochs)
    new_wall, new_host, nb_new = _measure(lambda: iter(batches), warmup, epochs)
    fold = ds.packed_fold(DataFold.TRAIN)
    out(f"{name}: {fold.num_graphs} graphs, {int(fold.node_ptr[-1])} nodes, {num_edge_types} edge types, "
        f"{sum(int(p[-1]) for p in fold.edge_ptr)} edges, F = {fold.features.shape[1]}, max_nodes_per_batch = {max_nodes}, "
        f"about {nb_old} batches per epoch; {warmup} warm-up + {epochs} measured epochs"
        + (f"; node column node_labels of width {node_column_width}" if node_column_width else ""))
    out(f"  pack + upload of the fold, once:        {pack * 1e3:9.3f} ms")
    out(f"  per-batch route  host time per batch:   {_fmt(old_host, 1e6, 'us')}")
    out(f"  fold store       host time per batch:   {_fmt(new_host, 1e6, 'us')}")
    out(f"  per-batch route  wall time per epoch:   {_fmt(old_wall, 1e3, 'ms')}")
    out(f"  fold store       wall time per epoch:   {_fmt(new_wall, 1e3, 'ms')}")
    gain = statistics.median(old_wall) - statistics.median(new_wall)
    spread = max(old_wall) - min(old_wall)
    verdict = "beats" if gain > spread else "does NOT beat"
    out(f"  median epoch gain {gain * 1e3:.3f} ms against the per-batch route's own spread (max - min) {spread * 1e3:.3f} ms: the fold "
        f"store {verdict} it by more than that spread ({statistics.median(old_wall) / statistics.median(new_wall):.2f}x)")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--epochs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--qm9-graphs", type=int, default=8192)
    ap.add_argument("--ppi-graphs", type=int, default=20)
    ap.add_argument("--node-column-width", type=int, default=0,
                    help="labels per node of the PPI-shaped fold, carried as a node column (0: none; PPI has 121)")
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dataset_probe needs a ROCm device"
    dev = torch.device("cuda", 0)
    lines = []

    def out(line):
        print(line, flush=True)
        lines.append(line)

    out(f"dataset_probe on {torch.cuda.get_device_name(0)}")
    np.random.seed(0)
    samples, L = qm9_fold(args.qm9_graphs)
    probe("QM9-shaped", samples, L, 10000, args.warmup, args.epochs, dev, out)
    samples, L = ppi_fold(args.ppi_graphs)
    probe("PPI-shaped", samples, L, 8000, args.warmup, args.epochs, dev, out, node_column_width=args.node_column_width)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
