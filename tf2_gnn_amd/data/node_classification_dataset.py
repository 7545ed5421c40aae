"""Transductive node classification: one class per node, known for part of the nodes, and folds that are node masks over
the SAME graph(s) (ogbn-arxiv style).  The reference has no such dataset.

A data directory holds numpy files only:
  ``node_features.npy`` [V, F] - optional: without it the dataset is FEATURELESS (``node_feature_shape`` is (0,), a batch's
  ``node_features`` a float32 [V, 0], and a task model needs the hyper-parameter ``node_embedding_dim``, tasks.py: one
  learned row per node, looked up through a sampled batch's ``sampled_node_ids``); ``node_labels.npy`` int [V], -1 where the
  class is unknown, which also gives V;
  ``edges.npy`` [E, 2] (one forward edge type) or ``edges_0.npy``, ``edges_1.npy``, ... (one file per forward edge type),
  (source, target) pairs over the node axis;
  optionally ``node_graph_id.npy`` [V]: the graph of every node, each graph's nodes contiguous along the node axis as in
  PPIDataset - without it all nodes form one graph;
  ``train_idx.npy``, ``valid_idx.npy``, ``test_idx.npy``: the node indices of the three folds.

Every fold is the whole graph.  The folds share node features and adjacency lists (the same host arrays) and differ in one
of the two node columns [V, 1] that come out of every batch's single tfgnn_batch_assemble launch, next to each other in
``batch_labels``: ``node_labels`` - the class as float32, -1 where unknown - and ``node_label_weights`` - 1 for the fold's
indices, 0 elsewhere.  That is what NodeClassificationTask reads.  With the default ``max_nodes_per_batch`` everything int32
offsets admit is ONE batch, so an epoch is one step and a CapturedStep of it replays for every epoch; copying another
fold's ``node_label_weights`` over the batch's column in place evaluates that fold with the same captured step.  (A smaller
``max_nodes_per_batch`` cuts batches between graphs by the reference's rule, plan_batches - the empty batch in front of a
first graph over the limit included.)

The fold is processed at once with numpy, as in PPIDataset; inputs that do not describe such a dataset raise ValueError.

Neighbour-sampled mini-batches.  With the hyper-parameter ``neighbor_fanouts`` set (a list of K fanouts, one per hop, -1 for
every in-edge; the default None is the route above, untouched) ``get_batches(fold)`` yields one batch per chunk of
``seeds_per_batch`` of the fold's indices - the last, partial chunk included - each the K-hop subgraph the device sampler
draws around its seeds (data/neighbor_sampling.py, include/tfgnn.h "Neighbour sampling"): the seeds are rows
0 .. ``num_seed_nodes`` - 1, ``node_label_weights`` is the fold's weight there and 0 below, ``sampled_node_ids`` names the rows'
nodes.  TRAIN draws a fresh np.random permutation of ``train_idx`` per ``iter()`` and samples with the key
``batch_key(sampling_seed, epoch counter, batch index)``, the counter advancing with every ``iter()``; VALIDATION and TEST keep
file order and epoch 0 (with ``eval_neighbor_fanouts``, default: the training fanouts), so their batches are the same on
every ``iter()``.  K should be at least the number of message passing layers: then a seed's output is exact for the sampled
graph (all of it at fanout -1).  A sampled batch is one graph of a single-graph dataset, so ``node_graph_id`` with several
graphs raises ValueError, and so do repeated indices in a fold; graph-global exchange sees only the sampled subgraph; the
counts of every batch are read back once, so a sampled batch cannot be captured in a CapturedStep.  The sampler takes its
per-type tables as kernel arguments, so the sampled route keeps its limit of 48 processed edge types (NeighborStore raises
ValueError above it); the full-batch route has none, batch assembly chunks the types 48 to a call."""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, Iterator, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from .graph_dataset import DataFold, GraphDataset, PackedFold
from .neighbor_sampling import NeighborStore, batch_key, check_fanouts, plan_seed_chunks, sampled_batch
from .utils import compute_number_of_edge_types, get_tied_edge_types

_FOLD_NAMES = ((DataFold.TRAIN, "train"), (DataFold.VALIDATION, "valid"), (DataFold.TEST, "test"))


class NodeClassificationDataset(GraphDataset):
    @classmethod
    def get_default_hyperparameters(cls) -> Dict[str, Any]:
        hypers = super().get_default_hyperparameters()
        hypers.update({
            "max_nodes_per_batch": 2 ** 31 - 1,  # no fold of int32 node ids reaches it: the fold is one batch
            "add_self_loop_edges": True,
            "tie_fwd_bkwd_edges": False,
            "num_node_classes": None,  # None: the largest label + 1
            "neighbor_fanouts": None,  # None: full-batch; a list of K fanouts (-1: every in-edge): neighbour-sampled batches
            "eval_neighbor_fanouts": None,  # None: the same fanouts as training
            "seeds_per_batch": 1024,
            "sampling_seed": 0,
        })
        return hypers

    @staticmethod
    def default_data_path() -> str:
        return "data/node_classification"

    def __init__(self, params: Dict[str, Any], metadata: Optional[Dict[str, Any]] = None, **kwargs):
        super().__init__(params, metadata=metadata, **kwargs)
        self._num_fwd_edge_types: Optional[int] = None
        self._num_node_classes: Optional[int] = None
        self._fold_indices: Dict[DataFold, np.ndarray] = {}
        self._neighbor_stores: Dict[Tuple[DataFold, str], NeighborStore] = {}
        self._sampling_epoch = 0

    def _loaded(self, what: str):
        if self._num_fwd_edge_types is None:
            raise ValueError(f"{what} is known once data has been loaded")

    @property
    def num_edge_types(self) -> int:
        self._loaded("num_edge_types")
        return compute_number_of_edge_types(
            tied_fwd_bkwd_edge_types=get_tied_edge_types(self.params["tie_fwd_bkwd_edges"], self._num_fwd_edge_types),
            num_fwd_edge_types=self._num_fwd_edge_types,
            add_self_loop_edges=self.params["add_self_loop_edges"],
        )

    @property
    def node_feature_shape(self) -> Tuple:
        self._loaded("node_feature_shape")
        some_fold = next(iter(self._loaded_data.values()))
        return (int(some_fold.features.shape[1]),)

    @property
    def num_node_classes(self) -> int:
        self._loaded("num_node_classes")
        return self._num_node_classes

    @property
    def num_nodes(self) -> int:
        """The nodes of the whole graph (all graphs of ``node_graph_id`` together): the rows of a learned embedding table."""
        self._loaded("num_nodes")
        some_fold = next(iter(self._loaded_data.values()))
        return int(some_fold.features.shape[0])

    # ---- loading ------------------------------------------------------------------------------------------------------------
    def load_data(self, path, folds_to_load: Optional[Set[DataFold]] = None) -> None:
        data_dir = Path(path)
        if (data_dir / "edges.npy").exists():
            edges = [np.load(data_dir / "edges.npy")]
        else:
            edges = []
            while (data_dir / f"edges_{len(edges)}.npy").exists():
                edges.append(np.load(data_dir / f"edges_{len(edges)}.npy"))
            if not edges:
                raise ValueError(f"{data_dir}: neither edges.npy nor edges_0.npy")
        graph_id_file, features_file = data_dir / "node_graph_id.npy", data_dir / "node_features.npy"
        self.load_data_from_arrays(
            np.load(features_file) if features_file.exists() else None,
            np.load(data_dir / "node_labels.npy"),
            edges,
            **{f"{name}_idx": np.load(data_dir / f"{name}_idx.npy") for fold, name in _FOLD_NAMES
               if folds_to_load is None or fold in folds_to_load},
            node_graph_id=np.load(graph_id_file) if graph_id_file.exists() else None,
            what=str(data_dir),
        )

    def load_data_from_list(self, datapoints: List[Dict[str, Any]], target_fold: DataFold = DataFold.TEST):
        raise NotImplementedError()

    def load_data_from_arrays(self, node_features, node_labels, edges, train_idx=None, valid_idx=None, test_idx=None,
                              node_graph_id=None, what: str = "arrays") -> None:
        """The files of ``load_data`` as arrays.  ``edges``: one [E, 2] array, or a sequence of them, one per forward edge
        type; a fold whose indices are None is not loaded.  ``node_features`` None: a featureless dataset, its node count the
        length of ``node_labels``."""
        fold_indices = {fold: idx for (fold, _), idx in zip(_FOLD_NAMES, (train_idx, valid_idx, test_idx)) if idx is not None}
        raw_labels = np.asarray(node_labels).reshape(-1)
        V = raw_labels.shape[0]
        feats = np.zeros((V, 0), dtype=np.float32) if node_features is None else np.asarray(node_features, dtype=np.float32)
        if feats.ndim != 2 or feats.shape[0] != V:
            raise ValueError(f"{what}: features {list(feats.shape)} and {V} labels do not describe the same nodes")
        if raw_labels.dtype.kind not in "iu":
            if not np.all(raw_labels == np.floor(raw_labels)):  # NaN included
                raise ValueError(f"{what}: node labels must be integers (-1 for unknown)")
        labels = raw_labels.astype(np.int64)
        if V and labels.min() < -1:
            raise ValueError(f"{what}: node label {labels.min()} (-1 stands for unknown, classes count from 0)")
        num_classes = self.params.get("num_node_classes")
        if num_classes is None:
            num_classes = max(int(labels.max()) + 1 if V else 0, 1)
        num_classes = int(num_classes)
        if V and labels.max() >= num_classes:
            v = int(np.flatnonzero(labels >= num_classes)[0])
            raise ValueError(f"{what}: node {v} has label {labels[v]}, the dataset has {num_classes} classes")
        if num_classes > 2 ** 24:
            raise ValueError(f"{what}: {num_classes} classes do not fit float32 labels")

        weights = {}
        for fold, idx in fold_indices.items():
            idx = np.asarray(idx).reshape(-1)
            if idx.dtype.kind not in "iu":
                raise ValueError(f"{what}: the {fold.name} indices must be integers")
            idx = idx.astype(np.int64)
            outside = (idx < 0) | (idx >= V)
            if outside.any():
                raise ValueError(f"{what}: {fold.name} index {idx[outside][0]} is outside the {V} nodes")
            unknown = labels[idx] < 0
            if unknown.any():
                raise ValueError(f"{what}: {fold.name} index {idx[unknown][0]} names a node without a label")
            if self.sampled and np.unique(idx).shape[0] != idx.shape[0]:
                raise ValueError(f"{what}: the {fold.name} indices repeat a node; neighbour sampling needs distinct seeds")
            w = np.zeros((V, 1), dtype=np.float32)
            w[idx] = 1.0
            weights[fold] = w

        if isinstance(edges, np.ndarray) and edges.ndim == 2:
            edges = [edges]
        base = self._pack_graphs(feats, [np.asarray(e) for e in edges], node_graph_id, labels.astype(np.float32), what)
        if self.sampled and base.num_graphs != 1:
            raise ValueError(f"{what}: neighbour sampling (neighbor_fanouts) needs a single graph, node_graph_id describes "
                             f"{base.num_graphs}: a sampled batch is one graph and node_to_graph_map must be sorted")
        self._num_fwd_edge_types, self._num_node_classes = len(edges), num_classes
        for fold, w in weights.items():
            # the same host arrays for every fold; only the weight column is the fold's own
            self._set_fold(fold, PackedFold(base.node_counts, base.features, base.edge_counts, base.edges,
                                            node_columns={"node_labels": base.node_columns["node_labels"], "node_label_weights": w}))
            self._fold_indices[fold] = np.asarray(fold_indices[fold]).reshape(-1).astype(np.int64)
            for key in [k for k in self._neighbor_stores if k[0] == fold]:
                del self._neighbor_stores[key]

    def _pack_graphs(self, feats: np.ndarray, edges: Sequence[np.ndarray], node_graph_id, labels: np.ndarray, what: str) -> PackedFold:
        V = feats.shape[0]
        graph_ids = np.zeros(V, dtype=np.int64) if node_graph_id is None else np.asarray(node_graph_id).reshape(-1)
        if graph_ids.shape[0] != V:
            raise ValueError(f"{what}: {graph_ids.shape[0]} graph ids for {V} nodes")
        # graphs in first-seen order of their ids: a new graph starts wherever the id changes
        starts = np.flatnonzero(np.concatenate([[True], graph_ids[1:] != graph_ids[:-1]])) if V else np.zeros(0, dtype=np.int64)
        unique_ids, seen = np.unique(graph_ids[starts], return_counts=True)
        if (seen > 1).any():
            raise ValueError(f"{what}: the nodes of graph {unique_ids[seen > 1][0]} are not contiguous along the node axis")
        N = starts.shape[0]
        node_graph = np.repeat(np.arange(N, dtype=np.int64), np.diff(np.concatenate([starts, [V]])))
        per_type = []  # per forward type: the graphs' edge lists with graph-local ids
        for t, e in enumerate(edges):
            if e.ndim != 2 or e.shape[1] != 2 or e.dtype.kind not in "iu":
                raise ValueError(f"{what}: the edges of type {t} must be an integer [E, 2] array, not {e.dtype} {list(e.shape)}")
            src, dst = e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)
            outside = (src < 0) | (src >= V) | (dst < 0) | (dst >= V)
            if outside.any():
                k = int(np.flatnonzero(outside)[0])
                raise ValueError(f"{what}: edge {k} of type {t} ({src[k]} -> {dst[k]}) names a node outside the {V} nodes")
            src_graph = node_graph[src]
            crossing = src_graph != node_graph[dst]
            if crossing.any():
                k = int(np.flatnonzero(crossing)[0])
                raise ValueError(f"{what}: edge {k} of type {t} ({src[k]} -> {dst[k]}) joins graph {graph_ids[src[k]]} and "
                                 f"graph {graph_ids[dst[k]]}")
            by_graph = np.argsort(src_graph, kind="stable")  # grouped by graph, the file's order kept within each
            offset = starts[src_graph[by_graph]]
            local = np.stack([src[by_graph] - offset, dst[by_graph] - offset], axis=1).astype(np.int32)
            per_type.append(np.split(local, np.cumsum(np.bincount(src_graph, minlength=N))[:-1]) if N else [])
        return PackedFold.from_raw_graphs(
            node_features=np.split(feats, starts[1:]) if N else [],
            raw_adjacency_lists=[[per_type[t][g] for t in range(len(edges))] for g in range(N)],
            num_fwd_edge_types=len(edges),
            add_self_loop_edges=self.params["add_self_loop_edges"],
            tied_fwd_bkwd_edge_types=get_tied_edge_types(self.params["tie_fwd_bkwd_edges"], len(edges)),
            feature_dim=int(feats.shape[1]),
            node_columns={"node_labels": labels.reshape(-1, 1)},
        )

    # ---- neighbour-sampled batches ----------------------------------------------------------------------------------------
    @property
    def sampled(self) -> bool:
        return self.params.get("neighbor_fanouts") is not None

    def fanouts(self, data_fold: DataFold) -> List[int]:
        """The fold's fanouts: ``eval_neighbor_fanouts`` for VALIDATION and TEST when it is set, else ``neighbor_fanouts``."""
        fanouts = self.params.get("neighbor_fanouts")
        if data_fold != DataFold.TRAIN and self.params.get("eval_neighbor_fanouts") is not None:
            fanouts = self.params["eval_neighbor_fanouts"]
        if fanouts is None:
            raise ValueError("neighbor_fanouts is not set: the dataset is full-batch")
        return check_fanouts(fanouts)

    def neighbor_store(self, data_fold: DataFold, device=None) -> NeighborStore:
        """The fold in the sampler's form on the device; built at the first request, the graph, features and labels shared
        between the folds."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        key = (data_fold, str(dev))
        if key not in self._neighbor_stores:
            other = next((s for (_, d), s in self._neighbor_stores.items() if d == str(dev)), None)
            self._neighbor_stores[key] = NeighborStore(self._loaded_data[data_fold], dev, share=other)
        return self._neighbor_stores[key]

    def plan_sampled_epoch(self, data_fold: DataFold) -> Tuple[np.ndarray, List[Tuple[int, int]], int]:
        """(seed order, chunk ranges, epoch number) of a new epoch: TRAIN permutes its indices with numpy's global generator
        and takes the next epoch number; the other folds keep file order and epoch 0."""
        idx = self._fold_indices[data_fold]
        if data_fold == DataFold.TRAIN:
            order, epoch = idx[np.random.permutation(idx.shape[0])], self._sampling_epoch
            self._sampling_epoch += 1
        else:
            order, epoch = idx, 0
        return order, plan_seed_chunks(idx.shape[0], int(self.params.get("seeds_per_batch", 1024))), epoch

    def get_batches(self, data_fold: DataFold, device=None):
        if not self.sampled:
            return super().get_batches(data_fold, device)
        return _SampledBatches(self, data_fold, device)


class _SampledBatches:
    """What ``get_batches`` returns with ``neighbor_fanouts`` set: every ``iter()`` is one epoch of sampled batches; the
    epoch's seed order goes to the device in one copy."""

    def __init__(self, dataset: NodeClassificationDataset, data_fold: DataFold, device=None):
        self._dataset, self._data_fold, self._device = dataset, data_fold, device

    def __iter__(self) -> Iterator[Tuple[Dict[str, Any], Dict[str, Any]]]:
        ds, fold = self._dataset, self._data_fold
        fanouts = ds.fanouts(fold)
        store = ds.neighbor_store(fold, self._device)
        order, chunks, epoch = ds.plan_sampled_epoch(fold)
        seeds = torch.from_numpy(order.astype(np.int32)).to(store.device)
        for b, (s, e) in enumerate(chunks):
            yield sampled_batch(store, seeds[s:e], fanouts, batch_key(ds.params.get("sampling_seed", 0), epoch, b))
