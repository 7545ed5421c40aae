"""The protein-protein interaction dataset - mirror of tf2_gnn/data/ppi_dataset.py:11-193.

A data directory holds, per fold (``train``, ``valid``, ``test``), the four files of the published archive:
``<fold>_graph.json`` (only its "links" are read: a list of {"source": node, "target": node} over fold-wide node ids),
``<fold>_feats.npy`` [V, F], ``<fold>_labels.npy`` [V, 121] and ``<fold>_graph_id.npy`` [V].  Graphs come in first-seen order
of their ids along the node axis; each graph's edges keep the order of "links", grouped by the graph of the source node and
shifted to graph-local ids.  There is one forward edge type.  The labels travel as the node column ``node_labels`` and come
out of every batch as a float32 [V, 121] - what NodeMulticlassTask reads.

The reference walks the node axis in Python and, for inputs it was not written for, mangles them silently: a graph whose
nodes are not contiguous gets edges shifted by the wrong offset, an edge between two graphs lands in the source's graph with
a target outside it.  Here the fold is processed at once with numpy and such inputs raise ValueError."""
from __future__ import annotations

import json
from pathlib import Path
from typing import Any, Dict, Iterator, List, Optional, Set, Tuple

import numpy as np

from .graph_dataset import DataFold, GraphDataset, PackedFold
from .utils import compute_number_of_edge_types, get_tied_edge_types

_FOLD_NAMES = ((DataFold.TRAIN, "train"), (DataFold.VALIDATION, "valid"), (DataFold.TEST, "test"))
NUM_PPI_LABELS = 121


class PPIGraphSample:
    """Data structure holding a single PPI graph (the reference's constructor and properties)."""

    def __init__(self, adjacency_lists: List[np.ndarray], type_to_node_to_num_inedges: np.ndarray, node_features: np.ndarray,
                 node_labels: np.ndarray):
        self._adjacency_lists = adjacency_lists
        self._type_to_node_to_num_inedges = type_to_node_to_num_inedges
        self._node_features = node_features
        self._node_labels = node_labels

    @property
    def adjacency_lists(self) -> List[np.ndarray]:
        return self._adjacency_lists

    @property
    def type_to_node_to_num_inedges(self) -> np.ndarray:
        return self._type_to_node_to_num_inedges

    @property
    def node_features(self) -> np.ndarray:
        return self._node_features

    @property
    def node_labels(self) -> np.ndarray:
        """Node labels to predict as ndarray of shape [V, C]"""
        return self._node_labels


class PPIDataset(GraphDataset):
    @classmethod
    def get_default_hyperparameters(cls) -> Dict[str, Any]:
        hypers = super().get_default_hyperparameters()
        hypers.update({"max_nodes_per_batch": 10000, "add_self_loop_edges": True, "tie_fwd_bkwd_edges": False})
        return hypers

    @staticmethod
    def default_data_path() -> str:
        return "data/ppi"

    def __init__(self, params: Dict[str, Any], metadata: Optional[Dict[str, Any]] = None, **kwargs):
        super().__init__(params, metadata=metadata, **kwargs)
        self._tied_fwd_bkwd_edge_types = get_tied_edge_types(tie_fwd_bkwd_edges=params["tie_fwd_bkwd_edges"], num_fwd_edge_types=1)
        self._num_edge_types = compute_number_of_edge_types(
            tied_fwd_bkwd_edge_types=self._tied_fwd_bkwd_edge_types,
            num_fwd_edge_types=1,
            add_self_loop_edges=params["add_self_loop_edges"],
        )

    @property
    def num_edge_types(self) -> int:
        return self._num_edge_types

    @property
    def node_feature_shape(self) -> Tuple:
        some_fold = next(iter(self._loaded_data.values()))
        return (int(some_fold.features.shape[1]),)

    @property
    def num_node_target_labels(self) -> int:
        return NUM_PPI_LABELS

    # ---- loading ------------------------------------------------------------------------------------------------------------
    def load_data(self, path, folds_to_load: Optional[Set[DataFold]] = None) -> None:
        if folds_to_load is None:
            folds_to_load = {DataFold.TRAIN, DataFold.VALIDATION, DataFold.TEST}
        for data_fold, data_name in _FOLD_NAMES:
            if data_fold in folds_to_load:
                self._set_fold(data_fold, self._load_fold(Path(path), data_name))

    def load_data_from_list(self, datapoints: List[Dict[str, Any]], target_fold: DataFold = DataFold.TEST):
        raise NotImplementedError()

    def _load_fold(self, data_dir: Path, data_name: str) -> PackedFold:
        with open(data_dir / f"{data_name}_graph.json", "rt", encoding="utf-8") as f:
            links = json.load(f)["links"]
        return self._pack_fold(
            links,
            np.load(data_dir / f"{data_name}_feats.npy"),
            np.load(data_dir / f"{data_name}_labels.npy"),
            np.load(data_dir / f"{data_name}_graph_id.npy"),
            what=f"{data_dir / data_name}",
        )

    def _pack_fold(self, links: List[Dict[str, Any]], node_to_features, node_to_labels, node_to_graph_id, what: str = "fold") -> PackedFold:
        """__load_data (ppi_dataset.py:95-163) for the whole fold at once."""
        feats = np.asarray(node_to_features, dtype=np.float32)
        labels = np.asarray(node_to_labels, dtype=np.float32)
        graph_ids = np.asarray(node_to_graph_id).reshape(-1)
        V = graph_ids.shape[0]
        if feats.ndim != 2 or feats.shape[0] != V or labels.ndim != 2 or labels.shape[0] != V:
            raise ValueError(f"{what}: features {list(feats.shape)}, labels {list(labels.shape)} and {V} graph ids do not describe the same nodes")
        if labels.shape[1] != NUM_PPI_LABELS:
            raise ValueError(f"{what}: label rows have width {labels.shape[1]}, PPI has {NUM_PPI_LABELS} labels per node")
        # graphs in first-seen order of their ids: a new graph starts wherever the id changes
        starts = np.flatnonzero(np.concatenate([[True], graph_ids[1:] != graph_ids[:-1]])) if V else np.zeros(0, dtype=np.int64)
        ids_in_order = graph_ids[starts]
        unique_ids, seen = np.unique(ids_in_order, return_counts=True)
        if (seen > 1).any():
            raise ValueError(f"{what}: the nodes of graph {unique_ids[seen > 1][0]} are not contiguous along the node axis")
        N = starts.shape[0]
        node_counts = np.diff(np.concatenate([starts, [V]]))
        node_graph = np.repeat(np.arange(N, dtype=np.int64), node_counts)

        src = np.array([e["source"] for e in links], dtype=np.int64)
        dst = np.array([e["target"] for e in links], dtype=np.int64)
        outside = (src < 0) | (src >= V) | (dst < 0) | (dst >= V)
        if outside.any():
            k = int(np.flatnonzero(outside)[0])
            raise ValueError(f"{what}: edge {k} ({src[k]} -> {dst[k]}) names a node outside the {V} nodes of the fold")
        src_graph = node_graph[src]
        crossing = src_graph != node_graph[dst]
        if crossing.any():
            k = int(np.flatnonzero(crossing)[0])
            raise ValueError(f"{what}: edge {k} ({src[k]} -> {dst[k]}) joins graph {graph_ids[src[k]]} and graph {graph_ids[dst[k]]}")
        by_graph = np.argsort(src_graph, kind="stable")  # grouped by graph, the order of "links" kept within each
        offset = starts[src_graph[by_graph]]
        local = np.stack([src[by_graph] - offset, dst[by_graph] - offset], axis=1).astype(np.int32)
        edge_cuts = np.cumsum(np.bincount(src_graph, minlength=N))[:-1] if N else []
        return PackedFold.from_raw_graphs(
            node_features=np.split(feats, starts[1:]) if N else [],
            raw_adjacency_lists=[[e] for e in np.split(local, edge_cuts)] if N else [],
            num_fwd_edge_types=1,
            add_self_loop_edges=self.params["add_self_loop_edges"],
            tied_fwd_bkwd_edge_types=self._tied_fwd_bkwd_edge_types,
            feature_dim=int(feats.shape[1]),
            node_columns={"node_labels": labels},
        )

    # ---- the host route -----------------------------------------------------------------------------------------------------
    def _graph_iterator(self, data_fold: DataFold) -> Iterator[PPIGraphSample]:
        fold = self._loaded_data[data_fold]
        labels = fold.node_columns["node_labels"]
        for i in self.epoch_order(data_fold):
            s = fold.sample(int(i))
            yield PPIGraphSample(s.adjacency_lists, s.type_to_node_to_num_inedges, s.node_features,
                                 labels[int(fold.node_ptr[i]):int(fold.node_ptr[i + 1])])
