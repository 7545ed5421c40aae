"""The QM9 molecule dataset - mirror of tf2_gnn/data/qm9_dataset.py:18-191.

A data directory holds ``train.jsonl.gz``, ``valid.jsonl.gz`` and ``test.jsonl.gz``.  The line format differs from the one
JsonLGraphDataset reads: "graph" is a list of (src, type, dst) triples with bond types counted from 1, "node_features" sits
at top level, and "targets" holds one list per task whose first entry is that task's label.  There are 4 forward edge types;
the label of task ``task_id`` becomes the per-graph column ``target_value`` - what QM9RegressionTask reads."""
from __future__ import annotations

import logging
from pathlib import Path
from typing import Any, Dict, Iterator, List, Optional, Set, Tuple

import numpy as np

from .graph_dataset import DataFold, GraphDataset, PackedFold
from .jsonl_graph_dataset import _FOLD_FILES, _read_jsonl_gz
from .utils import compute_number_of_edge_types, get_tied_edge_types

logger = logging.getLogger(__name__)


class QM9GraphSample:
    """Data structure holding a single QM9 graph (the reference's constructor and properties)."""

    def __init__(self, adjacency_lists: List[np.ndarray], type_to_node_to_num_incoming_edges: np.ndarray,
                 node_features: List[np.ndarray], target_value: float):
        self._adjacency_lists = adjacency_lists
        self._type_to_node_to_num_inedges = type_to_node_to_num_incoming_edges
        self._node_features = node_features
        self._target_value = target_value

    @property
    def adjacency_lists(self) -> List[np.ndarray]:
        return self._adjacency_lists

    @property
    def type_to_node_to_num_inedges(self) -> np.ndarray:
        return self._type_to_node_to_num_inedges

    @property
    def node_features(self):
        return self._node_features

    @property
    def target_value(self) -> float:
        """Target value of the regression task."""
        return self._target_value

    def __str__(self):
        return f"Adj:            {self._adjacency_lists}\nNode_features:  {self._node_features}\nTarget_values:  {self._target_value}"


class QM9Dataset(GraphDataset):
    @classmethod
    def get_default_hyperparameters(cls) -> Dict[str, Any]:
        hypers = super().get_default_hyperparameters()
        hypers.update({"max_nodes_per_batch": 10000, "add_self_loop_edges": True, "tie_fwd_bkwd_edges": True, "task_id": 0})
        return hypers

    def __init__(self, params: Dict[str, Any], metadata: Optional[Dict[str, Any]] = None, **kwargs):
        super().__init__(params, metadata=metadata, **kwargs)
        self._num_fwd_edge_types = 4
        self._tied_fwd_bkwd_edge_types = get_tied_edge_types(
            tie_fwd_bkwd_edges=params["tie_fwd_bkwd_edges"], num_fwd_edge_types=self._num_fwd_edge_types
        )
        self._num_edge_types = compute_number_of_edge_types(
            tied_fwd_bkwd_edge_types=self._tied_fwd_bkwd_edge_types,
            num_fwd_edge_types=self._num_fwd_edge_types,
            add_self_loop_edges=params["add_self_loop_edges"],
        )

    @property
    def num_edge_types(self) -> int:
        return self._num_edge_types

    @property
    def node_feature_shape(self) -> Tuple:
        some_fold = next(iter(self._loaded_data.values()))
        return (int(some_fold.features.shape[1]),)

    # ---- loading ------------------------------------------------------------------------------------------------------------
    def load_data(self, path, folds_to_load: Optional[Set[DataFold]] = None) -> None:
        if path is None:
            raise ValueError("QM9Dataset.load_data needs the directory of train/valid/test.jsonl.gz: no data ships with the package")
        logger.info(f"Starting to load data from {path}.")
        if folds_to_load is None:
            folds_to_load = {DataFold.TRAIN, DataFold.VALIDATION, DataFold.TEST}
        for data_fold, file_name in _FOLD_FILES:
            if data_fold in folds_to_load:
                self._set_fold(data_fold, self._pack_datapoints(_read_jsonl_gz(Path(path) / file_name)))
                logger.debug(f"Done loading {file_name}.")

    def load_data_from_list(self, datapoints: List[Dict[str, Any]], target_fold: DataFold = DataFold.TEST):
        raise NotImplementedError()

    def _raw_adjacency_lists(self, graph, which: int) -> List[np.ndarray]:
        """__graph_to_adjacency_lists (qm9_dataset.py:140-147): the (src, dst) pairs per forward type, in the graph's order"""
        triples = np.asarray(graph, dtype=np.int64).reshape(-1, 3)
        types = triples[:, 1] - 1  # raw QM9 data counts from 1
        bad = (types < 0) | (types >= self._num_fwd_edge_types)
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            raise ValueError(f"graph {which}: edge {k} has type {triples[k, 1]}, QM9 bond types are 1..{self._num_fwd_edge_types}")
        return [triples[types == t][:, [0, 2]] for t in range(self._num_fwd_edge_types)]

    def _extra_graph_columns(self, datapoints: List[Dict[str, Any]]) -> Dict[str, np.ndarray]:
        task_id = self.params["task_id"]
        return {"target_value": np.array([float(d["targets"][task_id][0]) for d in datapoints], dtype=np.float32)}

    def _pack_datapoints(self, datapoints: List[Dict[str, Any]]) -> PackedFold:
        """__process_raw_graphs (qm9_dataset.py:124-138) for a whole list at once."""
        return PackedFold.from_raw_graphs(
            node_features=[d["node_features"] for d in datapoints],
            raw_adjacency_lists=[self._raw_adjacency_lists(d["graph"], i) for i, d in enumerate(datapoints)],
            num_fwd_edge_types=self._num_fwd_edge_types,
            add_self_loop_edges=self.params["add_self_loop_edges"],
            tied_fwd_bkwd_edge_types=self._tied_fwd_bkwd_edge_types,
            columns=self._extra_graph_columns(datapoints),
            node_columns=self._extra_node_columns(datapoints),
        )

    # ---- the host route -----------------------------------------------------------------------------------------------------
    def _graph_iterator(self, data_fold: DataFold) -> Iterator[QM9GraphSample]:
        fold = self._loaded_data[data_fold]
        for i in self.epoch_order(data_fold):
            s = fold.sample(int(i))
            yield QM9GraphSample(s.adjacency_lists, s.type_to_node_to_num_inedges, s.node_features,
                                 float(fold.columns["target_value"][i]))
