"""JSON-lines datasets with one numeric property per graph - mirror of tf2_gnn/data/jsonl_graph_property_dataset.py:11-117.

Every line carries, next to "graph", a "Property" entry with a floating point value; it becomes the per-graph label
``target_value`` of the batches."""
from __future__ import annotations

from typing import Any, Dict, List, Optional

import numpy as np

from .jsonl_graph_dataset import JsonLGraphDataset


class GraphWithPropertySample:
    """A graph sample with a single numeric property (the reference's constructor and properties)."""

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
        return self._target_value

    def __str__(self):
        return f"Adj:            {self._adjacency_lists}\nNode_features:  {self._node_features}\nTarget_value:   {self._target_value}"


class JsonLGraphPropertyDataset(JsonLGraphDataset):
    @classmethod
    def get_default_hyperparameters(cls) -> Dict[str, Any]:
        hypers = super().get_default_hyperparameters()
        # None: the stored property is the (regression) target; a number: the target is 1.0 for properties strictly
        # greater than it and 0.0 otherwise
        hypers.update({"threshold_for_classification": None})
        return hypers

    def __init__(self, params: Dict[str, Any], metadata: Optional[Dict[str, Any]] = None, **kwargs):
        super().__init__(params, metadata=metadata, **kwargs)
        self._threshold_for_classification = params["threshold_for_classification"]

    def _extra_graph_columns(self, datapoints: List[Dict[str, Any]]) -> Dict[str, np.ndarray]:
        values = np.array([float(d["Property"]) for d in datapoints], dtype=np.float64)
        if self._threshold_for_classification is not None:
            values = (values > self._threshold_for_classification).astype(np.float64)
        return {"target_value": values.astype(np.float32)}

    def _graph_iterator(self, data_fold):
        fold = self._loaded_data[data_fold]
        for i in self.epoch_order(data_fold):
            s = fold.sample(int(i))
            yield GraphWithPropertySample(s.adjacency_lists, s.type_to_node_to_num_inedges, s.node_features,
                                          float(fold.columns["target_value"][i]))
