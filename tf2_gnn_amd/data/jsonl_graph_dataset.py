"""Datasets stored as JSON lines - mirror of tf2_gnn/data/jsonl_graph_dataset.py:14-145.

A data directory holds ``train.jsonl.gz``, ``valid.jsonl.gz`` and ``test.jsonl.gz``; every line is a JSON dictionary whose
"graph" entry has "node_features" (one list of numbers per node) and "adjacency_lists" (one list of (src, dst) pairs per
forward edge type).  An optional ``metadata.pkl.gz`` (a gzipped pickle of a dictionary) is read when no metadata was given to
the constructor.  Files are read with the standard library; paths are ``str`` or ``pathlib.Path``."""
from __future__ import annotations

import gzip
import json
import logging
import pickle
from pathlib import Path
from typing import Any, Dict, List, Optional, Set, Tuple

from .graph_dataset import DataFold, GraphDataset, PackedFold
from .utils import compute_number_of_edge_types, get_tied_edge_types

logger = logging.getLogger(__name__)

_FOLD_FILES = ((DataFold.TRAIN, "train.jsonl.gz"), (DataFold.VALIDATION, "valid.jsonl.gz"), (DataFold.TEST, "test.jsonl.gz"))


def _read_jsonl_gz(path: Path) -> List[Dict[str, Any]]:
    with gzip.open(path, "rt", encoding="utf-8") as f:
        return [json.loads(line) for line in f if line.strip()]


class JsonLGraphDataset(GraphDataset):
    @classmethod
    def get_default_hyperparameters(cls) -> Dict[str, Any]:
        hypers = super().get_default_hyperparameters()
        hypers.update({"num_fwd_edge_types": 3, "add_self_loop_edges": True, "tie_fwd_bkwd_edges": True})
        return hypers

    def __init__(self, params: Dict[str, Any], metadata: Optional[Dict[str, Any]] = None, **kwargs):
        super().__init__(params, metadata=metadata, **kwargs)
        self._num_fwd_edge_types = params["num_fwd_edge_types"]
        self._tied_fwd_bkwd_edge_types = get_tied_edge_types(
            tie_fwd_bkwd_edges=params["tie_fwd_bkwd_edges"], num_fwd_edge_types=params["num_fwd_edge_types"]
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
        shape = self.metadata.get("_node_feature_shape")
        if shape is None:
            some_fold = next(iter(self._loaded_data.values()))
            shape = (int(some_fold.features.shape[1]),)
            self.metadata["_node_feature_shape"] = shape
        return tuple(shape)

    def load_metadata(self, path) -> None:
        """Metadata stored with the data (vocabularies, property names, ...) unless the constructor was given some."""
        if self.metadata == {}:
            metadata_path = Path(path) / "metadata.pkl.gz"
            if metadata_path.exists():
                logger.info(f"Loading metadata from {metadata_path}")
                with gzip.open(metadata_path, "rb") as f:
                    self._metadata = pickle.load(f)
        else:
            logger.warning("Using metadata passed to constructor, not metadata stored with data.")

    def load_data(self, path, folds_to_load: Optional[Set[DataFold]] = None) -> None:
        logger.info(f"Starting to load data from {path}.")
        self.load_metadata(path)
        if folds_to_load is None:
            folds_to_load = {DataFold.TRAIN, DataFold.VALIDATION, DataFold.TEST}
        for data_fold, file_name in _FOLD_FILES:
            if data_fold in folds_to_load:
                self._set_fold(data_fold, self._pack_datapoints(_read_jsonl_gz(Path(path) / file_name)))
                logger.debug(f"Done loading {file_name}.")

    def load_data_from_list(self, datapoints: List[Dict[str, Any]], target_fold: DataFold = DataFold.TEST):
        """Appends to the fold, like the reference; the fold is packed again and goes to the device at its next use."""
        parts = [self._loaded_data[target_fold]] if target_fold in self._loaded_data else []
        parts.append(self._pack_datapoints(list(datapoints)))
        self._set_fold(target_fold, PackedFold.concatenate(parts))

    def _pack_datapoints(self, datapoints: List[Dict[str, Any]]) -> PackedFold:
        """_process_raw_datapoint (jsonl_graph_dataset.py:119-140) for a whole list at once."""
        shape = self.metadata.get("_node_feature_shape")
        return PackedFold.from_raw_graphs(
            node_features=[d["graph"]["node_features"] for d in datapoints],
            raw_adjacency_lists=[d["graph"]["adjacency_lists"] for d in datapoints],
            num_fwd_edge_types=self._num_fwd_edge_types,
            add_self_loop_edges=self.params["add_self_loop_edges"],
            tied_fwd_bkwd_edge_types=self._tied_fwd_bkwd_edge_types,
            columns=self._extra_graph_columns(datapoints),
            node_columns=self._extra_node_columns(datapoints),
            feature_dim=None if shape is None else int(shape[0]),
        )
