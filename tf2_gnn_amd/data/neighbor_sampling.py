"""Neighbour-sampled mini-batches of ONE big graph (GraphSAGE style) - the reference has no counterpart: its graphs are small
and a batch is a union of whole graphs.

``NeighborStore`` is a single-graph PackedFold on the device in the form the sampler reads (include/tfgnn.h "Neighbour
sampling"): per processed edge type the in-CSR ``in_ptr`` int32 [V + 1] / ``in_src`` int32 [E_t] - the sources of every
node's in-edges in the fold's edge-list order, built once on the host with numpy - next to the fold's features and node
columns.  ``sampled_batch`` turns a chunk of seed nodes into an ordinary ``(batch_features, batch_labels)`` pair by two
library calls (tfgnn_neighbor_sample, tfgnn_gather_node_rows) and ONE small device-to-host copy of the counts in between:
the sizes are data-dependent and the graph build needs them on the host.  A sampled batch is therefore not capturable in
a CapturedStep.

One subgraph serves all layers (DESIGN.md "Neighbour sampling"): with K = len(fanouts) >= the number of message passing
layers the seed rows of the model's output are those of the sampled graph computed exactly; only the first
``num_seed_nodes`` rows carry a label weight.  Graph-global exchange, where a model uses it, sees only the sampled
subgraph."""
from __future__ import annotations

import ctypes
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .. import _lib, ops
from .graph_dataset import PackedFold


def build_in_csr(edges: np.ndarray, num_nodes: int) -> Tuple[np.ndarray, np.ndarray]:
    """(in_ptr int32 [V + 1], in_src int32 [E]) of an edge list [E, 2] of (source, target): a stable sort by target, so the
    sources of a node's in-edges keep the list's order."""
    edges = np.asarray(edges).reshape(-1, 2)
    targets = edges[:, 1].astype(np.int64)
    if edges.shape[0] and (targets.min() < 0 or targets.max() >= num_nodes or edges[:, 0].min() < 0 or edges[:, 0].max() >= num_nodes):
        raise ValueError(f"an edge names a node outside the {num_nodes} nodes")
    in_ptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(targets, minlength=num_nodes), out=in_ptr[1:])
    return in_ptr.astype(np.int32), np.ascontiguousarray(edges[np.argsort(targets, kind="stable"), 0], dtype=np.int32)


def batch_key(sampling_seed: int, epoch: int, batch_index: int) -> int:
    """The 64-bit seed of one sampled batch: ``sampling_seed`` mod 2^24 in bits 40..63, ``epoch`` mod 2^20 in bits 20..39,
    ``batch_index`` mod 2^20 in bits 0..19 - distinct for distinct triples inside those ranges; the library mixes it with a
    splitmix64 step."""
    return ((int(sampling_seed) % 2 ** 24) << 40) | ((int(epoch) % 2 ** 20) << 20) | (int(batch_index) % 2 ** 20)


def plan_seed_chunks(num_seeds: int, seeds_per_batch: int) -> List[Tuple[int, int]]:
    """The [start, end) ranges of an epoch's batches over ``num_seeds`` seeds: full chunks, and the partial last one kept."""
    if seeds_per_batch < 1:
        raise ValueError("seeds_per_batch must be at least 1")
    return [(s, min(s + seeds_per_batch, num_seeds)) for s in range(0, num_seeds, seeds_per_batch)]


def check_fanouts(fanouts) -> List[int]:
    fanouts = [int(f) for f in fanouts]
    if not 1 <= len(fanouts) <= _lib.SAMPLE_MAX_HOPS:
        raise ValueError(f"neighbour sampling takes 1 to {_lib.SAMPLE_MAX_HOPS} fanouts (one per hop), not {len(fanouts)}")
    return fanouts


def check_store_limits(fold: PackedFold) -> None:
    """ValueError for a fold the sampler cannot take: its per-type tables are kernel arguments (a dataset that knows its
    route when it loads calls this then, NeighborStore always)."""
    if fold.num_edge_types > _lib.BATCH_MAX_EDGE_TYPES or len(fold.node_columns) > _lib.BATCH_MAX_NODE_COLUMNS:
        raise ValueError(f"at most {_lib.BATCH_MAX_EDGE_TYPES} edge types and {_lib.BATCH_MAX_NODE_COLUMNS} node columns")


def _array_key(a: np.ndarray):
    """names the memory an array shows: two folds of one dataset hold views of the same host arrays"""
    return (a.__array_interface__["data"][0], a.shape, a.strides, a.dtype.str)


class NeighborStore:
    """A single-graph PackedFold on the device for the sampler.  ``share``: a store of another fold of the same graph whose
    device arrays are reused wherever the host arrays are the same memory (the folds of NodeClassificationDataset share
    everything but the weight column)."""

    def __init__(self, fold: PackedFold, device=None, share: Optional["NeighborStore"] = None):
        if fold.num_graphs != 1:
            raise ValueError(f"neighbour sampling needs a fold of one graph, not {fold.num_graphs}: node_to_graph_map must be sorted, "
                             "and a sampled batch is one graph")
        check_store_limits(fold)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.fold = fold
        self.num_nodes = int(fold.features.shape[0])
        if self.num_nodes < 1:
            raise ValueError("a neighbour store needs at least one node")
        self.store_edges = [int(e.shape[0]) for e in fold.edges]
        if sum(self.store_edges) >= 2 ** 31:
            raise ValueError("2^31 or more edges do not fit the sampler's int32 slot offsets")
        shared = dict(share._uploaded) if share is not None and share.device == self.device else {}
        self._uploaded: Dict[Any, torch.Tensor] = {}  # the fold keeps the host arrays alive, so the keys stay theirs

        def up(host: np.ndarray) -> torch.Tensor:
            t = shared.get(_array_key(host))
            if t is None:
                t = torch.from_numpy(np.ascontiguousarray(host)).to(self.device)
            self._uploaded[_array_key(host)] = t
            return t

        self.in_ptr_host, self.in_src_host, self.in_ptr, self.in_src = [], [], [], []
        for t, e in enumerate(fold.edges):
            same = share is not None and t < len(share.fold.edges) and _array_key(share.fold.edges[t]) == _array_key(e)
            ptr, src = (share.in_ptr_host[t], share.in_src_host[t]) if same else build_in_csr(e, self.num_nodes)
            self.in_ptr_host.append(ptr)
            self.in_src_host.append(src)
            on_device = same and share.device == self.device
            self.in_ptr.append(share.in_ptr[t] if on_device else torch.from_numpy(ptr).to(self.device))
            self.in_src.append(share.in_src[t] if on_device else torch.from_numpy(src).to(self.device))
        self.max_in_degree = [int(np.diff(p).max()) for p in self.in_ptr_host]
        # a featureless fold (width 0): one placeholder column of zeros, tfgnn_gather_node_rows needs a width >= 1; a sampled
        # batch exposes the [n, 0] view of what the gather wrote
        self.featureless = fold.features.shape[1] == 0
        self.features = (torch.zeros((self.num_nodes, 1), dtype=torch.float32, device=self.device) if self.featureless
                         else up(fold.features))
        self.node_column_names = list(fold.node_columns)
        self.node_columns = [up(fold.node_columns[k]) for k in self.node_column_names]
        L = len(self.in_ptr)
        self._in_ptr_tab = (ctypes.c_void_p * max(L, 1))(*[t.data_ptr() for t in self.in_ptr])
        self._in_src_tab = (ctypes.c_void_p * max(L, 1))(*[t.data_ptr() for t in self.in_src])
        self._store_edges_tab = (ctypes.c_int64 * max(L, 1))(*self.store_edges)
        self._workspace: Optional[torch.Tensor] = None
        self._workspace_capacity = -1
        self._exclude_workspace: Optional[torch.Tensor] = None

    @property
    def num_edge_types(self) -> int:
        return len(self.in_ptr)

    def workspace(self, node_capacity: int) -> torch.Tensor:
        """The sampler's workspace for outputs of up to ``node_capacity`` nodes: allocated, and its local-id table filled
        with -1, when a larger one than before is asked for; every call leaves the table all -1, so it is reused as it is."""
        if node_capacity > self._workspace_capacity:
            nbytes = int(_lib.load().tfgnn_neighbor_sample_workspace_bytes(self.num_nodes, self.num_edge_types, node_capacity))
            if nbytes == 0:
                raise ValueError("no sampler workspace for these sizes (include/tfgnn.h: limits of tfgnn_neighbor_sample)")
            ws = torch.empty(nbytes // 4, dtype=torch.int32, device=self.device)
            ws[:self.num_nodes].fill_(-1)
            self._workspace, self._workspace_capacity = ws, node_capacity
        return self._workspace

    def exclude_workspace(self, words: int) -> torch.Tensor:
        """An int32 workspace of at least ``words`` words for ops.sample_exclude_edges (no initialisation): allocated when
        a larger one than before is asked for."""
        if self._exclude_workspace is None or self._exclude_workspace.numel() < words:
            self._exclude_workspace = torch.empty(words, dtype=torch.int32, device=self.device)
        return self._exclude_workspace

    def local_id_table(self) -> Optional[torch.Tensor]:
        """The first V words of the workspace (None before the first sample): all -1 between calls."""
        return None if self._workspace is None else self._workspace[:self.num_nodes]


def sampled_batch(store: NeighborStore, seeds: torch.Tensor, fanouts: Sequence[int], key: int,
                  seed_only_columns: Sequence[str] = ("node_label_weights",), exclude=None) -> Tuple[Dict[str, Any], Dict[str, Any]]:
    """The sampled K-hop subgraph of the int32 device tensor ``seeds`` as ``(batch_features, batch_labels)``: node_features
    [n, F], adjacency_list_<t> (local ids), node_to_graph_map = 0 and num_graphs_in_batch = 1, num_seed_nodes,
    sampled_node_ids (device, global ids; the seeds are rows 0 .. num_seed_nodes - 1) and hop_ptr (host); the store's node
    columns as labels [n, W], those named in ``seed_only_columns`` zero below the seed rows.  Not capturable: the counts are
    read back once between the two library calls.
    ``exclude`` = (positives int32 [B, 3] in local ids, fwd_type, inv_type) goes to ``ops.neighbor_sample``: those edges are
    taken out of the lists before the counts are read back - no further copy - and ``excluded_edge_counts`` (device int32
    [L]) says how many went from every list."""
    sample = ops.neighbor_sample(store, seeds, fanouts, key, exclude=exclude)
    if sample.status:
        raise ValueError(f"neighbour sampling failed with status {sample.status} (include/tfgnn.h TFGNN_SAMPLE_*: 4 a repeated "
                         "seed, 8 a seed outside the graph, 16 an in-CSR that disagrees with its sizes; 32 / 64 an excluded "
                         "positive with a relation / an endpoint outside the batch)")
    bad_flag = torch.zeros(1, dtype=torch.int32, device=store.device)
    nf, cols = ops.gather_node_rows(sample.nodes, sample.num_seeds, store.features, store.node_columns,
                                    seed_only=[name in seed_only_columns for name in store.node_column_names], bad_flag=bad_flag)
    n = int(sample.nodes.shape[0])
    if store.featureless:
        nf = nf[:, :0]  # float32 [n, 0]
    features: Dict[str, Any] = {
        "node_features": nf,
        "node_to_graph_map": torch.zeros(n, dtype=torch.int32, device=store.device),
        "num_graphs_in_batch": 1,
        "num_seed_nodes": sample.num_seeds,
        "sampled_node_ids": sample.nodes,
        "hop_ptr": sample.hop_ptr,
        "_bad_local_index": bad_flag,
    }
    for t, a in enumerate(sample.adjacency_lists):
        features[f"adjacency_list_{t}"] = a
    if sample.removed is not None:
        features["excluded_edge_counts"] = sample.removed
    return features, dict(zip(store.node_column_names, cols))
