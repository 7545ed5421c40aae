"""Device-resident graph datasets - mirror of tf2_gnn/data/graph_dataset.py:56-311 (DataFold, GraphDataset).

The reference keeps a fold as a Python list of GraphSample objects and builds every batch on the host, graph by graph.  Here
a fold is PACKED once - all graphs laid end to end, processed edge lists with graph-local node ids (``PackedFold`` on the
host, ``FoldStore`` on the device) - and a batch is a range of positions of an epoch's graph order:

  * ``EpochPlan`` draws nothing itself: it takes the order, applies the reference's batch rule (a graph that would push the
    node count over ``max_nodes_per_batch`` starts a new batch, graph_dataset.py:167-171) on the host counts, and uploads
    the order and the prefix sums of the node and edge counts along it in ONE copy ([L + 2, P + 1] int32);
  * ``assemble_batch`` is one library call (tfgnn_batch_assemble, csrc/batch.hip: one launch) per batch: no host-to-device
    copy, no synchronisation.  A fold of more than 48 edge types (``_lib.BATCH_MAX_EDGE_TYPES``, the call's limit) takes
    ceil(L / 48) calls: the first with the node arrays, the columns and types [0, 48), every further one with the next 48
    types alone - same stream, same flag, still no copy, synchronisation or extra allocation.

A fold may be FEATURELESS (``PackedFold.features`` of width 0: knowledge-graph entities, whose representation a task model
learns - ``node_embedding_dim``, tasks.py).  The C entries need a feature width >= 1, so the store keeps one placeholder
column of zeros; a batch exposes ``node_features`` as a float32 [V, 0] view of what the call wrote.

``GraphDataset.get_batches(fold)`` stands where the reference has ``get_tensorflow_dataset``: a re-iterable whose every
``iter()`` is one epoch of ``(batch_features, batch_labels)`` in the form run_one_epoch / predict / evaluate_model consume.
"""
from __future__ import annotations

import ctypes
from abc import abstractmethod
from enum import Enum
from typing import Any, Dict, Iterable, Iterator, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from .. import _lib, ops
from .batching import GraphSample

_INT32_LIMIT = 2 ** 31


class DataFold(Enum):
    TRAIN = 0
    VALIDATION = 1
    TEST = 2


def _prefix(counts: np.ndarray) -> np.ndarray:
    ptr = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=ptr[1:])
    return ptr


class PackedFold:
    """One fold on the host: N graphs end to end.

    ``node_counts`` int64 [N]; ``features`` float32 [sum V, F]; per processed edge type ``edge_counts[t]`` int64 [N] and
    ``edges[t]`` int32 [sum E_t, 2] (graph-local node ids, each graph's edges in the reference's order); ``columns``: name ->
    float32 [N], one value per graph (labels); ``node_columns``: name -> float32 [sum V, W], one row per node, laid out like
    ``features``, every column with its own width (per-node labels)."""

    def __init__(self, node_counts, features, edge_counts, edges, columns=None, node_columns=None):
        self.node_counts = np.asarray(node_counts, dtype=np.int64).reshape(-1)
        self.features = np.ascontiguousarray(features, dtype=np.float32)
        if self.features.ndim != 2:
            raise ValueError("node features must be [V, F]")
        self.edge_counts = [np.asarray(c, dtype=np.int64).reshape(-1) for c in edge_counts]
        self.edges = [np.ascontiguousarray(e, dtype=np.int32).reshape(-1, 2) for e in edges]
        self.columns = {k: np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for k, v in (columns or {}).items()}
        self.node_columns = {}
        for k, v in (node_columns or {}).items():
            v = np.ascontiguousarray(v, dtype=np.float32)
            self.node_columns[k] = v.reshape(-1, 1) if v.ndim == 1 else v
        N = self.num_graphs
        self.node_ptr = _prefix(self.node_counts)
        self.edge_ptr = [_prefix(c) for c in self.edge_counts]
        if int(self.node_ptr[-1]) != self.features.shape[0]:
            raise ValueError("node counts do not add up to the feature rows")
        if self.features.shape[0] >= _INT32_LIMIT:
            raise ValueError("a fold of 2^31 or more nodes does not fit int32 node ids")
        for c, p, e in zip(self.edge_counts, self.edge_ptr, self.edges):
            if len(c) != N or int(p[-1]) != e.shape[0]:
                raise ValueError("edge counts do not match the edge lists")
            if e.shape[0] >= _INT32_LIMIT:
                raise ValueError("a fold of 2^31 or more edges of one type does not fit int32 offsets")
        for k, v in self.columns.items():
            if v.shape[0] != N:
                raise ValueError(f"column {k!r} needs one value per graph")
        for k, v in self.node_columns.items():
            if k in self.columns:
                raise ValueError(f"{k!r} is both a per-graph column and a node column")
            if v.ndim != 2 or v.shape[0] != self.features.shape[0]:
                raise ValueError(f"node column {k!r} needs one row per node: [{self.features.shape[0]}, W], not {list(v.shape)}")
            if v.shape[1] < 1:
                raise ValueError(f"node column {k!r} needs a width >= 1")

    @property
    def num_graphs(self) -> int:
        return int(self.node_counts.shape[0])

    @property
    def num_edge_types(self) -> int:
        return len(self.edges)

    def __len__(self) -> int:
        return self.num_graphs

    @classmethod
    def from_samples(cls, samples: Sequence[Any], num_edge_types: int, columns: Optional[Dict[str, Any]] = None,
                     feature_dim: Optional[int] = None, node_columns: Optional[Dict[str, Any]] = None) -> "PackedFold":
        """Pack already processed graph samples (anything with ``node_features`` and ``adjacency_lists``).  ``node_columns``
        are given for the whole fold, the graphs' rows end to end."""
        feats = [np.asarray(s.node_features, dtype=np.float32) for s in samples]
        node_counts = np.array([len(f) for f in feats], dtype=np.int64)
        if feature_dim is None:
            feature_dim = next((int(np.prod(f.shape[1:])) for f in feats if len(f)), 0)
        rows = [f.reshape(len(f), feature_dim) for f in feats if len(f)]
        features = np.concatenate(rows) if rows else np.zeros((0, feature_dim), dtype=np.float32)
        edge_counts, edges = [], []
        for t in range(num_edge_types):
            per_graph = [np.asarray(s.adjacency_lists[t], dtype=np.int32).reshape(-1, 2) for s in samples]
            edge_counts.append(np.array([a.shape[0] for a in per_graph], dtype=np.int64))
            edges.append(np.concatenate(per_graph) if per_graph else np.zeros((0, 2), dtype=np.int32))
        return cls(node_counts, features, edge_counts, edges, columns, node_columns)

    @classmethod
    def from_raw_graphs(cls, node_features: Sequence[Any], raw_adjacency_lists: Sequence[Sequence[Any]], num_fwd_edge_types: int,
                        add_self_loop_edges: bool, tied_fwd_bkwd_edge_types: Set[int], columns: Optional[Dict[str, Any]] = None,
                        feature_dim: Optional[int] = None, node_columns: Optional[Dict[str, Any]] = None) -> "PackedFold":
        """Pack raw graphs and process their edge lists for the whole fold at once - what process_adjacency_lists
        (tf2_gnn/data/utils.py:9-58) does per graph: a tied forward type is followed, within each graph, by its flipped
        edges; the other forward types get fresh backward types behind all forward types, in forward-type order; the self
        loops (i, i) become type 0.  ``raw_adjacency_lists[g][t]``: the (src, dst) pairs of forward type t of graph g."""
        N = len(node_features)
        feats = [np.asarray(f, dtype=np.float32) for f in node_features]
        node_counts = np.array([len(f) for f in feats], dtype=np.int64)
        if feature_dim is None:
            feature_dim = next((int(np.prod(f.shape[1:])) for f in feats if len(f)), 0)
        rows = [f.reshape(len(f), feature_dim) for f in feats if len(f)]
        features = np.concatenate(rows) if rows else np.zeros((0, feature_dim), dtype=np.float32)
        for g, lists in enumerate(raw_adjacency_lists):
            if len(lists) != num_fwd_edge_types:
                raise ValueError(f"graph {g} has {len(lists)} adjacency lists, the dataset was configured for {num_fwd_edge_types}")
        tied = set(tied_fwd_bkwd_edge_types)
        fwd_counts, fwd_edges, bwd_counts, bwd_edges = [], [], [], []
        for t in range(num_fwd_edge_types):
            per_graph = [np.asarray(lists[t], dtype=np.int32).reshape(-1, 2) for lists in raw_adjacency_lists]
            cnt = np.array([a.shape[0] for a in per_graph], dtype=np.int64)
            raw = np.concatenate(per_graph) if per_graph else np.zeros((0, 2), dtype=np.int32)
            if t in tied:
                ptr = _prefix(cnt)
                k = np.arange(raw.shape[0], dtype=np.int64) - np.repeat(ptr[:-1], cnt)
                dst = np.repeat(2 * ptr[:-1], cnt) + k
                both = np.empty((2 * raw.shape[0], 2), dtype=np.int32)
                both[dst] = raw
                both[dst + np.repeat(cnt, cnt)] = raw[:, ::-1]
                fwd_counts.append(2 * cnt)
                fwd_edges.append(both)
            else:
                fwd_counts.append(cnt)
                fwd_edges.append(raw)
                bwd_counts.append(cnt)
                bwd_edges.append(np.ascontiguousarray(raw[:, ::-1]))
        edge_counts, edges = fwd_counts + bwd_counts, fwd_edges + bwd_edges
        if add_self_loop_edges:
            local = np.arange(int(node_counts.sum()), dtype=np.int64) - np.repeat(_prefix(node_counts)[:-1], node_counts)
            edge_counts.insert(0, node_counts.copy())
            edges.insert(0, np.stack([local, local], axis=1).astype(np.int32))
        assert len(node_counts) == N
        return cls(node_counts, features, edge_counts, edges, columns, node_columns)

    @classmethod
    def concatenate(cls, folds: Sequence["PackedFold"]) -> "PackedFold":
        if len(folds) == 1:
            return folds[0]
        first = folds[0]
        L = first.num_edge_types
        F = max(f.features.shape[1] for f in folds)
        for f in folds:
            if f.num_edge_types != L or set(f.columns) != set(first.columns) or (f.features.shape[0] and f.features.shape[1] != F):
                raise ValueError("the parts of a fold disagree on edge types, feature width or columns")
            if {k: v.shape[1] for k, v in f.node_columns.items()} != {k: v.shape[1] for k, v in first.node_columns.items()}:
                raise ValueError("the parts of a fold disagree on node columns or their widths")
        return cls(
            np.concatenate([f.node_counts for f in folds]),
            np.concatenate([f.features.reshape(f.features.shape[0], F) for f in folds]),
            [np.concatenate([f.edge_counts[t] for f in folds]) for t in range(L)],
            [np.concatenate([f.edges[t] for f in folds]) for t in range(L)],
            {k: np.concatenate([f.columns[k] for f in folds]) for k in first.columns},
            {k: np.concatenate([f.node_columns[k] for f in folds]) for k in first.node_columns},
        )

    def sample(self, i: int) -> GraphSample:
        """Graph i as the reference's GraphSample (graph_dataset.py:23-50): processed adjacency lists, the [L, V] in-degree
        counts (data/utils.py:116-124) and the node features."""
        n = int(self.node_counts[i])
        adj = [e[int(p[i]):int(p[i + 1])] for e, p in zip(self.edges, self.edge_ptr)]
        inedges = np.zeros((len(adj), n))
        for t, a in enumerate(adj):
            if a.shape[0]:
                inedges[t] = np.bincount(a[:, 1], minlength=n)[:n]
        return GraphSample(adj, inedges, self.features[int(self.node_ptr[i]):int(self.node_ptr[i + 1])])

    def to(self, device=None) -> "FoldStore":
        return FoldStore(self, device)


class FoldStore:
    """A PackedFold on the device - the fold store of tfgnn_batch_assemble (include/tfgnn.h): ``node_ptr`` int32 [N + 1],
    ``features`` float32 [sum V, F], per type ``edge_ptr[t]`` int32 [N + 1] and ``edges[t]`` int32 [sum E_t, 2], per column a
    float32 [N], per node column a float32 [sum V, W].  The per-graph counts stay on the host (``fold``), so planning an epoch
    reads nothing back."""

    def __init__(self, fold: PackedFold, device=None):
        if len(fold.columns) > _lib.BATCH_MAX_COLUMNS:  # (edge types: any number, assemble_batch chunks them)
            raise ValueError(f"at most {_lib.BATCH_MAX_COLUMNS} per-graph columns")
        if len(fold.node_columns) > _lib.BATCH_MAX_NODE_COLUMNS:
            raise ValueError(f"at most {_lib.BATCH_MAX_NODE_COLUMNS} node columns")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.fold = fold
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.node_ptr = up(fold.node_ptr.astype(np.int32))
        self.featureless = fold.features.shape[1] == 0
        # a featureless fold: one placeholder column of zeros, the C entry needs a width >= 1 (see the module docstring)
        self.features = (torch.zeros((fold.features.shape[0], 1), dtype=torch.float32, device=self.device) if self.featureless
                         else up(fold.features))
        self.edge_ptr = [up(p.astype(np.int32)) for p in fold.edge_ptr]
        self.edges = [up(e) for e in fold.edges]
        self.column_names = list(fold.columns)
        self.columns = [up(fold.columns[k]) for k in self.column_names]
        self.node_column_names = list(fold.node_columns)
        self.node_columns = [up(fold.node_columns[k]) for k in self.node_column_names]
        self.node_column_widths = [int(t.shape[1]) for t in self.node_columns]
        L, C, NC = len(self.edges), len(self.columns), len(self.node_columns)
        # host pointer tables of the argument struct; they live as long as the store
        self._edge_ptr_tab = (ctypes.c_void_p * max(L, 1))(*[t.data_ptr() for t in self.edge_ptr])
        self._edges_tab = (ctypes.c_void_p * max(L, 1))(*[t.data_ptr() for t in self.edges])
        self._columns_tab = (ctypes.c_void_p * max(C, 1))(*[t.data_ptr() for t in self.columns])
        self._node_columns_tab = (ctypes.c_void_p * max(NC, 1))(*[t.data_ptr() for t in self.node_columns])
        self._node_column_widths_tab = (ctypes.c_int64 * max(NC, 1))(*self.node_column_widths)

    @property
    def num_graphs(self) -> int:
        return self.fold.num_graphs

    @property
    def num_edge_types(self) -> int:
        return len(self.edges)

    @property
    def feature_dim(self) -> int:
        """The width of the stored feature rows: 1, the placeholder's, for a featureless fold."""
        return int(self.features.shape[1])

    def sample(self, i: int) -> GraphSample:
        """Graph i read back from the device arrays (a few small copies: for checks, not for the hot path)."""
        ptr = self.fold.node_ptr
        adj = [e[int(p[i]):int(p[i + 1])].cpu().numpy() for e, p in zip(self.edges, self.fold.edge_ptr)]
        feats = self.features[int(ptr[i]):int(ptr[i + 1]), :self.fold.features.shape[1]]
        return GraphSample(adj, None, feats.cpu().numpy())


def plan_batches(node_counts_in_order: np.ndarray, max_nodes_per_batch: int) -> List[Tuple[int, int]]:
    """The position ranges [p0, p1) of the batches graph_batch_iterator_from_graph_iterator (graph_dataset.py:161-181) cuts
    from graphs of these node counts: a graph that would push the node count over the limit closes the batch before it -
    the empty batch in front of a too large FIRST graph included - and the last batch is always yielded."""
    counts = np.asarray(node_counts_in_order, dtype=np.int64).reshape(-1)
    P = counts.shape[0]
    ptr = _prefix(counts)
    bounds: List[Tuple[int, int]] = []
    s = 0
    while True:
        e = min(int(np.searchsorted(ptr, ptr[s] + max_nodes_per_batch, side="right")) - 1, P)
        if e <= s and s < P:  # graph s alone is over the limit: it closes the batch so far and fills the next one
            if s == 0:
                bounds.append((0, 0))
            e = s + 1
        bounds.append((s, e))
        if e >= P:
            return bounds
        s = e


class EpochPlan:
    """One epoch over a fold store: the graph order, its batch boundaries, and - uploaded once, in one copy - the order and
    the prefix sums of the node and per-type edge counts along it ([L + 2, P + 1] int32)."""

    def __init__(self, store: FoldStore, order: Iterable[int], max_nodes_per_batch: int):
        fold = store.fold
        self.store = store
        self.order = np.asarray(order, dtype=np.int64).reshape(-1)
        P = self.order.shape[0]
        if P and (self.order.min() < 0 or self.order.max() >= fold.num_graphs):
            raise ValueError("graph id outside the fold")
        self.pos_node_ptr = _prefix(fold.node_counts[self.order])
        self.pos_edge_ptr = [_prefix(c[self.order]) for c in fold.edge_counts]
        if max(int(p[-1]) for p in [self.pos_node_ptr] + self.pos_edge_ptr) >= _INT32_LIMIT:
            raise ValueError("an epoch of 2^31 or more nodes or edges of one type does not fit int32 offsets")
        self.batches = plan_batches(fold.node_counts[self.order], max_nodes_per_batch)
        L = store.num_edge_types
        host = np.zeros((L + 2, P + 1), dtype=np.int32)
        host[0, :P] = self.order
        host[1] = self.pos_node_ptr
        for t in range(L):
            host[2 + t] = self.pos_edge_ptr[t]
        self.device_arrays = torch.from_numpy(host).to(store.device)
        self._pos_edge_ptr_tab = (ctypes.c_void_p * max(L, 1))(*[self.device_arrays[2 + t].data_ptr() for t in range(L)])
        self.bad_flags = torch.zeros(len(self.batches), dtype=torch.int32, device=store.device)

    def __len__(self) -> int:
        return len(self.batches)

    def sizes(self, p0: int, p1: int) -> Tuple[int, List[int]]:
        """(V, [E_t]) of the batch of positions [p0, p1), from the host's counts"""
        return int(self.pos_node_ptr[p1] - self.pos_node_ptr[p0]), [int(p[p1] - p[p0]) for p in self.pos_edge_ptr]


_ALIGN = 64  # elements: sub-buffers carved from one allocation start on 256-byte boundaries, like allocations of their own


def _carve(sizes: Sequence[int], dtype, device) -> List[torch.Tensor]:
    starts, total = [], 0
    for n in sizes:
        starts.append(total)
        total += -(-n // _ALIGN) * _ALIGN
    buf = torch.empty(total, dtype=dtype, device=device)
    return [buf[s:s + n] for s, n in zip(starts, sizes)]


def assemble_batch(plan: EpochPlan, p0: int, p1: int, out: Optional[Dict[str, Any]] = None,
                   bad_flag: Optional[torch.Tensor] = None) -> Tuple[Dict[str, Any], Dict[str, Any]]:
    """The batch of positions [p0, p1) of ``plan`` -> (batch_features, batch_labels), by one tfgnn_batch_assemble call on the
    current stream - ceil(L / 48) calls for a fold of L > 48 edge types, the further ones carrying edge types only.  ``out``
    may bring the output tensors (node_features [V, F], node_to_graph_map [V], adjacency_list_<t> [E_t, 2], one [G] per column
    name, one [V, W] per node column name), ``bad_flag`` a zeroed int32 [1]; what is missing is allocated here (two
    allocations).  The node columns come back in ``batch_labels`` next to the per-graph columns.  A featureless store: F = 1
    for ``out`` (the placeholder column), and the batch's ``node_features`` is the [V, 0] view of it."""
    store = plan.store
    L, C, F = store.num_edge_types, len(store.columns), store.feature_dim
    NC, widths = len(store.node_columns), store.node_column_widths
    V, E = plan.sizes(p0, p1)
    G = p1 - p0
    dev = store.device
    if out is None:
        ints = _carve([2 * e for e in E] + [V], torch.int32, dev)
        floats = _carve([V * F] + [G] * C + [V * w for w in widths], torch.float32, dev)
        out = {"node_features": floats[0].view(V, F), "node_to_graph_map": ints[L]}
        for t in range(L):
            out[f"adjacency_list_{t}"] = ints[t].view(E[t], 2)
        for c, name in enumerate(store.column_names):
            out[name] = floats[1 + c]
        for c, name in enumerate(store.node_column_names):
            out[name] = floats[1 + C + c].view(V, widths[c])
    if bad_flag is None:
        bad_flag = torch.zeros(1, dtype=torch.int32, device=dev)
    nf, n2g = out["node_features"], out["node_to_graph_map"]
    adj = [out[f"adjacency_list_{t}"] for t in range(L)]
    cols = [out[name] for name in store.column_names]
    node_cols = [out[name] for name in store.node_column_names]
    if tuple(nf.shape) != (V, F) or nf.dtype != torch.float32 or not nf.is_contiguous() or n2g.numel() != V or n2g.dtype != torch.int32:
        raise ValueError("node_features / node_to_graph_map outputs have the wrong shape or type")
    for t, a in enumerate(adj):
        if tuple(a.shape) != (E[t], 2) or a.dtype != torch.int32 or not a.is_contiguous():
            raise ValueError(f"adjacency_list_{t} output must be a contiguous int32 [{E[t]}, 2]")
    for c in cols:
        if c.numel() != G or c.dtype != torch.float32 or not c.is_contiguous():
            raise ValueError("a column output must be a contiguous float32 [G]")
    for name, w, c in zip(store.node_column_names, widths, node_cols):
        if tuple(c.shape) != (V, w) or c.dtype != torch.float32 or not c.is_contiguous():
            raise ValueError(f"the {name} output must be a contiguous float32 [{V}, {w}]")
    a = _lib.BatchAssembleArgs()
    a.struct_size = ctypes.sizeof(_lib.BatchAssembleArgs)
    a.num_columns = C
    a.num_graphs, a.store_nodes, a.feature_dim = store.num_graphs, int(store.features.shape[0]), F
    a.node_ptr, a.features = store.node_ptr.data_ptr(), store.features.data_ptr()
    a.columns = ctypes.addressof(store._columns_tab)
    a.order_len = plan.order.shape[0]
    a.order, a.pos_node_ptr = plan.device_arrays[0].data_ptr(), plan.device_arrays[1].data_ptr()
    a.p0, a.p1, a.num_nodes = p0, p1, V
    num_edges = (ctypes.c_int64 * max(L, 1))(*E)
    adj_tab = (ctypes.c_void_p * max(L, 1))(*[t.data_ptr() for t in adj])
    col_tab = (ctypes.c_void_p * max(C, 1))(*[t.data_ptr() for t in cols])
    a.column_out = ctypes.addressof(col_tab)

    def edge_types_from(t0: int) -> None:
        """the call's edge types: [t0, t0 + 48) of the fold's, every table advanced by t0 entries of 8 bytes (pointers, int64)"""
        a.num_edge_types = min(L - t0, _lib.BATCH_MAX_EDGE_TYPES)
        a.edge_ptr = ctypes.addressof(store._edge_ptr_tab) + 8 * t0
        a.edges = ctypes.addressof(store._edges_tab) + 8 * t0
        a.pos_edge_ptr = ctypes.addressof(plan._pos_edge_ptr_tab) + 8 * t0
        a.num_edges, a.adjacency_lists = ctypes.addressof(num_edges) + 8 * t0, ctypes.addressof(adj_tab) + 8 * t0

    edge_types_from(0)
    a.node_features, a.node_to_graph_map, a.bad_flag = nf.data_ptr(), n2g.data_ptr(), bad_flag.data_ptr()
    if NC:  # without node columns the four fields stay zero
        node_col_tab = (ctypes.c_void_p * NC)(*[t.data_ptr() for t in node_cols])
        a.num_node_columns = NC
        a.node_column_widths = ctypes.addressof(store._node_column_widths_tab)
        a.node_columns, a.node_column_out = ctypes.addressof(store._node_columns_tab), ctypes.addressof(node_col_tab)
    lib, stream = _lib.load(), ops._stream()
    _lib.check(lib.tfgnn_batch_assemble(ctypes.byref(a), stream))
    if L > _lib.BATCH_MAX_EDGE_TYPES:  # the types beyond the call's limit: calls that launch edge tiles only
        a.num_nodes = a.num_columns = a.num_node_columns = 0
        for t0 in range(_lib.BATCH_MAX_EDGE_TYPES, L, _lib.BATCH_MAX_EDGE_TYPES):
            edge_types_from(t0)
            _lib.check(lib.tfgnn_batch_assemble(ctypes.byref(a), stream))
    if store.featureless:
        nf = nf[:, :0]  # float32 [V, 0]
    features: Dict[str, Any] = {"node_features": nf, "node_to_graph_map": n2g, "num_graphs_in_batch": G}
    for t in range(L):
        features[f"adjacency_list_{t}"] = adj[t]
    features["_bad_local_index"] = bad_flag  # device flag, read lazily by ``check_batch``
    labels = dict(zip(store.column_names, cols))
    if NC:
        labels.update(zip(store.node_column_names, node_cols))
    return features, labels


def batch_assemble_launch_counts() -> int:
    """Kernel launches tfgnn_batch_assemble has enqueued in this process (a host counter)."""
    buf = (ctypes.c_int64 * 1)()
    _lib.check(_lib.load().tfgnn_batch_assemble_launch_counts(buf, 1))
    return int(buf[0])


class _Batches:
    """What ``GraphDataset.get_batches`` returns: every ``iter()`` plans a new epoch and yields its batches."""

    def __init__(self, dataset: "GraphDataset", data_fold: DataFold, device=None):
        self._dataset, self._data_fold, self._device = dataset, data_fold, device

    def __iter__(self) -> Iterator[Tuple[Dict[str, Any], Dict[str, Any]]]:
        plan = self._dataset.plan_epoch(self._data_fold, self._device)
        for b, (p0, p1) in enumerate(plan.batches):
            yield assemble_batch(plan, p0, p1, bad_flag=plan.bad_flags[b:b + 1])


class GraphDataset:
    """graph_dataset.py:56-311 on a fold store.  Subclasses load raw data into ``self._loaded_data[fold]`` (a PackedFold) and
    implement ``num_edge_types`` / ``node_feature_shape`` / ``load_data`` / ``load_data_from_list``.

    Where the reference lets subclasses add labels through _new_batch / _add_graph_to_batch / _finalise_batch, there are TWO
    hooks here.  ``_extra_graph_columns(datapoints)`` returns per-graph float32 columns (name -> [len(datapoints)]); they are
    packed with the fold, gathered per batch like ``target_value`` and handed out in ``batch_labels`` under their names.
    ``_extra_node_columns(datapoints)`` returns per-node float32 columns (name -> [sum V, W], the graphs' rows end to end);
    they travel the same way and come out as [V, W] next to the per-graph columns.  A name appears in only one of the two."""

    @classmethod
    def get_default_hyperparameters(cls) -> Dict[str, Any]:
        return {"max_nodes_per_batch": 10000}

    def __init__(self, params: Dict[str, Any], metadata: Optional[Dict[str, Any]] = None, use_worker_threads: bool = True):
        self._params = params
        self._metadata = metadata if metadata is not None else {}
        self._use_worker_threads = use_worker_threads  # accepted for the reference's signature; batches need no worker here
        self._loaded_data: Dict[DataFold, PackedFold] = {}
        self._stores: Dict[Tuple[DataFold, str], FoldStore] = {}
        self._fixed_plans: Dict[Tuple[DataFold, str], EpochPlan] = {}

    @property
    def name(self) -> str:
        return self.__class__.__name__

    @property
    def params(self) -> Dict[str, Any]:
        return self._params

    @property
    def metadata(self) -> Dict[str, Any]:
        return self._metadata

    @property
    @abstractmethod
    def num_edge_types(self) -> int:
        ...

    @property
    @abstractmethod
    def node_feature_shape(self) -> Tuple:
        ...

    @abstractmethod
    def load_data(self, path, folds_to_load: Optional[Set[DataFold]] = None) -> None:
        ...

    @abstractmethod
    def load_data_from_list(self, datapoints: List[Dict[str, Any]], target_fold: DataFold = DataFold.TEST):
        ...

    def _extra_graph_columns(self, datapoints: List[Dict[str, Any]]) -> Dict[str, np.ndarray]:
        """Per-graph float32 label columns of these raw datapoints (see the class docstring); none by default."""
        return {}

    def _extra_node_columns(self, datapoints: List[Dict[str, Any]]) -> Dict[str, np.ndarray]:
        """Per-node float32 label columns of these raw datapoints, [sum V, W] each (see the class docstring); none by default."""
        return {}

    # ---- folds --------------------------------------------------------------------------------------------------------------
    def _set_fold(self, data_fold: DataFold, fold: PackedFold) -> None:
        self._loaded_data[data_fold] = fold
        for cache in (self._stores, self._fixed_plans):
            for key in [k for k in cache if k[0] == data_fold]:
                del cache[key]

    def packed_fold(self, data_fold: DataFold) -> PackedFold:
        return self._loaded_data[data_fold]

    def fold_store(self, data_fold: DataFold, device=None) -> FoldStore:
        """The fold on the device; packed and uploaded at the first request, then kept."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        key = (data_fold, str(dev))
        if key not in self._stores:
            self._stores[key] = FoldStore(self._loaded_data[data_fold], dev)
        return self._stores[key]

    def epoch_order(self, data_fold: DataFold) -> np.ndarray:
        """The graph order of a new epoch: TRAIN draws a permutation from numpy's global generator (the reference shuffles
        with np.random.shuffle, jsonl_graph_dataset.py:142-145, so np.random.seed seeds it); the other folds keep file order."""
        n = self._loaded_data[data_fold].num_graphs
        return np.random.permutation(n) if data_fold == DataFold.TRAIN else np.arange(n)

    def plan_epoch(self, data_fold: DataFold, device=None) -> EpochPlan:
        store = self.fold_store(data_fold, device)
        if data_fold == DataFold.TRAIN:
            return EpochPlan(store, self.epoch_order(data_fold), self._params["max_nodes_per_batch"])
        key = (data_fold, str(store.device))
        plan = self._fixed_plans.get(key)
        if plan is None:
            plan = self._fixed_plans[key] = EpochPlan(store, self.epoch_order(data_fold), self._params["max_nodes_per_batch"])
        else:  # fresh flags: batches of an earlier pass may still hold theirs
            plan.bad_flags = torch.zeros(len(plan.batches), dtype=torch.int32, device=store.device)
        return plan

    # ---- batches ------------------------------------------------------------------------------------------------------------
    def _graph_iterator(self, data_fold: DataFold) -> Iterator[GraphSample]:
        """The fold's graphs as host samples, in a new epoch's order (the host route: cross-checks and tools)."""
        fold = self._loaded_data[data_fold]
        return (fold.sample(int(i)) for i in self.epoch_order(data_fold))

    def get_batches(self, data_fold: DataFold, device=None) -> _Batches:
        """Stands where the reference has get_tensorflow_dataset (graph_dataset.py:276-311): a re-iterable; every ``iter()``
        starts a new epoch of ``(batch_features, batch_labels)`` with the reference's keys - device tensors node_features,
        node_to_graph_map, adjacency_list_<i> (int32 [E, 2]) and the label columns (float32 [G]; node columns [V, W]), a Python int
        num_graphs_in_batch, and the ``_bad_local_index`` flag that ``check_batch`` reads."""
        return _Batches(self, data_fold, device)

    def graph_batch_iterator(self, data_fold: DataFold) -> Iterator[Tuple[Dict[str, Any], Dict[str, Any]]]:
        """graph_dataset.py:124-159: one epoch of minibatches, each the disjoint union of its graphs."""
        return iter(self.get_batches(data_fold))
