"""Transductive link prediction: one graph, typed edges, and folds that are sets of true triples (source, relation, target)
over the SAME node set (FB15k / WN18 style, the second experiment of the R-GCN paper).  The reference has no such dataset.

A data directory holds numpy files only:
  ``node_features.npy`` [V, F] - optional: without it the dataset is FEATURELESS (knowledge-graph entities have no features;
  ``node_feature_shape`` is (0,), a batch's ``node_features`` a float32 [V, 0], and a task model needs the hyper-parameter
  ``node_embedding_dim``, tasks.py), with V from the optional scalar ``num_nodes.npy``, else the largest node id in any edge
  file plus one;
  ``edges.npy`` [E, 2] (one forward edge type) or ``edges_0.npy``, ``edges_1.npy``, ... (one file per forward edge type),
  (source, target) pairs: the message-passing graph, and at the same time the TRAIN positives;
  ``valid_edges_<t>.npy`` / ``test_edges_<t>.npy`` (``valid_edges.npy`` / ``test_edges.npy`` with a single type): the
  positives of the other two folds; a missing file of a loaded fold stands for no edge of that type.

A triple's relation is its FORWARD edge type: ``num_relations`` is the number of ``edges`` files, whatever backward and
self-loop types message passing adds.  TRAIN positives are edges of the message-passing graph, as in the R-GCN paper: no
edge is held out of the graph while its score is trained.

Every fold is the whole graph and ONE batch (a ``max_nodes_per_batch`` below the node count raises ValueError); the graph
part of a batch comes out of tfgnn_batch_assemble like every dataset's: one launch up to 48 processed edge types, one per
48 beyond (238 types: five).  On top, a batch carries, in
``batch_labels`` and - the same tensors - in ``batch_features``:
  ``triples`` int32 [N, 3]: the fold's P positives followed by ``num_negatives_per_positive`` negatives per positive;
  ``triple_labels`` float32 [N] (1 / 0), ``triple_weights`` float32 [N] (1);
  ``triple_tables``: the four int32 tables of ops.build_triple_tables for these triples;
and in ``batch_labels`` alone what ``LinkPredictionTask.evaluate_model`` ranks: ``positive_triples`` int32 [P, 3] and
``rank_filters`` = {"dst": (offsets, ids), "src": (offsets, ids)}, per positive the sorted entities that make a KNOWN true
triple in the corrupted slot - known: a positive of any loaded fold.

A negative copies its positive and replaces the source or the target - a fair coin - with a node drawn uniformly from the
other V - 1 nodes, so exactly one slot differs; it is not filtered against the known triples.  TRAIN draws its negatives
anew from numpy's global generator at every ``iter()`` (where the other datasets draw the epoch's graph order, so
np.random.seed seeds it), rebuilds the tables on the host and copies everything IN PLACE into the same device buffers - N is
fixed - so a CapturedStep of a training step follows.  VALIDATION and TEST draw once, from a fixed seed.

``negative_sampling`` = "host" (the default, and what an absent key means) is the paragraph above.  With "device" the
positives are uploaded once and everything after happens on the device: ``triple_batch`` draws the negatives with
ops.draw_negative_triples (the dropout mask generator's numbers, include/tfgnn.h tfgnn_triples_draw_negatives - not numpy's,
so the two routes draw different negatives of the same distribution) and builds the tables with
ops.build_triple_tables_device; the relation tables are built once, since a negative keeps its relation.  VALIDATION and TEST
draw once from their fixed seed with the dropout epoch ignored.  A TRAIN batch additionally carries
``batch_features["triple_sampler"]`` (a ``DeviceTripleSampler``), whose ``redraw()`` LinkPredictionTask calls at the start of
every training step's task part: the draw and the node tables, in place, on the current stream, no allocation and no host
synchronisation.  Such a sampled batch IS capturable: a CapturedStep of ``_run_step(features, labels, training=True)`` trains
on new negatives at every ``replay()`` - the draw follows the dropout epoch word the captured step advances - with no
``next(iter(train))`` in between.  The draw's 64-bit seed is (``negative_sampling_seed`` << 32) | (draws & 0xFFFFFFFF),
``draws`` counting the sampler's ``redraw()`` calls on the host: eager steps differ through the counter, replays of one
captured step through the epoch word.

Mini-batches.  Three hyper-parameters, read with ``.get`` and in no defaults dictionary: ``neighbor_fanouts`` (absent or None:
everything above, untouched; a list of 1 .. SAMPLE_MAX_HOPS fanouts, one per hop, -1 for every in-edge: the route below; it
needs ``negative_sampling`` = "device" - ValueError otherwise), ``triples_per_batch`` (absent: 1024; >= 1) and
``sampling_seed`` (absent: 0).  Only TRAIN is mini-batched: filtered ranking needs every entity's representation and
inference keeps no activations, so VALIDATION and TEST stay the single full-graph batch.  Every ``iter()`` of the TRAIN
batches draws a fresh np.random.permutation of the P positives (numpy's global generator, as every dataset's epoch order),
uploads it in one copy, takes the next epoch number and walks the chunks of ``plan_seed_chunks(P, triples_per_batch)``, the
partial last one included.  A batch is three steps on the device:
  ``ops.triple_batch`` (include/tfgnn.h "Triple batches", six launches): the chunk's positives, ``num_negatives_per_positive``
  negatives each - the draw of the "device" route with seed (``negative_sampling_seed`` << 32) | (batches built so far &
  0xFFFFFFFF) and the dropout epoch ignored -, their distinct endpoints in increasing id and the triples in local ids;
  ``sampled_batch`` around those endpoints with ``batch_key(sampling_seed, epoch, batch index)``: the seeds are rows 0 .. S - 1;
  ``ops.build_triple_tables_device`` on the local triples, for the batch's n nodes.
``batch_features`` holds the sampled batch's keys (node_features, adjacency_list_<t>, node_to_graph_map, num_graphs_in_batch,
num_seed_nodes, sampled_node_ids, hop_ptr, _bad_local_index) and ``triples`` - in LOCAL ids: rows of the batch -,
``triple_labels`` (B ones, B K zeros), ``triple_weights`` (ones) and ``triple_tables``; ``batch_labels`` the same four tensors
and ``global_triples`` int32 [N, 3].  No ``triple_sampler``, ``positive_triples`` or ``rank_filters``: ``evaluate_model`` on
these batches raises ValueError.  The triple buffers, the id table and the table build's workspace are allocated once for a
full chunk and reused: a batch's triple tensors are overwritten by the next batch.  Two small device-to-host copies per batch
(S, then the sampler's counts): a mini-batch, like every sampled batch, cannot be captured.  TRAIN positives stay in the
message-passing graph, as on the full-batch route, unless ``exclude_batch_positives`` (read with ``.get``, in no defaults
dictionary; absent or False: everything above, launch for launch; True without ``neighbor_fanouts``: ValueError at
construction) is True.  Then every TRAIN mini-batch's subgraph loses, for every positive (u, t, v) of the batch - rows [0, B)
of its triples; a negative is never excluded, even when it coincides with a true edge - the edges u -> v of the processed
type that carries forward relation t and the edges v -> u of its inverse type: the same list for a tied relation, the
backward type otherwise (``exclusion_type_tables``).  Self loops are never touched.  Both endpoints of a positive are seeds,
so without this the sampler hands the encoder, at hop 1, the very edge whose score is trained.  Draw first, then drop:
the sampler draws as always, ops.sample_exclude_edges (include/tfgnn.h "Excluding a batch's positives", four launches) then
takes the edges out before the counts are read back, so ``sampled_node_ids`` and ``hop_ptr`` do not change, a batch still
costs two small copies, and at a finite fanout a row may keep FEWER than f edges - nothing is drawn in their place.
``batch_features["excluded_edge_counts"]`` (device int32 [L]) counts the edges removed per list.  VALIDATION and TEST are
full-graph batches and unaffected.  The sampler's limit of 48 processed edge types stands (the NeighborStore error, raised when the data is
loaded): FB15k-237 with its 238 types stays on the full-batch route."""
from __future__ import annotations

from pathlib import Path
from typing import Any, Dict, Iterator, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from .. import ops
from .graph_dataset import DataFold, GraphDataset, PackedFold, assemble_batch
from .neighbor_sampling import (NeighborStore, batch_key, check_fanouts, check_store_limits, plan_seed_chunks,
                                sampled_batch)
from .utils import compute_number_of_edge_types, get_tied_edge_types

_EVAL_NEGATIVES_SEED = {DataFold.VALIDATION: 0x5EED0001, DataFold.TEST: 0x5EED0002}


def sample_negatives(positives: np.ndarray, num_nodes: int, per_positive: int, rng) -> np.ndarray:
    """``per_positive`` negatives for every positive, in the positives' order ([P * per_positive, 3]): a copy with the source or
    the target - a fair coin - replaced by a node drawn uniformly from the OTHER num_nodes - 1 nodes, so exactly one slot
    differs.  ``rng``: np.random or a RandomState."""
    neg = np.repeat(np.asarray(positives, dtype=np.int32).reshape(-1, 3), per_positive, axis=0)
    n = neg.shape[0]
    if n == 0:
        return neg
    if num_nodes < 2:
        raise ValueError("a negative needs a second node to put in place of the first")
    rows = np.arange(n)
    slot = np.where(rng.randint(0, 2, size=n) == 0, 0, 2)
    draw = rng.randint(0, num_nodes - 1, size=n)
    neg[rows, slot] = draw + (draw >= neg[rows, slot])
    return neg


def _filter_csr(positives: np.ndarray, known: np.ndarray, slot: int, num_nodes: int, num_relations: int):
    """per positive (u, t, v): the sorted unique entities x such that the triple with x in ``slot`` (0: source, 2: target) is
    known -> (offsets int32 [P + 1], ids int32)"""
    keep = 2 - slot  # the slot that stays
    key = lambda a: a[:, keep].astype(np.int64) * num_relations + a[:, 1].astype(np.int64)
    pairs = np.unique(np.stack([key(known), known[:, slot].astype(np.int64)], axis=1), axis=0)  # sorted by key, then entity
    starts = np.searchsorted(pairs[:, 0], key(positives), side="left")
    ends = np.searchsorted(pairs[:, 0], key(positives), side="right")
    offsets = np.zeros(len(positives) + 1, dtype=np.int64)
    np.cumsum(ends - starts, out=offsets[1:])
    take = np.repeat(starts - offsets[:-1], ends - starts) + np.arange(offsets[-1])
    return offsets.astype(np.int32), pairs[take, 1].astype(np.int32)


class DeviceTripleSampler:
    """The TRAIN negatives of the "device" route: ``redraw()`` overwrites the negatives of ``triples`` and the node tables in
    place, on the current stream (one draw launch and the node pair's table launches; capturable).  ``draws`` counts the calls
    on the host, ``seed_of_last_draw`` is the 64-bit seed the last one passed; together with the dropout epoch the kernel read
    it determines the negatives (tests/negative_sample_reference.py restates them)."""

    def __init__(self, triples: torch.Tensor, tables: Dict[str, torch.Tensor], num_positives: int, num_nodes: int,
                 num_relations: int, seed: int, workspace: torch.Tensor):
        self.triples, self.tables, self.workspace = triples, tables, workspace
        self.num_positives, self.num_nodes, self.num_relations = int(num_positives), int(num_nodes), int(num_relations)
        self.seed = int(seed)
        self.draws = 0
        self.seed_of_last_draw: Optional[int] = None

    def redraw(self) -> None:
        seed = (self.seed << 32) | (self.draws & 0xFFFFFFFF)
        ops.draw_negative_triples(self.triples, self.num_positives, self.num_nodes, seed, use_epoch=True)
        ops.build_triple_tables_device(self.triples, self.num_nodes, self.num_relations, out=self.tables, node=True, rel=False,
                                       workspace=self.workspace)
        self.seed_of_last_draw = seed
        self.draws += 1


class _LinkBatches:
    """What ``LinkPredictionDataset.get_batches`` returns: every ``iter()`` is one epoch of the fold's single batch."""

    def __init__(self, dataset: "LinkPredictionDataset", data_fold: DataFold, device=None):
        self._dataset, self._data_fold, self._device = dataset, data_fold, device

    def __iter__(self) -> Iterator[Tuple[Dict[str, Any], Dict[str, Any]]]:
        ds, fold = self._dataset, self._data_fold
        plan = ds.plan_epoch(fold, self._device)
        assert plan.batches == [(0, 1)]
        features, labels = assemble_batch(plan, 0, 1, bad_flag=plan.bad_flags[0:1])
        triple_part = ds.triple_batch(fold, plan.store.device)
        labels.update({k: v for k, v in triple_part.items() if k != "triple_sampler"})
        features.update({k: triple_part[k] for k in ("triples", "triple_labels", "triple_weights", "triple_tables", "triple_sampler")
                         if k in triple_part})
        yield features, labels


class _LinkMiniBatches:
    """What ``LinkPredictionDataset.get_batches(TRAIN)`` returns with ``neighbor_fanouts`` set: every ``iter()`` is one epoch
    of mini-batches over a fresh permutation of the positives, which goes to the device in one copy.  The triple buffers are
    the dataset's and are overwritten by the next batch."""

    def __init__(self, dataset: "LinkPredictionDataset", device=None):
        self._dataset, self._device = dataset, device

    def __iter__(self) -> Iterator[Tuple[Dict[str, Any], Dict[str, Any]]]:
        ds = self._dataset
        store = ds.neighbor_store(self._device)
        order, chunks, epoch = ds.plan_minibatch_epoch()
        ids = torch.from_numpy(order.astype(np.int32)).to(store.device)
        for b, (s, e) in enumerate(chunks):
            yield ds.minibatch(store, ids[s:e], epoch, b)


class LinkPredictionDataset(GraphDataset):
    @classmethod
    def get_default_hyperparameters(cls) -> Dict[str, Any]:
        hypers = super().get_default_hyperparameters()
        hypers.update({
            "max_nodes_per_batch": 2 ** 31 - 1,  # no graph of int32 node ids reaches it: the fold is one batch
            "add_self_loop_edges": True,
            "tie_fwd_bkwd_edges": False,
            "num_negatives_per_positive": 1,
            "negative_sampling": "host",  # or "device": negatives and tables on the device, redrawn per training step
            "negative_sampling_seed": 0,
        })
        return hypers

    @staticmethod
    def default_data_path() -> str:
        return "data/link_prediction"

    def __init__(self, params: Dict[str, Any], metadata: Optional[Dict[str, Any]] = None, **kwargs):
        super().__init__(params, metadata=metadata, **kwargs)
        self._negative_sampling = params.get("negative_sampling", "host")
        if self._negative_sampling not in ("host", "device"):
            raise ValueError(f"negative_sampling must be 'host' or 'device', not {self._negative_sampling!r}")
        seed = params.get("negative_sampling_seed", 0)
        if not isinstance(seed, (int, np.integer)) or isinstance(seed, bool) or not 0 <= seed < 2 ** 32:
            raise ValueError(f"negative_sampling_seed must be an integer in [0, 2^32), not {seed!r}")
        self._negative_sampling_seed = int(seed)
        # the mini-batch route (module docstring): keys read with .get, in no defaults dictionary
        fanouts = params.get("neighbor_fanouts")
        self._fanouts: Optional[List[int]] = None if fanouts is None else check_fanouts(fanouts)
        if self._fanouts is not None and self._negative_sampling != "device":
            raise ValueError("neighbor_fanouts needs negative_sampling = 'device': the mini-batch route draws its negatives on the "
                             f"device only, not {self._negative_sampling!r}")
        per_batch = params.get("triples_per_batch", 1024)
        if not isinstance(per_batch, (int, np.integer)) or isinstance(per_batch, bool) or per_batch < 1:
            raise ValueError(f"triples_per_batch must be an integer >= 1, not {per_batch!r}")
        self._triples_per_batch = int(per_batch)
        self._exclude_batch_positives = bool(params.get("exclude_batch_positives", False))
        if self._exclude_batch_positives and self._fanouts is None:
            raise ValueError("exclude_batch_positives needs neighbor_fanouts: only a mini-batch's sampled subgraph can lose its "
                             "positives; a full-batch fold is the whole graph")
        self._sampling_epoch = 0
        self._batches_built = 0
        self.seed_of_last_batch: Optional[int] = None
        self._neighbor_stores: Dict[str, NeighborStore] = {}
        self._minibatch_buffers: Dict[str, Dict[str, Any]] = {}
        self._num_fwd_edge_types: Optional[int] = None
        self._num_nodes = 0
        self._positives: Dict[DataFold, np.ndarray] = {}
        self._filters: Dict[DataFold, Dict[str, Tuple[np.ndarray, np.ndarray]]] = {}
        self._triple_buffers: Dict[Tuple[DataFold, str], Dict[str, Any]] = {}

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
    def num_relations(self) -> int:
        self._loaded("num_relations")
        return self._num_fwd_edge_types

    @property
    def num_nodes(self) -> int:
        self._loaded("num_nodes")
        return self._num_nodes

    @property
    def node_feature_shape(self) -> Tuple:
        self._loaded("node_feature_shape")
        some_fold = next(iter(self._loaded_data.values()))
        return (int(some_fold.features.shape[1]),)

    # ---- loading ------------------------------------------------------------------------------------------------------------
    def load_data(self, path, folds_to_load: Optional[Set[DataFold]] = None) -> None:
        data_dir = Path(path)
        if (data_dir / "edges.npy").exists():
            edges, single = [np.load(data_dir / "edges.npy")], True
        else:
            edges, single = [], False
            while (data_dir / f"edges_{len(edges)}.npy").exists():
                edges.append(np.load(data_dir / f"edges_{len(edges)}.npy"))
            if not edges:
                raise ValueError(f"{data_dir}: neither edges.npy nor edges_0.npy")

        def fold_edges(name: str):
            files = [data_dir / (f"{name}_edges.npy" if single else f"{name}_edges_{t}.npy") for t in range(len(edges))]
            if not any(f.exists() for f in files):
                raise ValueError(f"{data_dir}: no {name}_edges file")
            return [np.load(f) if f.exists() else np.zeros((0, 2), dtype=np.int64) for f in files]

        wanted = lambda fold: folds_to_load is None or fold in folds_to_load
        features_file, num_nodes_file = data_dir / "node_features.npy", data_dir / "num_nodes.npy"
        self.load_data_from_arrays(
            np.load(features_file) if features_file.exists() else None, edges,
            valid_edges=fold_edges("valid") if wanted(DataFold.VALIDATION) else None,
            test_edges=fold_edges("test") if wanted(DataFold.TEST) else None,
            load_train=wanted(DataFold.TRAIN), what=str(data_dir),
            num_nodes=np.load(num_nodes_file) if num_nodes_file.exists() else None,
        )

    def load_data_from_list(self, datapoints: List[Dict[str, Any]], target_fold: DataFold = DataFold.TEST):
        raise NotImplementedError()

    @staticmethod
    def _edge_lists(edges, num_types: Optional[int], V: int, what: str) -> List[np.ndarray]:
        if isinstance(edges, np.ndarray) and edges.ndim == 2:
            edges = [edges]
        edges = [np.asarray(e) for e in edges]
        if num_types is not None and len(edges) != num_types:
            raise ValueError(f"{what}: {len(edges)} edge lists for {num_types} forward edge types")
        for t, e in enumerate(edges):
            if e.ndim != 2 or e.shape[1] != 2 or e.dtype.kind not in "iu":
                raise ValueError(f"{what}: the edges of type {t} must be an integer [E, 2] array, not {e.dtype} {list(e.shape)}")
            if e.shape[0] and (e.min() < 0 or e.max() >= V):
                k = int(np.flatnonzero((e < 0).any(axis=1) | (e >= V).any(axis=1))[0])
                raise ValueError(f"{what}: edge {k} of type {t} ({e[k, 0]} -> {e[k, 1]}) names a node outside the {V} nodes")
        return edges

    @staticmethod
    def _as_triples(edges: Sequence[np.ndarray]) -> np.ndarray:
        parts = [np.stack([e[:, 0], np.full(e.shape[0], t), e[:, 1]], axis=1) for t, e in enumerate(edges)]
        return np.ascontiguousarray(np.concatenate(parts), dtype=np.int32)

    def load_data_from_arrays(self, node_features, edges, valid_edges=None, test_edges=None, load_train: bool = True,
                              what: str = "arrays", num_nodes=None) -> None:
        """The files of ``load_data`` as arrays.  ``edges`` / ``valid_edges`` / ``test_edges``: one [E, 2] array, or a sequence
        of them, one per forward edge type; a fold whose edges are None is not loaded.  ``node_features`` None: a featureless
        dataset of ``num_nodes`` nodes (``num_nodes.npy``, a scalar), or, without it, of the largest node id of any given edge
        array plus one; with features ``num_nodes``, if given, has to agree with them."""
        if num_nodes is not None:
            n = np.asarray(num_nodes).reshape(-1)
            if n.shape[0] != 1 or n.dtype.kind not in "iu" or int(n[0]) < 1:
                raise ValueError(f"{what}: num_nodes must be one integer >= 1, not {num_nodes!r}")
            num_nodes = int(n[0])
        if node_features is None:
            if num_nodes is None:
                every = [edges, valid_edges, test_edges]
                arrays = [np.asarray(e) for part in every if part is not None
                          for e in ([part] if isinstance(part, np.ndarray) and part.ndim == 2 else part)]
                largest = [int(e.max()) for e in arrays if e.ndim == 2 and e.shape[0] and e.dtype.kind in "iu"]
                if not largest:
                    raise ValueError(f"{what}: neither node features, nor num_nodes, nor an edge to take the node count from")
                num_nodes = max(largest) + 1
            if num_nodes >= 2 ** 31:
                raise ValueError(f"{what}: {num_nodes} nodes do not fit int32 node ids")
            feats = np.zeros((max(num_nodes, 1), 0), dtype=np.float32)
        else:
            feats = np.asarray(node_features, dtype=np.float32)
            if feats.ndim != 2 or feats.shape[0] < 1:
                raise ValueError(f"{what}: node features must be [V, F] with V >= 1, not {list(feats.shape)}")
            if num_nodes is not None and num_nodes != feats.shape[0]:
                raise ValueError(f"{what}: num_nodes = {num_nodes}, but there are features of {feats.shape[0]} nodes")
        V = feats.shape[0]
        if self.params["max_nodes_per_batch"] < V:
            raise ValueError(f"{what}: max_nodes_per_batch = {self.params['max_nodes_per_batch']} would cut the graph of {V} nodes; "
                             "a link-prediction fold is one batch")
        K = self.params["num_negatives_per_positive"]
        if not isinstance(K, (int, np.integer)) or K < 0:
            raise ValueError(f"{what}: num_negatives_per_positive must be an integer >= 0, not {K!r}")
        if V < 2 and K > 0:
            raise ValueError(f"{what}: negatives need at least two nodes")
        graph = self._edge_lists(edges, None, V, what)
        if not graph:
            raise ValueError(f"{what}: no edge type")
        T = len(graph)
        positives = {}
        if load_train:
            positives[DataFold.TRAIN] = self._as_triples(graph)
        for fold, name, e in ((DataFold.VALIDATION, "valid", valid_edges), (DataFold.TEST, "test", test_edges)):
            if e is not None:
                positives[fold] = self._as_triples(self._edge_lists(e, T, V, f"{what} ({name})"))
        for fold, p in positives.items():
            if p.shape[0] == 0:
                raise ValueError(f"{what}: the {fold.name} fold has no edge")
            if p.shape[0] * (1 + int(K)) > 2 ** 30:
                raise ValueError(f"{what}: more than 2^30 triples in the {fold.name} fold")
        base = PackedFold.from_raw_graphs(
            node_features=[feats],
            raw_adjacency_lists=[[e.astype(np.int32) for e in graph]],
            num_fwd_edge_types=T,
            add_self_loop_edges=self.params["add_self_loop_edges"],
            tied_fwd_bkwd_edge_types=get_tied_edge_types(self.params["tie_fwd_bkwd_edges"], T),
            feature_dim=int(feats.shape[1]),
        )
        if self.minibatched:  # the sampler's limit, known at load time: FB15k-237's 238 types stay on the full-batch route
            check_store_limits(base)
        self._num_fwd_edge_types, self._num_nodes = T, V
        self._positives, self._triple_buffers = positives, {}
        self._neighbor_stores, self._minibatch_buffers = {}, {}
        known = np.concatenate(list(positives.values())) if positives else np.zeros((0, 3), dtype=np.int32)
        self._filters = {fold: {"dst": _filter_csr(p, known, 2, V, T), "src": _filter_csr(p, known, 0, V, T)}
                         for fold, p in positives.items()}
        for fold in positives:  # the same host arrays for every fold
            self._set_fold(fold, base)

    # ---- triples ------------------------------------------------------------------------------------------------------------
    def positive_triples(self, data_fold: DataFold) -> np.ndarray:
        return self._positives[data_fold]

    def rank_filters(self, data_fold: DataFold) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
        return self._filters[data_fold]

    def draw_triples(self, data_fold: DataFold) -> np.ndarray:
        """positives followed by freshly drawn negatives (TRAIN: numpy's global generator; the other folds: their fixed seed)"""
        pos = self._positives[data_fold]
        rng = np.random if data_fold == DataFold.TRAIN else np.random.RandomState(_EVAL_NEGATIVES_SEED[data_fold])
        return np.concatenate([pos, sample_negatives(pos, self._num_nodes, int(self.params["num_negatives_per_positive"]), rng)])

    def triple_batch(self, data_fold: DataFold, device=None) -> Dict[str, Any]:
        """The triple part of the fold's batch on ``device`` (any torch device; the kernels need a ROCm one).  The buffers are
        allocated at the first call and kept; every call for TRAIN draws new negatives and rewrites triples and tables in
        place, the other folds are written once."""
        self._loaded("triple_batch")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        key = (data_fold, str(dev))
        buffers = self._triple_buffers.get(key)
        if buffers is not None and data_fold != DataFold.TRAIN:
            return buffers
        V, T = self._num_nodes, self._num_fwd_edge_types
        if self._negative_sampling == "device":
            if buffers is None:
                buffers = self._triple_buffers[key] = self._device_triple_buffers(data_fold, dev)
            else:  # TRAIN: new negatives and node tables, as every iter() of the host route
                buffers["triple_sampler"].redraw()
            return buffers
        triples = self.draw_triples(data_fold)
        tables = ops.build_triple_tables(triples, V, T)
        if buffers is None:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            pos = self._positives[data_fold]
            P, N = pos.shape[0], triples.shape[0]
            labels = np.zeros(N, dtype=np.float32)
            labels[:P] = 1.0
            buffers = self._triple_buffers[key] = {
                "triples": up(triples),
                "triple_labels": up(labels),
                "triple_weights": up(np.ones(N, dtype=np.float32)),
                "triple_tables": {name: up(tables[name]) for name in ops.TRIPLE_TABLE_NAMES},
                "positive_triples": up(pos),
                "rank_filters": {side: (up(off), up(ids)) for side, (off, ids) in self._filters[data_fold].items()},
            }
        else:  # the positives, labels and weights stay; the negatives and with them the tables change
            buffers["triples"].copy_(torch.from_numpy(triples))
            for name in ops.TRIPLE_TABLE_NAMES:
                buffers["triple_tables"][name].copy_(torch.from_numpy(tables[name]))
        return buffers

    def _device_triple_buffers(self, data_fold: DataFold, dev: torch.device) -> Dict[str, Any]:
        """The "device" route's buffers of a fold, first draw and all four tables included: the positives are uploaded, the
        rest is written by kernels."""
        V, T, K = self._num_nodes, self._num_fwd_edge_types, int(self.params["num_negatives_per_positive"])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        pos = self._positives[data_fold]
        P = pos.shape[0]
        N = P * (1 + K)
        triples = torch.empty((N, 3), dtype=torch.int32, device=dev)
        triples[:P].copy_(torch.from_numpy(pos))
        labels = np.zeros(N, dtype=np.float32)
        labels[:P] = 1.0
        sizes = {"node_offsets": V + 1, "node_entries": 2 * N, "rel_offsets": T + 1, "rel_order": N}
        tables = {name: torch.empty(sizes[name], dtype=torch.int32, device=dev) for name in ops.TRIPLE_TABLE_NAMES}
        workspace = ops.triple_tables_workspace(N, V, T, device=dev)
        buffers = {
            "triples": triples,
            "triple_labels": up(labels),
            "triple_weights": up(np.ones(N, dtype=np.float32)),
            "triple_tables": tables,
            "positive_triples": up(pos),
            "rank_filters": {side: (up(off), up(ids)) for side, (off, ids) in self._filters[data_fold].items()},
        }
        if data_fold == DataFold.TRAIN:
            sampler = buffers["triple_sampler"] = DeviceTripleSampler(triples, tables, P, V, T, self._negative_sampling_seed, workspace)
            sampler.redraw()
            ops.build_triple_tables_device(triples, V, T, out=tables, node=False, rel=True, workspace=workspace)  # once
        else:
            ops.draw_negative_triples(triples, P, V, _EVAL_NEGATIVES_SEED[data_fold], use_epoch=False)
            ops.build_triple_tables_device(triples, V, T, out=tables, workspace=workspace)
        return buffers

    # ---- mini-batches (TRAIN, with ``neighbor_fanouts``) --------------------------------------------------------------------
    @property
    def minibatched(self) -> bool:
        return self._fanouts is not None

    def neighbor_store(self, device=None) -> NeighborStore:
        """The TRAIN fold - the message-passing graph - in the sampler's form on the device; built at the first request."""
        self._loaded("neighbor_store")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if str(dev) not in self._neighbor_stores:
            self._neighbor_stores[str(dev)] = NeighborStore(self._loaded_data[DataFold.TRAIN], dev)
        return self._neighbor_stores[str(dev)]

    def exclusion_type_tables(self) -> Tuple[np.ndarray, np.ndarray]:
        """(fwd_type, inv_type), int32 [num_relations] each: the processed edge type that carries the forward edges of a
        relation and the one that carries their inverses, as PackedFold.from_raw_graphs lays the types out - the self loops
        first where there are any, then the forward types (a tied one holds its own inverses), then one backward type per
        untied forward type, in forward-type order."""
        self._loaded("exclusion_type_tables")
        T = self._num_fwd_edge_types
        tied = get_tied_edge_types(self.params["tie_fwd_bkwd_edges"], T)
        first = int(bool(self.params["add_self_loop_edges"]))
        untied = [t for t in range(T) if t not in tied]
        fwd = np.arange(first, first + T, dtype=np.int32)
        inv = np.array([first + t if t in tied else first + T + untied.index(t) for t in range(T)], dtype=np.int32)
        return fwd, inv

    def plan_minibatch_epoch(self) -> Tuple[np.ndarray, List[Tuple[int, int]], int]:
        """(order of the TRAIN positives, chunk ranges, epoch number) of a new epoch: a fresh permutation from numpy's global
        generator - where every dataset draws its epoch order - and the next epoch number."""
        P = self._positives[DataFold.TRAIN].shape[0]
        epoch = self._sampling_epoch
        self._sampling_epoch += 1
        return np.random.permutation(P), plan_seed_chunks(P, self._triples_per_batch), epoch

    def _minibatch_state(self, dev: torch.device) -> Dict[str, Any]:
        """What the mini-batches of one device share, allocated once at the capacity of a full chunk: the uploaded positives,
        the output buffers of ops.triple_batch, its id-table workspace and the table build's workspace."""
        state = self._minibatch_buffers.get(str(dev))
        if state is None:
            V, T, K = self._num_nodes, self._num_fwd_edge_types, int(self.params["num_negatives_per_positive"])
            pos = self._positives[DataFold.TRAIN]
            N = min(self._triples_per_batch, pos.shape[0]) * (1 + K)
            new = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
            state = self._minibatch_buffers[str(dev)] = {
                "positives": torch.from_numpy(pos).to(dev),
                "triples": new(N, 3), "local_triples": new(N, 3), "seeds": new(min(2 * N, V)),
                "id_workspace": ops.triple_batch_workspace(V, dev),
                "table_workspace": ops.triple_tables_workspace(N, V, T, device=dev),
                "labels": {},  # B -> (triple_labels, triple_weights): a full chunk's and the partial last one's
            }
        return state

    def minibatch(self, store: NeighborStore, positive_ids: torch.Tensor, epoch: int, batch_index: int):
        """One TRAIN mini-batch of the positives ``positive_ids`` (device int32 [B], B <= triples_per_batch) as
        ``(batch_features, batch_labels)``: ops.triple_batch, the sampler around its seeds, the triple tables in local ids.
        ``seed_of_last_batch`` is the 64-bit seed the negatives were drawn with (tests/triple_batch_reference.py restates
        them)."""
        state = self._minibatch_state(store.device)
        V, T, K = self._num_nodes, self._num_fwd_edge_types, int(self.params["num_negatives_per_positive"])
        B = int(positive_ids.shape[0])
        N = B * (1 + K)
        seed = (self._negative_sampling_seed << 32) | (self._batches_built & 0xFFFFFFFF)
        self._batches_built += 1
        self.seed_of_last_batch = seed
        out = (state["triples"][:N], state["local_triples"][:N], state["seeds"][:min(2 * N, V)])
        triples, local, seeds, S, status = ops.triple_batch(state["positives"], positive_ids, K, V, seed, state["id_workspace"],
                                                            out=out)
        if status:
            raise ValueError(f"building the triple batch failed with status {status} (include/tfgnn.h TFGNN_TRIPLE_BATCH_*)")
        exclude = None
        if self._exclude_batch_positives:  # rows [0, B) of the local triples are the positives; negatives are never excluded
            if "exclusion_tables" not in state:
                state["exclusion_tables"] = tuple(t.tolist() for t in self.exclusion_type_tables())
            exclude = (local[:B],) + state["exclusion_tables"]
        features, labels = sampled_batch(store, seeds, self._fanouts,
                                         batch_key(self.params.get("sampling_seed", 0), epoch, batch_index), seed_only_columns=(),
                                         exclude=exclude)
        n = int(features["sampled_node_ids"].shape[0])
        tables = ops.build_triple_tables_device(local, n, T, workspace=state["table_workspace"])
        if B not in state["labels"]:
            y = torch.zeros(N, dtype=torch.float32, device=store.device)
            y[:B] = 1.0
            state["labels"][B] = (y, torch.ones(N, dtype=torch.float32, device=store.device))
        y, w = state["labels"][B]
        triple_part = {"triples": local, "triple_labels": y, "triple_weights": w, "triple_tables": tables}
        features.update(triple_part)
        labels.update(triple_part)
        labels["global_triples"] = triples
        return features, labels

    def get_batches(self, data_fold: DataFold, device=None):
        if self.minibatched and data_fold == DataFold.TRAIN:
            return _LinkMiniBatches(self, device)
        return _LinkBatches(self, data_fold, device)
