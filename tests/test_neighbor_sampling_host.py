"""Neighbour sampling as far as it goes without a device: the in-CSR of the store, the epoch planning of the sampled
route of NodeClassificationDataset and its errors, the capacity bound, and the host-side checks of tfgnn_neighbor_sample
and tfgnn_gather_node_rows through the loaded library (refused before any HIP call).  The sampler itself:
tests/test_gpu_neighbor_sample.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import neighbor_sample_reference as ref
from tests.neighbor_sample_cases import device_test_graph

ROOT = Path(__file__).resolve().parent.parent
NEW = ("tfgnn_neighbor_sample", "tfgnn_neighbor_sample_workspace_bytes", "tfgnn_gather_node_rows", "tfgnn_sample_launch_counts")


# ---- the store's in-CSR ------------------------------------------------------------------------------------------------------
def test_in_csr_against_a_brute_force_grouping():
    from tf2_gnn_amd.data import build_in_csr

    edges, in_ptr, in_src = device_test_graph()
    V = 200
    for e, ptr_ref, src_ref in zip(edges, in_ptr, in_src):
        ptr, src = build_in_csr(e, V)
        assert ptr.dtype == src.dtype == np.int32 and ptr.shape == (V + 1,) and src.shape == (len(e),)
        groups = [[] for _ in range(V)]
        for s, t in e.tolist():  # the list's order within each target
            groups[t].append(s)
        assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(g) for g in groups])]).tolist()
        assert src.tolist() == [s for g in groups for s in g]
        assert np.array_equal(ptr, ptr_ref) and np.array_equal(src, src_ref)  # the reference's builder agrees
    with pytest.raises(ValueError, match="outside the 5 nodes"):
        build_in_csr(np.array([[0, 5]]), 5)


# ---- the dataset's sampled route ----------------------------------------------------------------------------------------------
def _arrays(V=90, seed=0):
    rng = np.random.default_rng(seed)
    feats = rng.standard_normal((V, 3)).astype(np.float32)
    labels = rng.integers(0, 4, size=V)
    labels[::9] = -1
    edges = [rng.integers(0, V, size=(200, 2))]
    known = rng.permutation(np.flatnonzero(labels >= 0))
    return feats, labels, edges, {"train_idx": known[:47], "valid_idx": known[47:60], "test_idx": known[60:]}


def _dataset(**over):
    from tf2_gnn_amd.data import NodeClassificationDataset

    params = NodeClassificationDataset.get_default_hyperparameters()
    params.update(over)
    return NodeClassificationDataset(params)


def test_hyperparameter_defaults_leave_the_full_batch_route():
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.data.graph_dataset import _Batches

    ds = _dataset()
    assert {k: ds.params[k] for k in ("neighbor_fanouts", "eval_neighbor_fanouts", "seeds_per_batch", "sampling_seed")} == {
        "neighbor_fanouts": None, "eval_neighbor_fanouts": None, "seeds_per_batch": 1024, "sampling_seed": 0}
    feats, labels, edges, idx = _arrays()
    ds.load_data_from_arrays(feats, labels, edges, **idx)
    assert not ds.sampled and type(ds.get_batches(DataFold.TRAIN, "cpu")) is _Batches
    with pytest.raises(ValueError, match="full-batch"):
        ds.fanouts(DataFold.TRAIN)


def test_epoch_planning_chunks_reshuffles_train_and_keeps_validation():
    from tf2_gnn_amd.data import DataFold, batch_key, plan_seed_chunks

    assert plan_seed_chunks(47, 20) == [(0, 20), (20, 40), (40, 47)]  # the partial last chunk is kept
    assert plan_seed_chunks(40, 20) == [(0, 20), (20, 40)] and plan_seed_chunks(3, 1024) == [(0, 3)] and plan_seed_chunks(0, 8) == []
    with pytest.raises(ValueError, match="seeds_per_batch"):
        plan_seed_chunks(5, 0)
    feats, labels, edges, idx = _arrays()
    ds = _dataset(neighbor_fanouts=[3, 2], eval_neighbor_fanouts=[-1, -1], seeds_per_batch=20, sampling_seed=7)
    ds.load_data_from_arrays(feats, labels, edges, **idx)
    assert ds.sampled and ds.fanouts(DataFold.TRAIN) == [3, 2] and ds.fanouts(DataFold.VALIDATION) == ds.fanouts(DataFold.TEST) == [-1, -1]
    np.random.seed(5)
    o1, chunks, e1 = ds.plan_sampled_epoch(DataFold.TRAIN)
    o2, _, e2 = ds.plan_sampled_epoch(DataFold.TRAIN)
    assert chunks == [(0, 20), (20, 40), (40, 47)] and (e1, e2) == (0, 1)
    assert sorted(o1.tolist()) == sorted(o2.tolist()) == sorted(idx["train_idx"].tolist()) and o1.tolist() != o2.tolist()
    np.random.seed(5)
    ds._sampling_epoch = 0
    assert ds.plan_sampled_epoch(DataFold.TRAIN)[0].tolist() == o1.tolist()  # np.random.seed seeds it
    for _ in range(2):
        order, chunks, epoch = ds.plan_sampled_epoch(DataFold.VALIDATION)
        assert order.tolist() == idx["valid_idx"].tolist() and chunks == [(0, 13)] and epoch == 0
    assert ds.fanouts(DataFold.TRAIN) == [3, 2]
    # without eval fanouts the training fanouts serve every fold
    assert _dataset(neighbor_fanouts=[4]).fanouts(DataFold.TEST) == [4]
    keys = {batch_key(s, e, b) for s in (0, 1, 7) for e in range(5) for b in range(6)}
    assert len(keys) == 90 and all(0 <= k < 2 ** 64 for k in keys)
    assert batch_key(7, 3, 2) == (7 << 40) | (3 << 20) | 2


def test_sampled_route_errors():
    from tf2_gnn_amd.data import DataFold, NeighborStore

    feats, labels, edges, idx = _arrays()
    graph_id = np.repeat([0, 1], [50, 40])
    inside = [np.concatenate([np.random.default_rng(0).integers(0, 50, size=(30, 2)), np.random.default_rng(1).integers(50, 90, size=(30, 2))])]
    _dataset().load_data_from_arrays(feats, labels, inside, node_graph_id=graph_id, **idx)  # fine without fanouts
    with pytest.raises(ValueError, match="needs a single graph"):
        _dataset(neighbor_fanouts=[2]).load_data_from_arrays(feats, labels, inside, node_graph_id=graph_id, **idx)
    repeated = dict(idx, valid_idx=np.concatenate([idx["valid_idx"], idx["valid_idx"][:1]]))
    _dataset().load_data_from_arrays(feats, labels, edges, **repeated)  # fine without fanouts
    with pytest.raises(ValueError, match="VALIDATION indices repeat a node"):
        _dataset(neighbor_fanouts=[2]).load_data_from_arrays(feats, labels, edges, **repeated)
    for bad in ([], [1] * 9):
        ds = _dataset(neighbor_fanouts=bad)
        ds.load_data_from_arrays(feats, labels, edges, **idx)
        with pytest.raises(ValueError, match="1 to 8 fanouts"):
            ds.fanouts(DataFold.TRAIN)
    two = _dataset()
    two.load_data_from_arrays(feats, labels, inside, node_graph_id=graph_id, **idx)
    with pytest.raises(ValueError, match="fold of one graph"):
        NeighborStore(two.packed_fold(DataFold.TRAIN), "cpu")


def test_capacity_bound_holds_on_50_random_cases():
    from tf2_gnn_amd.ops import sample_capacities

    rng = np.random.default_rng(12)
    tight = 0
    for case in range(50):
        V = int(rng.integers(5, 120))
        L = int(rng.integers(1, 4))
        edges = [rng.integers(0, V, size=(int(rng.integers(0, 6 * V)), 2)) for _ in range(L)]
        if case % 5 == 0:  # a hub
            edges[0] = np.concatenate([edges[0], np.stack([rng.integers(0, V, size=3 * V), np.zeros(3 * V, dtype=np.int64)], axis=1)])
        csr = [ref.build_in_csr(e, V) for e in edges]
        K = int(rng.integers(1, 4))
        fanouts = [int(rng.choice([-1, 0, 1, 2, 5])) for _ in range(K)]
        S = int(rng.integers(1, min(V, 20) + 1))
        seeds = rng.choice(V, size=S, replace=False)
        s = ref.neighbor_sample([c[0] for c in csr], [c[1] for c in csr], seeds, fanouts, seed=case)
        node_cap, edge_cap = sample_capacities(S, fanouts, V, [len(e) for e in edges], [int(np.diff(c[0]).max()) for c in csr])
        assert S <= node_cap <= V and len(s.nodes) <= node_cap
        for t in range(L):
            assert len(s.adjacency_lists[t]) <= edge_cap[t] <= len(edges[t])
        tight += node_cap < V
    assert tight >= 5  # the bound is not always just V


# ---- the C entries ------------------------------------------------------------------------------------------------------------
def _declared(header, struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header, flags=re.S).group(1)
    return [name for decl in body.split(";") for name in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]


def test_symbols_structs_and_abi():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    declared = set(re.findall(r"\b(tfgnn_\w+)\s*\(", header))
    assert len(declared) > 100 and set(NEW) <= declared
    for name in sorted(declared):  # the library still exports every declared symbol
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in text
    assert _declared(header, "tfgnn_neighbor_sample_args") == [f[0] for f in _lib.NeighborSampleArgs._fields_]
    assert _declared(header, "tfgnn_gather_node_rows_args") == [f[0] for f in _lib.GatherNodeRowsArgs._fields_]
    assert _declared(header, "tfgnn_batch_assemble_args") == [f[0] for f in _lib.BatchAssembleArgs._fields_]  # untouched
    # LP64: every field is 8 bytes but the ints, which pair up or are padded
    assert ctypes.sizeof(_lib.NeighborSampleArgs) == 8 * 17 and ctypes.sizeof(_lib.GatherNodeRowsArgs) == 8 * 14
    macros = {"TFGNN_SAMPLE_MAX_HOPS": _lib.SAMPLE_MAX_HOPS, "TFGNN_SAMPLE_META_STATUS": _lib.SAMPLE_META_STATUS,
              "TFGNN_SAMPLE_META_NODES": _lib.SAMPLE_META_NODES, "TFGNN_SAMPLE_META_EDGES": _lib.SAMPLE_META_EDGES,
              "TFGNN_SAMPLE_NODE_OVERFLOW": _lib.SAMPLE_NODE_OVERFLOW, "TFGNN_SAMPLE_EDGE_OVERFLOW": _lib.SAMPLE_EDGE_OVERFLOW,
              "TFGNN_SAMPLE_REPEATED_SEED": _lib.SAMPLE_REPEATED_SEED, "TFGNN_SAMPLE_BAD_SEED": _lib.SAMPLE_BAD_SEED,
              "TFGNN_SAMPLE_BAD_STORE": _lib.SAMPLE_BAD_STORE}
    for macro, value in macros.items():
        m = re.search(r"#define %s (\d+)" % macro, header)
        assert m and int(m.group(1)) == value, macro
    assert "#define TFGNN_SAMPLE_META_WORDS(L, K) (2 + (L) + (K) + 2)" in header and _lib.sample_meta_words(3, 2) == 9


def _sample_args(L=2, K=2, **over):
    """A well-formed struct whose device pointers are made-up addresses: the host-side checks never read them."""
    from tf2_gnn_amd import _lib

    a = _lib.NeighborSampleArgs()
    a.struct_size = ctypes.sizeof(_lib.NeighborSampleArgs)
    a.num_edge_types, a.num_hops, a.num_nodes = L, K, 1000
    keep = {
        "in_ptr": (ctypes.c_void_p * 4)(0x1000, 0x2000, 0x3000, 0x4000),
        "in_src": (ctypes.c_void_p * 4)(0x5000, 0x6000, 0x7000, 0x8000),
        "store_edges": (ctypes.c_int64 * 4)(50, 60, 70, 80),
        "fanouts": (ctypes.c_int32 * 8)(3, 2, 1, 1, 1, 1, 1, 1),
        "edge_capacity": (ctypes.c_int64 * 4)(40, 40, 40, 40),
        "adjacency_lists": (ctypes.c_void_p * 4)(0xD000, 0xE000, 0xF000, 0x10000),
    }
    for k, v in keep.items():
        setattr(a, k, ctypes.addressof(v))
    a.seed, a.num_seeds, a.node_capacity = 1, 8, 100
    for k in ("seeds", "nodes", "meta", "workspace"):
        setattr(a, k, 0x20000)
    a.workspace_bytes = 1 << 20
    for k, v in over.items():
        if isinstance(v, ctypes.Array):
            keep[k] = v
            v = ctypes.addressof(v)
        setattr(a, k, v)
    return a, keep


def test_neighbor_sample_rejections_before_any_hip_call():
    from tf2_gnn_amd import _lib

    lib = _lib.load()

    def refused(match, status=-1, **over):
        a, keep = _sample_args(**over)
        assert lib.tfgnn_neighbor_sample(ctypes.byref(a), None) == status, over
        assert match in lib.tfgnn_last_error(), (over, lib.tfgnn_last_error())

    assert lib.tfgnn_neighbor_sample(None, None) == -1 and b"struct_size" in lib.tfgnn_last_error()
    refused(b"struct_size", struct_size=ctypes.sizeof(_lib.NeighborSampleArgs) - 8)
    refused(b"struct_size", struct_size=0)
    for K in (0, -1, 9):
        refused(b"num_hops", K=K)
    for S in (0, -5):
        refused(b"at least one seed", num_seeds=S)
    refused(b"2^31 or more nodes", num_nodes=2 ** 31)
    refused(b"negative size", num_nodes=-1)
    refused(b"negative size", L=-1)
    refused(b"at most 48 edge types", status=-4, L=49)
    refused(b"negative capacity", node_capacity=-1)
    refused(b"negative capacity", edge_capacity=(ctypes.c_int64 * 2)(5, -1))
    refused(b"negative size", store_edges=(ctypes.c_int64 * 2)(5, -1))
    refused(b"2^31 or more edges", store_edges=(ctypes.c_int64 * 2)(2 ** 30, 2 ** 30))
    refused(b"node capacity", node_capacity=7)  # below the 8 seeds
    refused(b"node capacity", node_capacity=1001)  # above V
    for name in ("fanouts", "seeds", "nodes", "meta", "workspace", "in_ptr", "adjacency_lists"):
        refused(b"NULL", **{name: None})
    refused(b"NULL", in_ptr=(ctypes.c_void_p * 2)(0x1000, None))
    refused(b"8-byte aligned", adjacency_lists=(ctypes.c_void_p * 2)(0xD000, 0xE004))
    need = lib.tfgnn_neighbor_sample_workspace_bytes(1000, 2, 100)
    assert need >= 4 * (1000 + 2 * 100) and need % 16 == 0
    refused(b"workspace", workspace_bytes=need - 1)
    refused(b"workspace", workspace=0x20004)
    assert lib.tfgnn_neighbor_sample_workspace_bytes(2 ** 31, 2, 100) == 0 and lib.tfgnn_neighbor_sample_workspace_bytes(10, 49, 5) == 0
    assert lib.tfgnn_neighbor_sample_workspace_bytes(10, 2, 11) == 0 and lib.tfgnn_neighbor_sample_workspace_bytes(10, 2, -1) == 0
    with pytest.raises(ValueError, match="num_hops"):
        _lib.check(lib.tfgnn_neighbor_sample(ctypes.byref(_sample_args(K=0)[0]), None))


def _gather_args(NC=2, **over):
    from tf2_gnn_amd import _lib

    a = _lib.GatherNodeRowsArgs()
    a.struct_size = ctypes.sizeof(_lib.GatherNodeRowsArgs)
    a.store_nodes, a.num_rows, a.num_seeds, a.feature_dim, a.num_node_columns = 1000, 50, 8, 12, NC
    keep = {
        "node_column_widths": (ctypes.c_int64 * 5)(1, 1, 1, 1, 1),
        "node_columns": (ctypes.c_void_p * 5)(0x1000, 0x2000, 0x3000, 0x4000, 0x5000),
        "node_column_out": (ctypes.c_void_p * 5)(0x6000, 0x7000, 0x8000, 0x9000, 0xA000),
        "seed_only": (ctypes.c_int32 * 5)(0, 1, 0, 0, 0),
    }
    for k, v in keep.items():
        setattr(a, k, ctypes.addressof(v))
    for k in ("nodes", "features", "node_features", "bad_flag"):
        setattr(a, k, 0x20000)
    for k, v in over.items():
        if isinstance(v, ctypes.Array):
            keep[k] = v
            v = ctypes.addressof(v)
        setattr(a, k, v)
    return a, keep


def test_gather_node_rows_rejections_before_any_hip_call():
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()

    def refused(match, status=-1, **over):
        a, keep = _gather_args(**over)
        assert lib.tfgnn_gather_node_rows(ctypes.byref(a), None) == status, over
        assert match in lib.tfgnn_last_error(), (over, lib.tfgnn_last_error())

    assert lib.tfgnn_gather_node_rows(None, None) == -1 and b"struct_size" in lib.tfgnn_last_error()
    refused(b"struct_size", struct_size=ctypes.sizeof(_lib.GatherNodeRowsArgs) + 8)
    for name in ("store_nodes", "num_rows", "num_seeds", "NC"):
        refused(b"negative size", **{name: -1})
    refused(b"2^31 or more nodes", store_nodes=2 ** 31)
    refused(b"2^31 or more nodes", num_rows=2 ** 31)
    for F in (0, -2, 2 ** 31):
        refused(b"feature_dim", feature_dim=F)
    refused(b"at most 4 node columns", status=-4, NC=5)
    for name in ("node_column_widths", "node_columns", "node_column_out", "seed_only"):
        refused(b"NULL pointer table", **{name: None})
    refused(b"node column width", node_column_widths=(ctypes.c_int64 * 2)(3, 0))
    for name in ("nodes", "features", "node_features"):
        refused(b"NULL pointer", **{name: None})
    refused(b"NULL pointer", node_columns=(ctypes.c_void_p * 2)(0x1000, None))
    a, keep = _gather_args(num_rows=0, nodes=None, features=None, node_features=None)  # nothing to do: no launch, no pointer needed
    before = ops.sample_launch_counts()
    assert lib.tfgnn_gather_node_rows(ctypes.byref(a), None) == 0
    assert ops.sample_launch_counts() == before
    assert lib.tfgnn_sample_launch_counts(None, 1) == -1


def test_ops_wrappers_refuse_cpu_tensors():
    import torch

    from tf2_gnn_amd import ops

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.neighbor_sample(None, torch.zeros(3, dtype=torch.int32), [2], 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_node_rows(torch.zeros(3, dtype=torch.int32), 1, torch.zeros(5, 2))
