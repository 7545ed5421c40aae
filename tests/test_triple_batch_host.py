"""tfgnn_triple_batch_build and the mini-batch route of LinkPredictionDataset as far as they go without a device: the numpy
restatement against a plain loop, header, symbols and binding, the host-side refusals (all before any launch) and the
dataset's validation.  CPU-only; the kernels: tests/test_gpu_triple_batch.py, the route: tests/test_gpu_link_prediction_minibatch.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import negative_sample_reference as nref
from tests import triple_batch_reference as ref

ROOT = Path(__file__).resolve().parent.parent
NEW = ("tfgnn_triple_batch_build", "tfgnn_triple_batch_workspace_bytes", "tfgnn_triple_batch_launch_counts")


# ---- the restatement --------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert len(a) == len(b) == 5
    for x, y in zip(a[:3], b[:3]):
        assert x.dtype == y.dtype == np.int32 and x.shape == y.shape and np.array_equal(x, y)
    assert a[3:] == b[3:]


@pytest.mark.parametrize("V,P,B,K", [(2, 1, 1, 1), (7, 5, 4, 0), (7, 5, 6, 3), (40, 30, 9, 2), (3, 8, 8, 1)])
def test_restatement_against_a_plain_loop(V, P, B, K):
    rng = np.random.default_rng(V * 1000 + B)
    pos = np.stack([rng.integers(0, V, P), rng.integers(0, 3, P), rng.integers(0, V, P)], axis=1).astype(np.int32)
    ids = rng.integers(0, P, B)  # repeats included
    N = B * (1 + K)
    full = ref.build(pos, ids, K, V, seed=99, seed_capacity=min(2 * N, V))
    _same(full, ref.build_loop(pos, ids, K, V, seed=99, seed_capacity=min(2 * N, V)))
    triples, local, seeds, S, status = full
    assert status == 0 and S == seeds.shape[0] and triples.shape == local.shape == (N, 3)
    assert np.array_equal(triples, nref.triples(pos[ids], K, V, 99, use_epoch=False))  # the draw, restated unchanged
    assert np.array_equal(seeds, np.unique(triples[:, [0, 2]])) and np.array_equal(seeds[local[:, [0, 2]]], triples[:, [0, 2]])
    assert np.array_equal(local[:, 1], triples[:, 1])
    if S > 1:  # the capacity rule: S stops at the capacity, the endpoints beyond it get -1
        cut = ref.build(pos, ids, K, V, seed=99, seed_capacity=S - 1)
        _same(cut, ref.build_loop(pos, ids, K, V, seed=99, seed_capacity=S - 1))
        assert cut[4] == ref.SEED_OVERFLOW and cut[3] == S - 1 and np.array_equal(cut[2], seeds[:S - 1])
        beyond = triples[:, [0, 2]] == seeds[S - 1]
        assert np.array_equal(cut[1][:, [0, 2]], np.where(beyond, -1, local[:, [0, 2]]))


def test_restatement_of_bad_ids_and_endpoints():
    V, K = 9, 2
    pos = np.array([[1, 0, 2], [3, 1, 12], [-4, 2, 5], [6, 0, 6]], dtype=np.int32)  # rows 1 and 2 name nodes outside [0, 9)
    ids = np.array([0, 4, 3, -1, 1, 2])  # two entries outside [0, 4)
    out = ref.build(pos, ids, K, V, seed=5, seed_capacity=V)
    _same(out, ref.build_loop(pos, ids, K, V, seed=5, seed_capacity=V))
    triples, local, seeds, S, status = out
    assert status == ref.BAD_POSITIVE_ID | ref.BAD_ENDPOINT
    B = len(ids)
    for i in (1, 3):  # the row and the rows of its negatives
        rows = [i] + [B + K * i + k for k in range(K)]
        assert (triples[rows] == -1).all() and (local[rows] == -1).all()
    assert triples[4].tolist() == [3, 1, 12] and local[4, 2] == -1 and local[4, 0] >= 0
    assert triples[5].tolist() == [-4, 2, 5] and local[5, 0] == -1 and local[5, 2] >= 0
    assert seeds.min() >= 0 and seeds.max() < V
    assert ref.build(pos[[0, 3]], [0, 1], K, V, 5, V)[4] == 0
    assert ref.batch_seed(3, 2 ** 32 + 5) == (3 << 32) | 5


# ---- entry points -----------------------------------------------------------------------------------------------------------
def _count(lib):
    buf = (ctypes.c_int64 * 2)()
    assert lib.tfgnn_triple_batch_launch_counts(buf, 2) == 0 and buf[1] == 0
    return buf[0]


def test_header_symbols_and_binding_agree():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in header
    # the contract is stated: the struct, the status bits, the table convention, the launches
    assert "typedef struct tfgnn_triple_batch_args" in header and "size_t struct_size;" in header
    for bit, value in (("SEED_OVERFLOW", 1), ("BAD_POSITIVE_ID", 2), ("BAD_ENDPOINT", 4)):
        assert f"#define TFGNN_TRIPLE_BATCH_{bit} {value}" in header
    assert (_lib.TRIPLE_BATCH_SEED_OVERFLOW, _lib.TRIPLE_BATCH_BAD_POSITIVE_ID, _lib.TRIPLE_BATCH_BAD_ENDPOINT) == (1, 2, 4)
    for phrase in ("Exactly 6 launches", "ALL -1 ON ENTRY", "LEFT ALL -1 ON EXIT", "increasing global id", "use_epoch = 0",
                   "min(2 N, V) always suffices", "tests/triple_batch_reference.py"):
        assert phrase in text, phrase
    fields = [f for f, _ in _lib.TripleBatchArgs._fields_]
    struct = re.search(r"typedef struct tfgnn_triple_batch_args \{(.*?)\} tfgnn_triple_batch_args;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+);", struct) == fields
    # the workspace: the id table [V rounded up to 4 words] and one word per chunk of 1024 ids plus one, rounded up to 4
    assert lib.tfgnn_triple_batch_workspace_bytes(1) == (4 + 4) * 4
    assert lib.tfgnn_triple_batch_workspace_bytes(1025) == (1028 + 4) * 4
    assert lib.tfgnn_triple_batch_workspace_bytes(263000) == (263000 + 260) * 4
    assert lib.tfgnn_triple_batch_workspace_bytes(0) == 0 and lib.tfgnn_triple_batch_workspace_bytes(2 ** 31) == 0
    # a sampler workspace always holds one
    assert lib.tfgnn_neighbor_sample_workspace_bytes(5000, 1, 1) >= lib.tfgnn_triple_batch_workspace_bytes(5000)
    assert lib.tfgnn_triple_batch_launch_counts(None, 1) == -1


def test_the_call_refuses_bad_arguments_before_any_launch():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    before = _count(lib)
    ptrs = dict(zip(("positives", "positive_ids", "triples", "local_triples", "seeds", "meta", "workspace"),
                    (0x1000 * (i + 1) for i in range(7))))  # never dereferenced: every call below is refused before a launch

    def call(struct_size=None, **over):
        a = _lib.TripleBatchArgs()
        a.struct_size = ctypes.sizeof(_lib.TripleBatchArgs) if struct_size is None else struct_size
        values = dict(num_nodes=50, num_positives=10, batch_size=4, negatives_per_positive=1, seed=1, seed_capacity=16,
                      workspace_bytes=lib.tfgnn_triple_batch_workspace_bytes(50), **ptrs)
        values.update(over)
        for k, v in values.items():
            setattr(a, k, v)
        return lib.tfgnn_triple_batch_build(ctypes.byref(a), None)

    def refused(status, text):
        assert status == -1
        assert text in lib.tfgnn_last_error().decode(), lib.tfgnn_last_error()

    refused(lib.tfgnn_triple_batch_build(None, None), "struct_size")
    refused(call(struct_size=8), "struct_size")
    refused(call(batch_size=0), "empty batch")
    refused(call(negatives_per_positive=-1), "negatives_per_positive")
    refused(call(batch_size=2 ** 29, negatives_per_positive=2), "2^30")
    refused(call(batch_size=2 ** 30 + 1, negatives_per_positive=0), "2^30")
    refused(call(num_positives=0), "P in [1, 2^31)")
    refused(call(num_nodes=0), "V must be in [1, 2^31)")
    refused(call(num_nodes=2 ** 31), "V must be in [1, 2^31)")
    refused(call(num_nodes=1), "second node")
    refused(call(seed_capacity=0), "seed capacity")
    for name in ptrs:
        refused(call(**{name: None}), "NULL pointer")
    refused(call(workspace_bytes=lib.tfgnn_triple_batch_workspace_bytes(50) - 4), "workspace")
    refused(call(workspace=ptrs["workspace"] + 8), "workspace")
    assert _count(lib) == before


# ---- the dataset's validation ------------------------------------------------------------------------------------------------
def _dataset(**over):
    from tf2_gnn_amd.data import LinkPredictionDataset

    params = LinkPredictionDataset.get_default_hyperparameters()
    params.update(over)
    return LinkPredictionDataset(params)


def _edges(V, types, per_type=20, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, V, size=(per_type, 2)) for _ in range(types)]


def test_dataset_validation_of_the_minibatch_keys():
    from tf2_gnn_amd import tasks
    from tf2_gnn_amd.data import DataFold, LinkPredictionDataset
    from tf2_gnn_amd.data.link_prediction_dataset import _LinkBatches, _LinkMiniBatches

    # the keys are in no defaults dictionary
    defaults = LinkPredictionDataset.get_default_hyperparameters()
    assert defaults == {"max_nodes_per_batch": 2 ** 31 - 1, "add_self_loop_edges": True, "tie_fwd_bkwd_edges": False,
                        "num_negatives_per_positive": 1, "negative_sampling": "host", "negative_sampling_seed": 0}
    task_defaults = tasks.LinkPredictionTask.get_default_hyperparameters("rgcn")
    for key in ("neighbor_fanouts", "triples_per_batch", "sampling_seed"):
        assert key not in defaults and key not in task_defaults
    with pytest.raises(ValueError, match="neighbor_fanouts"):
        _dataset(neighbor_fanouts=[2, 2])  # "host" sampling, the default
    with pytest.raises(ValueError, match="neighbor_fanouts"):
        _dataset(neighbor_fanouts=[2, 2], negative_sampling="host")
    with pytest.raises(ValueError, match="triples_per_batch"):
        _dataset(neighbor_fanouts=[2, 2], negative_sampling="device", triples_per_batch=0)
    with pytest.raises(ValueError, match="triples_per_batch"):
        _dataset(triples_per_batch=0)
    with pytest.raises(ValueError, match="fanouts"):
        _dataset(neighbor_fanouts=[], negative_sampling="device")
    with pytest.raises(ValueError, match="fanouts"):
        _dataset(neighbor_fanouts=[1] * 9, negative_sampling="device")
    # absent keys, and an explicit None: today's route
    V = 30
    for ds in (_dataset(), _dataset(negative_sampling="device"), _dataset(neighbor_fanouts=None)):
        ds.load_data_from_arrays(np.zeros((V, 2), np.float32), _edges(V, 2), valid_edges=_edges(V, 2, 5, 1))
        assert not ds.minibatched
        for fold in (DataFold.TRAIN, DataFold.VALIDATION):
            assert type(ds.get_batches(fold, "cpu")) is _LinkBatches
    # the route: TRAIN alone is mini-batched
    ds = _dataset(neighbor_fanouts=[3, -1], negative_sampling="device", triples_per_batch=16)
    ds.load_data_from_arrays(np.zeros((V, 2), np.float32), _edges(V, 2), valid_edges=_edges(V, 2, 5, 1))
    assert ds.minibatched
    assert type(ds.get_batches(DataFold.TRAIN, "cpu")) is _LinkMiniBatches and type(ds.get_batches(DataFold.VALIDATION, "cpu")) is _LinkBatches
    np.random.seed(3)
    o1, chunks, e1 = ds.plan_minibatch_epoch()
    o2, _, e2 = ds.plan_minibatch_epoch()
    assert chunks == [(0, 16), (16, 32), (32, 40)] and (e1, e2) == (0, 1)
    assert sorted(o1.tolist()) == sorted(o2.tolist()) == list(range(40)) and o1.tolist() != o2.tolist()
    np.random.seed(3)
    assert ds.plan_minibatch_epoch()[0].tolist() == o1.tolist()  # np.random.seed seeds it
    assert _dataset(neighbor_fanouts=[1], negative_sampling="device")._triples_per_batch == 1024


def test_a_49_type_fold_raises_the_neighbor_store_error():
    from tf2_gnn_amd.data import DataFold, NeighborStore

    V = 12
    edges = _edges(V, 24, per_type=3)  # 24 forward + 24 backward + self loops = 49 processed types
    ds = _dataset(neighbor_fanouts=[2], negative_sampling="device")
    with pytest.raises(ValueError, match="at most 48 edge types") as raised:
        ds.load_data_from_arrays(None, edges, num_nodes=V)
    full = _dataset(negative_sampling="device")  # the full-batch route has no such limit
    full.load_data_from_arrays(None, edges, num_nodes=V)
    assert full.num_edge_types == 49
    with pytest.raises(ValueError) as stores:
        NeighborStore(full.packed_fold(DataFold.TRAIN), "cpu")
    assert str(stores.value) == str(raised.value)  # the store's error as it stands
    ok = _dataset(neighbor_fanouts=[2], negative_sampling="device", add_self_loop_edges=False)
    ok.load_data_from_arrays(None, edges, num_nodes=V)
    assert ok.num_edge_types == 48


def test_evaluate_model_refuses_a_batch_without_rank_filters():
    import torch

    from tf2_gnn_amd import tasks

    task = tasks.LinkPredictionTask.__new__(tasks.LinkPredictionTask)
    labels = {"triples": torch.zeros((2, 3), dtype=torch.int32), "global_triples": torch.zeros((2, 3), dtype=torch.int32)}
    with pytest.raises(ValueError, match="VALIDATION or TEST"):
        task.rank_counts({}, labels)
