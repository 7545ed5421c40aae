"""tfgnn_sample_exclude_edges and ``exclude_batch_positives`` of LinkPredictionDataset as far as they go without a device: the
numpy restatement on hand-worked cases, header, symbols and binding, the host-side refusals (all before any HIP call) and
the dataset's validation and type tables.  CPU-only; the kernels: tests/test_gpu_sample_exclude.py, the route:
tests/test_gpu_link_minibatch_exclude.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import sample_exclude_reference as ref

ROOT = Path(__file__).resolve().parent.parent
NEW = ("tfgnn_sample_exclude_edges", "tfgnn_sample_exclude_workspace_bytes", "tfgnn_sample_exclude_launch_counts")
UNSUPPORTED = -4  # TFGNN_ERR_UNSUPPORTED


# ---- the restatement, by hand ------------------------------------------------------------------------------------------------
def _lists():
    # three lists sorted by target: 0 the self loops, 1 a forward type, 2 its backward type
    loops = [[0, 0], [1, 1], [2, 2], [3, 3]]
    fwd = [[1, 0], [2, 0], [0, 1], [0, 1], [3, 1], [1, 2], [-1, 2], [0, 3]]  # (0, 1) twice: a multi-edge
    bwd = [[1, 0], [1, 0], [3, 0], [0, 1], [0, 2], [1, 3]]
    return [np.array(a, dtype=np.int32) for a in (loops, fwd, bwd)]


def test_restatement_hand_worked_untied():
    lists = _lists()
    # positive 0 -(r 0)-> 1: both copies of (0, 1) leave list 1 and both copies of (1, 0) leave list 2; given twice: no more
    out, removed, status = ref.exclude(lists, [[0, 0, 1], [0, 0, 1]], fwd_type=[1], inv_type=[2], num_seeds=4)
    assert status == 0 and removed.tolist() == [0, 2, 2]
    assert out[0].tolist() == lists[0].tolist()
    assert out[1].tolist() == [[1, 0], [2, 0], [3, 1], [1, 2], [-1, 2], [0, 3]]
    assert out[2].tolist() == [[3, 0], [0, 1], [0, 2], [1, 3]]
    assert all(a.dtype == np.int32 for a in out) and removed.dtype == np.int32
    # no inverse type: forward only
    out, removed, status = ref.exclude(lists, [[0, 0, 1]], fwd_type=[1], inv_type=[-1], num_seeds=4)
    assert removed.tolist() == [0, 2, 0] and out[2].tolist() == lists[2].tolist()
    # nothing matches: (2, 3) is no edge; the source -1 is never a positive's endpoint
    out, removed, status = ref.exclude(lists, [[2, 0, 3]], fwd_type=[1], inv_type=[2], num_seeds=4)
    assert status == 0 and removed.tolist() == [0, 0, 0] and all(a.tolist() == b.tolist() for a, b in zip(out, lists))


def test_restatement_hand_worked_tied_and_skipped_rows():
    tied = np.array([[1, 0], [0, 1], [1, 1], [1, 1], [2, 1], [1, 2]], dtype=np.int32)  # u -> v and v -> u in ONE list
    out, removed, status = ref.exclude([tied], [[0, 0, 1]], fwd_type=[0], inv_type=[0], num_seeds=3)
    assert status == 0 and removed.tolist() == [2] and out[0].tolist() == [[1, 1], [1, 1], [2, 1], [1, 2]]
    out, removed, status = ref.exclude([tied], [[1, 0, 1]], fwd_type=[0], inv_type=[0], num_seeds=3)  # u == v: the loops (1, 1)
    assert removed.tolist() == [2] and out[0].tolist() == [[1, 0], [0, 1], [2, 1], [1, 2]]
    # skipped rows: (-1, -1, -1) in silence; a relation of T, an endpoint >= S with their bits
    rows = [[-1, -1, -1], [0, 1, 1], [0, 0, 3], [2, 0, 1]]
    out, removed, status = ref.exclude([tied], rows, fwd_type=[0], inv_type=[0], num_seeds=3)
    assert status == ref.BAD_RELATION | ref.BAD_ENDPOINT
    assert removed.tolist() == [2] and out[0].tolist() == [[1, 0], [0, 1], [1, 1], [1, 1]]  # only (2, 0, 1) counted
    assert ref.exclude([tied], [[-1, -1, -1]], [0], [0], 3)[2] == 0
    assert ref.exclude([tied], [[0, 1, 1]], [0], [0], 3)[2] == ref.BAD_RELATION
    assert ref.exclude([tied], [[0, 0, 3]], [0], [0], 3)[2] == ref.BAD_ENDPOINT
    with pytest.raises(AssertionError, match="sorted by target"):
        ref.exclude([tied[::-1]], [[0, 0, 1]], [0], [0], 3)


# ---- entry points -----------------------------------------------------------------------------------------------------------
def _count(lib):
    buf = (ctypes.c_int64 * 2)()
    assert lib.tfgnn_sample_exclude_launch_counts(buf, 2) == 0 and buf[1] == 0
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
    assert f"#define TFGNN_SAMPLE_EXCLUDE_LAUNCHES {ref.LAUNCHES}" in header and _lib.SAMPLE_EXCLUDE_LAUNCHES == ref.LAUNCHES
    assert f"#define TFGNN_SAMPLE_EXCLUDE_BAD_RELATION {ref.BAD_RELATION}" in header
    assert f"#define TFGNN_SAMPLE_EXCLUDE_BAD_ENDPOINT {ref.BAD_ENDPOINT}" in header
    assert (_lib.SAMPLE_EXCLUDE_BAD_RELATION, _lib.SAMPLE_EXCLUDE_BAD_ENDPOINT) == (ref.BAD_RELATION, ref.BAD_ENDPOINT)
    sampler_bits = _lib.SAMPLE_NODE_OVERFLOW | _lib.SAMPLE_EDGE_OVERFLOW | _lib.SAMPLE_REPEATED_SEED | _lib.SAMPLE_BAD_SEED | _lib.SAMPLE_BAD_STORE
    assert sampler_bits & (ref.BAD_RELATION | ref.BAD_ENDPOINT) == 0  # both live in the sampler's status word
    for phrase in ("Exactly TFGNN_SAMPLE_EXCLUDE_LAUNCHES = 4 launches", "sorted by target", "Nothing is written at or beyond the OLD",
                   "An edge whose source is -1", "atomic is an OR into the status word", "tests/sample_exclude_reference.py"):
        assert phrase in text, phrase
    fields = [f for f, _ in _lib.SampleExcludeArgs._fields_]
    struct = re.search(r"typedef struct tfgnn_sample_exclude_args \{(.*?)\} tfgnn_sample_exclude_args;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+);", struct) == fields

    def ws(caps):
        tab = (ctypes.c_int64 * max(len(caps), 1))(*caps)
        return lib.tfgnn_sample_exclude_workspace_bytes(len(caps), ctypes.addressof(tab))

    # per chunk of 1024 slots 1024 packed edges of two words; one offset word per chunk plus one, rounded up to 4
    assert ws([]) == 4 * 4
    assert ws([1]) == (2048 + 4) * 4
    assert ws([1024, 1025, 0]) == (3 * 2048 + 4) * 4
    assert ws([3000] * 4) == (12 * 2048 + 16) * 4
    assert ws([-1]) == 0 and ws([2 ** 31]) == 0 and ws([2 ** 30, 2 ** 30]) == 0 and ws([0] * 49) == 0
    assert lib.tfgnn_sample_exclude_workspace_bytes(1, None) == 0
    assert lib.tfgnn_sample_exclude_launch_counts(None, 1) == -1


def test_the_call_refuses_bad_arguments_before_any_launch():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    before = _count(lib)
    # device pointers that are never dereferenced: every call below is refused before a launch
    ptrs = dict(zip(("positives", "meta", "record", "workspace"), (0x1000 * (i + 1) for i in range(4))))

    def call(struct_size=None, caps=(100, 2000, 0), fwd=(1, 2), inv=(1, -1), lists=(0x10000, 0x20000, 0x30000), **over):
        a = _lib.SampleExcludeArgs()
        a.struct_size = ctypes.sizeof(_lib.SampleExcludeArgs) if struct_size is None else struct_size
        L, T = len(caps), len(fwd)
        cap_tab = (ctypes.c_int64 * max(L, 1))(*caps)
        fwd_tab, inv_tab = (ctypes.c_int32 * max(T, 1))(*fwd), (ctypes.c_int32 * max(T, 1))(*inv)
        list_tab = (ctypes.c_void_p * max(L, 1))(*lists)
        good = (ctypes.c_int64 * 3)(100, 2000, 0)
        values = dict(num_edge_types=L, num_relations=T, num_seeds=50, num_positives=8, fwd_type=ctypes.addressof(fwd_tab),
                      inv_type=ctypes.addressof(inv_tab), edge_capacity=ctypes.addressof(cap_tab),
                      adjacency_lists=ctypes.addressof(list_tab),
                      workspace_bytes=lib.tfgnn_sample_exclude_workspace_bytes(3, ctypes.addressof(good)), **ptrs)
        values.update(over)
        for k, v in values.items():
            setattr(a, k, v)
        return lib.tfgnn_sample_exclude_edges(ctypes.byref(a), None)

    def refused(status, text, code=-1):
        assert status == code
        assert text in lib.tfgnn_last_error().decode(), lib.tfgnn_last_error()

    refused(lib.tfgnn_sample_exclude_edges(None, None), "struct_size")
    refused(call(struct_size=8), "struct_size")
    refused(call(num_edge_types=-1), "negative size")
    refused(call(num_relations=-1), "negative size")
    refused(call(num_seeds=-1), "negative size")
    refused(call(caps=(100, -1, 0)), "negative capacity")
    refused(call(num_positives=0), "empty batch")
    refused(call(num_positives=-3), "empty batch")
    refused(call(num_positives=2 ** 30 + 1), "2^30")
    refused(call(num_seeds=2 ** 31), "2^31")
    refused(call(caps=(100, 2 ** 31, 0)), "2^31")
    refused(call(caps=(2 ** 30, 2 ** 30, 0)), "2^31")
    refused(call(fwd=(1, 3)), "type table entry")
    refused(call(inv=(1, -2)), "type table entry")
    for name in list(ptrs) + ["fwd_type", "inv_type", "edge_capacity", "adjacency_lists"]:
        refused(call(**{name: None}), "NULL pointer")
    refused(call(lists=(0x10000, None, 0x30000)), "NULL pointer")
    refused(call(lists=(0x10000, 0x20004, 0x30000)), "8-byte aligned")
    refused(call(workspace_bytes=(2 * 2048 + 4) * 4), "workspace")  # three chunks are needed
    refused(call(workspace=ptrs["workspace"] + 8), "workspace")
    # more types or relations than the kernel arguments hold: TFGNN_ERR_UNSUPPORTED
    refused(call(caps=(0,) * 49, lists=(0x10000,) * 49), "at most 48", code=UNSUPPORTED)
    refused(call(fwd=(0,) * 49, inv=(0,) * 49), "at most 48", code=UNSUPPORTED)
    assert _count(lib) == before


# ---- the dataset -------------------------------------------------------------------------------------------------------------
def _dataset(**over):
    from tf2_gnn_amd.data import LinkPredictionDataset

    params = LinkPredictionDataset.get_default_hyperparameters()
    params.update(over)
    return LinkPredictionDataset(params)


def test_the_flag_needs_fanouts_and_sits_in_no_defaults():
    from tf2_gnn_amd import tasks
    from tf2_gnn_amd.data import LinkPredictionDataset

    assert "exclude_batch_positives" not in LinkPredictionDataset.get_default_hyperparameters()
    assert "exclude_batch_positives" not in tasks.LinkPredictionTask.get_default_hyperparameters("rgcn")
    with pytest.raises(ValueError, match="exclude_batch_positives needs neighbor_fanouts"):
        _dataset(exclude_batch_positives=True)
    with pytest.raises(ValueError, match="exclude_batch_positives needs neighbor_fanouts"):
        _dataset(exclude_batch_positives=True, negative_sampling="device", neighbor_fanouts=None)
    assert _dataset(exclude_batch_positives=False)._exclude_batch_positives is False
    assert _dataset()._exclude_batch_positives is False
    assert _dataset(exclude_batch_positives=True, negative_sampling="device", neighbor_fanouts=[-1])._exclude_batch_positives is True


@pytest.mark.parametrize("tie,loops", [(True, True), (False, True), (False, False), ([1], True), ([0, 2], False)])
def test_type_tables_against_the_processed_edge_lists(tie, loops):
    from tf2_gnn_amd.data import DataFold

    V, T = 40, 3
    rng = np.random.default_rng(11)
    edges = [rng.integers(0, V, size=(15 + 5 * t, 2)) for t in range(T)]
    ds = _dataset(neighbor_fanouts=[-1], negative_sampling="device", exclude_batch_positives=True, tie_fwd_bkwd_edges=tie,
                  add_self_loop_edges=loops)
    with pytest.raises(ValueError, match="loaded"):
        ds.exclusion_type_tables()
    ds.load_data_from_arrays(None, edges, num_nodes=V)
    fwd, inv = ds.exclusion_type_tables()
    assert fwd.dtype == inv.dtype == np.int32 and fwd.shape == inv.shape == (T,)
    processed = ds.packed_fold(DataFold.TRAIN).edges
    assert len(processed) == ds.num_edge_types
    tied = set(range(T)) if tie is True else set(tie or [])
    pairs = lambda a: sorted(map(tuple, np.asarray(a).tolist()))
    for t, e in enumerate(edges):
        flipped = e[:, ::-1]
        if t in tied:
            assert fwd[t] == inv[t] and pairs(processed[fwd[t]]) == pairs(np.concatenate([e, flipped]))
        else:
            assert fwd[t] != inv[t]
            assert pairs(processed[fwd[t]]) == pairs(e) and pairs(processed[inv[t]]) == pairs(flipped)
    named = set(fwd.tolist()) | set(inv.tolist())
    assert len(named) == 2 * T - len(tied)  # distinct lists
    untouched = set(range(ds.num_edge_types)) - named
    assert untouched == ({0} if loops else set())  # the self loops, and nothing else
    if loops:
        assert pairs(processed[0]) == [(i, i) for i in range(V)]
