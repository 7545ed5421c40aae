"""Graph readout entry points (include/tfgnn.h "Graph readout", csrc/pool_fused.hip), the part that needs no GPU: the three
new symbols are exported, declared and bound; the ABI number did not move; everything the header says is rejected on the host
is rejected with NULL device pointers; the no-op sizes return 0; the workspace query is monotone in V and 0 where no graph
can have been cut into chunks."""
import ctypes
import math
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = ["tfgnn_pool_forward", "tfgnn_pool_backward", "tfgnn_pool_workspace_bytes", "tfgnn_pool_launch_counts"]


def _args(struct, **over):
    from tf2_gnn_amd import _lib

    a = struct()
    a.struct_size = ctypes.sizeof(struct)
    a.kind = _lib.POOL_SOFTMAX
    a.V, a.G, a.GD, a.heads = 40, 3, 16, 4
    a.lo, a.hi = -math.inf, math.inf
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _entries():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    return lib, ((lib.tfgnn_pool_forward, _lib.PoolForwardArgs), (lib.tfgnn_pool_backward, _lib.PoolBackwardArgs))


def test_new_symbols_are_exported_declared_and_bound_and_the_abi_stays_5():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tfgnn.h").read_text(), flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5
    assert "#define TFGNN_ABI_VERSION 5" in (ROOT / "include" / "tfgnn.h").read_text()
    m = re.search(r"#define TFGNN_POOL_CHUNK_NODES (\d+)", header)
    assert m and int(m.group(1)) == _lib.POOL_CHUNK_NODES
    # the op-level entries stay
    for name in ("tfgnn_segment_softmax", "tfgnn_segment_weighted_sum", "tfgnn_segment_weighted_sum_backward",
                 "tfgnn_segment_softmax_backward", "tfgnn_clip", "tfgnn_clip_backward"):
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS


def test_struct_size_is_checked_first():
    lib, entries = _entries()
    for fn, struct in entries:
        a = _args(struct)
        a.struct_size = ctypes.sizeof(struct) - 8
        assert fn(ctypes.byref(a), None) == -1 and b"struct_size" in lib.tfgnn_last_error()
        assert fn(None, None) == -1


@pytest.mark.parametrize("over, word", [
    (dict(kind=4), b"unknown weighting kind"),
    (dict(kind=-1), b"unknown weighting kind"),
    (dict(GD=18), b"must divide"),
    (dict(heads=0), b"must divide"),
    (dict(V=-1), b"negative"),
    (dict(lo=1.0, hi=0.5), b"lower bound above"),
    (dict(lo=math.nan), b"lower bound above"),
    (dict(V=100000, workspace_bytes=64), b"workspace"),
])
def test_host_side_rejections_need_no_device_pointers(over, word):
    lib, entries = _entries()
    for fn, struct in entries:
        a = _args(struct, **over)
        assert fn(ctypes.byref(a), None) == -1, over
        assert word in lib.tfgnn_last_error(), (over, lib.tfgnn_last_error())


def test_null_pointers_are_rejected_after_the_sizes():
    lib, entries = _entries()
    for fn, struct in entries:
        assert fn(ctypes.byref(_args(struct)), None) == -1 and b"NULL pointer" in lib.tfgnn_last_error()


def test_empty_problems_are_no_ops():
    lib, entries = _entries()
    for fn, struct in entries:
        for over in (dict(V=0), dict(G=0), dict(GD=0)):
            assert fn(ctypes.byref(_args(struct, **over)), None) == 0, over


def test_too_small_workspace_raises_through_check():
    from tf2_gnn_amd import _lib

    lib, entries = _entries()
    for fn, struct in entries:
        a = _args(struct, V=100000)
        need = lib.tfgnn_pool_workspace_bytes(100000, 3, 16, 4, _lib.POOL_SOFTMAX)
        a.workspace_bytes = need - 4
        with pytest.raises(ValueError, match="workspace"):
            _lib.check(fn(ctypes.byref(a), None))


def test_workspace_query_is_monotone_and_zero_without_chunks():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    C = _lib.POOL_CHUNK_NODES
    for kind in range(4):
        for V in (0, 1, C - 1, C):
            assert lib.tfgnn_pool_workspace_bytes(V, 7, 128, 8, kind) == 0, (kind, V)
        assert lib.tfgnn_pool_workspace_bytes(10 ** 6, 0, 128, 8, kind) == 0
        last = 0
        for V in (C + 1, 2 * C, 2 * C + 1, 5000, 170000, 2 * 10 ** 6):
            b = lib.tfgnn_pool_workspace_bytes(V, 7, 128, 8, kind)
            assert b >= last and b > 0, (kind, V)
            last = b
    # two slots per tile of C nodes, each [GD] sums (+ 2 * heads statistics for the softmax)
    assert lib.tfgnn_pool_workspace_bytes(10 * C, 1, 128, 8, _lib.POOL_NONE) == 10 * 2 * 128 * 4
    assert lib.tfgnn_pool_workspace_bytes(10 * C, 1, 128, 8, _lib.POOL_SOFTMAX) == 10 * 2 * (128 + 16) * 4


def test_launch_counters_read_without_a_device():
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    buf = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    assert lib.tfgnn_pool_launch_counts(buf, 4) == 0
    assert buf[0] >= 0 and buf[1] >= 0 and buf[2] == 0 and buf[3] == 0
    assert set(ops.pool_launch_counts()) == {"pool_fwd", "pool_bwd"}
    assert lib.tfgnn_pool_launch_counts(None, 2) == -1
