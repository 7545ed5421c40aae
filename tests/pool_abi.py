"""tfgnn_pool_forward / tfgnn_pool_backward called through ctypes with the argument structs filled by hand: every pointer and
leading dimension is the caller's, nothing is made contiguous on the way.  Shared by tests/test_gpu_pool_entry.py and
tests/test_gpu_pool_reference.py."""
import ctypes
import math

import torch


def _raw_forward(kind, ptr, T, S, heads, lo, hi, w=None, ws_bytes=None, struct_size=None):
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    V, GD = T.shape
    G = ptr.numel() - 1
    a = _lib.PoolForwardArgs()
    a.struct_size = ctypes.sizeof(a) if struct_size is None else struct_size
    a.kind = ops._POOL_KINDS[kind]
    a.V, a.G, a.GD, a.heads = V, G, GD, heads
    a.ptr, a.T, a.ldT = ptr.data_ptr(), T.data_ptr(), T.stride(0)
    if S is not None:
        a.S, a.ldS = S.data_ptr(), S.stride(0)
    a.lo = -math.inf if lo is None else lo
    a.hi = math.inf if hi is None else hi
    out = torch.full((G, GD), float("nan"), dtype=torch.float32, device=T.device)
    a.out = out.data_ptr()
    if w is not None:
        a.w, a.ldw = w.data_ptr(), w.stride(0)
    need = lib.tfgnn_pool_workspace_bytes(V, G, GD, heads, a.kind)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=T.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need if ws_bytes is None else ws_bytes
    _lib.check(lib.tfgnn_pool_forward(ctypes.byref(a), ops._stream()))
    return out


def _raw_backward(kind, ptr, ids, g, T, w, heads, lo, hi, dT, dS):
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    V, GD = T.shape
    G = ptr.numel() - 1
    a = _lib.PoolBackwardArgs()
    a.struct_size = ctypes.sizeof(a)
    a.kind = ops._POOL_KINDS[kind]
    a.V, a.G, a.GD, a.heads = V, G, GD, heads
    a.ptr, a.ids, a.dOut = ptr.data_ptr(), ids.data_ptr(), g.data_ptr()
    a.T, a.ldT = T.data_ptr(), T.stride(0)
    if w is not None:
        a.w, a.ldw = w.data_ptr(), w.stride(0)
    a.lo = -math.inf if lo is None else lo
    a.hi = math.inf if hi is None else hi
    a.dT, a.lddT = dT.data_ptr(), dT.stride(0)
    if dS is not None:
        a.dS, a.lddS = dS.data_ptr(), dS.stride(0)
    need = lib.tfgnn_pool_workspace_bytes(V, G, GD, heads, a.kind)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=T.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    _lib.check(lib.tfgnn_pool_backward(ctypes.byref(a), ops._stream()))
