"""Tensor-level wrappers over the C ABI (include/tfgnn.h).

Inputs/outputs are torch tensors living on a ROCm device; torch supplies device memory and the
current HIP stream, every FLOP and byte of the hot path runs in libtfgnn.so.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .guard import (  # noqa: F401 - the GEMM mode, its spread guard and the in-stream repair: their public names are these
    GEMM_BF16X3, GEMM_BF16X3_EXACT, GEMM_F16X2, GEMM_FP32, capturing, demote_gemm_mode, f16x2_guard_flag_async,
    f16x2_guard_tripped_sync, get_gemm_mode, guard_repair, hold_spread_guard, rearm_spread_guard, repair_stats, set_gemm_mode,
    set_guard_repair)

ACT_NONE, ACT_RELU, ACT_TANH, ACT_LEAKY_RELU, ACT_ELU, ACT_SELU, ACT_GELU, ACT_SIGMOID = range(8)
REDUCE_SUM, REDUCE_MAX = 0, 1

_ACT_BY_NAME = {
    "none": ACT_NONE,
    "relu": ACT_RELU,
    "tanh": ACT_TANH,
    "leaky_relu": ACT_LEAKY_RELU,
    "elu": ACT_ELU,
    "selu": ACT_SELU,
    "gelu": ACT_GELU,
    "sigmoid": ACT_SIGMOID,
}


def act_id(name_or_id) -> int:
    if name_or_id is None:
        return ACT_NONE
    if isinstance(name_or_id, int):
        return name_or_id
    try:
        return _ACT_BY_NAME[name_or_id.lower()]
    except KeyError:
        raise ValueError(f"Unknown activation function: {name_or_id}")


class _NullScope:
    __slots__ = ()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NULL_SCOPE = _NullScope()


def op_scope(name: str, *tensors):
    """Marks a group of library launches that is not a wrapper of this module (the attention kernels of the RGAT layer call
    the C ABI directly): ``with ops.op_scope("rgat_attention_forward", s_src, att): ...``.  Does nothing; a profiler replaces
    this function with one that brackets the region with events (bench.py step_breakdown), like it wraps the wrappers."""
    return _NULL_SCOPE


_ENV_DATA = getattr(os.environ, "_data", None)  # posix: {bytes: bytes}, the dict behind os.environ (sees every later setenv)
_ENV_KEYS = {}


def env(name: str, default: Optional[str] = None) -> Optional[str]:
    """os.environ.get for the switches the layers consult on every call: the Mapping protocol of os.environ costs ~1 us per
    lookup (129 lookups per PPI-sized step, profiles/r06_ppi_host_profile_before.txt); its backing dict a tenth of that."""
    if _ENV_DATA is None:
        return os.environ.get(name, default)
    key = _ENV_KEYS.get(name)
    if key is None:
        key = _ENV_KEYS[name] = os.fsencode(name)
    v = _ENV_DATA.get(key)
    return default if v is None else os.fsdecode(v)


_get_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_get_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """hipStream_t of torch's current stream on the current device: the launch stream of a library call.
    torch.cuda.current_stream() builds a Stream object per call (~4 us: 74 calls = 0.3 ms of the 1.5 ms a PPI-sized step
    spends on the host, profiles/r06_ppi_host_profile_before.txt); the two private accessors it is made of cost ~0.3 us."""
    if _get_raw_stream is not None and _get_device is not None:
        return _get_raw_stream(_get_device())
    return torch.cuda.current_stream().cuda_stream


# ---- small passes that share a launch (include/tfgnn.h tfgnn_aux_launch) ---------------------------------------------------------
# The weight splits of a pass are built as jobs (``sp_split_rows_jobs`` / ``sp_split_cols_jobs``: allocate the operand, fill the
# job, launch nothing) and launched by whoever built them, at once: ``sp_weight_operand`` launches the one split it needs,
# ``presplit_weight_operands`` all stale operands of a pass together.  Nothing is queued between calls.
class SplitJobs:
    """A split operand that is still to be written: ``operand`` (allocated, empty), the jobs that write it - ``stage0``, then
    ``stage1`` in a launch after it (the conversion behind the column maxima of a two-pass weight split) - and ``keep``, the
    tensors the jobs read or write, to be held until ``aux_flush`` has launched them."""

    __slots__ = ("operand", "stage0", "stage1", "keep")

    def __init__(self, operand, stage0=(), stage1=(), keep=()):
        self.operand, self.stage0, self.stage1, self.keep = operand, stage0, stage1, keep


def aux_flush(batch) -> None:
    """Launch a sequence of ``SplitJobs`` on the current stream: the stage-0 jobs of all of them in one tfgnn_aux_launch, then
    the stage-1 jobs in a second one; empty jobs (kind 0, or no blocks) are skipped.  Returns when both launches have been
    issued.  (The module-level name is part of what bench.py measures: its step breakdown looks ``aux_flush`` up to attribute
    the launches at the start of a pass.)"""
    stream = _stream()
    for stage in ("stage0", "stage1"):
        live = [j for sj in batch for j in getattr(sj, stage) if j.kind != 0 and j.num_blocks != 0]
        if live:
            jobs = (_lib.AuxJob * len(live))(*live)
            _lib.check(_lib.load().tfgnn_aux_launch(jobs, len(jobs), stream))


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _require_dev(t: torch.Tensor, dtype, what: str):
    if not t.is_cuda:
        raise RuntimeError(
            f"tf2_gnn_amd: {what} must live on a ROCm device (got {t.device}); there is no CPU fallback"
        )
    if t.dtype != dtype:
        raise TypeError(f"tf2_gnn_amd: {what} must be {dtype}, got {t.dtype}")


def _rowmajor(t: torch.Tensor, what: str):
    """2-D tensor with unit inner stride -> (tensor, leading dimension)."""
    if t.dim() != 2:
        raise ValueError(f"{what} must be 2-D, got shape {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        t = t.contiguous()
    ld = t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)
    if ld < t.shape[1]:
        t = t.contiguous()
        ld = max(t.shape[1], 1)
    return t, ld


def _writes_out(fn):
    """The kernels write caller-provided ``out`` tensors through raw pointers, which torch does not see: bump the tensor's
    version counter so that everything keyed on (tensor, version) - the remembered split forms of ``sp_rows_of``, the
    split weight operands, the Graph cache - notices the new contents."""
    import functools

    import inspect

    try:
        out_pos = list(inspect.signature(fn).parameters).index("out")
    except ValueError:
        out_pos = None

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        res = fn(*args, **kwargs)
        out = kwargs.get("out")
        if out is None and out_pos is not None and len(args) > out_pos:  # ``out`` passed positionally
            out = args[out_pos]
        if isinstance(out, torch.Tensor):
            torch.autograd.graph.increment_version(out)
        return res

    return wrapper


class _DevArray:
    """Zero-copy view of a device array owned by the C library (``__cuda_array_interface__``)."""

    def __init__(self, ptr: int, count: int, typestr: str, owner):
        self._owner = owner
        self.__cuda_array_interface__ = {
            "shape": (count,),
            "typestr": typestr,
            "data": (ptr, False),
            "version": 2,
            "strides": None,
        }


# graph array ids (include/tfgnn.h tfgnn_graph_array_id)
(G_ROWPTR_BY_DST, G_COL_BY_DST, G_EID_BY_DST, G_COLL_BY_DST, G_ROWPTR_BY_SRC, G_COL_BY_SRC, G_EID_BY_SRC,
 G_COLL_BY_SRC, G_INVDEG_BY_DST, G_INVDEG_EDGE_BY_SRC, G_NODEPTR_BY_DST, G_NODEPTR_BY_SRC,
 G_INVDEG_EDGE_BY_DST, G_SRC2DST_POS, G_TARGET_BY_DST, G_NZ_CPOS_BY_DST, G_NZ_ROW_BY_DST, G_NZ_NODE_BY_DST,
 G_NZ_OFF_BY_DST, G_NZ_NODEPTR_BY_DST, G_NZ_COL_BY_DST, G_NZ_CPOS_BY_SRC, G_NZ_ROW_BY_SRC, G_NZ_NODE_BY_SRC,
 G_NZ_OFF_BY_SRC, G_NZ_NODEPTR_BY_SRC, G_NZ_COL_BY_SRC, G_PATTERN_POS_BY_DST, G_PATTERN_NODE_BY_DST,
 G_PATTERN_TILEMASK_BY_DST, G_PATTERN_NODE_BY_SRC, G_PATTERN_TILEMASK_BY_SRC) = range(32)
G_GATHER_ARRIVALS_VIEW0 = 32  # + view (0 - 3): the arrival counters of the gathers over that view (debugging aid; all zero at rest)
_FLOAT_ARRAYS = {G_INVDEG_BY_DST, G_INVDEG_EDGE_BY_SRC, G_INVDEG_EDGE_BY_DST}
_BYTE_ARRAYS = {G_PATTERN_TILEMASK_BY_DST, G_PATTERN_TILEMASK_BY_SRC}
# parts of a graph handle beyond the two sorted edge orders (include/tfgnn.h tfgnn_graph_part)
G_PART_PLAN_TYPED, G_PART_PLAN_NODE, G_PART_COMPACT, G_PART_EDGE_MAPS, G_PART_EDGE_IDS, G_PART_DST_PATTERN, G_PARTS_ALL = 1, 2, 4, 8, 16, 32, 63
G_PARTS_DEFAULT = G_PARTS_ALL & ~G_PART_DST_PATTERN  # the pattern order is built for the layers that ask for it
_VIEW_PARTS = {0: G_PART_PLAN_TYPED, 1: G_PART_PLAN_NODE, 2: G_PART_PLAN_TYPED, 3: G_PART_PLAN_NODE,
               4: G_PART_PLAN_TYPED | G_PART_COMPACT, 5: G_PART_PLAN_TYPED | G_PART_COMPACT,
               6: G_PART_PLAN_TYPED | G_PART_DST_PATTERN, 7: G_PART_PLAN_TYPED | G_PART_DST_PATTERN}


def _array_parts(array_id: int) -> int:
    if array_id == G_SRC2DST_POS:
        return G_PART_EDGE_MAPS | G_PART_EDGE_IDS
    if array_id in (G_EID_BY_DST, G_EID_BY_SRC):
        return G_PART_EDGE_IDS
    if G_PATTERN_POS_BY_DST <= array_id <= G_PATTERN_TILEMASK_BY_SRC:
        return G_PART_DST_PATTERN
    if G_GATHER_ARRIVALS_VIEW0 <= array_id <= G_GATHER_ARRIVALS_VIEW0 + 3:
        return _VIEW_PARTS[array_id - G_GATHER_ARRIVALS_VIEW0]
    return G_PART_COMPACT if G_NZ_CPOS_BY_DST <= array_id <= G_NZ_COL_BY_SRC else 0


_OPERAND_EPOCH = [0]


def gather_operands_touched() -> None:
    """Every graph-owned gather operand counts as unfilled from here on (its next gather writes every row).  ``CapturedStep``
    calls it around a capture and at every replay: the first gather of each direction INSIDE the captured sequence then writes
    the empty rows itself, and eager calls never rely on what a replay left behind."""
    _OPERAND_EPOCH[0] += 1


class _GatherOperand:
    """A graph-owned SP16 gather operand (``Graph.gather_operand``).  ``filled``: None, or what the last gather that wrote
    EVERY row of the pair ran with - (the row_scale tensor | None, its version, inside a capture?, the operand epoch); a
    gather whose own description equals it may leave the empty buckets' rows alone (include/tfgnn.h,
    tfgnn_graph_gather_reduce_sp_keep_empty)."""

    __slots__ = ("data", "inv_scale", "filled")

    def __init__(self, data: torch.Tensor, inv_scale: torch.Tensor):
        self.data, self.inv_scale, self.filled = data, inv_scale, None

    def _description(self, row_scale: Optional[torch.Tensor]):
        return (row_scale, row_scale._version if row_scale is not None else 0, capturing(), _OPERAND_EPOCH[0])

    def begin(self, row_scale: Optional[torch.Tensor]) -> bool:
        """-> may the gather about to run keep the empty rows?  Marks the pair unfilled until ``done`` (a call that fails
        leaves it so)."""
        rec, self.filled = self.filled, None
        if rec is None:
            return False
        t, version, in_capture, epoch = rec
        if in_capture != capturing() or epoch != _OPERAND_EPOCH[0]:
            return False
        if t is None or row_scale is None:
            return t is None and row_scale is None
        # the same values: the same memory (the record keeps its tensor alive, so the address cannot have been handed out
        # again) that nothing has written since - in-place writes, also the library's through raw pointers, raise the version
        same = t is row_scale or (t.data_ptr() == row_scale.data_ptr() and t.shape == row_scale.shape
                                  and t.stride() == row_scale.stride() and t.dtype == row_scale.dtype)
        return same and t._version == version and row_scale._version == version

    def done(self, row_scale: Optional[torch.Tensor]) -> None:
        self.filled = self._description(row_scale)


class Graph:
    """Edge-bucketed adjacency of one batch (``tfgnn_graph``); build once, reuse for every layer
    and for forward + backward.  ``adjacency_lists``: sequence of int32 device tensors [E_l, 2]
    with rows (source, target), exactly ``GNNInput.adjacency_lists`` (layers/gnn.py:241-244)."""

    def __init__(self, adjacency_lists: Sequence[torch.Tensor], num_nodes: int, wait: bool = True, parts: int = G_PARTS_DEFAULT):
        """wait=False: the build is only enqueued on the current stream (pipelining the next batch's
        bucketing behind the current step, like the reference's prefetching input pipeline); call
        ``wait()`` - and order the consuming stream after the build stream - before using it.
        parts: which derived tables to build now (G_PART_*; ``GNN.graph_parts`` names what a layer stack reads); a part that
        turns out to be missing is built on first use (``ensure``: correct, but it blocks the host once)."""
        lib = _lib.load()
        adjs = []
        for i, a in enumerate(adjacency_lists):
            _require_dev(a, torch.int32, f"adjacency_lists[{i}]")
            if a.dim() != 2 or a.shape[1] != 2:
                if a.numel() == 0:
                    a = a.reshape(0, 2)
                else:
                    raise ValueError(f"adjacency_lists[{i}] must have shape [E, 2], got {tuple(a.shape)}")
            adjs.append(a.contiguous())
        self._keep = adjs  # the edge lists must stay alive until the build has run
        L = len(adjs)
        ptrs = (ctypes.c_void_p * max(L, 1))(*[a.data_ptr() if a.numel() else None for a in adjs])
        counts = (ctypes.c_int64 * max(L, 1))(*[a.shape[0] for a in adjs])
        handle = ctypes.c_void_p()
        self._h = None
        _lib.check(
            lib.tfgnn_graph_create_parts_async(L, int(num_nodes), ptrs, counts, int(parts) & G_PARTS_ALL, _stream(),
                                               ctypes.byref(handle))
        )
        self._h = handle
        self.parts = int(parts) & G_PARTS_ALL
        if self.parts & G_PART_EDGE_MAPS:
            self.parts |= G_PART_EDGE_IDS
        self._lists = adjs  # ensure(G_PART_EDGE_IDS) reads the edge lists again: they live as long as the handle
        self._pending = True
        self.num_nodes = int(num_nodes)
        self.num_edge_types = L
        self.num_edges = int(sum(a.shape[0] for a in adjs))
        self.edges_per_type = tuple(int(a.shape[0]) for a in adjs)  # host-side: known without touching the device
        self.device = adjs[0].device if adjs else torch.device("cuda")
        self._cache = {}
        self._gather_operands = {}  # (view, width, stream) -> _GatherOperand: the aggregate operands of the layer-level calls
        if wait:
            self.wait()

    def wait(self):
        """Block the host until the bucketing has finished; raises ValueError for bad node indices."""
        if self._pending:
            if capturing():
                raise RuntimeError("tf2_gnn_amd: a batch's edges cannot be bucketed inside a hipGraph capture (the build reads "
                                   "sizes back); run the step eagerly once on the same adjacency tensors first (CapturedStep warmup)")
            self._pending = False
            self._keep = None
            try:
                _lib.check(_lib.load().tfgnn_graph_wait(self._h))
            except Exception:
                self.close()
                raise
        return self

    def ensure(self, parts: int) -> "Graph":
        """Build the parts that were not requested at creation, on the current stream (tfgnn_graph_ensure; blocks the host)."""
        if parts & ~self.parts:
            self.wait()
            _lib.check(_lib.load().tfgnn_graph_ensure(self._h, int(parts), _stream()))
            self.parts |= int(parts)
        return self

    def array(self, array_id: int) -> torch.Tensor:
        if array_id in self._cache:
            return self._cache[array_id]
        self.ensure(_array_parts(array_id))
        lib = _lib.load()
        p = ctypes.c_void_p()
        n = ctypes.c_int64()
        _lib.check(lib.tfgnn_graph_array(self._h, array_id, ctypes.byref(p), ctypes.byref(n)))
        if n.value == 0 or not p.value:
            dt = torch.float32 if array_id in _FLOAT_ARRAYS else torch.uint8 if array_id in _BYTE_ARRAYS else torch.int32
            t = torch.empty(0, dtype=dt, device=self.device)
        else:
            typestr = "<f4" if array_id in _FLOAT_ARRAYS else "|u1" if array_id in _BYTE_ARRAYS else "<i4"
            t = torch.as_tensor(_DevArray(p.value, n.value, typestr, self), device=self.device)
        self._cache[array_id] = t
        return t

    def nonempty_offsets(self, by_src: bool):
        """host list [L+1]: first compact index of each edge type among the non-empty buckets
        (type-major); the last entry is the number of non-empty buckets."""
        key = ("nz_off", bool(by_src))
        off = self._cache.get(key)
        if off is None:
            self.ensure(G_PART_COMPACT)
            buf = (ctypes.c_int32 * (self.num_edge_types + 1))()
            _lib.check(_lib.load().tfgnn_graph_nonempty_offsets(self._h, int(by_src), buf))
            off = list(buf)
            self._cache[key] = off
        return off

    def gather_operand(self, view: int, width: int) -> "_GatherOperand":
        """The graph's own SP16 gather operand for (``view``, ``width``, the current stream): data [rows, row bytes] + inverse
        scales, allocated on first use and kept until ``close()`` / ``release_gather_operands()``.  The layer-level calls
        (``mp_forward`` / ``mp_backward``) and ``graph_gather_sp_owned`` gather into it.  Which buckets of a view are empty depends
        on the graph alone, so only the first gather into a pair has to write their zero rows and marker scales; the pair
        records what it was filled with (``_GatherOperand.filled``) and later gathers leave those rows alone.  NOTHING but
        these gathers may write to the pair: whoever does resets ``filled`` to None."""
        key = (int(view), int(width), _stream())
        pair = self._gather_operands.get(key)
        if pair is None:
            typed = view in (VIEW_BY_DST_TYPED, VIEW_BY_SRC_TYPED, VIEW_BY_DST_TYPED_PATTERN)
            if view in (VIEW_BY_DST_TYPED_COMPACT, VIEW_BY_SRC_TYPED_COMPACT):
                rows, per = int(self.nonempty_offsets(view == VIEW_BY_SRC_TYPED_COMPACT)[-1]), 1
            else:
                rows, per = self.num_nodes, (self.num_edge_types if typed else 1)
            pair = _GatherOperand(torch.empty((rows, per * int(width) * 4), dtype=torch.uint8, device=self.device),
                                  torch.empty((rows, per), dtype=torch.float32, device=self.device))
            self._gather_operands[key] = pair
        return pair

    def release_gather_operands(self) -> None:
        """Drop the graph-owned gather operands (work already enqueued may still read them: the allocator reuses the memory in
        stream order); the next layer call allocates and fills its pair again."""
        self._gather_operands = {}

    def close(self):
        """Return the handle's memory to the library; work already enqueued on the current stream may
        still read it (the memory is only reused after that work)."""
        self._gather_operands = {}
        if getattr(self, "_h", None) is not None and self._h:
            self._cache = {}
            h, self._h = self._h, None
            _lib.check(_lib.load().tfgnn_graph_destroy_async(h, _stream()))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_workspaces = {}


def _workspace(device, nbytes: int) -> torch.Tensor:
    key = (device.type, device.index, _stream())
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def _aligned_workspace(device, nbytes: int, own: bool = False):
    """-> (pointer, length, buffer) of ``nbytes`` or more at a 256-byte aligned address, as the TN products take their workspace:
    in the shared buffer of this stream, or - own - in a buffer of the caller's (``buffer`` keeps it alive)."""
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=device) if own else _workspace(device, nbytes + 256)
    off = (-ws.data_ptr()) % 256
    return ws.data_ptr() + off, ws.numel() - off, ws


@_writes_out
def gather_reduce(
    rowptr: torch.Tensor,
    col: torch.Tensor,
    inp: torch.Tensor,
    *,
    edge_weight: Optional[torch.Tensor] = None,
    row_scale: Optional[torch.Tensor] = None,
    reduce: int = REDUCE_SUM,
    pre_act=ACT_NONE,
    post_act=ACT_NONE,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """out[r] = post_act(row_scale[r] * REDUCE_{e in row r} pre_act(edge_weight[e] * inp[col[e]]))."""
    lib = _lib.load()
    _require_dev(inp, torch.float32, "inp")
    _require_dev(rowptr, torch.int32, "rowptr")
    num_rows = rowptr.numel() - 1
    inp, ld_in = _rowmajor(inp, "inp")
    width = inp.shape[1]
    if out is None:
        out = torch.empty((num_rows, width), dtype=torch.float32, device=inp.device)
    out2, ld_out = _rowmajor(out, "out")
    if out2 is not out:
        raise ValueError("out must have unit inner stride")
    if out.shape[0] != num_rows or out.shape[1] != width:
        raise ValueError(f"out has shape {tuple(out.shape)}, expected {(num_rows, width)}")
    _lib.check(
        lib.tfgnn_csr_gather_reduce(
            _ptr(rowptr), _ptr(col), _ptr(edge_weight), _ptr(row_scale), num_rows, _ptr(inp), ld_in, width,
            _ptr(out), ld_out, int(reduce), act_id(pre_act), act_id(post_act), _stream(),
        )
    )
    return out


(VIEW_BY_DST_TYPED, VIEW_BY_DST_NODE, VIEW_BY_SRC_TYPED, VIEW_BY_SRC_NODE, VIEW_BY_DST_TYPED_COMPACT,
 VIEW_BY_SRC_TYPED_COMPACT, VIEW_BY_DST_TYPED_PATTERN) = range(7)


@_writes_out
def graph_gather(
    graph: "Graph",
    view: int,
    inp: torch.Tensor,
    *,
    col: Optional[torch.Tensor] = None,
    edge_weight: Optional[torch.Tensor] = None,
    row_scale: Optional[torch.Tensor] = None,
    reduce: int = REDUCE_SUM,
    pre_act=ACT_NONE,
    post_act=ACT_NONE,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """gather_reduce over one of the Graph's bucketed views (with its long-row plan).
    edge_weight: [E] or [E, K] (K heads of width/K floats each)."""
    lib = _lib.load()
    _require_dev(inp, torch.float32, "inp")
    if view == VIEW_BY_DST_TYPED_COMPACT:
        num_rows = graph.nonempty_offsets(False)[-1]
    elif view == VIEW_BY_SRC_TYPED_COMPACT:
        num_rows = graph.nonempty_offsets(True)[-1]
    else:  # (the pattern view writes every (node, type) bucket, like the typed views)
        typed = view in (VIEW_BY_DST_TYPED, VIEW_BY_SRC_TYPED, VIEW_BY_DST_TYPED_PATTERN)
        num_rows = graph.num_nodes * (graph.num_edge_types if typed else 1)
    if view == VIEW_BY_DST_TYPED_PATTERN and graph.num_edge_types > 8:
        raise ValueError("graph_gather: the pattern order exists for at most 8 edge types")
    inp, ld_in = _rowmajor(inp, "inp")
    width = inp.shape[1]
    if out is None:
        out = torch.empty((num_rows, width), dtype=torch.float32, device=inp.device)
    out2, ld_out = _rowmajor(out, "out")
    if out2 is not out or out.shape[0] != num_rows or out.shape[1] != width:
        raise ValueError(f"out must be [{num_rows},{width}] with unit inner stride, got {tuple(out.shape)}")
    heads = 1
    if edge_weight is not None:
        edge_weight = edge_weight.contiguous()
        heads = edge_weight.shape[1] if edge_weight.dim() == 2 else 1
    graph.ensure(_VIEW_PARTS[view])
    ws_bytes = lib.tfgnn_graph_gather_workspace_bytes(graph._h, view, width)
    ws = _workspace(inp.device, ws_bytes) if ws_bytes else None
    _lib.check(
        lib.tfgnn_graph_gather_reduce(
            graph._h, view, _ptr(col), _ptr(edge_weight), heads, _ptr(row_scale), _ptr(inp), ld_in, width,
            _ptr(out), ld_out, int(reduce), act_id(pre_act), act_id(post_act), _ptr(ws),
            ws.numel() if ws is not None else 0, _stream(),
        )
    )
    return out


def graph_gather_dot_supported(width: int, heads: int) -> bool:
    return bool(_lib.load().tfgnn_graph_gather_dot_supported(int(width), int(heads)))


def graph_gather_dot(graph: "Graph", view: int, inp: torch.Tensor, *, edge_weight: torch.Tensor, dot_rows: torch.Tensor,
                     dot_pos: Optional[torch.Tensor] = None):
    """graph_gather with per-head edge weights [E, K] that also returns, per edge e of the view and head k, the inner product
    of the gathered row inp[col(e)] with dot_rows[row of e] over the head's columns, written at position dot_pos[e] (None: e)
    (tfgnn_graph_gather_reduce_dot) -> (sums [rows, width], products [E, K])."""
    lib = _lib.load()
    _require_dev(inp, torch.float32, "inp")
    _require_dev(dot_rows, torch.float32, "dot_rows")
    typed = view in (VIEW_BY_DST_TYPED, VIEW_BY_SRC_TYPED)
    if view not in (VIEW_BY_DST_TYPED, VIEW_BY_SRC_TYPED, VIEW_BY_DST_NODE, VIEW_BY_SRC_NODE):
        raise ValueError("graph_gather_dot: the four plain views only")
    num_rows = graph.num_nodes * (graph.num_edge_types if typed else 1)
    inp, ld_in = _rowmajor(inp, "inp")
    dot_rows, ld_dot = _rowmajor(dot_rows, "dot_rows")
    width = inp.shape[1]
    if edge_weight.dim() != 2 or edge_weight.shape[0] != graph.num_edges:
        raise ValueError("graph_gather_dot: edge_weight must be [E, K]")
    edge_weight = edge_weight.contiguous()
    heads = edge_weight.shape[1]
    if tuple(dot_rows.shape) != (num_rows, width):
        raise ValueError(f"dot_rows must be [{num_rows},{width}], got {tuple(dot_rows.shape)}")
    if dot_pos is not None and (dot_pos.dtype != torch.int32 or dot_pos.numel() != graph.num_edges or not dot_pos.is_contiguous()):
        raise ValueError("dot_pos must be a contiguous int32 tensor with one entry per edge")
    dots = torch.empty((graph.num_edges, heads), dtype=torch.float32, device=inp.device)
    if graph.num_edges == 0:
        return torch.zeros((num_rows, width), dtype=torch.float32, device=inp.device), dots
    out = torch.empty((num_rows, width), dtype=torch.float32, device=inp.device)
    graph.ensure(_VIEW_PARTS[view])
    ws_bytes = lib.tfgnn_graph_gather_workspace_bytes(graph._h, view, width)
    ws = _workspace(inp.device, ws_bytes) if ws_bytes else None
    _lib.check(
        lib.tfgnn_graph_gather_reduce_dot(
            graph._h, view, _ptr(edge_weight), heads, _ptr(inp), ld_in, width, _ptr(out), out.stride(0), _ptr(dot_rows), ld_dot,
            _ptr(dot_pos), _ptr(dots), _ptr(ws), ws.numel() if ws is not None else 0, _stream(),
        )
    )
    return out, dots


class DropoutSpec:
    """A layer-input dropout whose mask is not stored: (rate, seed, shape).  The producer of the tensor applied the mask in its
    epilogue (``sp_gemm_nt(..., dropout=...)``); the backward pass hands the spec to a product that RECOMPUTES the mask, or -
    on a path without such an epilogue - materialises it once with ``mask()`` (the tensor ``dropout_forward`` would have
    returned for this seed)."""

    def __init__(self, rate: float, seed: int, shape, device):
        self.rate, self.seed, self.shape, self.device = float(rate), int(seed), tuple(shape), device
        self._mask = None

    @property
    def keep(self) -> float:
        return 1.0 - self.rate

    def mask(self) -> torch.Tensor:
        if self._mask is None:
            self._mask = dropout_mask(self.shape, self.rate, self.seed, self.device)
        return self._mask


def plain_epilogue(out_mul, act_grad):
    """-> (mask tensor | None, (activation, saved) | None): the gradient factors for a kernel WITHOUT the recomputing
    epilogue.  ``out_mul`` may be a DropoutSpec (materialised), ``act_grad`` a triple (activation, saved, saved_scale) -
    the derivative at saved * saved_scale, saved being a dropped activation (one more pass over it here)."""
    if isinstance(out_mul, DropoutSpec):
        out_mul = out_mul.mask()
    if act_grad is not None and len(act_grad) == 3:
        act, saved, scale = act_grad
        if float(scale) != 1.0:
            saved = add_scale(saved, saved, 0.5 * float(scale))
        act_grad = (act, saved)
    return out_mul, act_grad


def _native_epilogue(out_mul, act_grad, dropout, saved_scale):
    """the same specs for the split-operand product, which takes them as they are"""
    spec = out_mul if isinstance(out_mul, DropoutSpec) else None
    if spec is not None:
        if dropout is not None:
            raise ValueError("two dropout masks on one product")
        dropout, out_mul = (spec.rate, spec.seed), None
    if act_grad is not None and len(act_grad) == 3:
        saved_scale = float(act_grad[2])
        act_grad = (act_grad[0], act_grad[1])
        if (spec is not None and act_grad[0] == "relu" and abs(saved_scale - spec.keep) < 1e-12 and saved_scale != 1.0
                and tuple(act_grad[1].shape) == spec.shape):
            # the saved tensor is the relu output dropped with THIS mask: it is positive exactly where the unit was kept and
            # active - no mask needs to be recomputed (tfgnn_sp_gemm_nt_dropout, seed UINT64_MAX)
            dropout = (spec.rate, 0xFFFFFFFFFFFFFFFF)
    return out_mul, act_grad, dropout, saved_scale


@_writes_out
def gemm_grad(a, b, *, trans_b=False, out=None, out_mul=None, act_grad=None, accumulate=False) -> torch.Tensor:
    """out = (a @ op(b)) * out_mul * act'(saved) (+ out if ``accumulate``): an input-gradient product with the element-wise
    factors of the next backward step (dropout mask ``out_mul``, ``act_grad = (activation name, saved tensor)``) applied in the
    GEMM epilogue when the active kernel has one (tfgnn_gemm_grad_epilogue), by separate kernels otherwise.
    Use the RETURN value: on the unfused route the factors are applied out of place and ``out`` only holds the raw
    product (with ``accumulate`` the result is added into ``out`` and ``out`` is returned)."""
    if accumulate and out is None:
        raise ValueError("accumulate=True needs out")
    out_mul, act_grad = plain_epilogue(out_mul, act_grad)
    if out_mul is None and act_grad is None:
        return gemm(a, b, trans_b=trans_b, out=out, accumulate=accumulate)
    lib = _lib.load()
    a2, lda = _rowmajor(a, "a")
    b2, ldb = _rowmajor(b, "b")
    M, K = a2.shape
    N = b2.shape[0] if trans_b else b2.shape[1]
    res = out if out is not None else torch.empty((M, N), dtype=torch.float32, device=a.device)
    res2, ldc = _rowmajor(res, "out")
    act_name, saved = act_grad if act_grad is not None else (None, None)

    def plain(t):
        return t is None or (t.dim() == 2 and t.stride(1) == 1 and tuple(t.shape) == (M, N))

    if plain(out_mul) and plain(saved) and res2 is res:
        ws_bytes = lib.tfgnn_gemm_workspace_bytes(M, N, K)
        ws = _workspace(a.device, ws_bytes) if ws_bytes else None
        rc = lib.tfgnn_gemm_grad_epilogue(
            0, int(trans_b), M, N, K, _ptr(a2), lda, _ptr(b2), ldb, _ptr(res), ldc, _ptr(out_mul),
            out_mul.stride(0) if out_mul is not None else 0, act_id(act_name), _ptr(saved),
            saved.stride(0) if saved is not None else 0, int(accumulate), _ptr(ws), ws.numel() if ws is not None else 0, _stream(),
        )
        if rc == 0:
            return res
        if rc != -4:  # TFGNN_ERR_UNSUPPORTED: no fused epilogue for this mode / shape
            _lib.check(rc)
    res = gemm(a, b, trans_b=trans_b, out=None if accumulate else out)
    if out_mul is not None:
        res = mul(res, out_mul)
    if act_grad is not None:
        res = activation_backward(act_name, res, saved)
    if accumulate:
        out.copy_(add_scale(out, res, 1.0))
        return out
    return res


KERNEL_FAMILIES = ("gemm_fp32", "gemm_bf16x3", "sp_nt", "sp_tn", "gather_sp", "gather", "fused_nt", "gemm_stream", "stream_f16x2")


def launch_counts() -> dict:
    """tfgnn_launch_counts as a dict: kernel family -> launches this process has enqueued so far (host counters, no device
    work).  bench.py reports the per-step differences as ``products`` so that a line says which product kernels ran."""
    buf = (ctypes.c_int64 * len(KERNEL_FAMILIES))()
    _lib.check(_lib.load().tfgnn_launch_counts(buf, len(KERNEL_FAMILIES)))
    return dict(zip(KERNEL_FAMILIES, (int(v) for v in buf)))


@_writes_out
def gemm(
    a: torch.Tensor,
    b: torch.Tensor,
    *,
    trans_a: bool = False,
    trans_b: bool = False,
    bias: Optional[torch.Tensor] = None,
    act=ACT_NONE,
    out: Optional[torch.Tensor] = None,
    accumulate: bool = False,
) -> torch.Tensor:
    """out = act(op(a) @ op(b) + bias) (+ out).  a, b: 2-D fp32 device tensors, unit inner stride."""
    lib = _lib.load()
    _require_dev(a, torch.float32, "a")
    _require_dev(b, torch.float32, "b")
    a, lda = _rowmajor(a, "a")
    b, ldb = _rowmajor(b, "b")
    M, K = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    Kb, N = (b.shape[1], b.shape[0]) if trans_b else (b.shape[0], b.shape[1])
    if K != Kb:
        raise ValueError(f"gemm: inner dimensions differ ({K} vs {Kb})")
    if (not trans_a and not trans_b and M >= 4096 and K * N <= (1 << 22) and K >= 64 and K % 4 == 0
            and (N % 320 == 0 or N % 128 == 0) and get_gemm_mode() != GEMM_FP32):
        # a small [K, N] right operand against many rows: the split-operand kernel stages K-contiguous operands
        # fastest (no register transposes; QM9-sized GRU product 1.44 -> 0.8 ms), so hand it B^T (one small copy)
        b, ldb, trans_b = transpose_batched(b), K, True
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs out")
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    out2, ldc = _rowmajor(out, "out")
    if out2 is not out or tuple(out.shape) != (M, N):
        raise ValueError(f"out must be [{M},{N}] with unit inner stride")
    if bias is not None:
        _require_dev(bias, torch.float32, "bias")
        if bias.numel() != N:
            raise ValueError("bias must have N elements")
        bias = bias.contiguous()
    ws_bytes = lib.tfgnn_gemm_workspace_bytes(M, N, K)
    ws = _workspace(a.device, ws_bytes) if ws_bytes else None
    _lib.check(
        lib.tfgnn_gemm(
            int(trans_a), int(trans_b), M, N, K, _ptr(a), lda, _ptr(b), ldb, _ptr(out), ldc, _ptr(bias),
            act_id(act), int(accumulate), _ptr(ws), ws.numel() if ws is not None else 0, _stream(),
        )
    )
    return out


_ident_ptrs = {}


def _identity_rowptr(device, n: int) -> torch.Tensor:
    """[0, 1, ..., n] int32 (rows of one element each: turns tfgnn_csr_gather_reduce into a plain row gather)."""
    key = str(device)
    t = _ident_ptrs.get(key)
    if t is None or t.numel() < n + 1:
        t = torch.arange(max(n + 1, 1 << 16), dtype=torch.int32, device=device)
        _ident_ptrs[key] = t
    return t[: n + 1]


@_writes_out
def gemm_gathered(a: torch.Tensor, row_index: torch.Tensor, b: torch.Tensor, *, trans_b: bool = False,
                  bias: Optional[torch.Tensor] = None, act=ACT_NONE, out: Optional[torch.Tensor] = None,
                  accumulate: Optional[str] = None) -> torch.Tensor:
    """out[m] = act(a[row_index[m]] @ op(b) + bias)  (tfgnn_gemm_gathered: tf.nn.embedding_lookup + Dense, the gathered rows are
    never written).  ``accumulate``: None, "after" (out += act(..)) or "before" (out = act(out + ..), the second half of a
    product over concatenated inputs).  Shapes the streaming kernel does not take run as a row gather + gemm."""
    lib = _lib.load()
    _require_dev(a, torch.float32, "a")
    _require_dev(b, torch.float32, "b")
    _require_dev(row_index, torch.int32, "row_index")
    if accumulate not in (None, "after", "before"):
        raise ValueError('accumulate is None, "after" or "before"')
    a2, lda = _rowmajor(a, "a")
    b2, ldb = _rowmajor(b, "b")
    K = a2.shape[1]
    Kb, N = (b2.shape[1], b2.shape[0]) if trans_b else (b2.shape[0], b2.shape[1])
    if K != Kb:
        raise ValueError(f"gemm_gathered: inner dimensions differ ({K} vs {Kb})")
    M = row_index.numel()
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    out2, ldc = _rowmajor(out, "out")
    if out2 is not out or tuple(out.shape) != (M, N):
        raise ValueError(f"out must be [{M},{N}] with unit inner stride")
    if bias is not None:
        _require_dev(bias, torch.float32, "bias")
        bias = bias.contiguous()
    if M == 0:
        return out
    row_index = row_index.contiguous()
    rc = lib.tfgnn_gemm_gathered(
        int(trans_b), M, N, K, _ptr(a2), lda, a2.shape[0], _ptr(row_index), _ptr(b2), ldb, _ptr(out), ldc, _ptr(bias),
        act_id(act), {None: 0, "after": 1, "before": 2}[accumulate], _stream(),
    )
    if rc == 0:
        return out
    if rc != -4:  # TFGNN_ERR_UNSUPPORTED: the caller-side route below
        _lib.check(rc)
    rows = gather_reduce(_identity_rowptr(a.device, M), row_index, a2)
    if accumulate == "before":
        gemm(rows, b2, trans_b=trans_b, bias=bias, out=out, accumulate=True)
        if act_id(act) != act_id(ACT_NONE):
            if out.is_contiguous():
                activation_forward(act, out, out=out)
            else:
                out.copy_(activation_forward(act, out))
        return out
    return gemm(rows, b2, trans_b=trans_b, bias=bias, act=act, out=out, accumulate=accumulate == "after")


@_writes_out
def activation_forward(act, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = _lib.load()
    _require_dev(x, torch.float32, "x")
    x = x.contiguous()
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.tfgnn_activation_forward(act_id(act), _ptr(x), _ptr(out), x.numel(), _stream()))
    return out


@_writes_out
def activation_backward(act, dy: torch.Tensor, saved: torch.Tensor, out: Optional[torch.Tensor] = None,
                        mul: Optional[torch.Tensor] = None):
    """dx = dy * act'(.), derivative evaluated from the saved output (saved input for gelu).  ``mul``: dx = (dy * mul) * act'(.)
    in the same pass (tfgnn_activation_backward_mul)."""
    lib = _lib.load()
    _require_dev(dy, torch.float32, "dy")
    dy = dy.contiguous()
    saved = saved.contiguous()
    if out is None:
        out = torch.empty_like(dy)
    if mul is not None:
        mul = mul.contiguous()
        if mul.shape != dy.shape:
            raise ValueError("activation_backward: mul must have the gradient's shape")
        if (dy.data_ptr() | saved.data_ptr() | mul.data_ptr() | out.data_ptr()) % 16 == 0:
            _lib.check(lib.tfgnn_activation_backward_mul(act_id(act), _ptr(dy), _ptr(saved), _ptr(mul), _ptr(out), dy.numel(),
                                                         _stream()))
            return out
        tmp = torch.empty_like(dy)  # (unaligned views: the two-pass form)
        _lib.check(lib.tfgnn_mul(_ptr(dy), _ptr(mul), _ptr(tmp), dy.numel(), _stream()))
        dy = tmp
    _lib.check(
        lib.tfgnn_activation_backward(act_id(act), _ptr(dy), _ptr(saved), _ptr(out), dy.numel(), _stream())
    )
    return out


def gru_gates_forward(mx, mh, h, save_gates: bool = True):
    """h' = GRU gate math on the two pre-computed matmuls ([ext] Keras GRUCell reset_after=True)."""
    lib = _lib.load()
    V, H = h.shape
    h = h.contiguous()
    h_new = torch.empty_like(h)
    gates = torch.empty((V, 3 * H), dtype=torch.float32, device=h.device) if save_gates else None
    _lib.check(
        lib.tfgnn_gru_gates_forward(_ptr(mx), _ptr(mh), _ptr(h), _ptr(h_new), _ptr(gates), V, H, _stream())
    )
    return h_new, gates


_gru_perm = {}


def gru_kernel_regrouped(kernel: torch.Tensor, bias: Optional[torch.Tensor]):
    """Keras GRUCell kernel [K, 3H] (+ bias [3H]) -> the operand form of tfgnn_gemm_gru: [3H, K], K contiguous, rows
    regrouped per 192-row block as [z | r | h] of the same 64 units (an index gather on a small weight matrix)."""
    K, H3 = kernel.shape
    H = H3 // 3
    key = (H, kernel.device)
    perm = _gru_perm.get(key)
    if perm is None:  # (seven tiny launches per call otherwise: once per width and device)
        t = torch.arange(H // 64, device=kernel.device).view(-1, 1, 1)
        g = torch.arange(3, device=kernel.device).view(1, -1, 1)
        c = torch.arange(64, device=kernel.device).view(1, 1, -1)
        perm = _gru_perm[key] = (g * H + t * 64 + c).reshape(-1)
    return transpose_batched(kernel.index_select(1, perm)), (None if bias is None else bias.index_select(0, perm).contiguous())


def gemm_gru(x, kernel, bias, mh, h, save_gates: bool = True):
    """h' = GRUCell gate math on (x @ kernel + bias, mh, h) with the matmul and the gates in one kernel
    (tfgnn_gemm_gru) -> (h', gates or None), or None when the library has no such kernel for this mode / shape."""
    H = h.shape[1]
    if get_gemm_mode() == GEMM_FP32 or H % 64 != 0 or kernel.shape[0] < 64 or kernel.shape[0] % 4 != 0:
        return None
    lib = _lib.load()
    x, ldx = _rowmajor(x, "x")
    mh = mh.contiguous()
    h = h.contiguous()
    kt, bp = gru_kernel_regrouped(kernel, bias)
    V, K = x.shape
    h_new = torch.empty_like(h)
    gates = torch.empty_like(mh) if save_gates else None
    rc = lib.tfgnn_gemm_gru(V, H, K, _ptr(x), ldx, _ptr(kt), _ptr(bp), _ptr(mh), _ptr(h), _ptr(h_new), _ptr(gates), _stream())
    if rc == -4:
        return None
    _lib.check(rc)
    return h_new, gates


def gemm_gru2(x, kernel, bias, h, recurrent_kernel, recurrent_bias):
    """The whole GRUCell forward in ONE kernel (tfgnn_gemm_gru2): h' = GRU(x @ kernel + bias, h @ recurrent_kernel +
    recurrent_bias, h) - mh is neither produced by a product of its own nor read back (3.5 GB per layer at the QM9 size).
    -> (h', gates [V, 3H], mh [V, 3H] of which ONLY the candidate third is written: all the backward pass reads), or None when
    the library has no such kernel (mode other than f16x2, H not in {64, 128}, fewer than 65536 rows)."""
    H = h.shape[1]
    if get_gemm_mode() != GEMM_F16X2 or H not in (64, 128) or kernel.shape[0] != H or h.shape[0] < 65536:
        return None
    lib = _lib.load()
    x, ldx = _rowmajor(x, "x")
    h = h.contiguous()
    kt, bp = gru_kernel_regrouped(kernel, bias)
    rt, rbp = gru_kernel_regrouped(recurrent_kernel, recurrent_bias)
    V = x.shape[0]
    h_new = torch.empty_like(h)
    gates = torch.empty((V, 3 * H), dtype=torch.float32, device=h.device)
    mh = torch.empty((V, 3 * H), dtype=torch.float32, device=h.device)
    rc = lib.tfgnn_gemm_gru2(V, H, _ptr(x), ldx, _ptr(kt), _ptr(bp), _ptr(h), _ptr(rt), _ptr(rbp), _ptr(h_new), _ptr(gates), _ptr(mh),
                             _stream())
    if rc == -4:
        return None
    _lib.check(rc)
    return h_new, gates, mh


def gru_gates_backward(dh_new, gates, mh, h):
    lib = _lib.load()
    V, H = h.shape
    dh_new = dh_new.contiguous()
    dmx = torch.empty((V, 3 * H), dtype=torch.float32, device=h.device)
    dmh = torch.empty_like(dmx)
    dh_direct = torch.empty_like(h)
    _lib.check(
        lib.tfgnn_gru_gates_backward(
            _ptr(dh_new), _ptr(gates), _ptr(mh), _ptr(h.contiguous()), _ptr(dmx), _ptr(dmh), _ptr(dh_direct),
            V, H, _stream(),
        )
    )
    return dmx, dmh, dh_direct


def gru_gates_backward_sp(dh_new, gates, mh, h, out_mul=None):
    """gru_gates_backward with dmx / dmh written ONLY as SP16 split operands (one scale per row) and the bias gradients
    [2, 3H] folded in (tfgnn_gru_gates_backward_sp) -> (dmx_sp, dmh_sp, dh_direct, bias_grad), or None when the library has
    no such kernel for this width (H % 64 != 0 or H > 512).  ``out_mul`` [V, H]: factor of dh_direct (a dropout mask); a
    DropoutSpec: the mask is recomputed from (rate, seed) in the kernel (tfgnn_gru_gates_backward_sp_dropout)."""
    lib = _lib.load()
    V, H = h.shape
    if H % 64 != 0 or H > 512:
        return None
    dh_new = dh_new.contiguous()
    dev = h.device
    dmx = SplitOperand(torch.empty((V, 3 * H * 4), dtype=torch.uint8, device=dev), torch.empty((V, 1), dtype=torch.float32, device=dev),
                       V, 3 * H, 3 * H)
    dmh = SplitOperand(torch.empty((V, 3 * H * 4), dtype=torch.uint8, device=dev), torch.empty((V, 1), dtype=torch.float32, device=dev),
                       V, 3 * H, 3 * H)
    dh_direct = torch.empty_like(h)
    bias_grad = torch.empty((2, 3 * H), dtype=torch.float32, device=dev)
    ws_bytes = lib.tfgnn_gru_gates_backward_sp_workspace_bytes(V, H)
    ws = _workspace(dev, ws_bytes) if ws_bytes else None
    if isinstance(out_mul, DropoutSpec):
        if out_mul.shape != (V, H):
            raise ValueError("gru_gates_backward_sp: the dropout spec is not one of the layer input")
        rc = lib.tfgnn_gru_gates_backward_sp_dropout(_ptr(dh_new), _ptr(gates), _ptr(mh), _ptr(h.contiguous()), _ptr(dmx.data),
                                                     _ptr(dmx.inv_scale), _ptr(dmh.data), _ptr(dmh.inv_scale), _ptr(dh_direct),
                                                     float(out_mul.rate), int(out_mul.seed) & (2**64 - 1), _ptr(bias_grad), V, H,
                                                     _ptr(ws), ws.numel() if ws is not None else 0, _stream())
    else:
        rc = lib.tfgnn_gru_gates_backward_sp(_ptr(dh_new), _ptr(gates), _ptr(mh), _ptr(h.contiguous()), _ptr(dmx.data),
                                             _ptr(dmx.inv_scale), _ptr(dmh.data), _ptr(dmh.inv_scale), _ptr(dh_direct),
                                             _ptr(out_mul.contiguous() if out_mul is not None else None), _ptr(bias_grad), V, H,
                                             _ptr(ws), ws.numel() if ws is not None else 0, _stream())
    if rc == -4:
        return None
    _lib.check(rc)
    return dmx, dmh, dh_direct, bias_grad


def colsum(x: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    x, ld = _rowmajor(x, "x")
    out = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    ws_bytes = lib.tfgnn_colsum_workspace_bytes(x.shape[0], x.shape[1])
    ws = _workspace(x.device, ws_bytes) if ws_bytes else None
    _lib.check(lib.tfgnn_colsum(_ptr(x), x.shape[0], x.shape[1], ld, _ptr(out), _ptr(ws),
                                ws.numel() if ws is not None else 0, _stream()))
    return out


def add_scale(x: torch.Tensor, y: torch.Tensor, alpha: float) -> torch.Tensor:
    """alpha * (x + y)"""
    lib = _lib.load()
    x = x.contiguous()
    y = y.contiguous()
    out = torch.empty_like(x)
    _lib.check(lib.tfgnn_add_scale(_ptr(x), _ptr(y), float(alpha), _ptr(out), x.numel(), _stream()))
    return out


def dropout_forward(x: torch.Tensor, rate: float, seed: int, want_mask: bool = True):
    """-> (y, mask) with mask in {0, 1/(1-rate)}.  In f16x2 mode a 2-D result that can be a split operand (width a
    multiple of 16, <= 512) is also written in the SP16 format by the same kernel and remembered for ``sp_rows_of``.
    want_mask=False: the mask is not stored (-> (y, None)); whoever needs it recomputes it from (rate, seed)
    (``DropoutSpec``, the epilogues of the split-operand products, ``dropout_mask``)."""
    lib = _lib.load()
    x = x.contiguous()
    y = torch.empty_like(x)
    mask = torch.empty_like(x) if want_mask else None
    if get_gemm_mode() == GEMM_F16X2 and x.dim() == 2 and x.shape[1] % 16 == 0 and 32 <= x.shape[1] <= 512 and x.shape[0] > 0:
        rows, cols = x.shape
        op = SplitOperand(torch.empty((rows, cols * 4), dtype=torch.uint8, device=x.device),
                          torch.empty((rows, 1), dtype=torch.float32, device=x.device), rows, cols, cols)
        _lib.check(lib.tfgnn_dropout_forward_sp(_ptr(x), _ptr(y), _ptr(mask), rows, cols, float(rate), int(seed) & (2**64 - 1),
                                                _ptr(op.data), op.data.stride(0), _ptr(op.inv_scale), _stream()))
        _remember_split_rows(y, op)
        return y, mask
    _lib.check(
        lib.tfgnn_dropout_forward(_ptr(x), _ptr(y), _ptr(mask), x.numel(), float(rate), int(seed) & (2**64 - 1), _stream())
    )
    return y, mask


def dropout_epoch() -> int:
    """The dropout epoch (include/tfgnn.h: masks are a function of (seed, element, epoch); 0 unless something advanced it).
    Waits for the current stream."""
    v = ctypes.c_uint32()
    _lib.check(_lib.load().tfgnn_dropout_epoch_get(ctypes.byref(v), _stream()))
    return int(v.value)


def dropout_epoch_advance() -> None:
    """epoch += 1 by a kernel on the current stream (capturable: the first node of ``capture.CapturedStep``)."""
    _lib.check(_lib.load().tfgnn_dropout_epoch_advance(_stream()))


def dropout_epoch_set(value: int) -> None:
    _lib.check(_lib.load().tfgnn_dropout_epoch_set(int(value) & 0xFFFFFFFF, _stream()))


def dropout_mask(shape, rate: float, seed: int, device=None) -> torch.Tensor:
    """The mask (0 or 1/(1-rate)) a dropout call with this seed draws for a tensor of ``shape`` - what ``dropout_forward``
    returns and what the fused producers (``sp_gemm_nt(..., dropout=(rate, seed))``) apply without storing it."""
    lib = _lib.load()
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    mask = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    if mask.numel():
        _lib.check(lib.tfgnn_dropout_forward(None, None, _ptr(mask), mask.numel(), float(rate), int(seed) & (2**64 - 1), _stream()))
    return mask


def clip(x: torch.Tensor, lower: Optional[float], upper: Optional[float]) -> torch.Tensor:
    """tf.minimum(tf.maximum(x, lower), upper); None = no bound."""
    lib = _lib.load()
    x = x.contiguous()
    y = torch.empty_like(x)
    lo = float("-inf") if lower is None else float(lower)
    hi = float("inf") if upper is None else float(upper)
    _lib.check(lib.tfgnn_clip(_ptr(x), x.numel(), lo, hi, _ptr(y), _stream()))
    return y


def clip_backward(dy: torch.Tensor, x: torch.Tensor, lower: Optional[float], upper: Optional[float]) -> torch.Tensor:
    lib = _lib.load()
    dy, x = dy.contiguous(), x.contiguous()
    dx = torch.empty_like(dy)
    lo = float("-inf") if lower is None else float(lower)
    hi = float("inf") if upper is None else float(upper)
    _lib.check(lib.tfgnn_clip_backward(_ptr(dy), _ptr(x), x.numel(), lo, hi, _ptr(dx), _stream()))
    return dx


_POOL_KINDS = {"softmax": _lib.POOL_SOFTMAX, "sigmoid": _lib.POOL_SIGMOID, "none": _lib.POOL_NONE, "average": _lib.POOL_AVERAGE}


def _pool_common(a, kind: str, ptr: torch.Tensor, T: torch.Tensor, heads: int, lower, upper):
    """Fills the fields the two graph-readout argument structs share; -> (T as passed, workspace tensor or None)."""
    lib = _lib.load()
    _require_dev(T, torch.float32, "T")
    T, ldT = _rowmajor(T, "T")
    V, GD = (int(v) for v in T.shape)
    G = int(ptr.numel()) - 1
    a.struct_size = ctypes.sizeof(type(a))
    a.kind = _POOL_KINDS[kind]
    a.V, a.G, a.GD, a.heads = V, G, GD, int(heads)
    a.ptr = ptr.data_ptr()
    a.T, a.ldT = T.data_ptr(), ldT
    a.lo = float("-inf") if lower is None else float(lower)
    a.hi = float("inf") if upper is None else float(upper)
    ws_bytes = lib.tfgnn_pool_workspace_bytes(V, G, GD, int(heads), a.kind)
    ws = _workspace(T.device, ws_bytes) if ws_bytes else None
    a.workspace, a.workspace_bytes = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    return T, ws


def pool_forward(kind: str, ptr: torch.Tensor, T: torch.Tensor, S: Optional[torch.Tensor], heads: int, lower=None, upper=None):
    """Graph readout forward in ONE library call (tfgnn_pool_forward): per-graph softmax of the scores S [V, heads] (kind
    "softmax"; "sigmoid": S already holds the weights; "none" / "average": S is None), clip of T [V, GD] to [lower, upper]
    (None = no bound) and the weighted sum per graph of ptr [G + 1].  -> (out [G, GD], w [V, heads] for "softmax" else None)."""
    a = _lib.PoolForwardArgs()
    T, ws = _pool_common(a, kind, ptr, T, heads, lower, upper)
    out = (torch.empty if a.V else torch.zeros)((a.G, a.GD), dtype=torch.float32, device=T.device)
    w = None
    if S is not None:
        _require_dev(S, torch.float32, "S")
        S, ldS = _rowmajor(S, "S")
        a.S, a.ldS = S.data_ptr(), ldS
        if kind == "softmax":
            w = torch.empty((a.V, int(heads)), dtype=torch.float32, device=T.device)
            a.w, a.ldw = w.data_ptr(), int(heads)
    a.out = out.data_ptr()
    stream = _stream()
    with op_scope("pool_forward", T, S, out):
        _lib.check(_lib.load().tfgnn_pool_forward(ctypes.byref(a), stream))
    return out, w


def pool_backward(kind: str, ptr: torch.Tensor, ids: Optional[torch.Tensor], grad_out: torch.Tensor, T: torch.Tensor,
                  w: Optional[torch.Tensor], heads: int, lower=None, upper=None, want_scores_grad: bool = True):
    """Gradient of ``pool_forward`` in ONE library call (tfgnn_pool_backward).  ``w``: what the forward returned ("softmax") or
    the sigmoid weights S ("sigmoid").  -> (dT [V, GD], dS [V, heads] or None): dS is the gradient with respect to the scores
    ("softmax") or to the sigmoid weights ("sigmoid")."""
    a = _lib.PoolBackwardArgs()
    T, ws = _pool_common(a, kind, ptr, T, heads, lower, upper)
    _require_dev(grad_out, torch.float32, "grad_out")
    grad_out = grad_out.contiguous()
    if tuple(grad_out.shape) != (a.G, a.GD):
        raise ValueError(f"pool_backward: grad_out must be [{a.G}, {a.GD}], got {tuple(grad_out.shape)}")
    dT = torch.empty((a.V, a.GD), dtype=torch.float32, device=T.device)
    dS = None
    if w is not None:
        w, ldw = _rowmajor(w, "w")
        a.w, a.ldw = w.data_ptr(), ldw
        if want_scores_grad:
            dS = torch.empty((a.V, int(heads)), dtype=torch.float32, device=T.device)
            a.dS, a.lddS = dS.data_ptr(), int(heads)
    a.ids = ids.data_ptr() if ids is not None else None
    a.dOut = grad_out.data_ptr()
    a.dT, a.lddT = dT.data_ptr(), a.GD
    stream = _stream()
    with op_scope("pool_backward", T, grad_out, dT):
        _lib.check(_lib.load().tfgnn_pool_backward(ctypes.byref(a), stream))
    return dT, dS


def pool_launch_counts() -> dict:
    """tfgnn_pool_launch_counts: kernel launches of the two graph-readout calls so far (host counters)."""
    buf = (ctypes.c_int64 * 2)()
    _lib.check(_lib.load().tfgnn_pool_launch_counts(buf, 2))
    return {"pool_fwd": int(buf[0]), "pool_bwd": int(buf[1])}


def _node_walk_vectors(who: str, graph: "Graph", anchor: torch.Tensor, anchor_name: str, edge_weights, node_scale):
    """The per-edge weights ([(name, tensor or None)]) and the node scale of a node-view walk: float32 device vectors of E / V
    floats on the device of ``anchor`` (the weight tensor, named ``anchor_name`` in the message)."""
    for name, t, n in [(k, t, graph.num_edges) for k, t in edge_weights] + [("node_scale", node_scale, graph.num_nodes)]:
        if t is None:
            continue
        _require_dev(t, torch.float32, name)
        if t.dim() != 1 or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous vector of {n} floats, got {tuple(t.shape)}")
        if t.device != anchor.device:
            raise ValueError(f"{who}: {name} lives on {t.device}, {anchor_name} on {anchor.device}")


def _node_walk_matrix(who: str, t: torch.Tensor, rows: int, cols: int, what: str, device, writable: bool = False):
    """A [rows, cols] float32 operand of a node-view walk -> (tensor with unit inner stride, row stride).  The device message
    names the basis layer's anchor whoever calls."""
    _require_dev(t, torch.float32, what)
    if t.dim() != 2 or tuple(t.shape) != (rows, cols):
        raise ValueError(f"{who}: {what} must be [{rows}, {cols}], got {tuple(t.shape)}")
    if t.device != device:
        raise ValueError(f"{who}: {what} lives on {t.device}, coeff on {device}")
    t2, ld = _rowmajor(t, what)
    if writable and t2 is not t:
        raise ValueError(f"{who}: {what} must have unit inner stride")
    return t2, ld


def _node_plan_partials(graph: "Graph"):
    """-> (by target, by source): the partial rows the node views' plans keep for rows made of several items"""
    lib = _lib.load()
    graph.ensure(G_PART_PLAN_NODE)
    return (lib.tfgnn_graph_gather_workspace_bytes(graph._h, VIEW_BY_DST_NODE, 1) // 4,
            lib.tfgnn_graph_gather_workspace_bytes(graph._h, VIEW_BY_SRC_NODE, 1) // 4)


def _basis_common(who: str, graph: "Graph", coeff: torch.Tensor, edge_weights, node_scale):
    """The checks the two basis-gather wrappers share -> (L, B, contiguous coeff)."""
    _require_dev(coeff, torch.float32, "coeff")
    L = graph.num_edge_types
    if coeff.dim() != 2 or coeff.shape[0] != L:
        raise ValueError(f"{who}: coeff must be [{L}, num_bases] (one row per edge type), got {tuple(coeff.shape)}")
    B = int(coeff.shape[1])
    if not 1 <= B <= _lib.BASIS_MAX_BASES:
        raise ValueError(f"{who}: num_bases = {B} is outside the limit 1 <= num_bases <= {_lib.BASIS_MAX_BASES}")
    _node_walk_vectors(who, graph, coeff, "coeff", edge_weights, node_scale)
    return L, B, coeff.contiguous()


def _basis_workspace(graph: "Graph", B: int, D: int, device):
    nbytes = _lib.load().tfgnn_basis_workspace_bytes(graph.num_nodes, graph.num_edges, graph.num_edge_types, B, D,
                                                     *_node_plan_partials(graph))
    return _aligned_workspace(device, nbytes) if nbytes else (None, 0, None)


@_writes_out
def basis_gather_forward(graph: "Graph", coeff: torch.Tensor, X: torch.Tensor, *, edge_weight: Optional[torch.Tensor] = None,
                         node_scale: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """R-GCN basis decomposition, the gather (tfgnn_basis_gather_forward): Z[v, b*D:(b+1)*D] = node_scale[v] * sum over the
    edges (u -> v) of type l of edge_weight[e] * coeff[l, b] * X[u].  ``edge_weight`` / ``node_scale``: what ``graph_scales``
    returns as ``edge_weight_by_dst`` / ``node_scale`` (None = 1).  X and ``out`` may be column slices of wider arrays."""
    who = "basis_gather_forward"
    L, B, coeff = _basis_common(who, graph, coeff, [("edge_weight", edge_weight)], node_scale)
    V = graph.num_nodes
    if X.dim() != 2 or X.shape[0] != V or X.shape[1] < 1:
        raise ValueError(f"{who}: X must be [{V}, D] with D >= 1, got {tuple(X.shape)}")
    D = int(X.shape[1])
    X, ldX = _node_walk_matrix(who, X, V, D, "X", coeff.device)
    if out is None:
        out = torch.empty((V, B * D), dtype=torch.float32, device=X.device)
    out, ldZ = _node_walk_matrix(who, out, V, B * D, "out", coeff.device, writable=True)
    ws_ptr, ws_len, ws = _basis_workspace(graph, B, D, X.device)
    a = _lib.BasisForwardArgs()
    a.struct_size = ctypes.sizeof(a)
    a.graph, a.B, a.D = graph._h, B, D
    a.coeff, a.X, a.ldX = coeff.data_ptr(), X.data_ptr(), ldX
    a.edge_weight_by_dst = None if edge_weight is None else edge_weight.data_ptr()
    a.node_scale = None if node_scale is None else node_scale.data_ptr()
    a.Z, a.ldZ = out.data_ptr(), ldZ
    a.workspace, a.workspace_bytes = ws_ptr, ws_len
    stream = _stream()
    with op_scope("basis_gather_forward", X, coeff, out):
        _lib.check(_lib.load().tfgnn_basis_gather_forward(ctypes.byref(a), stream))
    return out


def basis_gather_backward(graph: "Graph", coeff: torch.Tensor, dZ: torch.Tensor, X: Optional[torch.Tensor] = None, *,
                          edge_weight_by_dst: Optional[torch.Tensor] = None, edge_weight_by_src: Optional[torch.Tensor] = None,
                          node_scale: Optional[torch.Tensor] = None, want_dx: bool = True, want_dcoeff: bool = True,
                          out_dx: Optional[torch.Tensor] = None):
    """The two reverse passes of ``basis_gather_forward`` (tfgnn_basis_gather_backward) -> (dX [V, D] or None, dcoeff [L, B] or
    None).  ``edge_weight_by_src`` is ``graph_scales``' (it carries the target's node scale); X is read for dcoeff only.
    ``out_dx``: write dX there (may be a column slice of a wider array)."""
    who = "basis_gather_backward"
    L, B, coeff = _basis_common(who, graph, coeff, [("edge_weight_by_dst", edge_weight_by_dst),
                                                     ("edge_weight_by_src", edge_weight_by_src)], node_scale)
    V = graph.num_nodes
    if dZ.dim() != 2 or dZ.shape[0] != V or dZ.shape[1] < B or dZ.shape[1] % B:
        raise ValueError(f"{who}: dZ must be [{V}, num_bases * D] with num_bases = {B}, got {tuple(dZ.shape)}")
    D = int(dZ.shape[1]) // B
    dZ, lddZ = _node_walk_matrix(who, dZ, V, B * D, "dZ", coeff.device)
    a = _lib.BasisBackwardArgs()
    a.struct_size = ctypes.sizeof(a)
    a.graph, a.B, a.D = graph._h, B, D
    a.coeff, a.dZ, a.lddZ = coeff.data_ptr(), dZ.data_ptr(), lddZ
    dX = dcoeff = None
    if want_dcoeff:
        if X is None:
            raise ValueError(f"{who}: dcoeff needs X")
        X, ldX = _node_walk_matrix(who, X, V, D, "X", coeff.device)
        a.X, a.ldX = X.data_ptr(), ldX
        dcoeff = torch.empty((L, B), dtype=torch.float32, device=coeff.device)
        a.dcoeff = dcoeff.data_ptr()
    if want_dx:
        dX = out_dx if out_dx is not None else torch.empty((V, D), dtype=torch.float32, device=coeff.device)
        dX, lddX = _node_walk_matrix(who, dX, V, D, "out_dx", coeff.device, writable=True)
        a.dX, a.lddX = dX.data_ptr(), lddX
    a.edge_weight_by_dst = None if edge_weight_by_dst is None else edge_weight_by_dst.data_ptr()
    a.edge_weight_by_src = None if edge_weight_by_src is None else edge_weight_by_src.data_ptr()
    a.node_scale = None if node_scale is None else node_scale.data_ptr()
    ws_ptr, ws_len, ws = _basis_workspace(graph, B, D, coeff.device)
    a.workspace, a.workspace_bytes = ws_ptr, ws_len
    stream = _stream()
    with op_scope("basis_gather_backward", dZ, X, coeff, dX, dcoeff):
        _lib.check(_lib.load().tfgnn_basis_gather_backward(ctypes.byref(a), stream))
    if dX is not None:
        torch.autograd.graph.increment_version(dX)
    return dX, dcoeff


def basis_launch_counts() -> dict:
    """tfgnn_basis_launch_counts: kernel launches of the basis gather and its two reverse passes so far (host counters)."""
    buf = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().tfgnn_basis_launch_counts(buf, 3))
    return {"basis_fwd": int(buf[0]), "basis_dx": int(buf[1]), "basis_dcoeff": int(buf[2])}


def blockdiag_chunk_table(edges_per_type, chunk: int = _lib.BLOCKDIAG_CHUNK):
    """The chunk table of the block-diagonal weight gradient, on the host from the per-type edge counts alone: the concatenated
    edge lists are type-major, chunk k of type l is the list positions [first_l + chunk*k, first_l + min(E_l, chunk*(k+1))).
    -> (chunk_type, chunk_first, chunk_count, type_chunk_ptr [L + 1]) as lists; types ascending, a type's chunks ascending."""
    chunk_type, chunk_first, chunk_count, type_chunk_ptr = [], [], [], [0]
    first = 0
    for l, n in enumerate(int(n) for n in edges_per_type):
        for k in range(0, n, chunk):
            chunk_type.append(l)
            chunk_first.append(first + k)
            chunk_count.append(min(chunk, n - k))
        first += n
        type_chunk_ptr.append(len(chunk_type))
    return chunk_type, chunk_first, chunk_count, type_chunk_ptr


def _blockdiag_tables(graph: "Graph"):
    """The per-graph type-major tables tfgnn_blockdiag_backward reads for dQb, built once and kept with the Graph:
    -> (list_to_dst [E], chunk_first, chunk_count [num_chunks], type_chunk_ptr [L + 1], num_chunks).  list_to_dst inverts
    G_EID_BY_DST - a permutation, so one scatter without races; the chunk table comes from the host's edge counts (no read-back)."""
    hit = graph._cache.get("blockdiag_tables")
    if hit is None:
        if capturing():
            raise RuntimeError("tf2_gnn_amd: the block-diagonal layer's per-graph tables cannot be built inside a hipGraph capture; "
                               "run the step eagerly once on the same graph first (CapturedStep warmup)")
        E = graph.num_edges
        eid = graph.array(G_EID_BY_DST)
        list_to_dst = torch.empty(E, dtype=torch.int32, device=graph.device)
        if E:
            list_to_dst[eid.long()] = torch.arange(E, dtype=torch.int32, device=graph.device)
        _, first, count, ptr = blockdiag_chunk_table(graph.edges_per_type)
        n = len(first)
        host = torch.tensor(first + count + ptr, dtype=torch.int32)
        dev = host.to(graph.device)
        hit = (list_to_dst, dev[:n], dev[n:2 * n], dev[2 * n:], n)
        graph._cache["blockdiag_tables"] = hit
    return hit


def _blockdiag_common(who: str, graph: "Graph", Qb: torch.Tensor, num_blocks: int, edge_weights, node_scale):
    """The checks the two block-diagonal wrappers share -> (L, C, di, H, contiguous Qb)."""
    _require_dev(Qb, torch.float32, "Qb")
    L, C = graph.num_edge_types, int(num_blocks)
    if Qb.dim() != 3 or Qb.shape[0] != L or Qb.shape[1] < 1 or Qb.shape[2] < 1:
        raise ValueError(f"{who}: Qb must be [{L}, D / num_blocks, H] (banded blocks, one slab per edge type), got {tuple(Qb.shape)}")
    di, H = int(Qb.shape[1]), int(Qb.shape[2])
    if C < 1 or H % C:
        raise ValueError(f"{who}: num_blocks = {C} must be at least 1 and divide H = {H}")
    if di > _lib.BLOCKDIAG_MAX_BLOCK or H // C > _lib.BLOCKDIAG_MAX_BLOCK:
        raise ValueError(f"{who}: blocks of {di} x {H // C} are above the limit D / num_blocks <= {_lib.BLOCKDIAG_MAX_BLOCK} and "
                         f"H / num_blocks <= {_lib.BLOCKDIAG_MAX_BLOCK}")
    _node_walk_vectors(who, graph, Qb, "Qb", edge_weights, node_scale)
    return L, C, di, H, Qb.contiguous()


def _blockdiag_workspace(graph: "Graph", C: int, D: int, H: int, num_chunks: int, device):
    pd, ps = _node_plan_partials(graph)
    nbytes = _lib.load().tfgnn_blockdiag_workspace_bytes(C, D, H, pd, ps, num_chunks)
    return _aligned_workspace(device, nbytes) if nbytes else (None, 0, None)


@_writes_out
def blockdiag_forward(graph: "Graph", Qb: torch.Tensor, X: torch.Tensor, num_blocks: int, *,
                      edge_weight: Optional[torch.Tensor] = None, node_scale: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """R-GCN block-diagonal decomposition, forward (tfgnn_blockdiag_forward): pre[v, h] = node_scale[v] * sum over the edges
    (u -> v) of type l of edge_weight[e] * sum_i X[u, c(h)*di + i] * Qb[l, i, h], Qb [L, di, H] the banded blocks.
    ``edge_weight`` / ``node_scale``: what ``graph_scales`` returns as ``edge_weight_by_dst`` / ``node_scale`` (None = 1).  X and
    ``out`` may be column slices of wider arrays."""
    who = "blockdiag_forward"
    L, C, di, H, Qb = _blockdiag_common(who, graph, Qb, num_blocks, [("edge_weight", edge_weight)], node_scale)
    V, D = graph.num_nodes, C * di
    X, ldX = _node_walk_matrix(who, X, V, D, "X", Qb.device)
    if out is None:
        out = torch.empty((V, H), dtype=torch.float32, device=X.device)
    out, ldpre = _node_walk_matrix(who, out, V, H, "out", Qb.device, writable=True)
    ws_ptr, ws_len, ws = _blockdiag_workspace(graph, C, D, H, 0, X.device)
    a = _lib.BlockdiagForwardArgs()
    a.struct_size = ctypes.sizeof(a)
    a.graph, a.C, a.D, a.H = graph._h, C, D, H
    a.Qb, a.X, a.ldX = Qb.data_ptr(), X.data_ptr(), ldX
    a.edge_weight_by_dst = None if edge_weight is None else edge_weight.data_ptr()
    a.node_scale = None if node_scale is None else node_scale.data_ptr()
    a.pre, a.ldpre = out.data_ptr(), ldpre
    a.workspace, a.workspace_bytes = ws_ptr, ws_len
    stream = _stream()
    with op_scope("blockdiag_forward", X, Qb, out):
        _lib.check(_lib.load().tfgnn_blockdiag_forward(ctypes.byref(a), stream))
    return out


def blockdiag_backward(graph: "Graph", Qb: torch.Tensor, dPre: torch.Tensor, X: Optional[torch.Tensor], num_blocks: int, *,
                       edge_weight_by_dst: Optional[torch.Tensor] = None, edge_weight_by_src: Optional[torch.Tensor] = None,
                       node_scale: Optional[torch.Tensor] = None, want_dx: bool = True, want_dq: bool = True,
                       out_dx: Optional[torch.Tensor] = None):
    """The two reverse passes of ``blockdiag_forward`` (tfgnn_blockdiag_backward) -> (dX [V, D] or None, dQb [L, di, H] or None).
    ``edge_weight_by_src`` is ``graph_scales``' (it carries the target's node scale); X is read for dQb only.  ``out_dx``: write
    dX there (may be a column slice of a wider array)."""
    who = "blockdiag_backward"
    L, C, di, H, Qb = _blockdiag_common(who, graph, Qb, num_blocks, [("edge_weight_by_dst", edge_weight_by_dst),
                                                                    ("edge_weight_by_src", edge_weight_by_src)], node_scale)
    V, D = graph.num_nodes, C * di
    dPre, lddPre = _node_walk_matrix(who, dPre, V, H, "dPre", Qb.device)
    a = _lib.BlockdiagBackwardArgs()
    a.struct_size = ctypes.sizeof(a)
    a.graph, a.C, a.D, a.H = graph._h, C, D, H
    a.Qb, a.dPre, a.lddPre = Qb.data_ptr(), dPre.data_ptr(), lddPre
    dX = dQb = tables = None
    num_chunks = 0
    if want_dq:
        if X is None:
            raise ValueError(f"{who}: dQb needs X")
        X, ldX = _node_walk_matrix(who, X, V, D, "X", Qb.device)
        a.X, a.ldX = X.data_ptr(), ldX
        dQb = torch.empty((L, di, H), dtype=torch.float32, device=Qb.device)
        a.dQb = dQb.data_ptr()
        tables = _blockdiag_tables(graph)
        num_chunks = tables[4]
        a.list_to_dst, a.chunk_first, a.chunk_count, a.type_chunk_ptr = (t.data_ptr() for t in tables[:4])
        a.num_chunks = num_chunks
    if want_dx:
        dX = out_dx if out_dx is not None else torch.empty((V, D), dtype=torch.float32, device=Qb.device)
        dX, lddX = _node_walk_matrix(who, dX, V, D, "out_dx", Qb.device, writable=True)
        a.dX, a.lddX = dX.data_ptr(), lddX
    a.edge_weight_by_dst = None if edge_weight_by_dst is None else edge_weight_by_dst.data_ptr()
    a.edge_weight_by_src = None if edge_weight_by_src is None else edge_weight_by_src.data_ptr()
    a.node_scale = None if node_scale is None else node_scale.data_ptr()
    ws_ptr, ws_len, ws = _blockdiag_workspace(graph, C, D, H, num_chunks, Qb.device)
    a.workspace, a.workspace_bytes = ws_ptr, ws_len
    stream = _stream()
    with op_scope("blockdiag_backward", dPre, X, Qb, dX, dQb):
        _lib.check(_lib.load().tfgnn_blockdiag_backward(ctypes.byref(a), stream))
    if dX is not None:
        torch.autograd.graph.increment_version(dX)
    return dX, dQb


def blockdiag_launch_counts() -> dict:
    """tfgnn_blockdiag_launch_counts: kernel launches of the block-diagonal forward and its two reverse passes so far."""
    buf = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().tfgnn_blockdiag_launch_counts(buf, 3))
    return {"fwd": int(buf[0]), "dx": int(buf[1]), "dq": int(buf[2])}


def graph_scales_edge_dropout(graph: "Graph", normalize: bool, aggregation_mode: int, rates: torch.Tensor, seed: int):
    """One step's edge dropout (tfgnn_graph_scales_edge_dropout) -> (node_scale [V], edge_weight_by_src [E], edge_weight_by_dst
    [E]): edge e of type l is kept iff element e of the mask ``dropout_forward`` draws for (seed, rates[l]) at the current
    dropout epoch is non-zero; the counts that divide are those of the kept edges, and where none divides (``normalize`` False,
    mode 0) kept edges carry 1 / (1 - rates[l]).  ``rates``: float32 device tensor [L], every rate in [0, 1) (the caller's to
    validate: the kernel clamps).  Needs the handle's part EDGE_MAPS, which cannot be built inside a hipGraph capture."""
    who = "graph_scales_edge_dropout"
    _require_dev(rates, torch.float32, "rates")
    L = graph.num_edge_types
    if rates.dim() != 1 or rates.numel() != L or not rates.is_contiguous():
        raise ValueError(f"{who}: rates must be a contiguous vector of {L} floats (one per edge type), got {tuple(rates.shape)}")
    if rates.device != graph.device:
        raise ValueError(f"{who}: rates live on {rates.device}, the graph on {graph.device}")
    if aggregation_mode not in (0, 1, 2):
        raise ValueError(f"{who}: aggregation_mode must be 0 (sum), 1 (mean) or 2 (sqrt_n), got {aggregation_mode!r}")
    need = G_PART_EDGE_MAPS | G_PART_EDGE_IDS
    if need & ~graph.parts:
        if capturing():
            raise RuntimeError("tf2_gnn_amd: edge dropout needs the graph's part EDGE_MAPS, which cannot be built inside a hipGraph "
                               "capture (the build reads sizes back); run the step eagerly once on the same graph first "
                               "(CapturedStep warmup), or name the part when the graph is made (GNN.graph_parts does)")
        graph.ensure(need)
    dev = graph.device
    node_scale = torch.empty(graph.num_nodes, dtype=torch.float32, device=dev)
    ew_s = torch.empty(graph.num_edges, dtype=torch.float32, device=dev)
    ew_d = torch.empty(graph.num_edges, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().tfgnn_graph_scales_edge_dropout(
        graph._h, int(bool(normalize)), int(aggregation_mode), _ptr(rates), int(seed) & (2**64 - 1), _ptr(node_scale),
        _ptr(ew_s), _ptr(ew_d), _stream()))
    return node_scale, ew_s, ew_d


def edge_dropout_launch_counts() -> dict:
    """tfgnn_edge_dropout_launch_counts: launches of ``graph_scales_edge_dropout``'s kernel so far (host counter)."""
    buf = (ctypes.c_int64 * 1)()
    _lib.check(_lib.load().tfgnn_edge_dropout_launch_counts(buf, 1))
    return {"edge_dropout_scales": int(buf[0])}


def mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    a = a.contiguous()
    b = b.contiguous()
    out = torch.empty_like(a)
    _lib.check(lib.tfgnn_mul(_ptr(a), _ptr(b), _ptr(out), a.numel(), _stream()))
    return out


def layernorm_forward(x, gamma, beta, eps: float = 1e-3):
    lib = _lib.load()
    x = x.contiguous()
    rows, H = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    _lib.check(
        lib.tfgnn_layernorm_forward(_ptr(x), _ptr(gamma), _ptr(beta), float(eps), rows, H, _ptr(y), _ptr(mean),
                                    _ptr(rstd), _stream())
    )
    return y, mean, rstd


def layernorm_backward(dy, x, gamma, mean, rstd):
    """-> (dx, dgamma, dbeta)"""
    lib = _lib.load()
    dy = dy.contiguous()
    rows, H = x.shape
    dx = torch.empty_like(x)
    dy_xhat = torch.empty_like(x)
    _lib.check(
        lib.tfgnn_layernorm_backward(_ptr(dy), _ptr(x), _ptr(gamma), _ptr(mean), _ptr(rstd), rows, H, _ptr(dx),
                                     _ptr(dy_xhat), _stream())
    )
    return dx, colsum(dy_xhat), colsum(dy)


def permute_021(x: torch.Tensor) -> torch.Tensor:
    """[A, B, C] -> [B, A, C] (contiguous copy)."""
    lib = _lib.load()
    x = x.contiguous()
    A, B, C = x.shape
    out = torch.empty((B, A, C), dtype=torch.float32, device=x.device)
    _lib.check(lib.tfgnn_permute_021(_ptr(x), A, B, C, _ptr(out), _stream()))
    return out


def edge_aggregate_backward(msg, target, grad_agg, *, msg_row=None, edge_weight=None, node_scale=None, pre_act=ACT_NONE,
                            reduce=REDUCE_SUM, agg_max=None, num_selected=None, phase=1) -> torch.Tensor:
    """Per-edge gradient through agg[t] = node_scale[t] * REDUCE_{e->t} pre_act(w_e * msg[row_e]) (phase 1), or the
    0/1 indicator of the edges that attain a target's maximum (phase 0).  -> [E, width]"""
    lib = _lib.load()
    _require_dev(msg, torch.float32, "msg")
    msg, ld = _rowmajor(msg, "msg")
    E = target.numel()
    width = msg.shape[1]
    out = torch.empty((E, width), dtype=torch.float32, device=msg.device)
    for t in (grad_agg, agg_max, num_selected):
        if t is not None and (not t.is_contiguous() or t.shape[-1] != width):
            raise ValueError("grad_agg / agg_max / num_selected must be contiguous [V, width]")
    _lib.check(
        lib.tfgnn_edge_aggregate_backward(
            E, width, _ptr(msg), ld, _ptr(msg_row), _ptr(target), _ptr(edge_weight), _ptr(node_scale), act_id(pre_act),
            int(reduce), _ptr(grad_agg), _ptr(agg_max), _ptr(num_selected), int(phase), _ptr(out), _stream(),
        )
    )
    return out


def transpose_batched(x: torch.Tensor) -> torch.Tensor:
    """[B, R, C] -> [B, C, R] (contiguous copy); a 2-D input is one batch."""
    lib = _lib.load()
    _require_dev(x, torch.float32, "x")
    x = x.contiguous()
    squeeze = x.dim() == 2
    if squeeze:
        x = x.unsqueeze(0)
    B, R, C = x.shape
    out = torch.empty((B, C, R), dtype=torch.float32, device=x.device)
    _lib.check(lib.tfgnn_transpose_batched(_ptr(x), B, R, C, _ptr(out), _stream()))
    return out[0] if squeeze else out


@_writes_out
def gemm_grouped_rows(a, group_off_dev, group_off_host, b_stack, *, trans_b=False, act=ACT_NONE, out=None, act_grad=None):
    """out[rows g] = act(a[rows g] @ op(b_stack[g])) for row groups [off[g], off[g+1]).
    b_stack: [G, K, N] (or [G, N, K] with trans_b).  act_grad = (activation, saved [rows, N]): the result times act'(saved),
    in the product's epilogue where the active kernel has one (tfgnn_gemm_grouped_rows_grad), by a separate pass otherwise."""
    lib = _lib.load()
    a, lda = _rowmajor(a, "a")
    G = b_stack.shape[0]
    K = a.shape[1]
    N = b_stack.shape[1] if trans_b else b_stack.shape[2]
    b_stack = b_stack.contiguous()
    if (not trans_b and a.shape[0] >= 4096 * max(G, 1) // 8 and K >= 64 and K % 4 == 0
            and (N % 320 == 0 or N % 128 == 0) and get_gemm_mode() != GEMM_FP32):
        # as in gemm(): the split-operand kernel stages K-contiguous weights fastest; [G, K, N] -> [G, N, K] once
        b_stack, trans_b = transpose_batched(b_stack), True
    if out is None:
        out = torch.empty((a.shape[0], N), dtype=torch.float32, device=a.device)
    out2, ldc = _rowmajor(out, "out")
    max_rows = max((group_off_host[i + 1] - group_off_host[i] for i in range(G)), default=0)
    if act_grad is not None:
        if act_id(act) != act_id(ACT_NONE):
            raise ValueError("gemm_grouped_rows: act and act_grad exclude each other")
        saved, ld_saved = _rowmajor(act_grad[1], "saved")
        if tuple(saved.shape) != (a.shape[0], N):
            raise ValueError(f"saved must be [{a.shape[0]},{N}]")
        rc = lib.tfgnn_gemm_grouped_rows_grad(
            int(trans_b), G, _ptr(group_off_dev), max_rows, N, K, _ptr(a), lda, _ptr(b_stack), b_stack.stride(1),
            b_stack.stride(0), _ptr(out), ldc, act_id(act_grad[0]), _ptr(saved), ld_saved, _stream())
        if rc == 0:
            return out
        if rc != -4:
            _lib.check(rc)
        res = gemm_grouped_rows(a, group_off_dev, group_off_host, b_stack, trans_b=trans_b, out=out)
        return activation_backward(act_grad[0], res, act_grad[1])
    _lib.check(
        lib.tfgnn_gemm_grouped_rows(
            int(trans_b), G, _ptr(group_off_dev), max_rows, N, K, _ptr(a), lda, _ptr(b_stack), b_stack.stride(1),
            b_stack.stride(0), _ptr(out), ldc, act_id(act), _stream(),
        )
    )
    return out


@_writes_out
def gemm_grouped_k(a, b, group_off_dev, group_off_host, num_groups, out=None):
    """out[g] = a[rows g]^T @ b[rows g]  ->  [G, M, N]."""
    lib = _lib.load()
    a, lda = _rowmajor(a, "a")
    b, ldb = _rowmajor(b, "b")
    M, N = a.shape[1], b.shape[1]
    if out is None:
        out = torch.empty((num_groups, M, N), dtype=torch.float32, device=a.device)
    max_rows = max((group_off_host[i + 1] - group_off_host[i] for i in range(num_groups)), default=0)
    ws_bytes = lib.tfgnn_gemm_grouped_k_workspace_bytes(num_groups, max_rows, M, N)
    ws = _workspace(a.device, ws_bytes) if ws_bytes else None
    _lib.check(
        lib.tfgnn_gemm_grouped_k(
            num_groups, _ptr(group_off_dev), max_rows, M, N, _ptr(a), lda, _ptr(b), ldb, _ptr(out), out.stride(1),
            out.stride(0), _ptr(ws), ws.numel() if ws is not None else 0, _stream(),
        )
    )
    return out


def sigmoid_ce_metrics(logits: torch.Tensor, labels: torch.Tensor, need_grad: bool = True):
    """NodeMulticlassTask._fast_task_metrics (tf2_gnn/models/node_multiclass_task.py:62-70) ->
    (metrics [2] = (loss, micro-F1) on the device, counts [3] int64 = (tp, fp, fn), d loss / d logits or None)."""
    lib = _lib.load()
    _require_dev(logits, torch.float32, "logits")
    _require_dev(labels, torch.float32, "labels")
    logits, ldx = _rowmajor(logits, "logits")
    labels, ldz = _rowmajor(labels, "labels")
    if logits.shape != labels.shape:
        raise ValueError(f"logits {tuple(logits.shape)} and labels {tuple(labels.shape)} differ in shape")
    V, C = logits.shape
    metrics = torch.empty(2, dtype=torch.float32, device=logits.device)
    counts = torch.empty(3, dtype=torch.int64, device=logits.device)
    grad = torch.empty((V, C), dtype=torch.float32, device=logits.device) if need_grad else None
    nbytes = lib.tfgnn_task_metrics_workspace_bytes()
    ws = _workspace(logits.device, nbytes)
    _lib.check(lib.tfgnn_sigmoid_ce_metrics(_ptr(logits), ldx, _ptr(labels), ldz, V, C, _ptr(metrics), _ptr(counts), _ptr(grad),
                                            _ptr(ws), ws.numel(), _stream()))
    return metrics, counts, grad


def regression_metrics(pred: torch.Tensor, target: torch.Tensor, need_grad: bool = True):
    """tf.losses.mean_squared_error / mean_absolute_error of per-graph outputs
    (tf2_gnn/models/graph_regression_task.py:157-158) -> (metrics [2] = (mse, mae), d mse / d pred or None)."""
    lib = _lib.load()
    _require_dev(pred, torch.float32, "pred")
    _require_dev(target, torch.float32, "target")
    pred = pred.contiguous().view(-1)
    target = target.contiguous().view(-1)
    if pred.shape != target.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    metrics = torch.empty(2, dtype=torch.float32, device=pred.device)
    grad = torch.empty_like(pred) if need_grad else None
    nbytes = lib.tfgnn_task_metrics_workspace_bytes()
    ws = _workspace(pred.device, nbytes)
    _lib.check(lib.tfgnn_regression_metrics(_ptr(pred), _ptr(target), pred.numel(), _ptr(metrics), _ptr(grad), _ptr(ws),
                                            ws.numel(), _stream()))
    return metrics, grad


def binary_ce_metrics(logits: torch.Tensor, target: torch.Tensor, need_grad: bool = True, want_prob: bool = True):
    """GraphBinaryClassificationTask.compute_task_metrics on the per-graph logits
    (tf2_gnn/models/graph_binary_classification_task.py:31-58; the arithmetic: include/tfgnn.h tfgnn_binary_ce_metrics) ->
    (metrics [2] = (loss, batch accuracy) on the device, counts [4] int64 = (tp, fp, tn, fn), sigmoid(logits) or None,
    d loss / d logits or None)."""
    lib = _lib.load()
    _require_dev(logits, torch.float32, "logits")
    _require_dev(target, torch.float32, "target")
    logits = logits.contiguous().view(-1)
    target = target.contiguous().view(-1)
    if logits.shape != target.shape:
        raise ValueError(f"logits {tuple(logits.shape)} and target {tuple(target.shape)} differ in shape")
    metrics = torch.empty(2, dtype=torch.float32, device=logits.device)
    counts = torch.empty(4, dtype=torch.int64, device=logits.device)
    prob = torch.empty_like(logits) if want_prob else None
    grad = torch.empty_like(logits) if need_grad else None
    nbytes = lib.tfgnn_task_metrics_workspace_bytes()
    ws = _workspace(logits.device, nbytes)
    _lib.check(lib.tfgnn_binary_ce_metrics(_ptr(logits), _ptr(target), logits.numel(), _ptr(prob), _ptr(metrics), _ptr(counts),
                                           _ptr(grad), _ptr(ws), ws.numel(), _stream()))
    return metrics, counts, prob, grad


def _node_column(t: torch.Tensor, V: int, what: str):
    """One fp32 value per node - [V], [V, 1] or a strided column view of either - as (tensor, element stride); no copy."""
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1 or t.shape[0] != V:
        raise ValueError(f"{what} {tuple(t.shape)} must hold one value per node: [{V}] or [{V}, 1]")
    stride = t.stride(0) if V > 1 else 1
    if stride < 1:  # an expanded (stride 0) or flipped view
        t, stride = t.contiguous(), 1
    return t, stride


@_writes_out
def softmax_ce_metrics(logits: torch.Tensor, labels: torch.Tensor, weights: Optional[torch.Tensor] = None,
                       need_grad: bool = True, want_pred: bool = False, out: Optional[torch.Tensor] = None):
    """Weighted softmax cross-entropy of per-node logits [V, C] against one class per node (include/tfgnn.h
    tfgnn_softmax_ce_metrics: a node is counted iff its weight is > 0 and its label an integer in [0, C)) ->
    (metrics [2] = (loss, accuracy) on the device, counts [2] int64 = (correct, counted), d loss / d logits or None,
    argmax int32 [V] or None).  ``labels`` / ``weights``: [V], [V, 1] or a strided column view (passed by stride, not
    copied); integer labels are cast to float32 once.  ``out``: where the gradient goes instead of a new tensor - a float32
    [V, C] with unit inner stride, e.g. C columns of a wider array, whose other columns stay as they are."""
    lib = _lib.load()
    _require_dev(logits, torch.float32, "logits")
    if not labels.is_floating_point():
        labels = labels.to(torch.float32)
    _require_dev(labels, torch.float32, "labels")
    if weights is not None:
        _require_dev(weights, torch.float32, "weights")
    logits, ldx = _rowmajor(logits, "logits")
    V, C = logits.shape
    labels, ldy = _node_column(labels, V, "labels")
    ldw = 0
    if weights is not None:
        weights, ldw = _node_column(weights, V, "weights")
    metrics = torch.empty(2, dtype=torch.float32, device=logits.device)
    counts = torch.empty(2, dtype=torch.int64, device=logits.device)
    grad, ldd = None, max(C, 1)
    if out is not None:
        _require_dev(out, torch.float32, "out")
        if tuple(out.shape) != (V, C) or (C > 1 and out.stride(1) != 1) or (V > 1 and out.stride(0) < C):
            raise ValueError(f"out must be a float32 [{V}, {C}] with unit inner stride, got {tuple(out.shape)} / {out.stride()}")
        grad, ldd = out, (out.stride(0) if V > 1 else max(C, 1))
    elif need_grad:
        grad = torch.empty((V, C), dtype=torch.float32, device=logits.device)
    pred = torch.empty(V, dtype=torch.int32, device=logits.device) if want_pred else None
    ws = _workspace(logits.device, lib.tfgnn_softmax_ce_workspace_bytes())
    _lib.check(lib.tfgnn_softmax_ce_metrics(_ptr(logits), ldx, _ptr(labels), ldy, _ptr(weights), ldw, V, C, _ptr(metrics),
                                            _ptr(counts), _ptr(grad), ldd, _ptr(pred), _ptr(ws), ws.numel(), _stream()))
    return metrics, counts, grad, pred


# ---- link prediction decoders: include/tfgnn.h tfgnn_distmult_* / tfgnn_complex_*, csrc/link.hip ---------------------------
def check_triples(triples, V: int, T: int, what: str = "triples") -> np.ndarray:
    """Host triples [N, 3] (source, relation, target) as a contiguous int32 array, every index in range - the check the
    kernels leave to the host (include/tfgnn.h).  Raises ValueError otherwise."""
    a = np.asarray(triples)
    if a.ndim != 2 or a.shape[1] != 3 or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be an integer [N, 3] array of (source, relation, target), not {a.dtype} {list(a.shape)}")
    if a.shape[0] > 2 ** 30:
        raise ValueError(f"{what}: more than 2^30 triples")
    if not (1 <= V < 2 ** 31 and 1 <= T < 2 ** 31):
        raise ValueError(f"{what}: the numbers of nodes ({V}) and relations ({T}) must be in [1, 2^31)")
    a = a.astype(np.int64)
    if a.shape[0]:
        bad = (a[:, 0] < 0) | (a[:, 0] >= V) | (a[:, 2] < 0) | (a[:, 2] >= V) | (a[:, 1] < 0) | (a[:, 1] >= T)
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            raise ValueError(f"{what}: row {k} {tuple(int(x) for x in a[k])} is outside {V} nodes / {T} relations")
    return np.ascontiguousarray(a, dtype=np.int32)


def build_triple_tables(triples, V: int, T: int) -> Dict[str, np.ndarray]:
    """The int32 tables tfgnn_distmult_backward walks (include/tfgnn.h "Triple tables"), from host triples [N, 3]:
    ``node_offsets`` [V + 1] / ``node_entries`` [2 N] (entry 2 e + role, role 0 = source, 1 = target, ascending within a
    node) and ``rel_offsets`` [T + 1] / ``rel_order`` [N] (triples grouped by relation, stably).  Validates the triples."""
    a = check_triples(triples, V, T).astype(np.int64)
    N = a.shape[0]
    nodes = np.stack([a[:, 0], a[:, 2]], axis=1).reshape(-1)  # position 2 e + role holds the node of that role
    node_entries = np.argsort(nodes, kind="stable")
    node_offsets = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(nodes, minlength=V), out=node_offsets[1:])
    rel_order = np.argsort(a[:, 1], kind="stable")
    rel_offsets = np.zeros(T + 1, dtype=np.int64)
    np.cumsum(np.bincount(a[:, 1], minlength=T), out=rel_offsets[1:])
    as_i32 = lambda x: x.astype(np.uint32).view(np.int32)  # 2 N = 2^31 at the limit: the kernels read offsets as unsigned
    return {"node_offsets": as_i32(node_offsets), "node_entries": node_entries.astype(np.int32),
            "rel_offsets": as_i32(rel_offsets), "rel_order": rel_order.astype(np.int32)}


TRIPLE_TABLE_NAMES = ("node_offsets", "node_entries", "rel_offsets", "rel_order")


LINK_DECODERS = ("distmult", "complex")


def _link_common(H: torch.Tensor, R: torch.Tensor, triples, what: str, decoder: str = "distmult"):
    """-> (H, ld_H, R, triples on the device, V, T, N, D).  Host triples (numpy) are validated and uploaded; a device tensor is
    taken as validated by whoever uploaded it (build_triple_tables / check_triples): reading it back would synchronise.
    ``decoder`` "complex": a row is [re ; im], so an odd width is a ValueError."""
    if decoder == "complex" and isinstance(H, torch.Tensor) and H.dim() == 2 and H.shape[1] % 2:
        raise ValueError(f"the ComplEx decoder reads a row as [re ; im] halves: the width must be even, not {H.shape[1]}")
    _require_dev(H, torch.float32, "H")
    _require_dev(R, torch.float32, "R")
    H, ldh = _rowmajor(H, "H")
    if R.dim() != 2 or R.shape[1] != H.shape[1]:
        raise ValueError(f"R {tuple(R.shape)} must be [T, {H.shape[1]}]")
    R = R.contiguous()
    V, D = H.shape
    T = R.shape[0]
    if not isinstance(triples, torch.Tensor):
        triples = torch.from_numpy(check_triples(triples, V, T, what)).to(H.device)
    _require_dev(triples, torch.int32, what)
    if triples.dim() != 2 or triples.shape[1] != 3:
        raise ValueError(f"{what} must be [N, 3], got {tuple(triples.shape)}")
    triples = triples.contiguous()
    return H, ldh, R, triples, V, T, triples.shape[0], D


def _link_ce_metrics(decoder, H, R, triples, labels, weights, need_grad, want_scores, want_counts):
    lib = _lib.load()
    H, ldh, R, triples, V, T, N, D = _link_common(H, R, triples, "triples", decoder)
    _require_dev(labels, torch.float32, "labels")
    labels, ldy = _node_column(labels, N, "labels")
    ldw = 0
    if weights is not None:
        _require_dev(weights, torch.float32, "weights")
        weights, ldw = _node_column(weights, N, "weights")
    dev = H.device
    metrics = torch.empty(2, dtype=torch.float32, device=dev)
    counts = torch.empty(4, dtype=torch.int64, device=dev) if want_counts else None
    scores = torch.empty(N, dtype=torch.float32, device=dev) if want_scores else None
    gscore = torch.empty(N, dtype=torch.float32, device=dev) if need_grad else None
    ws = _workspace(dev, getattr(lib, f"tfgnn_{decoder}_ce_workspace_bytes")())
    _lib.check(getattr(lib, f"tfgnn_{decoder}_ce_metrics")(_ptr(H), ldh, _ptr(R), _ptr(triples), _ptr(labels), ldy, _ptr(weights), ldw,
                                                           V, T, N, D, _ptr(metrics), _ptr(counts), _ptr(scores), _ptr(gscore),
                                                           _ptr(ws), ws.numel(), _stream()))
    return metrics, counts, scores, gscore


def distmult_ce_metrics(H: torch.Tensor, R: torch.Tensor, triples, labels: torch.Tensor, weights: Optional[torch.Tensor] = None,
                        need_grad: bool = True, want_scores: bool = True, want_counts: bool = True):
    """DistMult scores of ``triples`` [N, 3] from node representations H [V, D] and relation embeddings R [T, D], their
    weighted sigmoid cross-entropy against ``labels`` (0 / 1), confusion counts and d loss / d score (include/tfgnn.h
    tfgnn_distmult_ce_metrics: a triple is counted iff its weight is > 0 and its label exactly 0 or 1) ->
    (metrics [2] = (loss, accuracy), counts int64 [4] = (tp, fp, tn, fn) or None, scores [N] or None, gscore [N] or None),
    all on the device.  ``labels`` / ``weights``: [N], [N, 1] or a strided column view, passed by stride."""
    return _link_ce_metrics("distmult", H, R, triples, labels, weights, need_grad, want_scores, want_counts)


def complex_ce_metrics(H: torch.Tensor, R: torch.Tensor, triples, labels: torch.Tensor, weights: Optional[torch.Tensor] = None,
                       need_grad: bool = True, want_scores: bool = True, want_counts: bool = True):
    """``distmult_ce_metrics`` with the ComplEx score s = Re sum_k H[u, k] R[t, k] conj(H[v, k]), a row of H or R being the
    complex vector [re ; im] (include/tfgnn.h tfgnn_complex_ce_metrics): the same arguments, outputs and counting rule.  An
    odd width is a ValueError."""
    return _link_ce_metrics("complex", H, R, triples, labels, weights, need_grad, want_scores, want_counts)


def _link_backward(decoder, H, R, triples, gscore, tables, want_dH, want_dR, accumulate, out):
    lib = _lib.load()
    H, ldh, R, triples, V, T, N, D = _link_common(H, R, triples, "triples", decoder)
    _require_dev(gscore, torch.float32, "gscore")
    if gscore.dim() != 1 or gscore.shape[0] != N:
        raise ValueError(f"gscore {tuple(gscore.shape)} must be [{N}]")
    gscore = gscore.contiguous()
    sizes = {"node_offsets": V + 1, "node_entries": 2 * N, "rel_offsets": T + 1, "rel_order": N}
    tabs = {}
    for name in TRIPLE_TABLE_NAMES:
        t = tables[name]
        _require_dev(t, torch.int32, name)
        if t.dim() != 1 or t.shape[0] != sizes[name] or not t.is_contiguous():
            raise ValueError(f"{name} {tuple(t.shape)} must be a contiguous int32 [{sizes[name]}]")
        tabs[name] = t
    dev = H.device
    dH, ldd = None, max(D, 1)
    if out is not None:
        _require_dev(out, torch.float32, "out")
        if tuple(out.shape) != (V, D) or (D > 1 and out.stride(1) != 1) or (V > 1 and out.stride(0) < D):
            raise ValueError(f"out must be a float32 [{V}, {D}] with unit inner stride, got {tuple(out.shape)} / {out.stride()}")
        dH, ldd = out, (out.stride(0) if V > 1 else max(D, 1))
    elif want_dH:
        if accumulate:
            raise ValueError("accumulate needs the tensor to add to: out=")
        dH = torch.empty((V, D), dtype=torch.float32, device=dev)
    dR = torch.empty((T, D), dtype=torch.float32, device=dev) if want_dR else None
    ws = _workspace(dev, getattr(lib, f"tfgnn_{decoder}_backward_workspace_bytes")(N, D))
    _lib.check(getattr(lib, f"tfgnn_{decoder}_backward")(_ptr(H), ldh, _ptr(R), _ptr(triples), _ptr(gscore), _ptr(tabs["node_offsets"]),
                                                         _ptr(tabs["node_entries"]), _ptr(tabs["rel_offsets"]), _ptr(tabs["rel_order"]),
                                                         V, T, N, D, _ptr(dH), ldd, int(bool(accumulate)), _ptr(dR), _ptr(ws),
                                                         ws.numel(), _stream()))
    return dH, dR


@_writes_out
def distmult_backward(H: torch.Tensor, R: torch.Tensor, triples, gscore: torch.Tensor, tables: Dict[str, torch.Tensor],
                      want_dH: bool = True, want_dR: bool = True, accumulate: bool = False, out: Optional[torch.Tensor] = None):
    """d loss / d H [V, D] and d loss / d R [T, D] from ``gscore`` [N] (include/tfgnn.h tfgnn_distmult_backward; the sum order is
    stated there) -> (dH or None, dR or None).  ``tables``: the four int32 device tensors of ``build_triple_tables``.  ``out``:
    where dH goes instead of a new tensor - a float32 [V, D] with unit inner stride, e.g. D columns of a wider array whose
    other columns stay as they are; with ``accumulate`` the sums are added to what it holds."""
    return _link_backward("distmult", H, R, triples, gscore, tables, want_dH, want_dR, accumulate, out)


@_writes_out
def complex_backward(H: torch.Tensor, R: torch.Tensor, triples, gscore: torch.Tensor, tables: Dict[str, torch.Tensor],
                     want_dH: bool = True, want_dR: bool = True, accumulate: bool = False, out: Optional[torch.Tensor] = None):
    """``distmult_backward`` for the ComplEx score (include/tfgnn.h tfgnn_complex_backward: the same tables, the same sum
    order, the term of an entry depending on whether the node is the triple's source or target)."""
    return _link_backward("complex", H, R, triples, gscore, tables, want_dH, want_dR, accumulate, out)


def check_rank_filter(filter_offsets, filter_ids, Q: int, V: int):
    """Host filter CSR of tfgnn_distmult_rank as two contiguous int32 arrays: offsets [Q + 1] ascending from 0, ids in [0, V),
    strictly ascending within a query.  Raises ValueError otherwise."""
    off = np.asarray(filter_offsets).astype(np.int64).reshape(-1)
    ids = np.asarray(filter_ids).astype(np.int64).reshape(-1)
    if off.shape[0] != Q + 1 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != ids.shape[0] or ids.shape[0] >= 2 ** 31:
        raise ValueError(f"filter_offsets must be [{Q + 1}], ascending from 0 to the number of filter ids ({ids.shape[0]})")
    if ids.shape[0]:
        if ids.min() < 0 or ids.max() >= V:
            raise ValueError(f"a filter id is outside the {V} nodes")
        inner = np.ones(ids.shape[0], dtype=bool)
        inner[off[:-1][off[:-1] < ids.shape[0]]] = False  # first id of a query
        if (np.diff(ids) <= 0)[inner[1:]].any():
            raise ValueError("filter ids must be sorted and unique within a query")
    return np.ascontiguousarray(off, dtype=np.int32), np.ascontiguousarray(ids, dtype=np.int32)


def _link_rank(decoder, H, R, queries, corrupt, filter_offsets, filter_ids):
    lib = _lib.load()
    if corrupt not in ("dst", "src"):
        raise ValueError(f"corrupt must be 'dst' or 'src', not {corrupt!r}")
    H, ldh, R, queries, V, T, Q, D = _link_common(H, R, queries, "queries", decoder)
    if (filter_offsets is None) != (filter_ids is None):
        raise ValueError("a filter needs both filter_offsets and filter_ids")
    if filter_offsets is not None:
        if not isinstance(filter_offsets, torch.Tensor) or not isinstance(filter_ids, torch.Tensor):
            to_np = lambda a: a.cpu().numpy() if isinstance(a, torch.Tensor) else a
            off, ids = check_rank_filter(to_np(filter_offsets), to_np(filter_ids), Q, V)
            filter_offsets, filter_ids = torch.from_numpy(off).to(H.device), torch.from_numpy(ids).to(H.device)
        _require_dev(filter_offsets, torch.int32, "filter_offsets")
        _require_dev(filter_ids, torch.int32, "filter_ids")
        if filter_offsets.dim() != 1 or filter_offsets.shape[0] != Q + 1 or filter_ids.dim() != 1:
            raise ValueError(f"filter_offsets must be [{Q + 1}] and filter_ids 1-D")
        filter_offsets, filter_ids = filter_offsets.contiguous(), filter_ids.contiguous()
        if filter_ids.numel() == 0:  # an empty tensor has no address; the kernel never reads an id then
            filter_ids = torch.zeros(1, dtype=torch.int32, device=H.device)
    greater = torch.empty(Q, dtype=torch.int32, device=H.device)
    equal = torch.empty(Q, dtype=torch.int32, device=H.device)
    if decoder == "complex":
        ws = _workspace(H.device, lib.tfgnn_complex_rank_workspace_bytes(Q, D))
    else:
        ws = _workspace(H.device, lib.tfgnn_distmult_rank_workspace_bytes(Q))
    _lib.check(getattr(lib, f"tfgnn_{decoder}_rank")(_ptr(H), ldh, _ptr(R), _ptr(queries), Q, 0 if corrupt == "dst" else 1,
                                                     _ptr(filter_offsets), _ptr(filter_ids), V, T, D, _ptr(greater), _ptr(equal),
                                                     _ptr(ws), ws.numel(), _stream()))
    return greater, equal


def distmult_rank(H: torch.Tensor, R: torch.Tensor, queries, corrupt: str = "dst", filter_offsets=None, filter_ids=None):
    """For every query triple, how many candidate entities in the corrupted slot (``corrupt``: "dst" or "src") score above /
    exactly as the true triple, the true entity and the filter's ids left out (include/tfgnn.h tfgnn_distmult_rank) ->
    (greater int32 [Q], equal int32 [Q]) on the device.  Host arrays (numpy) are validated and uploaded; device tensors are
    taken as validated."""
    return _link_rank("distmult", H, R, queries, corrupt, filter_offsets, filter_ids)


def complex_rank(H: torch.Tensor, R: torch.Tensor, queries, corrupt: str = "dst", filter_offsets=None, filter_ids=None):
    """``distmult_rank`` with the ComplEx score (include/tfgnn.h tfgnn_complex_rank: one query vector per query, every score
    of the call the dot product of that vector with a node's row)."""
    return _link_rank("complex", H, R, queries, corrupt, filter_offsets, filter_ids)


def link_launch_counts() -> dict:
    """tfgnn_link_launch_counts: kernel launches of the three DistMult calls so far (host counters)."""
    buf = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().tfgnn_link_launch_counts(buf, 3))
    return {"distmult_fwd": int(buf[0]), "distmult_bwd": int(buf[1]), "distmult_rank": int(buf[2])}


def complex_launch_counts() -> dict:
    """tfgnn_complex_launch_counts: kernel launches of the three ComplEx calls so far (host counters)."""
    buf = (ctypes.c_int64 * 3)()
    _lib.check(_lib.load().tfgnn_complex_launch_counts(buf, 3))
    return {"complex_fwd": int(buf[0]), "complex_bwd": int(buf[1]), "complex_rank": int(buf[2])}


def _device_triples(triples: torch.Tensor, what: str) -> int:
    _require_dev(triples, torch.int32, what)
    if triples.dim() != 2 or triples.shape[1] != 3 or not triples.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int32 [N, 3], got {tuple(triples.shape)}")
    return triples.shape[0]


def draw_negative_triples(triples: torch.Tensor, num_positives: int, V: int, seed: int, use_epoch: bool = True) -> torch.Tensor:
    """tfgnn_triples_draw_negatives, in place: ``triples`` int32 [N, 3] on the device holds P = ``num_positives`` positives in
    its first rows and N = P (1 + K); rows P .. N - 1 are written with K negatives per positive, in np.repeat order, each its
    positive with the source or the target replaced by one of the other V - 1 nodes (include/tfgnn.h states the random
    numbers: the dropout mask generator's words for ``seed`` and - ``use_epoch`` - the current dropout epoch).  One launch on
    the current stream, capturable; K = 0 launches nothing.  Returns ``triples``."""
    N = _device_triples(triples, "triples")
    P = int(num_positives)
    if P < 1 or N % P:
        raise ValueError(f"triples [{N}, 3] are not P (1 + K) rows for P = {P} positives")
    _lib.check(_lib.load().tfgnn_triples_draw_negatives(_ptr(triples), N, P, N // P - 1, int(V), int(seed) & (2 ** 64 - 1),
                                                        int(bool(use_epoch)), _stream()))
    torch.autograd.graph.increment_version(triples)  # written through a raw pointer, which torch does not see
    return triples


def triple_tables_workspace(triples_or_N, V: int, T: int, device=None) -> torch.Tensor:
    """A workspace of tfgnn_triple_tables_workspace_bytes(N, V, T) bytes for ``build_triple_tables_device`` - to be allocated
    once by a caller whose builds are captured into a hipGraph."""
    N = triples_or_N.shape[0] if isinstance(triples_or_N, torch.Tensor) else int(triples_or_N)
    if device is None:
        device = triples_or_N.device if isinstance(triples_or_N, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
    return torch.empty(max(int(_lib.load().tfgnn_triple_tables_workspace_bytes(N, int(V), int(T))), 16), dtype=torch.uint8, device=device)


def build_triple_tables_device(triples: torch.Tensor, V: int, T: int, out: Optional[Dict[str, torch.Tensor]] = None,
                               node: bool = True, rel: bool = True, workspace: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """``build_triple_tables`` on the device (tfgnn_triple_tables_build): from DEVICE triples int32 [N, 3] - taken as validated,
    like every device triple array - the same int32 tables, bit for bit, as device tensors.  ``node`` / ``rel``: which pair to
    build (node_offsets + node_entries, rel_offsets + rel_order); a pair that is not requested is neither built nor touched.
    ``out``: a dict of the tables to write into (the requested names; others are ignored) - else new tensors; the result holds
    the requested names only.  ``workspace``: a uint8 tensor of ``triple_tables_workspace``'s size; without one the stream's
    shared workspace is used, which may allocate - pass one when the call is captured.  2 passes(V) + 1 launches for the node
    pair, 2 passes(T) + 1 for the relation pair (include/tfgnn.h), on the current stream; no host synchronisation."""
    lib = _lib.load()
    N = _device_triples(triples, "triples")
    if not (node or rel):
        raise ValueError("build_triple_tables_device: neither the node pair nor the relation pair is requested")
    V, T = int(V), int(T)
    dev = triples.device
    sizes = {"node_offsets": V + 1, "node_entries": 2 * N, "rel_offsets": T + 1, "rel_order": N}
    wanted = (("node_offsets", "node_entries") if node else ()) + (("rel_offsets", "rel_order") if rel else ())
    tabs: Dict[str, Optional[torch.Tensor]] = dict.fromkeys(TRIPLE_TABLE_NAMES)
    for name in wanted:
        if out is not None:
            t = out[name]
            _require_dev(t, torch.int32, name)
            if t.dim() != 1 or t.shape[0] != sizes[name] or not t.is_contiguous() or t.device != dev:
                raise ValueError(f"{name} {tuple(t.shape)} must be a contiguous int32 [{sizes[name]}] on {dev}")
        else:
            t = torch.empty(sizes[name], dtype=torch.int32, device=dev)
        tabs[name] = t
    need = int(lib.tfgnn_triple_tables_workspace_bytes(N, V, T))
    if workspace is None:
        workspace = _workspace(dev, need)
    else:
        _require_dev(workspace, torch.uint8, "workspace")
    _lib.check(lib.tfgnn_triple_tables_build(_ptr(triples), N, V, T, _ptr(tabs["node_offsets"]), _ptr(tabs["node_entries"]),
                                             _ptr(tabs["rel_offsets"]), _ptr(tabs["rel_order"]), _ptr(workspace),
                                             workspace.numel(), _stream()))
    if out is not None:
        for name in wanted:
            torch.autograd.graph.increment_version(tabs[name])
    return {name: tabs[name] for name in wanted}


def triple_table_passes(X: int) -> int:
    """passes(X) of include/tfgnn.h: 9-bit digit passes of the table sort for keys in [0, X)"""
    return max(1, -(-max(int(X) - 1, 0).bit_length() // _lib.TRIPLE_SORT_DIGIT_BITS))


def negatives_launch_counts() -> dict:
    """tfgnn_negatives_launch_counts: kernel launches of the draws and of the table builds so far (host counters)."""
    buf = (ctypes.c_int64 * 2)()
    _lib.check(_lib.load().tfgnn_negatives_launch_counts(buf, 2))
    return {"draw_negatives": int(buf[0]), "triple_tables": int(buf[1])}


# ---- split-operand ("f16x2") products: include/tfgnn.h tfgnn_sp_*, csrc/gemm_sp.hip ------------------------------
class SplitOperand:
    """An fp32 matrix [rows, cols] in the SP16 operand format: ``data`` uint8 [rows, 4 * cols] (per row and 16 columns
    one 64-byte granule [16 x fp16 h | 16 x fp16 l]) and ``inv_scale`` fp32 [rows, cols // scale_block] (2^-e)."""

    __slots__ = ("data", "inv_scale", "rows", "cols", "scale_block")

    def __init__(self, data, inv_scale, rows, cols, scale_block):
        self.data, self.inv_scale, self.rows, self.cols, self.scale_block = data, inv_scale, rows, cols, scale_block


def _split_rows_args(x, scale_block, segments, fixed_inv_scale, out):
    """-> (out, the arguments tfgnn_sp_split_rows and tfgnn_sp_split_rows_job share, the tensors they point into)"""
    _require_dev(x, torch.float32, "x")
    x, ld = _rowmajor(x, "x")
    rows = x.shape[0]
    if segments is None:
        seg_len, seg_stride, cols = 0, 0, x.shape[1]
    else:
        seg_len, seg_stride, cols = (int(v) for v in segments)
    sb = int(scale_block) if scale_block and scale_block > 0 else cols
    if out is None:
        data = torch.empty((rows, cols * 4), dtype=torch.uint8, device=x.device)
        if fixed_inv_scale is not None:
            out = SplitOperand(data, fixed_inv_scale, rows, cols, 0)  # one scale for the whole tensor
        else:
            out = SplitOperand(data, torch.empty((rows, cols // sb), dtype=torch.float32, device=x.device), rows, cols, sb)
    args = (_ptr(x), ld, seg_len, seg_stride, rows, cols, sb, _ptr(out.data), out.data.stride(0),
            None if fixed_inv_scale is not None else _ptr(out.inv_scale), _ptr(fixed_inv_scale))
    return out, args, (x, out.data, out.inv_scale, fixed_inv_scale)


def sp_split_rows(x: torch.Tensor, *, scale_block: int = 0, segments=None, fixed_inv_scale: Optional[torch.Tensor] = None,
                  out: Optional[SplitOperand] = None) -> SplitOperand:
    """SP16 form of the rows of ``x`` [R, C] (unit inner stride).  ``segments = (seg_len, seg_stride, cols)``: row r is
    assembled from cols / seg_len pieces x.data[r * ld + j * seg_stride : ... + seg_len] (e.g. row d of
    [W_0[d, :] | W_1[d, :] | ...] from stacked kernels [L, D, H]: x = W[0], segments = (H, D * H, L * H))."""
    out, args, _ = _split_rows_args(x, scale_block, segments, fixed_inv_scale, out)
    _lib.check(_lib.load().tfgnn_sp_split_rows(*args, _stream()))
    return out


def sp_split_rows_jobs(x: torch.Tensor, *, scale_block: int = 0, segments=None, fixed_inv_scale: Optional[torch.Tensor] = None,
                       out: Optional[SplitOperand] = None) -> SplitJobs:
    """``sp_split_rows`` as a job of a shared small-pass launch (weights: nothing but launch latency): allocates the operand and
    fills the job, launches nothing - ``aux_flush`` does."""
    out, args, keep = _split_rows_args(x, scale_block, segments, fixed_inv_scale, out)
    if out.rows <= 0:
        return SplitJobs(out)
    job = _lib.AuxJob()
    _lib.check(_lib.load().tfgnn_sp_split_rows_job(*args, ctypes.byref(job)))
    return SplitJobs(out, (job,), (), keep)


_sp_rows_memo = {}  # id(tensor) -> (weakref, version, SplitOperand): split forms written by the kernel that produced the tensor


def _remember_split_rows(t: torch.Tensor, op: SplitOperand) -> None:
    import weakref

    for k in [k for k, (ref, _, _) in _sp_rows_memo.items() if ref() is None]:  # a handful of entries: layer inputs of one step
        del _sp_rows_memo[k]
    _sp_rows_memo[id(t)] = (weakref.ref(t), t._version, op)


def sp_rows_of(x: torch.Tensor) -> SplitOperand:
    """SP16 rows (one scale per row) of ``x``: the form its producer already wrote (dropout_forward in f16x2 mode), when that
    is still valid for this very tensor object and version, else a split pass."""
    hit = _sp_rows_memo.get(id(x))
    if hit is not None and hit[0]() is x and hit[1] == x._version:
        return hit[2]
    op = sp_split_rows(x)
    _remember_split_rows(x, op)  # forward and backward products of a step share it
    return op


def _split_cols_operand(w, out):
    """-> (w, its leading dimension, K, N, data, inv_scale) of the SP16 form of w^T"""
    _require_dev(w, torch.float32, "w")
    w, ld = _rowmajor(w, "w")
    K, N = w.shape
    if out is not None:
        if out.rows != N or out.cols != K:
            raise ValueError("sp_split_cols: out must hold N rows of K columns")
        return w, ld, K, N, out.data, out.inv_scale
    return (w, ld, K, N, torch.empty((N, K * 4), dtype=torch.uint8, device=w.device),
            torch.empty((N, 1), dtype=torch.float32, device=w.device))


def sp_split_cols(w: torch.Tensor, out: Optional[SplitOperand] = None) -> SplitOperand:
    """SP16 form of w^T for a row-major [K, N] matrix (a Keras kernel): rows = N, cols = K, one scale per row.
    out: write into this operand (N rows of K columns: a slice of a stack of per-group operands)."""
    w, ld, K, N, data, inv = _split_cols_operand(w, out)
    _lib.check(_lib.load().tfgnn_sp_split_cols(_ptr(w), ld, K, N, _ptr(data), data.stride(0), _ptr(inv), _stream()))
    return SplitOperand(data, inv, N, K, K)


def sp_split_cols_jobs(w: torch.Tensor, out: Optional[SplitOperand] = None) -> SplitJobs:
    """``sp_split_cols`` as jobs of shared small-pass launches: allocates the operand and fills the jobs, launches nothing -
    ``aux_flush`` does.  Long K (the stacked kernels of many relations, tfgnn_sp_split_cols_two_pass_bytes > 0): the column
    maxima as a stage-0 job, the conversion - which then reads every byte once instead of once per K slice - as a stage-1 job."""
    lib = _lib.load()
    w, ld, K, N, data, inv = _split_cols_operand(w, out)
    op = SplitOperand(data, inv, N, K, K)
    two_pass = lib.tfgnn_sp_split_cols_two_pass_bytes(K, N)
    if two_pass:
        cm = torch.empty(two_pass, dtype=torch.uint8, device=w.device)
        mjob, sjob = _lib.AuxJob(), _lib.AuxJob()
        _lib.check(lib.tfgnn_sp_split_cols_jobs(_ptr(w), ld, K, N, _ptr(data), data.stride(0), _ptr(inv), _ptr(cm), two_pass,
                                                ctypes.byref(mjob), ctypes.byref(sjob)))
        return SplitJobs(op, (mjob,), (sjob,), (w, data, inv, cm))
    job = _lib.AuxJob()
    _lib.check(lib.tfgnn_sp_split_cols_job(_ptr(w), ld, K, N, _ptr(data), data.stride(0), _ptr(inv), ctypes.byref(job)))
    return SplitJobs(op, (job,), (), (w, data, inv))


def _tile_kmask(t, M):
    if t is not None and (t.dtype != torch.uint8 or not t.is_cuda or t.numel() < (M + 127) // 128 or not t.is_contiguous()):
        raise ValueError("tile_kmask must be a contiguous uint8 device tensor with one byte per 128-row tile")
    return t


def _row_map(t, M):
    if t is not None and (t.dtype != torch.int32 or not t.is_cuda or t.numel() != M or not t.is_contiguous()):
        raise ValueError("row_map must be a contiguous int32 device tensor with one entry per product row")
    return t


_SPLITK_WS = {}  # "ws": the workspace tensor of the in-launch K split (tfgnn_sp_gemm_nt_set_splitk_workspace), once per process
_SPLITK_BYTES = 80 << 20


def _ensure_splitk_workspace(device, rows: int) -> None:
    """Products over few row tiles (a batch of some thousand nodes) split K inside their launch so that more than one
    workgroup per tile works (include/tfgnn.h): the workspace is registered the first time such a product is issued - one
    per process, on that product's device (one process drives one GPU).  TFGNN_NT_SPLITK=0 keeps the unsplit product."""
    if rows > 56000 or "done" in _SPLITK_WS or capturing():  # (few row tiles: K split; masked products up to ~430 tiles: helpers)
        return
    _SPLITK_WS["done"] = True
    if env("TFGNN_NT_SPLITK", "1") == "0":
        return
    ws = torch.empty(_SPLITK_BYTES, dtype=torch.uint8, device=device)
    _lib.check(_lib.load().tfgnn_sp_gemm_nt_set_splitk_workspace(_ptr(ws), _SPLITK_BYTES))
    _SPLITK_WS["ws"] = ws


def sp_gemm_nt_splitk(enable: Optional[bool] = None):
    """-> (splits can happen, a reducer ever timed out, products launched with a split so far).  enable: switch the in-launch
    K split of products over few row tiles on / off (include/tfgnn.h tfgnn_sp_gemm_nt_set_splitk_workspace)."""
    t, n = ctypes.c_int(0), ctypes.c_int64(0)
    on = _lib.load().tfgnn_sp_gemm_nt_splitk_status(-1 if enable is None else int(bool(enable)), ctypes.byref(t), ctypes.byref(n))
    return bool(on), bool(t.value), int(n.value)


def sp_tile_width(N: int) -> int:
    """Column tile of the split-operand NT product for N output columns (gemm_sp.hip sp_tile_width); 0: unsupported."""
    return 320 if N % 320 == 0 else (256 if N % 256 == 0 else (128 if N % 128 == 0 else 0))


def sp_tiles(N: int) -> bool:
    """Do the split-operand products tile N output columns (320 / 256 / 128 wide tiles)?"""
    return N % 128 == 0 or N % 320 == 0


def sp_one_tile(N: int) -> bool:
    """Is N exactly one column tile of the split-operand NT product (128, 256 or 320: what ``sp_gemm_nt_split`` takes)?"""
    return sp_tile_width(N) == N


def _empty_split(rows: int, cols: int, device, per_row: bool = False) -> SplitOperand:
    """An unwritten SP16 operand [rows, cols] for a kernel to fill: a product's split result, which carries one scale per row
    and COLUMN TILE (cols = 512: blocks of 256 columns), or - per_row - an operand with one scale per row."""
    bn = cols if per_row else sp_tile_width(cols)
    return SplitOperand(torch.empty((rows, cols * 4), dtype=torch.uint8, device=device),
                        torch.empty((rows, max(1, cols // max(bn, 1))), dtype=torch.float32, device=device), rows, cols, bn if bn else cols)


def _c_epilogue(out_mul, act_grad, dropout, saved_scale):
    """The epilogue specs of a split-operand product as the C ABI takes them
    -> (out_mul tensor | None, activation id of ``saved``, saved tensor | None, saved_scale, dropout rate, dropout seed)."""
    out_mul, act_grad, dropout, saved_scale = _native_epilogue(out_mul, act_grad, dropout, saved_scale)
    act_name, saved = act_grad if act_grad is not None else (None, None)
    rate, seed = dropout if dropout is not None else (0.0, 0)
    return out_mul, act_id(act_name), saved, float(saved_scale), float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF


def _product_out(out, M: int, N: int, accumulate, device):
    """-> (out, leading dimension): the fp32 result [M, N] of a product, the caller's tensor checked or a new one"""
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs out")
        out = torch.empty((M, N), dtype=torch.float32, device=device)
    out2, ldc = _rowmajor(out, "out")
    if out2 is not out or tuple(out.shape) != (M, N):
        raise ValueError(f"out must be [{M},{N}] with unit inner stride")
    return out, ldc


class RowGroups:
    """Consecutive row groups (rows of group g: [offsets[g], offsets[g + 1])) cut into the row tiles of the grouped product
    (tfgnn_sp_gemm_nt_grouped d_tile_table): int32 [tiles, 4] = (first row, rows, group, 0) on the device, built once per
    grouping (a batch's non-empty (source, type) rows: cached on its Graph)."""

    def __init__(self, offsets_host, device):
        import numpy as np

        off = [int(o) for o in offsets_host]
        rows = []
        for gi in range(len(off) - 1):
            for r0 in range(off[gi], off[gi + 1], 128):
                rows.append((r0, min(128, off[gi + 1] - r0), gi, 0))
        self.offsets = off
        self.num_groups = len(off) - 1
        self.num_rows = off[-1]
        self.num_tiles = len(rows)
        tab = np.asarray(rows if rows else [(0, 0, 0, 0)], dtype=np.int32)
        self.table = torch.from_numpy(tab).to(device)
        self._tn = None

    def tn_tables(self):
        """-> (K ranges int32 [S, 2] = (first row, rows <= TN_GROUPED_MAX_CHUNK), first range of every group int32 [G + 1], S):
        the row groups cut into the K ranges of the grouped weight-gradient product (tfgnn_sp_gemm_tn_grouped)"""
        if self._tn is None:
            import numpy as np

            ranges, first = [], [0]
            for gi in range(self.num_groups):
                r0, r1 = self.offsets[gi], self.offsets[gi + 1]
                n = -(-(r1 - r0) // TN_GROUPED_MAX_CHUNK)
                if n:
                    chunk = -(-(-(-(r1 - r0) // n)) // 16) * 16  # equal shares, whole k16 steps
                    for r in range(r0, r1, chunk):
                        ranges.append((r, min(chunk, r1 - r)))
                first.append(len(ranges))
            dev = self.table.device
            self._tn = (torch.from_numpy(np.asarray(ranges if ranges else [(0, 0)], dtype=np.int32)).to(dev),
                        torch.from_numpy(np.asarray(first, dtype=np.int32)).to(dev), len(ranges))
        return self._tn


def sp_gemm_nt_grouped(a: SplitOperand, b: SplitOperand, groups: RowGroups, *, a_rows=None, act=ACT_NONE, act_grad=None,
                       want_fp32: bool = True, want_split: bool = False, b_column_blocks: bool = False):
    """Per-group products on split operands (tfgnn_sp_gemm_nt_grouped): row r of group g -> epilogue(a_row(r) @ b_g^T).
    b: ``groups.num_groups`` stacked [N, K] operands with one scale per row ([G * N, K]), or - b_column_blocks - ONE operand
    [N, G * K] whose column block g is group g's (``sp_split_cols`` of G stacked Keras kernels [G * K, N]: one launch; the row
    scales are shared by the groups).  a_rows (int32 [rows]): row r reads a[a_rows[r]] (a then has any number of rows).
    act_grad = (name, saved [rows, N]).  -> (fp32 [rows, N] | None, SplitOperand | None)"""
    lib = _lib.load()
    M, K = groups.num_rows, a.cols
    G = max(groups.num_groups, 1)
    if b_column_blocks:
        if b.cols != G * K or b.scale_block != b.cols:
            raise ValueError("sp_gemm_nt_grouped: b must be [N, G * K] with one scale per row")
        N, stride_b, stride_scale = b.rows, 4 * K, 0
    else:
        if b.cols != K or b.rows % G or b.scale_block != K:
            raise ValueError("sp_gemm_nt_grouped: b must stack one [N, K] operand per group with one scale per row")
        N = b.rows // G
        stride_b, stride_scale = N * b.data.stride(0), N
    if a_rows is None and a.rows != M:
        raise ValueError(f"sp_gemm_nt_grouped: {a.rows} operand rows for {M} grouped rows")
    if a_rows is not None:
        a_rows = _row_map(a_rows, M)
    dev = a.data.device
    out = torch.empty((M, N), dtype=torch.float32, device=dev) if want_fp32 else None
    op = _empty_split(M, N, dev) if want_split else None
    if M == 0:
        return out, op
    _, act_of_saved, saved, _, _, _ = _c_epilogue(None, act_grad, None, 1.0)
    _lib.check(
        lib.tfgnn_sp_gemm_nt_grouped(
            M, N, K, _ptr(a.data), a.data.stride(0), _ptr(a.inv_scale), a.scale_block if a.scale_block else -1, _ptr(a_rows), a.rows,
            _ptr(groups.table), groups.num_tiles, G, _ptr(b.data), b.data.stride(0), stride_b, _ptr(b.inv_scale), stride_scale,
            _ptr(out), N, None, act_id(act), None, 0, act_of_saved, _ptr(saved), saved.stride(0) if saved is not None else 0,
            _ptr(op.data) if op is not None else None, op.data.stride(0) if op is not None else 0,
            _ptr(op.inv_scale) if op is not None else None, _stream(),
        )
    )
    if out is not None and op is not None:
        _remember_split_rows(out, op)
    return out, op


TN_WIDE_MAX_ROWS = 512 * 2016  # rows one launch of the two-factor TN product covers (512 K ranges)
TN_GROUPED_MAX_RANGES = 512  # K ranges one launch of the grouped two-factor product takes (tfgnn_sp_gemm_tn_grouped)
TN_GROUPED_MAX_CHUNK = 2016  # rows of a K range of the wide-range product (gemm_sp.hip SP_TN_BSC_MAX_CHUNK)


def sp_gemm_tn_grouped(a: SplitOperand, b: SplitOperand, groups: RowGroups, out: torch.Tensor, transposed: bool = False) -> torch.Tensor:
    """out[g] = a_g^T b_g over the rows of group g, all groups in ONE launch of the wide-range product (tfgnn_sp_gemm_tn_grouped):
    ``a`` [rows, M] with per-(row, block) scales, ``b`` [rows, N] with one scale per row, out [G, M, N] (transposed: [G, N, M],
    element (m, n) of product g at out[g, n, m])."""
    lib = _lib.load()
    if a.scale_block <= 0 or b.scale_block != b.cols or a.rows != b.rows or a.rows != groups.num_rows:
        raise ValueError("sp_gemm_tn_grouped: operands must share the grouped rows; b needs one scale per row")
    M, N, G = a.cols, b.cols, groups.num_groups
    if not out.is_contiguous() or out.numel() != G * M * N:
        raise ValueError("sp_gemm_tn_grouped: out must be contiguous [G, M, N]")
    tab = groups.tn_tables()
    if tab[2] > TN_GROUPED_MAX_RANGES:
        raise ValueError(f"sp_gemm_tn_grouped: {tab[2]} K ranges, at most {TN_GROUPED_MAX_RANGES} per launch (callers take another route)")
    # (with the in-stream repair armed - set_guard_repair - the size includes the tail of the per-range trip words)
    # (0 for a shape the product rejects: the call below says which)
    ws_bytes = lib.tfgnn_sp_gemm_tn_grouped_workspace_bytes(M, N, a.cols, a.scale_block, tab[2])
    ws_ptr, ws_len, _ = _aligned_workspace(a.data.device, ws_bytes)
    sr, sc = (1, M) if transposed else (N, 1)
    _lib.check(lib.tfgnn_sp_gemm_tn_grouped(M, N, _ptr(a.data), a.data.stride(0), _ptr(a.inv_scale), a.cols, a.scale_block, _ptr(b.data),
                                            b.data.stride(0), _ptr(b.inv_scale), G, _ptr(tab[1]), tab[2], _ptr(tab[0]), _ptr(out), M * N, sr, sc,
                                            ctypes.c_void_p(ws_ptr), ws_len, _stream()))
    return out


def sp_gather_rows(a: SplitOperand, index: torch.Tensor) -> SplitOperand:
    """rows ``index`` of a split operand, with their scales (tfgnn_sp_gather_rows)."""
    lib = _lib.load()
    _require_dev(index, torch.int32, "index")
    n = int(index.numel())
    per = a.inv_scale.shape[1] if a.inv_scale.dim() == 2 else 1
    out = SplitOperand(torch.empty((n, a.cols * 4), dtype=torch.uint8, device=a.data.device),
                       torch.empty((n, per), dtype=torch.float32, device=a.data.device), n, a.cols, a.scale_block)
    _lib.check(lib.tfgnn_sp_gather_rows(_ptr(a.data), a.data.stride(0), _ptr(a.inv_scale), per, _ptr(index.contiguous()), n, a.rows, a.cols,
                                        _ptr(out.data), out.data.stride(0), _ptr(out.inv_scale), _stream()))
    return out


def _nt_shape(who: str, a: SplitOperand, b: SplitOperand):
    """-> (M, K, N) of a [M, K] @ b [N, K]^T, after the operand checks of the NT product"""
    M, K, N = a.rows, a.cols, b.rows
    if b.cols != K:
        raise ValueError(f"{who}: inner dimensions differ ({K} vs {b.cols})")
    if b.scale_block != K:
        raise ValueError(f"{who}: the right operand must carry one scale per row")
    return M, K, N


def _sp_gemm_nt_rows(a, b, M, N, K, out, ldc, op, bias, act, accumulate, epilogue, tile_kmask, row_map, a_rows, tail=None) -> None:
    """The one call of tfgnn_sp_gemm_nt_rows: ``out`` (fp32 [M, N], leading dimension ldc) and ``op`` (the split result) may
    each be None; ``epilogue`` as ``_c_epilogue`` returns it.  ``tail``: a ``TnReduceJob`` this launch carries
    (tfgnn_sp_gemm_nt_rows_tail); the call consumes it."""
    out_mul, act_of_saved, saved, saved_scale, rate, seed = epilogue
    if bias is not None:
        bias = bias.contiguous()
    _ensure_splitk_workspace(a.data.device, M)
    args = (
        M, N, K, _ptr(a.data), a.data.stride(0), _ptr(a.inv_scale), a.scale_block if a.scale_block else -1,
        _ptr(_row_map(a_rows, M)), _ptr(b.data), b.data.stride(0),
        _ptr(b.inv_scale), _ptr(out), ldc, _ptr(bias), act_id(act), int(accumulate), _ptr(out_mul),
        out_mul.stride(0) if out_mul is not None else 0, act_of_saved, _ptr(saved),
        saved.stride(0) if saved is not None else 0, saved_scale, _ptr(op.data) if op is not None else None,
        op.data.stride(0) if op is not None else 0, _ptr(op.inv_scale) if op is not None else None, rate, seed,
        _ptr(_tile_kmask(tile_kmask, M)), _ptr(_row_map(row_map, M)),
    )
    if tail is None:
        _lib.check(_lib.load().tfgnn_sp_gemm_nt_rows(*args, _stream()))
        return
    _lib.check(_lib.load().tfgnn_sp_gemm_nt_rows_tail(*args, ctypes.byref(tail._take()), _stream()))
    tail._issued()


class TnReduceJob:
    """The reduce pass of a weight-gradient product whose launch ``sp_gemm_tn_product`` left to the caller (tfgnn_tn_reduce_job):
    hand it to the NT product that follows on the same stream (``sp_gemm_nt(..., tail=job)``) or run it alone
    (``tn_reduce_launch``) - exactly once, before anything reads ``out``.  Built and consumed by the same caller: nothing
    queues these.  ``num_blocks``: the workgroups the carrying launch gives the pass (0: the product already ran it)."""

    def __init__(self, c_job, out: torch.Tensor, workspace):
        self._c, self.out, self._ws, self._done = c_job, out, workspace, False

    @property
    def num_blocks(self) -> int:
        return int(self._c.num_blocks)

    @num_blocks.setter
    def num_blocks(self, n: int) -> None:
        if self._c.num_blocks and n > 0:  # (an empty job stays empty)
            self._c.num_blocks = int(n)

    def _take(self):
        if self._done:
            raise RuntimeError("TnReduceJob: the reduce pass has been issued already")
        return self._c

    def _issued(self) -> None:
        self._done, self._ws = True, None  # (stream order keeps the workspace's memory until the launch is through)
        torch.autograd.graph.increment_version(self.out)


def tn_reduce_launch(job: TnReduceJob) -> torch.Tensor:
    """The reduce pass of ``job`` in a launch of its own (tfgnn_tn_reduce_launch) -> the product's ``out``."""
    _lib.check(_lib.load().tfgnn_tn_reduce_launch(ctypes.byref(job._take()), _stream()))
    job._issued()
    return job.out


def tn_reduce_counts() -> dict:
    """tfgnn_tn_reduce_counts: reduce passes of the weight-gradient products so far - launched on their own / carried by an NT
    launch (host counters)."""
    buf = (ctypes.c_int64 * 2)()
    _lib.check(_lib.load().tfgnn_tn_reduce_counts(buf, 2))
    return {"own": int(buf[0]), "carried": int(buf[1])}


@_writes_out
def sp_gemm_nt(a: SplitOperand, b: SplitOperand, *, bias=None, act=ACT_NONE, out=None, accumulate=False, out_mul=None,
               act_grad=None, dropout=None, saved_scale: float = 1.0, tile_kmask=None, row_map=None, a_rows=None,
               tail: Optional["TnReduceJob"] = None) -> torch.Tensor:
    """out [M, N] = epilogue(a [M, K] @ b [N, K]^T) from SP16 operands (tfgnn_sp_gemm_nt / tfgnn_sp_gemm_nt_dropout).
    tail: the reduce pass of the weight-gradient product enqueued just before on this stream (``sp_gemm_tn_product``), run by
    extra workgroups of this launch.
    tile_kmask (uint8 [ceil(M / 128)]): bit b = scale block b of ``a`` holds non-zeros in that row tile, the other blocks are
    skipped; row_map (int32 [M]): product row r is written at out[row_map[r]] (Graph pattern order, graph_gather_sp).
    dropout = (rate, seed): the result times the mask ``dropout_forward`` draws for that seed, applied in the epilogue
    (forward: the next layer's input dropout; gradient product: the recomputed forward mask).  saved_scale: the derivative
    of ``act_grad`` is taken at saved * saved_scale (saved is a dropped activation).  a_rows (int32 [M]): product row r reads
    row a_rows[r] of ``a`` (tfgnn_sp_gemm_nt_rows: the by-source pattern order of the input-gradient product)."""
    M, K, N = _nt_shape("sp_gemm_nt", a, b)
    out, ldc = _product_out(out, M, N, accumulate, a.data.device)
    _sp_gemm_nt_rows(a, b, M, N, K, out, ldc, None, bias, act, accumulate, _c_epilogue(out_mul, act_grad, dropout, saved_scale),
                     tile_kmask, row_map, a_rows, tail)
    return out


def sp_gemm_nt_split(a: SplitOperand, b: SplitOperand, *, bias=None, act=ACT_NONE, out_mul=None, act_grad=None,
                     want_fp32: bool = True, dropout=None, saved_scale: float = 1.0, tile_kmask=None, row_map=None, a_rows=None):
    """As sp_gemm_nt, with the result ALSO (or only: want_fp32=False) written as an SP16 operand with one scale per row
    by the product's epilogue (tfgnn_sp_gemm_nt_sp): the next product's operand without a split pass.  N must be one
    column tile (128, 256 or 320).  -> (fp32 [M, N] | None, SplitOperand); the fp32 tensor remembers its split form
    (``sp_rows_of``)."""
    M, K, N = _nt_shape("sp_gemm_nt_split", a, b)
    dev = a.data.device
    out = torch.empty((M, N), dtype=torch.float32, device=dev) if want_fp32 else None
    op = _empty_split(M, N, dev)
    _sp_gemm_nt_rows(a, b, M, N, K, out, N, op, bias, act, False, _c_epilogue(out_mul, act_grad, dropout, saved_scale),
                     tile_kmask, row_map, a_rows)
    if out is not None:
        _remember_split_rows(out, op)
    return out, op


def split_rows_remembered(x: torch.Tensor) -> SplitOperand:
    """Split ``x`` now and remember the operand for ``sp_rows_of(x)`` (an input pipeline preparing the node features of a
    batch for the first product, e.g. on the stream that also buckets the batch's edges)."""
    op = sp_split_rows(x)
    _remember_split_rows(x, op)
    return op


def graph_gather_sp(graph: "Graph", view: int, inp: torch.Tensor, *, col=None, edge_weight=None, row_scale=None,
                    fixed_inv_scale: Optional[torch.Tensor] = None, rows_per_operand_row: int = 1) -> SplitOperand:
    """graph_gather (plain sums) with the result written as an SP16 operand (tfgnn_graph_gather_reduce_sp).
    ``rows_per_operand_row`` = L folds the rows (v, l) of a typed view into the [V, L * width] operand with one scale
    block per edge type.  Compact views: one operand row (and scale) per non-empty bucket."""
    lib = _lib.load()
    _require_dev(inp, torch.float32, "inp")
    typed = view in (VIEW_BY_DST_TYPED, VIEW_BY_SRC_TYPED, VIEW_BY_DST_TYPED_PATTERN)
    if view in (VIEW_BY_DST_TYPED_COMPACT, VIEW_BY_SRC_TYPED_COMPACT):
        if rows_per_operand_row != 1:
            raise ValueError("graph_gather_sp: compact rows are operand rows (rows_per_operand_row = 1)")
        num_rows = int(graph.nonempty_offsets(view == VIEW_BY_SRC_TYPED_COMPACT)[-1])
    else:
        num_rows = graph.num_nodes * (graph.num_edge_types if typed else 1)
    if view == VIEW_BY_DST_TYPED_PATTERN and graph.num_edge_types > 8:
        raise ValueError("graph_gather_sp: the pattern order exists for at most 8 edge types")
    inp, ld_in = _rowmajor(inp, "inp")
    width = inp.shape[1]
    R = int(rows_per_operand_row)
    if num_rows % R:
        raise ValueError("rows_per_operand_row must divide the number of rows of the view")
    data = torch.empty((num_rows // R, R * width * 4), dtype=torch.uint8, device=inp.device)
    inv = None
    if fixed_inv_scale is None:
        inv = torch.empty((num_rows // R, R), dtype=torch.float32, device=inp.device)
    graph.ensure(_VIEW_PARTS[view])
    ws_bytes = lib.tfgnn_graph_gather_workspace_bytes(graph._h, view, width)
    ws = _workspace(inp.device, ws_bytes) if ws_bytes else None
    _lib.check(
        lib.tfgnn_graph_gather_reduce_sp(
            graph._h, view, _ptr(col), _ptr(edge_weight), _ptr(row_scale), _ptr(inp), ld_in, width, _ptr(data), width * 4,
            _ptr(inv), _ptr(fixed_inv_scale), _ptr(ws), ws.numel() if ws is not None else 0, _stream(),
        )
    )
    if fixed_inv_scale is not None:
        return SplitOperand(data, fixed_inv_scale, num_rows // R, R * width, 0)  # scale_block 0: one scale for the tensor
    return SplitOperand(data, inv, num_rows // R, R * width, width)


def graph_gather_sp_owned(graph: "Graph", view: int, inp: torch.Tensor, *, edge_weight=None, row_scale=None) -> SplitOperand:
    """``graph_gather_sp`` into the operand the GRAPH owns for (view, width, stream) - ``Graph.gather_operand`` - as the
    layer-level calls gather: the rows (v, l) of a typed view folded into [V, L * width], one scale block per edge type.  The
    first gather into a pair writes every row; later ones with the same ``row_scale`` values leave the empty buckets' rows and
    marker scales alone (tfgnn_graph_gather_reduce_sp_keep_empty).  The result is a view of the graph's buffers: the next
    gather of the same (view, width) on this stream overwrites it - consume it first, and never write to it."""
    lib = _lib.load()
    _require_dev(inp, torch.float32, "inp")
    if view == VIEW_BY_DST_TYPED_PATTERN and graph.num_edge_types > 8:
        raise ValueError("graph_gather_sp_owned: the pattern order exists for at most 8 edge types")
    inp, ld_in = _rowmajor(inp, "inp")
    width = inp.shape[1]
    graph.ensure(_VIEW_PARTS[view])
    pair = graph.gather_operand(view, width)
    per = pair.inv_scale.shape[1]
    keep = pair.begin(row_scale)  # (unfilled from here until the call has succeeded)
    for t, what in ((edge_weight, "edge_weight"), (row_scale, "row_scale")):
        if t is not None:
            _require_dev(t, torch.float32, what)
    ws_bytes = lib.tfgnn_graph_gather_workspace_bytes(graph._h, view, width)
    ws = _workspace(inp.device, ws_bytes) if ws_bytes else None
    _lib.check(
        lib.tfgnn_graph_gather_reduce_sp_keep_empty(
            graph._h, view, None, _ptr(edge_weight), _ptr(row_scale), _ptr(inp), ld_in, width, _ptr(pair.data), width * 4,
            _ptr(pair.inv_scale), None, _ptr(ws), ws.numel() if ws is not None else 0, int(keep), _stream(),
        )
    )
    pair.done(row_scale)
    return SplitOperand(pair.data, pair.inv_scale, pair.data.shape[0], per * width, width)


# ---- layer-level entry points (include/tfgnn.h tfgnn_mp_forward / tfgnn_mp_backward, csrc/mp_layer.hip) --------------------------
def mp_entry_enabled() -> bool:
    """The aggregate-first layers drive ONE C call per pass (default) instead of the op-level calls it is made of
    (TFGNN_MP_ENTRY=0: the op-level route - same kernels, same arguments, bit-identical results)."""
    return env("TFGNN_MP_ENTRY", "1") != "0"


def _weight_operand_for_call(w: torch.Tensor, kind: str, rows: int, cols: int):
    """-> (operand, stale): the cached split form of weight ``w``, or (stale = True) a new, still EMPTY one that the
    layer-level call builds in its merged small-pass launch; the caller caches it (``_cache_weight_operand``) once that call
    has succeeded."""
    op = _cached_weight_operand(w, kind)
    if op is not None:
        return op, False
    return _empty_split(rows, cols, w.device, per_row=True), True


def mp_forward(graph: "Graph", view: int, x: torch.Tensor, W: torch.Tensor, *, row_scale=None, act=ACT_NONE, dropout=None,
               tile_kmask=None, row_map=None, want_split: bool = False, want_fp32: bool = True):
    """One aggregate-first message-passing layer forward in ONE library call (tfgnn_mp_forward): gather of the source rows per
    (node, type) bucket written as the split operand, W^T split when its cached form is stale, the small passes merged, the
    product with its epilogue.  W: stacked kernels [L, D, H].  -> (out [V, H] | None, split form of out | None)."""
    lib = _lib.load()
    _require_dev(x, torch.float32, "x")
    L, D, H = (int(v) for v in W.shape)
    V = graph.num_nodes
    if L != graph.num_edge_types or x.shape[1] != D or not W.is_contiguous():
        raise ValueError("mp_forward: W must be the contiguous [L, D, H] stack of the graph's edge types and of x's width")
    x, ldx = _rowmajor(x, "x")
    dev = x.device
    graph.ensure(_VIEW_PARTS[view])
    wt, stale = _weight_operand_for_call(W, "cols", H, L * D)
    # the aggregate is scratch of the call, but it stays with the graph: the layers of a stack gather into the same pair, and
    # only the first of them writes the rows of the empty buckets
    pair = graph.gather_operand(view, D)
    out = torch.empty((V, H), dtype=torch.float32, device=dev) if want_fp32 else None
    op = _empty_split(V, H, dev) if want_split else None
    ws_bytes = lib.tfgnn_graph_gather_workspace_bytes(graph._h, view, D)
    ws = _workspace(dev, ws_bytes) if ws_bytes else None
    rate, seed = dropout if dropout is not None else (0.0, 0)
    _ensure_splitk_workspace(dev, V)
    stream = _stream()
    a = _lib.MpForwardArgs()
    a.struct_size = ctypes.sizeof(_lib.MpForwardArgs)
    a.kind = 0
    a.graph = graph._h
    a.view = int(view)
    a.x, a.ldx, a.in_dim, a.hidden_dim = x.data_ptr(), ldx, D, H
    a.row_scale = row_scale.data_ptr() if row_scale is not None else None
    a.w = W.data_ptr() if stale else None
    a.wt_sp, a.ld_wt_sp_bytes, a.wt_inv_scale = wt.data.data_ptr(), wt.data.stride(0), wt.inv_scale.data_ptr()
    a.agg_sp, a.agg_inv_scale = pair.data.data_ptr(), pair.inv_scale.data_ptr()
    a.agg_filled = int(pair.begin(row_scale))
    a.bias = None
    a.act = act_id(act)
    a.dropout_rate, a.dropout_seed = float(rate), int(seed) & 0xFFFFFFFFFFFFFFFF
    a.tile_kmask = _tile_kmask(tile_kmask, V).data_ptr() if tile_kmask is not None else None
    a.row_map = _row_map(row_map, V).data_ptr() if row_map is not None else None
    a.out, a.ld_out = (out.data_ptr(), H) if out is not None else (None, 0)
    if op is not None:
        a.out_sp, a.ld_out_sp_bytes, a.out_inv_scale = op.data.data_ptr(), op.data.stride(0), op.inv_scale.data_ptr()
    a.workspace, a.workspace_bytes = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    _lib.check(lib.tfgnn_mp_forward(ctypes.byref(a), stream))
    pair.done(row_scale)
    if stale:
        _cache_weight_operand(W, "cols", wt)
    if out is not None and op is not None:
        _remember_split_rows(out, op)
    return out, op


def mp_backward(graph: "Graph", d_pre: torch.Tensor, W: torch.Tensor, x_sp: Optional[SplitOperand], *, edge_weight=None, out=None,
                accumulate: bool = False, out_mul=None, act_grad=None, want_split: bool = False, skip=None,
                need_weight_grad: bool = True):
    """The backward pass of that layer in ONE library call (tfgnn_mp_backward): the gather of ``d_pre`` over the by-source buckets
    as a split operand, the rows form of the kernels when stale, d(node states) = epilogue(G W^T) - ``out`` / ``accumulate`` /
    ``out_mul`` / ``act_grad`` as in ``sp_gemm_nt``; ``skip`` = dict(tile_kmask, a_rows, row_map) of the by-source pattern order -
    and the kernel gradients dW [L, D, H] = X^T G_l from the layer input's split form ``x_sp``.
    -> (dX [V, D], split form of dX | None, dW | None)."""
    lib = _lib.load()
    _require_dev(d_pre, torch.float32, "d_pre")
    L, D, H = (int(v) for v in W.shape)
    V = graph.num_nodes
    if L != graph.num_edge_types or d_pre.shape[1] != H or not W.is_contiguous():
        raise ValueError("mp_backward: W must be the contiguous [L, D, H] stack of the graph's edge types, d_pre [V, H]")
    d_pre, ldg = _rowmajor(d_pre, "d_pre")
    dev = d_pre.device
    graph.ensure(_VIEW_PARTS[VIEW_BY_SRC_TYPED])
    wh, stale = _weight_operand_for_call(W, "rows", D, L * H)
    pair = graph.gather_operand(VIEW_BY_SRC_TYPED, H)  # (as the aggregate of mp_forward)
    out, ldc = _product_out(out, V, D, accumulate, dev)
    if want_split and accumulate:
        raise ValueError("mp_backward: the split result needs no accumulation")
    op = _empty_split(V, D, dev) if want_split else None
    out_mul, act_of_saved, saved, saved_scale, rate, seed = _c_epilogue(out_mul, act_grad, None, 1.0)
    dW = torch.empty_like(W) if need_weight_grad else None
    ws_bytes = lib.tfgnn_graph_gather_workspace_bytes(graph._h, VIEW_BY_SRC_TYPED, H)
    ws = _workspace(dev, ws_bytes) if ws_bytes else None
    tn_ws, tn_ptr, tn_len = None, None, 0
    if need_weight_grad:
        if x_sp is None or x_sp.scale_block != x_sp.cols or x_sp.rows != V or x_sp.cols != D:
            raise ValueError("mp_backward: the kernel gradients need the layer input as a split operand with one scale per row")
        tn_bytes = lib.tfgnn_sp_gemm_tn_workspace_bytes(L * H, D, V, L * H, H)
        if tn_bytes:
            # (its own buffer: the gather's workspace above is the shared one of this stream)
            tn_ptr, tn_len, tn_ws = _aligned_workspace(dev, tn_bytes, own=True)
    _ensure_splitk_workspace(dev, V)
    stream = _stream()
    skip = skip or {}
    a = _lib.MpBackwardArgs()
    a.struct_size = ctypes.sizeof(_lib.MpBackwardArgs)
    a.kind = 0
    a.graph = graph._h
    a.d_pre, a.ld_d_pre, a.in_dim, a.hidden_dim = d_pre.data_ptr(), ldg, D, H
    a.edge_weight = edge_weight.data_ptr() if edge_weight is not None else None
    a.w = W.data_ptr() if stale else None
    a.wh_sp, a.ld_wh_sp_bytes, a.wh_inv_scale = wh.data.data_ptr(), wh.data.stride(0), wh.inv_scale.data_ptr()
    a.g_sp, a.g_inv_scale = pair.data.data_ptr(), pair.inv_scale.data_ptr()
    a.g_filled = int(pair.begin(None))  # (edge weights do not reach a row without an edge)
    a.dx, a.ld_dx, a.accumulate = out.data_ptr(), ldc, int(bool(accumulate))
    if out_mul is not None:
        a.mul, a.ld_mul = out_mul.data_ptr(), out_mul.stride(0)
    a.act_of_saved = act_of_saved
    if saved is not None:
        a.saved, a.ld_saved = saved.data_ptr(), saved.stride(0)
    a.saved_scale = saved_scale
    a.dropout_rate, a.dropout_seed = rate, seed
    if op is not None:
        a.dx_sp, a.ld_dx_sp_bytes, a.dx_inv_scale = op.data.data_ptr(), op.data.stride(0), op.inv_scale.data_ptr()
    for name, check in (("tile_kmask", _tile_kmask), ("a_rows", _row_map), ("row_map", _row_map)):
        t = skip.get(name)
        if t is not None:
            setattr(a, name, check(t, V).data_ptr())
    if dW is not None:
        a.dw = dW.data_ptr()
        a.x_sp, a.ld_x_sp_bytes, a.x_inv_scale = x_sp.data.data_ptr(), x_sp.data.stride(0), x_sp.inv_scale.data_ptr()
        a.tn_workspace, a.tn_workspace_bytes = tn_ptr, tn_len
    a.workspace, a.workspace_bytes = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    _lib.check(lib.tfgnn_mp_backward(ctypes.byref(a), stream))
    pair.done(None)
    if stale:
        _cache_weight_operand(W, "rows", wh)
    del tn_ws
    torch.autograd.graph.increment_version(out)
    if op is not None:
        _remember_split_rows(out, op)
    return out, op, dW


@_writes_out
def sp_gemm_tn(a: SplitOperand, b: SplitOperand, *, a_cols=None, b_cols=None, out: Optional[torch.Tensor] = None,
               scatter=None, accumulate: bool = False, wide: bool = False) -> torch.Tensor:
    """C[m, n] = sum_k a[k, a0 + m] * b[k, b0 + n] (tfgnn_sp_gemm_tn).  ``a`` carries one scale per (row, block),
    ``b`` one per row - what sp_split_rows / graph_gather_sp write.  ``a_cols`` / ``b_cols`` = (first column, count)
    select column ranges.  ``scatter`` = (group_rows, stride_group, stride_row, stride_col) writes element (m, n) at
    out.flatten()[(m // group_rows) * stride_group + (m % group_rows) * stride_row + n * stride_col]; default: row-major.
    wide: the two-factor form (tfgnn_sp_gemm_tn_wide) - each operand's row scales may spread over 2^22 within a K range,
    whatever their products do (rows that are un-normalised sums on both sides)."""
    lib = _lib.load()
    if a.scale_block <= 0 or b.scale_block != b.cols:
        raise ValueError("sp_gemm_tn: the left operand needs per-(row, block) scales, the right one one scale per row")
    if a.rows != b.rows:
        raise ValueError(f"sp_gemm_tn: K differs ({a.rows} vs {b.rows})")
    if wide and a.rows > TN_WIDE_MAX_ROWS:
        # the two-factor product takes at most 512 K ranges of 2016 rows per launch: longer operands (10^6 node rows) run as
        # consecutive row ranges, each adding into ``out``
        if out is None:
            raise ValueError("sp_gemm_tn(wide=True) over more than %d rows needs out" % TN_WIDE_MAX_ROWS)
        for r0 in range(0, a.rows, TN_WIDE_MAX_ROWS):
            r1 = min(a.rows, r0 + TN_WIDE_MAX_ROWS)
            sp_gemm_tn(SplitOperand(a.data[r0:r1], a.inv_scale[r0:r1], r1 - r0, a.cols, a.scale_block),
                       SplitOperand(b.data[r0:r1], b.inv_scale[r0:r1], r1 - r0, b.cols, b.scale_block),
                       a_cols=a_cols, b_cols=b_cols, out=out, scatter=scatter, accumulate=accumulate or r0 > 0, wide=True)
        return out
    a0, M = a_cols if a_cols is not None else (0, a.cols)
    b0, N = b_cols if b_cols is not None else (0, b.cols)
    K = a.rows
    if out is None:
        if scatter is not None or accumulate:
            raise ValueError("scatter / accumulate need out")
        out = torch.empty((M, N), dtype=torch.float32, device=a.data.device)
    if not out.is_contiguous() or out.numel() != M * N:
        raise ValueError(f"out must be contiguous with {M * N} elements")
    gr, sg, sr, sc = scatter if scatter is not None else (M, 0, N, 1)
    ws_bytes = (lib.tfgnn_sp_gemm_tn_wide_workspace_bytes if wide else lib.tfgnn_sp_gemm_tn_workspace_bytes)(M, N, K, a.cols, a.scale_block)
    ws_ptr, ws_len = None, 0  # (0 bytes for a shape the product rejects: the call below says which)
    if ws_bytes:
        ws_ptr, ws_len, _ = _aligned_workspace(a.data.device, ws_bytes)
        ws_ptr = ctypes.c_void_p(ws_ptr)
    _lib.check(
        (lib.tfgnn_sp_gemm_tn_wide if wide else lib.tfgnn_sp_gemm_tn)(
            M, N, K, _ptr(a.data), a.data.stride(0), a0, _ptr(a.inv_scale), a.cols, a.scale_block, _ptr(b.data),
            b.data.stride(0), b0, _ptr(b.inv_scale), _ptr(out), gr, sg, sr, sc, int(accumulate), ws_ptr, ws_len, _stream(),
        )
    )
    return out


def sp_gemm_tn_product(a: SplitOperand, b: SplitOperand, *, a_cols=None, b_cols=None, out: Optional[torch.Tensor] = None,
                        scatter=None, accumulate: bool = False):
    """``sp_gemm_tn`` (the one-factor form) up to and including the product (tfgnn_sp_gemm_tn_product): the reduce pass comes
    back as a ``TnReduceJob`` for the NT product that follows (``sp_gemm_nt(..., tail=job)``).  ``out`` holds the result
    once the job has run - bit for bit what ``sp_gemm_tn`` writes.  -> (out, job)"""
    lib = _lib.load()
    if a.scale_block <= 0 or b.scale_block != b.cols:
        raise ValueError("sp_gemm_tn: the left operand needs per-(row, block) scales, the right one one scale per row")
    if a.rows != b.rows:
        raise ValueError(f"sp_gemm_tn: K differs ({a.rows} vs {b.rows})")
    a0, M = a_cols if a_cols is not None else (0, a.cols)
    b0, N = b_cols if b_cols is not None else (0, b.cols)
    K = a.rows
    if out is None:
        if scatter is not None or accumulate:
            raise ValueError("scatter / accumulate need out")
        out = torch.empty((M, N), dtype=torch.float32, device=a.data.device)
    if not out.is_contiguous() or out.numel() != M * N:
        raise ValueError(f"out must be contiguous with {M * N} elements")
    gr, sg, sr, sc = scatter if scatter is not None else (M, 0, N, 1)
    ws_bytes = lib.tfgnn_sp_gemm_tn_workspace_bytes(M, N, K, a.cols, a.scale_block)
    ws_ptr, ws_len, ws = None, 0, None
    if ws_bytes:
        # (its own buffer: it stays live until the job has been issued, whatever takes the shared one in between)
        ws_ptr, ws_len, ws = _aligned_workspace(a.data.device, ws_bytes, own=True)
        ws_ptr = ctypes.c_void_p(ws_ptr)
    c_job = _lib.TnReduceJob()
    _lib.check(
        lib.tfgnn_sp_gemm_tn_product(
            M, N, K, _ptr(a.data), a.data.stride(0), a0, _ptr(a.inv_scale), a.cols, a.scale_block, _ptr(b.data),
            b.data.stride(0), b0, _ptr(b.inv_scale), _ptr(out), gr, sg, sr, sc, int(accumulate), ws_ptr, ws_len,
            ctypes.byref(c_job), _stream(),
        )
    )
    return out, TnReduceJob(c_job, out, ws)


def tensor_inv_scale(bound: torch.Tensor) -> torch.Tensor:
    """2^-e with bound * 2^e in [2^14, 2^15) for a positive finite device scalar ``bound`` (>= the largest magnitude
    of the tensor that will be written with this scale): the fixed_inv_scale of the SP16 producers."""
    lib = _lib.load()
    out = torch.empty(1, dtype=torch.float32, device=bound.device)
    _lib.check(lib.tfgnn_sp_inv_scale_from_bound(_ptr(bound.contiguous()), _ptr(out), _stream()))
    return out


def absmax(x: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """device scalar scale * max |x| (tfgnn_absmax; order-independent, hence reproducible)."""
    lib = _lib.load()
    _require_dev(x, torch.float32, "x")
    x = x.contiguous()
    out = torch.zeros(1, dtype=torch.float32, device=x.device)
    _lib.check(lib.tfgnn_absmax(_ptr(x), x.numel(), float(scale), _ptr(out), _stream()))
    return out


_sp_weight_cache: "dict" = {}
_CHECK_WEIGHT_CACHE = [None]


def clear_weight_operand_cache() -> None:
    """Forget the derived forms of the weights (split SP16 operands, transposed / re-stacked copies).  bench.py calls it
    once per step so that the per-step cost of splitting the updated weights is inside the timed region."""
    _sp_weight_cache.clear()


def notify_weights_changed(tensor: Optional[torch.Tensor] = None) -> None:
    """Tell the library that weight values were changed by something torch's version counter does not see - an update
    through ``tensor.data``, a raw-pointer optimizer kernel, another framework writing into the buffer.  Every derived form
    of ``tensor`` (or of all weights) is dropped and rebuilt at its next use.  ``Variable.assign`` / ``Variable.mark_updated``
    call this; in-place torch arithmetic on ``Variable.value`` itself is seen through the version counter as well."""
    if tensor is None:
        _sp_weight_cache.clear()
        return
    base = tensor._base if tensor._base is not None else tensor
    lo = base.data_ptr()
    hi = lo + base.numel() * base.element_size()
    for key in [k for k in _sp_weight_cache if lo <= k[0] < hi]:
        del _sp_weight_cache[key]


def _weight_key(w: torch.Tensor, kind: str):
    return (w.data_ptr(), tuple(w.shape), tuple(w.stride()), kind)


def _weight_checksum(w: torch.Tensor):
    """debug mode TFGNN_CHECK_WEIGHT_CACHE=1: a checksum of the weight beside every cached form; a hit whose weight no
    longer has that checksum was updated behind the library's back (see notify_weights_changed) and raises."""
    if _CHECK_WEIGHT_CACHE[0] is None:
        import os

        _CHECK_WEIGHT_CACHE[0] = os.environ.get("TFGNN_CHECK_WEIGHT_CACHE", "0") == "1"
    if not _CHECK_WEIGHT_CACHE[0]:
        return None
    v = w.detach().double()
    return (float(v.sum()), float(v.abs().sum()))


def sp_weight_operand(w: torch.Tensor, kind: str, build):
    """A derived form of a weight tensor (its SP16 operands; also the transposed / re-stacked fp32 copies the bf16x3 products
    take), built once per value: keyed on the tensor's storage and version (an in-place torch update bumps the version;
    ``Variable.assign`` and ``notify_weights_changed`` drop the entry explicitly), so forward and backward passes of a step -
    and every step of an evaluation loop - share it.  ``build()`` makes the operand.  Updates torch cannot see
    (``var.value.data.add_(...)``, raw-pointer kernels) MUST be followed by ``Variable.mark_updated()`` /
    ``notify_weights_changed``; TFGNN_CHECK_WEIGHT_CACHE=1 verifies every hit against a checksum of the weight."""
    op = _cached_weight_operand(w, kind)
    if op is None:
        op = build()
        if isinstance(op, SplitJobs):
            aux_flush([op])
            op = op.operand
        _cache_weight_operand(w, kind, op)
    return op


def presplit_weight_operands(requests) -> int:
    """Build every STALE derived form among ``requests`` = [(w, kind, build)] now, the split jobs among them in one shared
    small-pass launch (``aux_flush``): the start of a stack's forward or backward pass, where all the operands of the pass can be
    split at once - the weights do not change between the optimizer update and the end of the backward pass - instead of one
    launch in front of every layer's product.  ``build()`` is what the consumer would hand to ``sp_weight_operand``; the same
    jobs, launched earlier: bit-identical operands.  An operand enters the cache only after its job has been launched, so a
    failure on the way leaves no entry behind that a later call could mistake for a built operand.
    -> number of operands built."""
    made, seen = [], set()
    for w, kind, build in requests:
        key = _weight_key(w, kind)
        if key in seen or _cached_weight_operand(w, kind) is not None:
            continue
        seen.add(key)
        made.append((w, kind, build()))
    if made:
        aux_flush([op for _, _, op in made if isinstance(op, SplitJobs)])
        for w, kind, op in made:
            _cache_weight_operand(w, kind, op.operand if isinstance(op, SplitJobs) else op)
    return len(made)


def _cached_weight_operand(w: torch.Tensor, kind: str):
    """The cached form ``kind`` of the current value of ``w``, or None."""
    hit = _sp_weight_cache.get(_weight_key(w, kind))
    if hit is not None and hit[0] == w._version and hit[2]() is not None:
        if hit[3] is not None and hit[3] != _weight_checksum(w):
            raise RuntimeError("a weight tensor changed without a version bump (update through .data or a raw pointer?): "
                               "call Variable.mark_updated() / ops.notify_weights_changed() after such an update")
        return hit[1]
    return None


def _cache_weight_operand(w: torch.Tensor, kind: str, op) -> None:
    import weakref

    if len(_sp_weight_cache) > 256:
        _sp_weight_cache.clear()
    base = w._base if w._base is not None else w  # views are temporaries: the entry lives as long as the parameter buffer
    _sp_weight_cache[_weight_key(w, kind)] = (w._version, op, weakref.ref(base), _weight_checksum(w))


# ---- neighbour sampling (include/tfgnn.h "Neighbour sampling", csrc/sample.hip) -----------------------------------------------
class NeighborSample:
    """What ``neighbor_sample`` returns: ``nodes`` int32 [n] (device, global ids, the seeds first), ``hop_ptr`` (host numpy
    int32 [K + 2]), ``adjacency_lists`` (device int32 [E_t, 2], local ids), ``status`` (int, the TFGNN_SAMPLE_* bits).  The
    device tensors are prefix views of buffers allocated at the capacity."""

    __slots__ = ("nodes", "hop_ptr", "adjacency_lists", "status", "num_seeds", "removed")

    def __init__(self, nodes, hop_ptr, adjacency_lists, status, num_seeds, removed=None):
        self.nodes, self.hop_ptr, self.adjacency_lists, self.status, self.num_seeds = nodes, hop_ptr, adjacency_lists, status, num_seeds
        self.removed = removed  # with ``exclude``: device int32 [L], the edges taken out of every list; else None


def sample_capacities(num_seeds: int, fanouts: Sequence[int], num_nodes: int, store_edges: Sequence[int],
                      max_in_degree: Sequence[int]):
    """(node capacity, [edge capacity per type]) that a sample of ``num_seeds`` distinct seeds can never exceed: a frontier
    of B nodes draws at most B * min(f, largest in-degree of the type) edges of a type (f < 0: the largest in-degree) and
    reaches at most as many new nodes as it draws edges; a row is drawn once per call, so a type never yields more than its
    E_t edges, and there are no more than V nodes."""
    frontier, nodes = int(num_seeds), int(num_seeds)
    edges = [0] * len(store_edges)
    for f in fanouts:
        drawn = 0
        for t, (e, deg) in enumerate(zip(store_edges, max_in_degree)):
            per_row = int(deg) if f < 0 else min(int(f), int(deg))
            n = min(frontier * per_row, int(e))
            edges[t] = min(edges[t] + n, int(e))
            drawn += n
        frontier = min(drawn, num_nodes)
        nodes = min(nodes + frontier, num_nodes)
    return max(nodes, min(int(num_seeds), num_nodes)), edges


def sample_launch_counts():
    """(launches enqueued by tfgnn_neighbor_sample, by tfgnn_gather_node_rows) in this process: host counters"""
    buf = (ctypes.c_int64 * 2)()
    _lib.check(_lib.load().tfgnn_sample_launch_counts(buf, 2))
    return int(buf[0]), int(buf[1])


def sample_exclude_launch_counts() -> int:
    """tfgnn_sample_exclude_launch_counts: kernel launches of ``sample_exclude_edges`` so far (4 per call; a host counter)."""
    buf = (ctypes.c_int64 * 1)()
    _lib.check(_lib.load().tfgnn_sample_exclude_launch_counts(buf, 1))
    return int(buf[0])


def sample_exclude_workspace_words(edge_capacity: Sequence[int]) -> int:
    """int32 words of tfgnn_sample_exclude_workspace_bytes for lists of these capacities"""
    L = len(edge_capacity)
    caps = (ctypes.c_int64 * max(L, 1))(*[int(e) for e in edge_capacity])
    nbytes = int(_lib.load().tfgnn_sample_exclude_workspace_bytes(L, ctypes.addressof(caps)))
    if nbytes == 0:
        raise ValueError("no exclusion workspace for these capacities (include/tfgnn.h: limits of tfgnn_sample_exclude_edges)")
    return nbytes // 4


def sample_exclude_edges(adjacency_lists: Sequence[torch.Tensor], meta: torch.Tensor, num_seeds: int, positives: torch.Tensor,
                         fwd_type: Sequence[int], inv_type: Sequence[int], workspace: Optional[torch.Tensor] = None,
                         record: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Take a batch's positives out of a sampled subgraph by one tfgnn_sample_exclude_edges call (4 launches on the current
    stream; include/tfgnn.h "Excluding a batch's positives").  ``adjacency_lists``: the sampler's lists at their CAPACITY
    (int32 [cap_t, 2], local ids, sorted by target), ``meta`` its meta words on the device - the live counts are read and
    updated there -, ``positives`` int32 [B, 3] rows (u, r, v) in local ids, ``fwd_type`` / ``inv_type``: per relation the
    processed edge type of its forward edges and of their inverses (-1: none).  Every edge (u, v) of list fwd_type[r] and
    every edge (v, u) of list inv_type[r] goes; the kept edges keep their order.  -> ``record`` int32 [L + 1] on the device:
    the edges removed per list, then the status word (``_lib.SAMPLE_EXCLUDE_*``; also OR-ed into meta's status).  Nothing
    is read back here."""
    _require_dev(meta, torch.int32, "meta")
    L, T = len(adjacency_lists), len(fwd_type)
    if len(inv_type) != T:
        raise ValueError("fwd_type and inv_type name the same relations")
    for t in adjacency_lists:
        _require_dev(t, torch.int32, "an adjacency list")
        if t.dim() != 2 or t.shape[1] != 2 or not t.is_contiguous():
            raise ValueError(f"an adjacency list must be a contiguous int32 [capacity, 2], got {tuple(t.shape)}")
    if not meta.is_contiguous() or meta.numel() < _lib.SAMPLE_META_EDGES + L:
        raise ValueError("meta must be the sampler's contiguous meta words")
    B = _device_triples(positives, "positives")
    dev = meta.device
    edge_cap = [int(t.shape[0]) for t in adjacency_lists]
    if workspace is None:
        workspace = torch.empty(sample_exclude_workspace_words(edge_cap), dtype=torch.int32, device=dev)
    _require_dev(workspace, torch.int32, "workspace")
    if record is None:
        record = torch.empty(L + 1, dtype=torch.int32, device=dev)
    _require_dev(record, torch.int32, "record")
    if not record.is_contiguous() or record.numel() < L + 1:
        raise ValueError(f"record must be a contiguous int32 [{L + 1}]")
    a = _lib.SampleExcludeArgs()
    a.struct_size = ctypes.sizeof(_lib.SampleExcludeArgs)
    a.num_edge_types, a.num_relations, a.num_seeds, a.num_positives = L, T, int(num_seeds), B
    fwd = (ctypes.c_int32 * max(T, 1))(*[int(x) for x in fwd_type])
    inv = (ctypes.c_int32 * max(T, 1))(*[int(x) for x in inv_type])
    caps = (ctypes.c_int64 * max(L, 1))(*edge_cap)
    adj_tab = (ctypes.c_void_p * max(L, 1))(*[t.data_ptr() for t in adjacency_lists])
    a.positives, a.fwd_type, a.inv_type = positives.data_ptr(), ctypes.addressof(fwd), ctypes.addressof(inv)
    a.edge_capacity, a.adjacency_lists = ctypes.addressof(caps), ctypes.addressof(adj_tab)
    a.meta, a.record = meta.data_ptr(), record.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 4
    _lib.check(_lib.load().tfgnn_sample_exclude_edges(ctypes.byref(a), _stream()))
    for t in list(adjacency_lists) + [meta, record]:
        torch.autograd.graph.increment_version(t)  # written through raw pointers, which torch does not see
    return record


def neighbor_sample(store, seeds: torch.Tensor, fanouts: Sequence[int], seed: int, out=None, exclude=None) -> NeighborSample:
    """One K-hop neighbour sample (K = len(fanouts); a fanout < 0 takes every in-edge) of the int32 device tensor ``seeds``
    on ``store`` (data.NeighborStore: the in-CSR per edge type, kept on the device): 3 + 6 K launches on the current stream,
    then ONE small device-to-host copy of the counts - the sizes are data-dependent and the graph build needs them on the
    host.  That copy synchronises, so a sampled batch cannot be captured in a CapturedStep.  Buffers are allocated at
    ``sample_capacities`` - they cannot overflow - unless ``out`` = (nodes [cap], [adjacency_list [cap_t, 2]]) brings smaller
    ones; what does not fit then sets an overflow bit in ``status``.  The draw is a pure function of (seed, node, type).
    ``exclude`` = (positives int32 [B, 3] in local ids, fwd_type, inv_type): ``sample_exclude_edges`` is enqueued between
    the sampler and the copy - draw first, then drop; a row may keep fewer edges than its fanout - and ``removed`` of the
    result is the device int32 [L] of edges taken out of every list; ``nodes`` and ``hop_ptr`` are what they are without
    it.  None: the call above and nothing else."""
    _require_dev(seeds, torch.int32, "seeds")
    seeds = seeds.contiguous().view(-1)
    S, L, K, V = int(seeds.shape[0]), store.num_edge_types, len(fanouts), store.num_nodes
    dev = seeds.device
    if out is None:
        node_cap, edge_cap = sample_capacities(S, fanouts, V, store.store_edges, store.max_in_degree)
        nodes = torch.empty(node_cap, dtype=torch.int32, device=dev)
        flat = torch.empty(2 * sum(-(-e // 32) * 32 for e in edge_cap), dtype=torch.int32, device=dev)
        adj, at = [], 0
        for e in edge_cap:  # every list starts on a 256-byte boundary
            adj.append(flat[at:at + 2 * e].view(e, 2))
            at += 2 * (-(-e // 32) * 32)
    else:
        nodes, adj = out
        node_cap, edge_cap = int(nodes.shape[0]), [int(a.shape[0]) for a in adj]
        for a in [nodes] + list(adj):
            _require_dev(a, torch.int32, "a sample output")
            if not a.is_contiguous():
                raise ValueError("sample outputs must be contiguous")
    meta = torch.empty(_lib.sample_meta_words(L, K), dtype=torch.int32, device=dev)
    workspace = store.workspace(node_cap)
    a = _lib.NeighborSampleArgs()
    a.struct_size = ctypes.sizeof(_lib.NeighborSampleArgs)
    a.num_edge_types, a.num_hops, a.num_nodes = L, K, V
    a.in_ptr, a.in_src = ctypes.addressof(store._in_ptr_tab), ctypes.addressof(store._in_src_tab)
    a.store_edges = ctypes.addressof(store._store_edges_tab)
    fan = (ctypes.c_int32 * max(K, 1))(*[int(f) for f in fanouts])
    caps = (ctypes.c_int64 * max(L, 1))(*edge_cap)
    adj_tab = (ctypes.c_void_p * max(L, 1))(*[t.data_ptr() for t in adj])
    a.fanouts, a.seed, a.num_seeds, a.seeds = ctypes.addressof(fan), int(seed) & (2 ** 64 - 1), S, seeds.data_ptr()
    a.node_capacity, a.edge_capacity, a.nodes = node_cap, ctypes.addressof(caps), nodes.data_ptr()
    a.adjacency_lists, a.meta = ctypes.addressof(adj_tab), meta.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 4
    _lib.check(_lib.load().tfgnn_neighbor_sample(ctypes.byref(a), _stream()))
    removed = None
    if exclude is not None:
        positives, fwd_type, inv_type = exclude
        removed = sample_exclude_edges(adj, meta, S, positives, fwd_type, inv_type,
                                       workspace=store.exclude_workspace(sample_exclude_workspace_words(edge_cap)))[:L]
    host = meta.cpu().numpy()  # the one copy
    n = int(host[_lib.SAMPLE_META_NODES])
    counts = host[_lib.SAMPLE_META_EDGES:_lib.SAMPLE_META_EDGES + L]
    hop_ptr = host[_lib.SAMPLE_META_EDGES + L:].copy()
    return NeighborSample(nodes[:n], hop_ptr, [t[:int(c)] for t, c in zip(adj, counts)], int(host[_lib.SAMPLE_META_STATUS]), S,
                          removed)


def gather_node_rows(nodes: torch.Tensor, num_seeds: int, features: torch.Tensor, columns: Sequence[torch.Tensor] = (),
                     seed_only: Sequence[bool] = (), out=None, bad_flag: Optional[torch.Tensor] = None):
    """The rows of a sampled batch by one tfgnn_gather_node_rows launch: -> (features[nodes], [column[nodes] ...]), where a
    column whose ``seed_only`` flag is set is zero in the rows >= ``num_seeds``.  ``out`` = (node_features, [columns]) may
    bring the outputs; ``bad_flag`` (zeroed int32 [1]) is set by a node id outside the store."""
    _require_dev(nodes, torch.int32, "nodes")
    _require_dev(features, torch.float32, "features")
    nodes = nodes.contiguous().view(-1)
    n, V, F = int(nodes.shape[0]), int(features.shape[0]), int(features.shape[1])
    columns, seed_only = list(columns), [bool(s) for s in seed_only] + [False] * (len(columns) - len(seed_only))
    for c in [features] + columns:
        _require_dev(c, torch.float32, "a node column")
        if c.dim() != 2 or int(c.shape[0]) != V or c.stride(1) != 1 or c.stride(0) != c.shape[1]:
            raise ValueError("features and node columns must be row-contiguous [V, W] over the same nodes")
    widths = [int(c.shape[1]) for c in columns]
    if out is None:
        out = (torch.empty((n, F), dtype=torch.float32, device=nodes.device),
               [torch.empty((n, w), dtype=torch.float32, device=nodes.device) for w in widths])
    nf, cols = out
    for t, w in zip([nf] + list(cols), [F] + widths):
        _require_dev(t, torch.float32, "a gather output")
        if tuple(t.shape) != (n, w) or t.stride(1) != 1 or t.stride(0) != w:
            raise ValueError(f"a gather output must be a row-contiguous float32 [{n}, {w}]")
    NC = len(columns)
    a = _lib.GatherNodeRowsArgs()
    a.struct_size = ctypes.sizeof(_lib.GatherNodeRowsArgs)
    a.store_nodes, a.num_rows, a.num_seeds, a.nodes = V, n, int(num_seeds), nodes.data_ptr()
    a.feature_dim, a.features, a.node_features = F, features.data_ptr(), nf.data_ptr()
    if NC:
        width_tab = (ctypes.c_int64 * NC)(*widths)
        col_tab = (ctypes.c_void_p * NC)(*[c.data_ptr() for c in columns])
        out_tab = (ctypes.c_void_p * NC)(*[c.data_ptr() for c in cols])
        flag_tab = (ctypes.c_int32 * NC)(*[int(s) for s in seed_only])
        a.num_node_columns, a.node_column_widths = NC, ctypes.addressof(width_tab)
        a.node_columns, a.node_column_out, a.seed_only = ctypes.addressof(col_tab), ctypes.addressof(out_tab), ctypes.addressof(flag_tab)
    a.bad_flag = bad_flag.data_ptr() if bad_flag is not None else None
    _lib.check(_lib.load().tfgnn_gather_node_rows(ctypes.byref(a), _stream()))
    return nf, list(cols)


# ---- triple batches (include/tfgnn.h "Triple batches", csrc/triple_batch.hip) ----------------------------------------------------
def triple_batch_launch_counts() -> int:
    """tfgnn_triple_batch_launch_counts: kernel launches of ``triple_batch`` so far (6 per call; a host counter)."""
    buf = (ctypes.c_int64 * 1)()
    _lib.check(_lib.load().tfgnn_triple_batch_launch_counts(buf, 1))
    return int(buf[0])


def triple_batch_workspace(V: int, device=None) -> torch.Tensor:
    """An int32 workspace of tfgnn_triple_batch_workspace_bytes(V) for ``triple_batch``, its id table (the first V words)
    filled with -1 as every call expects and leaves it."""
    nbytes = int(_lib.load().tfgnn_triple_batch_workspace_bytes(int(V)))
    if nbytes == 0:
        raise ValueError(f"no triple-batch workspace for V = {V} (include/tfgnn.h: V in [1, 2^31))")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    ws[:int(V)].fill_(-1)
    return ws


def triple_batch(positives: torch.Tensor, positive_ids: torch.Tensor, K: int, V: int, seed: int, workspace: torch.Tensor,
                 out=None):
    """One mini-batch of link-prediction triples by one tfgnn_triple_batch_build call (6 launches on the current stream):
    ``positives`` int32 [P, 3] (device, global ids), ``positive_ids`` int32 [B] (device) -> ``(triples, local_triples,
    seeds[:S], S, status)``: triples int32 [B (1 + K), 3] = the B positives followed by K negatives each, drawn as
    ``draw_negative_triples(seed, use_epoch=False)`` draws them; seeds = their distinct endpoints in increasing id - what
    ``neighbor_sample`` takes as seeds; local_triples = the triples with every endpoint replaced by its position in seeds,
    which is its row in the sampled batch.  ``status``: the TFGNN_TRIPLE_BATCH_* bits (include/tfgnn.h).
    ``workspace``: int32, ``triple_batch_workspace(V)`` or a NeighborStore workspace of at least that size - its first V
    words are -1 on entry and on exit.  ``out`` = (triples [N, 3], local_triples [N, 3], seeds [capacity]) brings the
    outputs; otherwise they are allocated, seeds at min(2 N, V), which cannot overflow.
    After the call ONE 8-byte device-to-host copy reads (status, S): the sampler needs S on the host.  That copy
    synchronises: with the sampler's own copy of its counts a mini-batch costs two small copies, and - like every sampled
    batch - it cannot be captured in a CapturedStep."""
    _require_dev(positives, torch.int32, "positives")
    _require_dev(positive_ids, torch.int32, "positive_ids")
    _require_dev(workspace, torch.int32, "workspace")
    P = _device_triples(positives, "positives")
    if positive_ids.dim() != 1 or not positive_ids.is_contiguous():
        raise ValueError("positive_ids must be a contiguous int32 [B]")
    B, K, V = int(positive_ids.shape[0]), int(K), int(V)
    N = B * (1 + max(K, 0))
    dev = positives.device
    if out is None:
        out = (torch.empty((N, 3), dtype=torch.int32, device=dev), torch.empty((N, 3), dtype=torch.int32, device=dev),
               torch.empty(max(1, min(2 * N, V)), dtype=torch.int32, device=dev))
    triples, local, seeds = out
    for t, what in ((triples, "triples"), (local, "local_triples")):
        if _device_triples(t, what) != N:
            raise ValueError(f"{what} must hold B (1 + K) = {N} rows, not {t.shape[0]}")
    _require_dev(seeds, torch.int32, "seeds")
    if seeds.dim() != 1 or not seeds.is_contiguous():
        raise ValueError("seeds must be a contiguous int32 [capacity]")
    meta = torch.empty(2, dtype=torch.int32, device=dev)
    a = _lib.TripleBatchArgs()
    a.struct_size = ctypes.sizeof(_lib.TripleBatchArgs)
    a.num_nodes, a.num_positives, a.positives = V, P, positives.data_ptr()
    a.batch_size, a.positive_ids, a.negatives_per_positive = B, positive_ids.data_ptr(), K
    a.seed, a.seed_capacity = int(seed) & (2 ** 64 - 1), int(seeds.shape[0])
    a.triples, a.local_triples, a.seeds, a.meta = triples.data_ptr(), local.data_ptr(), seeds.data_ptr(), meta.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 4
    _lib.check(_lib.load().tfgnn_triple_batch_build(ctypes.byref(a), _stream()))
    for t in (triples, local, seeds):
        torch.autograd.graph.increment_version(t)  # written through raw pointers, which torch does not see
    status, S = (int(x) for x in meta.cpu().numpy())  # the one copy
    return triples, local, seeds[:S], S, status


# ---- node embeddings: include/tfgnn.h "Node embeddings", csrc/embedding.hip --------------------------------------------------------
def embedding_launch_count() -> int:
    """tfgnn_embedding_launch_count: kernel launches of ``embedding_scatter_rows`` so far (a host counter)."""
    return int(_lib.load().tfgnn_embedding_launch_count())


@_writes_out
def embedding_scatter_rows(rows: torch.Tensor, ids: torch.Tensor, num_rows: int, out: Optional[torch.Tensor] = None,
                           bad_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of ``table[ids]`` (``gather_node_rows``) with respect to a table of ``num_rows`` rows, dense: -> float32
    [num_rows, D] with row ids[i] = rows[i] and zeros elsewhere (tfgnn_embedding_scatter_rows: a fill and a scatter on the
    current stream; capturable).  The ids are DISTINCT by precondition.  ``rows`` [n, D] and ``out`` may be pitched (unit inner
    stride); the columns of ``out`` beyond D are left alone.  ``bad_flag`` (zeroed int32 [1]) is set by an id outside the table."""
    _require_dev(rows, torch.float32, "rows")
    _require_dev(ids, torch.int32, "ids")
    rows, ld_rows = _rowmajor(rows, "rows")
    ids = ids.contiguous().view(-1)
    n, D, N = int(rows.shape[0]), int(rows.shape[1]), int(num_rows)
    if int(ids.shape[0]) != n:
        raise ValueError(f"embedding_scatter_rows: {int(ids.shape[0])} ids for {n} rows")
    if out is None:
        out = torch.empty((max(N, 0), D), dtype=torch.float32, device=rows.device)
    _require_dev(out, torch.float32, "out")
    if out.dim() != 2 or tuple(out.shape) != (N, D) or (D and out.stride(1) != 1):
        raise ValueError(f"embedding_scatter_rows: out must be a float32 [{N}, {D}] with unit inner stride")
    ld_out = int(out.stride(0)) if N > 1 else max(int(out.stride(0)), D)
    if bad_flag is not None:
        _require_dev(bad_flag, torch.int32, "bad_flag")
    _lib.check(_lib.load().tfgnn_embedding_scatter_rows(_ptr(rows) if n else None, ld_rows, _ptr(ids) if n else None, n, D,
                                                        _ptr(out) if N else None, ld_out, N, _ptr(bad_flag), _stream()))
    return out
