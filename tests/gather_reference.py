"""fp64 host references of the planned graph gather (csrc/spmm.hip, ``ops.graph_gather``) and of the backward pass through a
general aggregation (csrc/edge.hip, ``ops.edge_aggregate_backward``).  Plain numpy / torch on the CPU, no device code:
rows and columns come from the host arrays only (oracle.adjacency_oracle.bucket_edges and the view definitions of
include/tfgnn.h).  tests/test_gather_reference_host.py pins these functions to the oracle's segment operations so that a
mistake here is not read as a kernel bug."""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import adjacency_oracle as ao

FLOAT_LOWEST = float(np.finfo(np.float32).min)  # an empty max row (tf.math.unsorted_segment_max on fp32)

(VIEW_BY_DST_TYPED, VIEW_BY_DST_NODE, VIEW_BY_SRC_TYPED, VIEW_BY_SRC_NODE, VIEW_BY_DST_TYPED_COMPACT,
 VIEW_BY_SRC_TYPED_COMPACT, VIEW_BY_DST_TYPED_PATTERN) = range(7)  # include/tfgnn.h tfgnn_graph_view


def _gelu(x):
    return x * 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x * x * x)))


_ACTS = {
    "relu": torch.relu,
    "tanh": torch.tanh,
    "leaky_relu": lambda x: torch.nn.functional.leaky_relu(x, 0.2),
    "elu": torch.nn.functional.elu,
    "selu": torch.nn.functional.selu,
    "gelu": _gelu,
    "sigmoid": torch.sigmoid,
}


def activation(name):
    """name -> fp64-capable function (None: identity)"""
    if name is None:
        return lambda x: x
    return _ACTS[name]


def _weights64(edge_weight, num_edges: int, width: int):
    """[E] or [E, K] edge weights -> fp64 [E, width] (head k covers columns k * width / K .. (k + 1) * width / K)"""
    if edge_weight is None:
        return None
    w = torch.as_tensor(edge_weight).double()
    if w.dim() == 1:
        assert w.shape[0] == num_edges
        return w.unsqueeze(1).expand(num_edges, width)
    K = w.shape[1]
    assert w.shape[0] == num_edges and width % K == 0
    return w.repeat_interleave(width // K, dim=1)


def gather_reference(rowptr, col, inp, *, edge_weight=None, row_scale=None, reduce="sum", pre_act=None, post_act=None):
    """out[r] = post_act(row_scale[r] * REDUCE_{e in row r} pre_act(w_e * inp[col_e])) in fp64 from the fp32 inputs.
    -> (out64 [R, width], l1_64 [R, width] = sum |terms| * max(1, |row_scale|), row_len int64 [R]).
    An empty max row is the lowest finite fp32 and is not scaled."""
    assert reduce in ("sum", "max")
    rowptr = np.asarray(rowptr, dtype=np.int64)
    col = torch.from_numpy(np.asarray(col, dtype=np.int64))
    R, E = rowptr.shape[0] - 1, int(col.shape[0])
    assert rowptr[0] == 0 and rowptr[-1] == E and np.all(np.diff(rowptr) >= 0)
    row_len = torch.from_numpy(np.diff(rowptr))
    width = inp.shape[1]
    terms = inp.detach().cpu().double()[col]
    w = _weights64(edge_weight, E, width)
    if w is not None:
        terms = terms * w
    terms = activation(pre_act)(terms)
    seg = torch.repeat_interleave(torch.arange(R), row_len)
    l1 = torch.zeros((R, width), dtype=torch.float64).index_add_(0, seg, terms.abs())
    rs = None if row_scale is None else torch.as_tensor(row_scale).detach().cpu().double().reshape(R, 1)
    if reduce == "sum":
        out = torch.zeros((R, width), dtype=torch.float64).index_add_(0, seg, terms)
        if rs is not None:
            out = out * rs
    else:
        out = torch.full((R, width), FLOAT_LOWEST, dtype=torch.float64)
        if E:
            out = out.scatter_reduce(0, seg.unsqueeze(1).expand(E, width), terms, reduce="amax", include_self=True)
        if rs is not None:
            nonempty = row_len > 0
            out[nonempty] = out[nonempty] * rs[nonempty]
    if rs is not None:
        l1 = l1 * rs.abs().clamp(min=1.0)
    return activation(post_act)(out), l1, row_len


def view_rows(adjacency_lists, num_nodes: int, view: int, pattern_pos=None):
    """Host arrays of one view of the graph handle -> (rowptr, col, out_rows): row i of the view's output is CSR row
    out_rows[i] (None: the identity).
      typed views    oracle.adjacency_oracle.bucket_edges (rows node * L + type)
      node views     rowptr[::L] with col * L + type (include/tfgnn.h)
      compact views  the non-empty buckets in type-major order
      pattern view   bucket (v, l) at row pattern_pos[v] * L + l (the device's TFGNN_G_PATTERN_POS_BY_DST, a permutation
                     of the nodes: the order inside a pattern is free by specification)"""
    L = len(adjacency_lists)
    by = "src" if view in (VIEW_BY_SRC_TYPED, VIEW_BY_SRC_NODE, VIEW_BY_SRC_TYPED_COMPACT) else "dst"
    rowptr, col, typ = ao.bucket_edges(adjacency_lists, num_nodes, by=by)
    rowptr, col, typ = rowptr.astype(np.int64), col.astype(np.int64), typ.astype(np.int64)
    if view in (VIEW_BY_DST_NODE, VIEW_BY_SRC_NODE):
        return rowptr[::L].copy(), col * L + typ, None
    if view in (VIEW_BY_DST_TYPED_COMPACT, VIEW_BY_SRC_TYPED_COMPACT):
        nonempty = (np.diff(rowptr) > 0).reshape(num_nodes, L)
        rows = [v * L + l for l in range(L) for v in range(num_nodes) if nonempty[v, l]]
        return rowptr, col, np.asarray(rows, dtype=np.int64)
    if view == VIEW_BY_DST_TYPED_PATTERN:
        pos = np.asarray(pattern_pos, dtype=np.int64)
        assert pos.shape == (num_nodes,) and np.array_equal(np.sort(pos), np.arange(num_nodes)), "not a permutation"
        out_rows = np.empty(num_nodes * L, dtype=np.int64)
        v = np.arange(num_nodes)
        for l in range(L):
            out_rows[pos * L + l] = v * L + l
        return rowptr, col, out_rows
    return rowptr, col, None


def aggregate_backward_reference(msg, target, grad_agg, *, num_targets: int, msg_row=None, edge_weight=None, node_scale=None,
                                 pre_act=None, reduce="sum"):
    """fp64 gradient of agg[t] = node_scale[t] * REDUCE_{e -> t} pre_act(w_e * msg[row_e]) with respect to every edge's
    msg[row_e] contribution, weighted by grad_agg [num_targets, width].
      sum -> grad [E, width] (torch.autograd)
      max -> (selected bool [E, width], num_ties [num_targets, width], grad [E, width], gap [num_targets, width]): the
             gradient is split evenly among the edges that attain the maximum; ties are decided on the fp32-rounded product
             u = fl32(w_e * msg) taken through the activation in fp64.  gap = distance of the best non-selected edge from
             the maximum, relative to max(1, |max|) (inf where every edge is selected): the caller's precondition."""
    assert reduce in ("sum", "max")
    msg = msg.detach().cpu()
    target = torch.as_tensor(target).long()
    E, width = int(target.shape[0]), msg.shape[1]
    row = torch.arange(E) if msg_row is None else torch.as_tensor(msg_row).long()
    w32 = None if edge_weight is None else torch.as_tensor(edge_weight).detach().cpu().float().reshape(E, 1)
    grad_agg = grad_agg.detach().cpu().double()
    act = activation(pre_act)
    m = msg.double()[row].clone().requires_grad_(True)
    u = m if w32 is None else m * w32.double()
    z = act(u)
    idx = target.unsqueeze(1).expand(E, width)
    if reduce == "sum":
        agg = torch.zeros((num_targets, width), dtype=torch.float64).index_add(0, target, z)
        if node_scale is not None:
            agg = agg * torch.as_tensor(node_scale).detach().cpu().double().reshape(num_targets, 1)
        (g,) = torch.autograd.grad((agg * grad_agg).sum(), m)
        return g
    assert node_scale is None, "the max branch takes no node scale"
    u32 = msg.float()[row] if w32 is None else msg.float()[row] * w32  # one fp32 rounding, as the kernels take it
    z32 = act(u32.double())
    top = torch.full((num_targets, width), -math.inf, dtype=torch.float64).scatter_reduce(0, idx, z32, reduce="amax")
    selected = z32 == top[target]
    num_ties = torch.zeros((num_targets, width), dtype=torch.float64).index_add_(0, target, selected.double())
    rest = torch.where(selected, torch.full_like(z32, -math.inf), z32)
    second = torch.full((num_targets, width), -math.inf, dtype=torch.float64).scatter_reduce(0, idx, rest, reduce="amax")
    gap = (top - second) / top.abs().clamp(min=1.0)
    gap[torch.isinf(top)] = math.inf  # targets without edges
    share = torch.where(selected, grad_agg[target] / num_ties[target].clamp(min=1.0), torch.zeros_like(z32))
    (g,) = torch.autograd.grad((z * share).sum(), m)
    return selected, num_ties, g, gap
