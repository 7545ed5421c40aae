"""tfgnn_graph_scales_edge_dropout (include/tfgnn.h) in numpy, written from the header's text: the keep decision of every edge
from tests/dropout_reference.py (edge id = position in concat(adjacency_lists), one rate per edge type), the kept in-degrees
c'[v, l] and N'[v] as integers, and the three arrays in float32 with the header's expressions.  Everything is returned in
EDGE-ID order; the device's two edge orders are reached through TFGNN_G_EID_BY_DST / _BY_SRC.  Independent of the library."""
from typing import NamedTuple

import numpy as np

from tests import dropout_reference as dr

SMALL = np.float32(1e-7)
ONE = np.float32(1.0)


class Scales(NamedTuple):
    keep: np.ndarray        # bool [E]
    c: np.ndarray           # int64 [V, L] kept in-edges per (target, type)
    n: np.ndarray           # int64 [V]    kept in-edges per target
    node_scale: np.ndarray  # float32 [V]  m_v
    s: np.ndarray           # float32 [E]  s_e  (the by-dst array's values)
    s_src: np.ndarray       # float32 [E]  s_e * m_target (the by-src array's values)


def edge_types(adjs) -> np.ndarray:
    return np.concatenate([np.full(a.shape[0], l, dtype=np.int64) for l, a in enumerate(adjs)]) if len(adjs) else np.zeros(0, np.int64)


def edge_targets(adjs) -> np.ndarray:
    return np.concatenate([a[:, 1].astype(np.int64) for a in adjs]) if len(adjs) else np.zeros(0, np.int64)


def keep_edges(edges_per_type, rates, seed: int, epoch: int = 0) -> np.ndarray:
    """bool [E]: edge e of type l is kept iff element e of the mask drawn for (seed, rates[l]) at `epoch` is non-zero"""
    assert len(rates) == len(edges_per_type)
    out, first = [], 0
    for n, rate in zip(edges_per_type, rates):
        out.append(dr.keep(seed, rate, epoch, first, int(n)))
        first += int(n)
    return np.concatenate(out) if out else np.zeros(0, dtype=bool)


def node_mult(n: np.ndarray, mode: int) -> np.ndarray:
    """m_v in float32: 1 | 1 / max(N, 1) | 1 / sqrt(max(N, 1))"""
    nf = np.maximum(n.astype(np.float32), ONE)
    if mode == 0:
        return np.ones(n.shape[0], dtype=np.float32)
    return (ONE / nf if mode == 1 else ONE / np.sqrt(nf)).astype(np.float32)


def scales_of_kept(adjs, V: int, keep: np.ndarray, normalize: bool, mode: int, kept_factor: np.ndarray) -> Scales:
    """the three arrays for a given keep pattern; kept_factor [L] float32 = the weight of a kept edge where no count divides"""
    L = len(adjs)
    t, tgt = edge_types(adjs), edge_targets(adjs)
    c = np.zeros((V, max(L, 1)), dtype=np.int64)
    np.add.at(c, (tgt[keep], t[keep]), 1)
    n = c.sum(axis=1)
    m = node_mult(n, mode)
    if normalize:
        kept_value = (ONE / (c[tgt, t].astype(np.float32) + SMALL)).astype(np.float32)
    elif mode == 0:
        kept_value = np.asarray(kept_factor, dtype=np.float32)[t]
    else:
        kept_value = np.ones(t.shape[0], dtype=np.float32)
    s = np.where(keep, kept_value, np.float32(0.0)).astype(np.float32)
    return Scales(keep, c[:, :L], n, m, s, (s * m[tgt]).astype(np.float32))


def scales(adjs, V: int, rates, seed: int, epoch: int, normalize: bool, mode: int) -> Scales:
    """tfgnn_graph_scales_edge_dropout: where a count divides it is the count of kept edges, where none does kept edges
    carry float32 1 / (1 - rate)"""
    keep = keep_edges([a.shape[0] for a in adjs], rates, seed, epoch)
    factor = np.array([dr.scale(r) for r in rates], dtype=np.float32)
    return scales_of_kept(adjs, V, keep, normalize, mode, factor)


def plain_scales(adjs, V: int, normalize: bool, mode: int):
    """today's tfgnn_graph_scales, stated directly: -> (node_scale [V], s [E], s_src [E]) in float32, edge-id order"""
    L = len(adjs)
    t, tgt = edge_types(adjs), edge_targets(adjs)
    c = np.zeros((V, max(L, 1)), dtype=np.int64)
    np.add.at(c, (tgt, t), 1)
    m = node_mult(c.sum(axis=1), mode)
    s = (ONE / (c[tgt, t].astype(np.float32) + SMALL)).astype(np.float32) if normalize else np.ones(t.shape[0], dtype=np.float32)
    return m, s, (s * m[tgt]).astype(np.float32)
