"""Host reference of the graph readout (include/tfgnn.h "Graph readout": tfgnn_pool_forward / tfgnn_pool_backward) in numpy
float64, written from that contract: plain loops over whole graphs, one (graph, head) at a time - no chunks, no tiles, no
workspace.  fp32 inputs are cast up: they are the common starting point of the kernels and of this file.

    h(f) = f // (GD // heads)
    out[g, f] = sum over the nodes v of graph g of w[v, h(f)] * clip(T[v, f])             (an empty graph: a zero row)
    softmax: w = exp(S - m) / (sum over the graph of exp(S - m) + 1e-7), m = the graph's largest score, per (graph, head)
    sigmoid: w = S      none: w = 1      average: w = 1 / max(number of nodes of g, 1)
    dT[v, f] = w[v, h(f)] * dOut[g, f] where lo <= T[v, f] <= hi, else 0
    dw[v, h] = sum over the features f of head h of clip(T[v, f]) * dOut[g, f]
    softmax: dS = w * (dw - sum over the graph of w * dw)      sigmoid: dS = dw      none, average: no dS

A bound of None is no operation at all, not a comparison with an infinity: without bounds a NaN in T passes through the
clip AND through dT (= w * dOut there, no mask).  With a bound the clip is tf.maximum / tf.minimum: a NaN stays a NaN, an
infinity clips, and the mask of dT is false at a NaN."""
from __future__ import annotations

import numpy as np

KINDS = ("softmax", "sigmoid", "average", "none")
SMALL_NUMBER = 1e-7


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def clip(T, lo, hi):
    """tf.maximum(T, lo) then tf.minimum(., hi), each only where its bound is present; NaN stays NaN"""
    R = _f64(T)
    if lo is not None:
        R = np.where(R < lo, float(lo), R)
    if hi is not None:
        R = np.where(R > hi, float(hi), R)
    return R


def pass_mask(T, lo, hi):
    """where the gradient passes the clip: lo <= T <= hi, equality included (TensorFlow's MaximumMinimumGrad)"""
    T = _f64(T)
    m = np.ones(T.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        if lo is not None:
            m &= T >= lo
        if hi is not None:
            m &= T <= hi
    return m


def weights(kind, ptr, S, heads, V):
    """w [V, heads] in float64 for every kind"""
    G = len(ptr) - 1
    w = np.ones((V, heads), dtype=np.float64)
    if kind == "sigmoid":
        return _f64(S).copy()
    if kind == "none":
        return w
    S = _f64(S)
    for g in range(G):
        a, b = int(ptr[g]), int(ptr[g + 1])
        if a == b:
            continue
        if kind == "average":
            w[a:b] = 1.0 / (b - a)
            continue
        assert kind == "softmax", kind
        for h in range(heads):
            s = S[a:b, h]
            with np.errstate(invalid="ignore", over="ignore"):
                m = np.max(s)  # NaN if any score is: so is everything below
                e = np.exp(s - m)  # +inf - +inf = NaN
                w[a:b, h] = e / (np.sum(e) + SMALL_NUMBER)
    return w


def forward(kind, ptr, T, S, heads, lo, hi):
    """-> (out [G, GD], w [V, heads]) in float64; w is returned for every kind (what the sum was weighted with)"""
    T = _f64(T)
    V, GD = T.shape
    G = len(ptr) - 1
    assert heads > 0 and GD % heads == 0
    ph = GD // heads
    w = weights(kind, ptr, S, heads, V)
    R = clip(T, lo, hi)
    out = np.zeros((G, GD), dtype=np.float64)
    wf = np.repeat(w, ph, axis=1)  # w[v, h(f)]
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(G):
            a, b = int(ptr[g]), int(ptr[g + 1])
            if b > a:
                out[g] = np.sum(wf[a:b] * R[a:b], axis=0)
    return out, w


def backward(kind, ptr, dOut, T, w_or_S, heads, lo, hi):
    """-> (dT [V, GD], dS [V, heads] or None).  ``w_or_S``: the softmax weights (softmax), the sigmoid weights S (sigmoid),
    ignored for none / average."""
    T, dOut = _f64(T), _f64(dOut)
    V, GD = T.shape
    G = len(ptr) - 1
    ph = GD // heads
    w = weights(kind, ptr, None, heads, V) if kind in ("none", "average") else _f64(w_or_S)
    R = clip(T, lo, hi)
    bounded = lo is not None or hi is not None
    mask = pass_mask(T, lo, hi)
    dT = np.zeros((V, GD), dtype=np.float64)
    dw = np.zeros((V, heads), dtype=np.float64)
    wf = np.repeat(w, ph, axis=1)  # w[v, h(f)]
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(G):
            a, b = int(ptr[g]), int(ptr[g + 1])
            if b == a:
                continue
            through = wf[a:b] * dOut[g]
            dT[a:b] = np.where(mask[a:b], through, 0.0) if bounded else through
            dw[a:b] = np.sum((R[a:b] * dOut[g]).reshape(b - a, heads, ph), axis=2)
        if kind in ("none", "average"):
            return dT, None
        if kind == "sigmoid":
            return dT, dw
        dS = np.zeros((V, heads), dtype=np.float64)
        for g in range(G):
            a, b = int(ptr[g]), int(ptr[g + 1])
            for h in range(heads):
                t = np.sum(w[a:b, h] * dw[a:b, h])
                dS[a:b, h] = w[a:b, h] * (dw[a:b, h] - t)
    return dT, dS
