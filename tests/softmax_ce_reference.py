"""The contract of tfgnn_softmax_ce_metrics (the comment in include/tfgnn.h) restated in float64 with numpy.

Not a test module: tests/test_softmax_ce_reference_host.py pins it against torch's float64 ``cross_entropy``, and
tests/test_gpu_softmax_ce.py holds the kernel to it.  The reference project has no counterpart (PARITY UNPINNED)."""
from typing import NamedTuple, Optional

import numpy as np


class SoftmaxCE(NamedTuple):
    loss: float           # sum over counted v of w_v (logsumexp(x_v) - x_v[y_v]) / W; 0.0 when W == 0
    accuracy: float       # correct / counted; nan when nothing is counted
    correct: int
    counted_nodes: int
    W: float              # sum of the counted nodes' weights
    pred: np.ndarray      # int64 [V]: lowest index of the row maximum, a NaN entry taking part as -inf
    dlogits: np.ndarray   # float64 [V, C]: (w_v / W) (softmax(x_v) - onehot(y_v)) for counted v, exactly 0 elsewhere
    counted: np.ndarray   # bool [V]


def counted_nodes(labels, weights, C: int) -> np.ndarray:
    """node v is counted iff w_v > 0 and its label is an integer in [0, C); NaN fails every comparison"""
    y = np.asarray(labels, dtype=np.float64).reshape(-1)
    w = np.ones_like(y) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (w > 0) & (y >= 0) & (y < C) & (y == np.floor(y))


def softmax_ce(logits, labels, weights: Optional[np.ndarray] = None) -> SoftmaxCE:
    x = np.asarray(logits, dtype=np.float64)
    V, C = x.shape
    y = np.asarray(labels, dtype=np.float64).reshape(-1)
    w = np.ones(V) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    assert y.shape == (V,) and w.shape == (V,)
    counted = counted_nodes(y, w, C)
    pred = np.argmax(np.where(np.isnan(x), -np.inf, x), axis=1)  # np.argmax: the first of equal maxima
    dlogits = np.zeros((V, C))
    rows = np.flatnonzero(counted)
    if rows.size == 0:
        return SoftmaxCE(0.0, float("nan"), 0, 0, 0.0, pred, dlogits, counted)
    xc, yc, wc = x[rows], y[rows].astype(np.int64), w[rows]
    W = float(np.sum(wc))
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.max(np.where(np.isnan(xc), -np.inf, xc), axis=1, keepdims=True)
        e = np.exp(xc - m)
        s = e.sum(axis=1, keepdims=True)
        row_loss = (m[:, 0] - xc[np.arange(rows.size), yc]) + np.log(s[:, 0])
        loss = float(np.sum(wc * row_loss) / W)
        g = e / s
        g[np.arange(rows.size), yc] -= 1.0
        dlogits[rows] = g * (wc / W)[:, None]
    correct = int(np.sum(pred[rows] == yc))
    return SoftmaxCE(loss, correct / rows.size, correct, int(rows.size), W, pred, dlogits, counted)
