"""Evaluation metrics of the task models' ``evaluate_model`` (tf2_gnn/models/graph_regression_task.py:184-203,
tf2_gnn/models/graph_binary_classification_task.py:70-101), in numpy / float64 on the host.

The reference imports ``sklearn.metrics`` for these numbers.  scikit-learn is not a dependency of this package, so the few
metrics the reference asks for are restated here by their definitions, with scikit-learn's conventions where a definition
leaves a choice (named at each function).  This is the evaluation loop - predictions and labels are copied to the host once
per ``evaluate_model`` call - not the training path.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np


def _as_vectors(labels, predictions) -> Tuple[np.ndarray, np.ndarray]:
    y = np.asarray(labels, dtype=np.float64).reshape(-1)
    p = np.asarray(predictions, dtype=np.float64).reshape(-1)
    if y.shape != p.shape:
        raise ValueError(f"labels {y.shape} and predictions {p.shape} differ in length")
    if y.size == 0:
        raise ValueError("evaluation metrics need at least one sample")
    return y, p


def _ratio(num: float, den: float) -> float:
    """num / den; a zero denominator gives 0.0 (the value of scikit-learn's default ``zero_division="warn"``)"""
    return float(num) / float(den) if den != 0 else 0.0


# ---- binary classification ---------------------------------------------------------------------------------------------
def confusion_counts(labels, predictions) -> Tuple[int, int, int, int]:
    """(tp, fp, tn, fn) of ``np.round(predictions)`` against 0 / 1 ``labels``.  ``np.round`` rounds half to even: a
    prediction of exactly 0.5 is a 0."""
    y, p = _as_vectors(labels, predictions)
    pred = np.round(p)
    tp = int(np.sum((pred == 1) & (y == 1)))
    fp = int(np.sum((pred == 1) & (y != 1)))
    tn = int(np.sum((pred != 1) & (y != 1)))
    fn = int(np.sum((pred != 1) & (y == 1)))
    return tp, fp, tn, fn


def _average_ranks(scores: np.ndarray) -> np.ndarray:
    """1-based ranks in ascending order; tied scores share the average of the ranks they cover"""
    order = np.argsort(scores, kind="mergesort")
    s = scores[order]
    starts = np.flatnonzero(np.concatenate(([True], s[1:] != s[:-1])))  # first position of every group of equal scores
    ends = np.concatenate((starts[1:], [s.size]))
    group_rank = (starts + 1 + ends) / 2.0  # mean of starts + 1 .. ends
    ranks = np.empty(s.size, dtype=np.float64)
    ranks[order] = np.repeat(group_rank, ends - starts)
    return ranks


def roc_auc(labels, scores) -> float:
    """Area under the ROC curve as the rank statistic U / (n_pos n_neg), U = sum of the positives' average ranks -
    n_pos (n_pos + 1) / 2: the probability that a positive outscores a negative, ties counting one half (the trapezoidal
    area ``sklearn.metrics.roc_auc_score`` integrates).  ``nan`` when the labels hold a single class."""
    y, s = _as_vectors(labels, scores)
    pos = y == 1
    n_pos = int(pos.sum())
    n_neg = y.size - n_pos
    if n_pos == 0 or n_neg == 0:
        return float("nan")
    u = _average_ranks(s)[pos].sum() - n_pos * (n_pos + 1) / 2.0
    return float(u / (float(n_pos) * float(n_neg)))


def average_precision(labels, scores) -> float:
    """sum_k (R_k - R_{k-1}) P_k over the distinct score thresholds in descending order, P_k / R_k the precision / recall of
    "score >= threshold k", R_0 = 0 (``sklearn.metrics.average_precision_score``: no interpolation).  ``nan`` when the
    labels hold a single class, like ``roc_auc``: the reference computes the two under one ``try`` and reports both as nan
    when the first fails (graph_binary_classification_task.py:80-87)."""
    y, s = _as_vectors(labels, scores)
    pos = (y == 1).astype(np.float64)
    n_pos = pos.sum()
    if n_pos == 0 or n_pos == y.size:
        return float("nan")
    order = np.argsort(-s, kind="mergesort")
    s, pos = s[order], pos[order]
    last = np.flatnonzero(np.concatenate((s[1:] != s[:-1], [True])))  # last position of every group of equal scores
    tp = np.cumsum(pos)[last]
    precision = tp / (last + 1.0)
    recall = tp / n_pos
    return float(np.sum(np.diff(np.concatenate(([0.0], recall))) * precision))


def binary_classification_metrics(labels, predictions) -> Dict[str, float]:
    """What GraphBinaryClassificationTask.evaluate_model reports (graph_binary_classification_task.py:89-99) from 0 / 1
    labels and predicted probabilities: threshold metrics of ``np.round(predictions)`` with class 1 as the positive class -
    a zero denominator gives 0.0, ``balanced_acc`` averages the recall over the classes present in the labels
    (``sklearn.metrics.balanced_accuracy_score`` leaves out a class without samples) - and the two ranking metrics."""
    tp, fp, tn, fn = confusion_counts(labels, predictions)
    n = tp + fp + tn + fn
    per_class_recall = [r / float(s) for r, s in ((tn, tn + fp), (tp, tp + fn)) if s > 0]
    return {
        "acc": (tp + tn) / float(n),
        "balanced_acc": float(sum(per_class_recall) / len(per_class_recall)),
        "precision": _ratio(tp, tp + fp),
        "recall": _ratio(tp, tp + fn),
        "f1_score": _ratio(2 * tp, 2 * tp + fp + fn),
        "roc_auc": roc_auc(labels, predictions),
        "average_precision": average_precision(labels, predictions),
    }


# ---- multiclass classification -----------------------------------------------------------------------------------------
def multiclass_metrics(labels, predictions, num_classes: int, weights=None) -> Dict[str, float]:
    """What NodeClassificationTask.evaluate_model reports from one class per sample (``labels``) and predicted classes
    (``predictions``).  A sample is counted iff its weight (1 without ``weights``) is > 0 and its label is an integer in
    [0, num_classes) - the rule of tfgnn_softmax_ce_metrics (include/tfgnn.h); weights select, they do not scale.  ``acc``:
    the share of counted samples with prediction == label.  ``macro_f1``: the unweighted mean of the per-class
    F1 = 2 tp / (2 tp + fp + fn) over the classes that occur among the counted labels or predictions
    (``sklearn.metrics.f1_score(average="macro")`` without a ``labels`` argument).  Both are ``nan`` without a counted sample."""
    y, p = _as_vectors(labels, predictions)
    w = np.ones_like(y) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape != y.shape:
        raise ValueError(f"weights {w.shape} and labels {y.shape} differ in length")
    with np.errstate(invalid="ignore"):
        counted = (w > 0) & (y >= 0) & (y < num_classes) & (y == np.floor(y))
    if not counted.any():
        return {"acc": float("nan"), "macro_f1": float("nan")}
    y, p = y[counted].astype(np.int64), p[counted].astype(np.int64)
    f1 = []
    for c in np.union1d(y, p):
        tp = int(np.sum((p == c) & (y == c)))
        fp = int(np.sum((p == c) & (y != c)))
        fn = int(np.sum((p != c) & (y == c)))
        f1.append(_ratio(2 * tp, 2 * tp + fp + fn))
    return {"acc": float(np.mean(p == y)), "macro_f1": float(np.mean(f1))}


# ---- ranking ------------------------------------------------------------------------------------------------------------
def ranking_metrics(greater, equal) -> Dict[str, float]:
    """What LinkPredictionTask.evaluate_model reports from the counts of tfgnn_distmult_rank (include/tfgnn.h): per query the
    number of candidates scoring above the true triple (``greater``) and exactly as it (``equal``).  The rank of a query is
    1 + greater + equal / 2 - ties split evenly, so a model that scores everything alike ranks in the middle, not first.
    ``mrr``: the mean of 1 / rank; ``hits@k`` (k = 1, 3, 10): the share of queries with rank <= k.  ``nan`` without a query."""
    g = np.asarray(greater, dtype=np.float64).reshape(-1)
    e = np.asarray(equal, dtype=np.float64).reshape(-1)
    if g.shape != e.shape:
        raise ValueError(f"greater {g.shape} and equal {e.shape} differ in length")
    if g.size and (g.min() < 0 or e.min() < 0):
        raise ValueError("negative count")
    if g.size == 0:
        return {"mrr": float("nan"), "hits@1": float("nan"), "hits@3": float("nan"), "hits@10": float("nan")}
    rank = 1.0 + g + e / 2.0
    out = {"mrr": float(np.mean(1.0 / rank))}
    for k in (1, 3, 10):
        out[f"hits@{k}"] = float(np.mean(rank <= k))
    return out


# ---- regression --------------------------------------------------------------------------------------------------------
def _one_minus_ratio(num: float, den: float) -> float:
    """1 - num / den; for a constant target (den = 0) a perfect fit scores 1.0 and anything else 0.0, scikit-learn's
    ``force_finite`` convention"""
    if den == 0:
        return 1.0 if num == 0 else 0.0
    return float(1.0 - num / den)


def regression_metrics(labels, predictions) -> Dict[str, float]:
    """What GraphRegressionTask.evaluate_model reports (graph_regression_task.py:193-201), single output, uniform weights:
    mean absolute / squared error, the largest absolute error, explained variance 1 - Var(y - p) / Var(y) and
    R^2 = 1 - sum (y - p)^2 / sum (y - mean y)^2."""
    y, p = _as_vectors(labels, predictions)
    err = y - p
    y_dev = y - y.mean()
    return {
        "mae": float(np.mean(np.abs(err))),
        "mse": float(np.mean(err * err)),
        "max_err": float(np.max(np.abs(err))),
        "expl_var": _one_minus_ratio(float(np.mean((err - err.mean()) ** 2)), float(np.mean(y_dev * y_dev))),
        "r2_score": _one_minus_ratio(float(np.sum(err * err)), float(np.sum(y_dev * y_dev))),
    }
