"""The contracts of tfgnn_distmult_ce_metrics, tfgnn_distmult_backward and tfgnn_distmult_rank (the comment in
include/tfgnn.h) restated in float64 with numpy: the mathematical values, which do not depend on a sum order, and next to
them the error bounds an fp32 evaluation in ANY order is held to.  tests/test_distmult_reference_host.py pins this file to
torch's float64 autograd and to a dense score matrix; the GPU tests compare the kernels with it.

U = 2^-24 is the unit roundoff of float32.
  score     |s_fp32 - s| <= ds = (D + 3) U sum_d |H[u, d] R[t, d] H[v, d]|: a lane's chain of at most ceil(D / 64) fused
            multiply-adds with one rounding of H R in front, and six butterfly additions.
  loss      2e-6 max(1, |loss|) + sum_e w_e ds_e / W: the element loss is 1-Lipschitz in s.
  gradient  an element of dH or dR is a sum of n terms g_e x y: (n + 8) U sum |terms| for the products and the additions in
            any order, and sum |x y| (w_e / W) (ds_e / 4 + 4 U) for the error of g_e - the sigmoid is 1/4-Lipschitz, and 4 U
            covers expf, the division, the subtraction and the rounding of w / W."""
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def scores_and_bounds(H, R, triples):
    """-> (s [N] float64, ds [N])"""
    H, R = _f64(H), _f64(R)
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    prod = H[t[:, 0]] * R[t[:, 1]] * H[t[:, 2]]
    return prod.sum(axis=1), (H.shape[1] + 3) * U * np.abs(prod).sum(axis=1)


def counted_mask(labels, weights, N):
    y = _f64(labels).reshape(-1)
    w = np.ones(N) if weights is None else _f64(weights).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (w > 0) & ((y == 0) | (y == 1)), y, w


@dataclass
class DistMultCE:
    scores: np.ndarray       # [N]
    score_bound: np.ndarray  # [N]
    counted: np.ndarray      # [N] bool
    W: float
    loss: float
    loss_bound: float
    counts: tuple            # (tp, fp, tn, fn), prediction s > 0
    accuracy: float
    gscore: np.ndarray       # [N], exactly 0 where uncounted


def _sigmoid(s):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-s))


def distmult_ce(H, R, triples, labels, weights=None, scores=None) -> DistMultCE:
    """``scores``: evaluate loss, counts and gradient at these scores (e.g. the kernel's own) instead of the exact ones."""
    s, ds = scores_and_bounds(H, R, triples)
    if scores is not None:
        s = _f64(scores).reshape(-1)
    N = s.shape[0]
    counted, y, w = counted_mask(labels, weights, N)
    W = float(w[counted].sum())
    sc, yc, wc = s[counted], y[counted], w[counted]
    elem = np.maximum(sc, 0.0) - sc * yc + np.log1p(np.exp(-np.abs(sc)))
    loss = float((wc * elem).sum() / W) if W > 0 else 0.0
    bound = 2e-6 * max(1.0, abs(loss)) + (float((wc * ds[counted]).sum() / W) if W > 0 else 0.0)
    pred = sc > 0
    tp, fp = int((pred & (yc == 1)).sum()), int((pred & (yc == 0)).sum())
    tn, fn = int((~pred & (yc == 0)).sum()), int((~pred & (yc == 1)).sum())
    n = int(counted.sum())
    g = np.zeros(N)
    if W > 0:
        g[counted] = (wc / W) * (_sigmoid(sc) - yc)
    return DistMultCE(s, ds, counted, W, loss, bound, (tp, fp, tn, fn), (tp + tn) / n if n else float("nan"), g)


def distmult_backward(H, R, triples, gscore, g_error=None):
    """dH [V, D], dR [T, D] in float64 from ``gscore`` [N], and their bounds.  ``g_error`` [N]: a bound on the error of each
    fp32 g_e against ``gscore`` (for the kernels: (w_e / W) (ds_e / 4 + 4 U) on the counted triples); None: no such term."""
    H, R, g = _f64(H), _f64(R), _f64(gscore).reshape(-1)
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    u, r, v = t[:, 0], t[:, 1], t[:, 2]
    ge = np.zeros_like(g) if g_error is None else _f64(g_error).reshape(-1)
    dH, dR = np.zeros_like(H), np.zeros_like(R)
    absH, absR = np.zeros_like(H), np.zeros_like(R)  # sum |terms|
    dgH, dgR = np.zeros_like(H), np.zeros_like(R)    # sum |d term / d g| g_error
    nH, nR = np.zeros(H.shape[0]), np.zeros(R.shape[0])
    src_term, dst_term, rel_term = R[r] * H[v], R[r] * H[u], H[u] * H[v]
    for node, term in ((u, src_term), (v, dst_term)):
        np.add.at(dH, node, g[:, None] * term)
        np.add.at(absH, node, np.abs(g[:, None] * term))
        np.add.at(dgH, node, ge[:, None] * np.abs(term))
        np.add.at(nH, node, 1.0)
    np.add.at(dR, r, g[:, None] * rel_term)
    np.add.at(absR, r, np.abs(g[:, None] * rel_term))
    np.add.at(dgR, r, ge[:, None] * np.abs(rel_term))
    np.add.at(nR, r, 1.0)
    return dH, dR, (nH[:, None] + 8) * U * absH + dgH, (nR[:, None] + 8) * U * absR + dgR


def gscore_error(ref: DistMultCE, weights=None):
    """the bound on |g_fp32 - g| per triple that goes into ``distmult_backward``"""
    N = ref.scores.shape[0]
    w = np.ones(N) if weights is None else _f64(weights).reshape(-1)
    out = np.zeros(N)
    if ref.W > 0:
        out[ref.counted] = (w[ref.counted] / ref.W) * (ref.score_bound[ref.counted] / 4.0 + 4.0 * U)
    return out


def distmult_rank(H, R, queries, corrupt="dst", filter_offsets=None, filter_ids=None):
    """-> (greater, equal, greater_lo, greater_hi) int64 [Q]: the exact counts in float64 - every candidate but the true entity
    and the filter's ids - and, for fp32 scores within their bounds, the interval greater must lie in: the candidates with
    s' > s + d, and those with s' >= s - d, d the sum of the two scores' bounds."""
    H, R = _f64(H), _f64(R)
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    V, D = H.shape
    greater, equal, lo, hi = (np.zeros(len(q), dtype=np.int64) for _ in range(4))
    for i, (u, t, v) in enumerate(q):
        fixed = H[u] * R[t] if corrupt == "dst" else R[t] * H[v]
        truth = v if corrupt == "dst" else u
        prod = fixed[None, :] * H  # [V, D]
        s, ds = prod.sum(axis=1), (D + 3) * U * np.abs(prod).sum(axis=1)
        keep = np.ones(V, dtype=bool)
        keep[truth] = False
        if filter_offsets is not None:
            keep[np.asarray(filter_ids, dtype=np.int64)[int(filter_offsets[i]):int(filter_offsets[i + 1])]] = False
        d = ds + ds[truth]
        with np.errstate(invalid="ignore"):
            greater[i] = int((s[keep] > s[truth]).sum())
            equal[i] = int((s[keep] == s[truth]).sum())
            lo[i] = int((s[keep] > s[truth] + d[keep]).sum())
            hi[i] = int((s[keep] >= s[truth] - d[keep]).sum())
    return greater, equal, lo, hi


def triple_tables_by_loop(triples, V, T):
    """build_triple_tables by a brute-force loop"""
    t = [tuple(int(x) for x in row) for row in np.asarray(triples).reshape(-1, 3)]
    node_lists = [[] for _ in range(V)]
    rel_lists = [[] for _ in range(T)]
    for e, (u, r, v) in enumerate(t):
        node_lists[u].append(2 * e)
        node_lists[v].append(2 * e + 1)
        rel_lists[r].append(e)
    out = {}
    for name, lists in (("node", node_lists), ("rel", rel_lists)):
        offsets, flat = [0], []
        for entries in lists:
            flat.extend(sorted(entries))
            offsets.append(len(flat))
        out[name + "_offsets"] = np.array(offsets, dtype=np.int32)
        out["node_entries" if name == "node" else "rel_order"] = np.array(flat, dtype=np.int32)
    return out
