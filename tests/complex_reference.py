"""The contracts of tfgnn_complex_ce_metrics, tfgnn_complex_backward and tfgnn_complex_rank (the comment in
include/tfgnn.h) restated in float64 with numpy, in the shape of tests/distmult_reference.py: the mathematical values, which
do not depend on a sum order, and next to them the error bounds an fp32 evaluation is held to.
tests/test_complex_reference_host.py pins this file to torch's float64 complex arithmetic and autograd, to a dense score
matrix and to tests/distmult_reference.py (R_im = 0); the GPU tests compare the kernels with it.

A row x of H or R is the complex vector x_re = x[:m], x_im = x[m:], m = D / 2 (halves).  For a triple (u, t, v), a = H[u],
r = R[t], b = H[v]:
  s = Re sum_k a r conj(b) = sum_k r_re (a_re b_re + a_im b_im) + r_im (a_re b_im - a_im b_re)
a sum of 4 m = 2 D products of three factors; P_e is the sum of their absolute values.

U = 2^-24 is the unit roundoff of float32.
  score     |s_fp32 - s| <= ds = (2 D + 3) U P_e.  Both device routines stay inside it.  The training score forms, per column,
            x = fma(a_im, b_im, a_re * b_re) and p = fma(r_re, x, p) (and the same with y, r_im): a product of three factors is
            rounded at most twice (the inner product, the inner fma) before it enters the lane sum, then passes at most
            2 ceil(m / 64) lane additions and 6 butterfly additions - fewer than the 2 D - 1 additions of any order.  The
            ranking score forms q = fma(r_re, a_re, -(r_im * a_im)) - again at most two roundings in front - and then a
            D-long fma dot product: at most ceil(D / 64) + 6 additions.  Additions with an exact 0 (idle lanes) are exact.
  loss      2e-6 max(1, |loss|) + sum_e w_e ds_e / W: the element loss is 1-Lipschitz in s.
  gradient  an element of dH or dR is a sum over n list entries of TWO terms g_e x y each (g_e x is rounded once, then one
            fma per term; chunk sums of long rows add at most n / 256 + 1 further additions): (2 n + 8) U sum |terms| for
            the products and the additions in any order, and sum (|x1 y1| + |x2 y2|) (w_e / W) (ds_e / 4 + 4 U) for the
            error of g_e - the sigmoid is 1/4-Lipschitz, and 4 U covers expf, the division, the subtraction and the
            rounding of w / W."""
from dataclasses import dataclass

import numpy as np

from tests.distmult_reference import _sigmoid, counted_mask, triple_tables_by_loop  # noqa: F401  (shared, decoder-free)

U = 2.0 ** -24


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _parts(x):
    m = x.shape[-1] // 2
    return x[..., :m], x[..., m:]


def _require_even(H, R):
    if H.shape[1] % 2 or R.shape[1] != H.shape[1]:
        raise ValueError(f"ComplEx rows are [re ; im]: the width must be even and shared, got {H.shape[1]} / {R.shape[1]}")


def score_products(a, r, b):
    """the 2 D products of three factors whose sum is the score: [..., 4, m]"""
    (ar, ai), (rr, ri), (br, bi) = _parts(a), _parts(r), _parts(b)
    return np.stack([rr * ar * br, rr * ai * bi, ri * ar * bi, -ri * ai * br], axis=-2)


def scores_and_bounds(H, R, triples):
    """-> (s [N] float64, ds [N])"""
    H, R = _f64(H), _f64(R)
    _require_even(H, R)
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    prod = score_products(H[t[:, 0]], R[t[:, 1]], H[t[:, 2]])
    return prod.sum(axis=(1, 2)), (2 * H.shape[1] + 3) * U * np.abs(prod).sum(axis=(1, 2))


@dataclass
class ComplExCE:
    scores: np.ndarray       # [N]
    score_bound: np.ndarray  # [N]
    counted: np.ndarray      # [N] bool
    W: float
    loss: float
    loss_bound: float
    counts: tuple            # (tp, fp, tn, fn), prediction s > 0
    accuracy: float
    gscore: np.ndarray       # [N], exactly 0 where uncounted


def complex_ce(H, R, triples, labels, weights=None, scores=None) -> ComplExCE:
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
    return ComplExCE(s, ds, counted, W, loss, bound, (tp, fp, tn, fn), (tp + tn) / n if n else float("nan"), g)


def gradient_terms(a, r, b):
    """d s / d a, d s / d b, d s / d r, each as its TWO terms per element: three pairs of [N, D] arrays."""
    (ar, ai), (rr, ri), (br, bi) = _parts(a), _parts(r), _parts(b)
    cat = lambda re, im: np.concatenate([re, im], axis=-1)
    src = (cat(rr * br, rr * bi), cat(ri * bi, -ri * br))   # the node is the source (role 0)
    dst = (cat(rr * ar, rr * ai), cat(-ri * ai, ri * ar))   # the node is the target (role 1)
    rel = (cat(ar * br, ar * bi), cat(ai * bi, -ai * br))
    return src, dst, rel


def complex_backward(H, R, triples, gscore, g_error=None):
    """dH [V, D], dR [T, D] in float64 from ``gscore`` [N], and their bounds.  ``g_error`` [N]: a bound on the error of each
    fp32 g_e against ``gscore`` (``gscore_error``); None: no such term."""
    H, R, g = _f64(H), _f64(R), _f64(gscore).reshape(-1)
    _require_even(H, R)
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    u, r, v = t[:, 0], t[:, 1], t[:, 2]
    ge = np.zeros_like(g) if g_error is None else _f64(g_error).reshape(-1)
    dH, dR = np.zeros_like(H), np.zeros_like(R)
    absH, absR = np.zeros_like(H), np.zeros_like(R)  # sum |terms|
    dgH, dgR = np.zeros_like(H), np.zeros_like(R)    # sum |d term / d g| g_error
    nH, nR = np.zeros(H.shape[0]), np.zeros(R.shape[0])
    src, dst, rel = gradient_terms(H[u], R[r], H[v])
    for out, a, dg, n, index, (t1, t2) in ((dH, absH, dgH, nH, u, src), (dH, absH, dgH, nH, v, dst), (dR, absR, dgR, nR, r, rel)):
        np.add.at(out, index, g[:, None] * (t1 + t2))
        np.add.at(a, index, np.abs(g[:, None] * t1) + np.abs(g[:, None] * t2))
        np.add.at(dg, index, ge[:, None] * (np.abs(t1) + np.abs(t2)))
        np.add.at(n, index, 1.0)
    return dH, dR, (2 * nH[:, None] + 8) * U * absH + dgH, (2 * nR[:, None] + 8) * U * absR + dgR


def gscore_error(ref: ComplExCE, weights=None):
    """the bound on |g_fp32 - g| per triple that goes into ``complex_backward``"""
    N = ref.scores.shape[0]
    w = np.ones(N) if weights is None else _f64(weights).reshape(-1)
    out = np.zeros(N)
    if ref.W > 0:
        out[ref.counted] = (w[ref.counted] / ref.W) * (ref.score_bound[ref.counted] / 4.0 + 4.0 * U)
    return out


def query_vector(x, r, corrupt):
    """q with s(u, t, c) = <q, H[c]> (corrupt "dst", x = H[u]) or s(c, t, v) = <q, H[c]> ("src", x = H[v])"""
    (xr, xi), (rr, ri) = _parts(x), _parts(r)
    if corrupt == "dst":
        return np.concatenate([rr * xr - ri * xi, rr * xi + ri * xr], axis=-1)
    return np.concatenate([rr * xr + ri * xi, rr * xi - ri * xr], axis=-1)


def complex_rank(H, R, queries, corrupt="dst", filter_offsets=None, filter_ids=None):
    """-> (greater, equal, greater_lo, greater_hi) int64 [Q]: the exact counts in float64 - every candidate but the true entity
    and the filter's ids - and, for fp32 scores within their bounds, the interval greater must lie in: the candidates with
    s' > s + d, and those with s' >= s - d, d the sum of the two scores' bounds."""
    H, R = _f64(H), _f64(R)
    _require_even(H, R)
    q = np.asarray(queries, dtype=np.int64).reshape(-1, 3)
    V, D = H.shape
    greater, equal, lo, hi = (np.zeros(len(q), dtype=np.int64) for _ in range(4))
    for i, (u, t, v) in enumerate(q):
        truth = v if corrupt == "dst" else u
        prod = score_products(H[u][None, :], R[t][None, :], H) if corrupt == "dst" else score_products(H, R[t][None, :], H[v][None, :])
        s, ds = prod.sum(axis=(1, 2)), (2 * D + 3) * U * np.abs(prod).sum(axis=(1, 2))
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
