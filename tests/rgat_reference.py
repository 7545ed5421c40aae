"""fp64 host references of RGAT's node-side operations (csrc/rgat.hip: tfgnn_rgat_node_scores, tfgnn_rgat_edge_dot,
tfgnn_rgat_scores_backward / _sp, tfgnn_rgat_alpha_grad).  Plain torch on the CPU, no device code.  Layouts are the library's:
    Y      [V*L, K, Hk]   row (v, l), Hk = H / K          alpha  [L, K, 2*Hk]   source half first
    scores [V*L, K]
Every function returns its result AND the magnitude sum S of the same expression (every factor replaced by its absolute value):
an fp32 evaluation of an n-term sum, in any order, with or without fused multiply-adds, is within gamma_n * S of the exact
value (gamma_n <= 1.01 n 2^-24 for n < 2^17).  tests/test_rgat_reference_host.py pins these functions to torch.autograd and to
the oracle's logits so that a mistake here is not read as a kernel bug."""
from __future__ import annotations

import torch

U32 = 2.0 ** -24  # unit roundoff of fp32


def _f64(t):
    return torch.as_tensor(t).detach().cpu().double()


def _shapes(Y, L, K):
    rows = Y.shape[0]
    assert L > 0 and K > 0 and rows % L == 0 and Y.numel() % max(1, rows * K) == 0
    return rows, Y.numel() // max(1, rows * K)


def gamma_bound(n, S):
    """the bound of an n-term fp32 sum with magnitude sum S"""
    assert n < 2 ** 17
    return 1.01 * n * U32 * S


def node_scores(Y, alpha, L, K):
    """-> (s_src, s_tgt, S_src, S_tgt), each [V*L, K]"""
    Y, alpha = _f64(Y), _f64(alpha)
    rows, Hk = _shapes(Y, L, K)
    Y = Y.reshape(rows // L, L, K, Hk)
    a = alpha.reshape(L, K, 2 * Hk)
    a_src, a_tgt = a[None, :, :, :Hk], a[None, :, :, Hk:]
    out = [(Y * a_src).sum(-1), (Y * a_tgt).sum(-1), (Y.abs() * a_src.abs()).sum(-1), (Y.abs() * a_tgt.abs()).sum(-1)]
    return tuple(t.reshape(rows, K) for t in out)


def edge_dot(coll, tgt, Y, d_agg, K):
    """coll [E] rows of Y, tgt [E] rows of d_agg [V, K, Hk] -> (da [E, K], S [E, K])"""
    Y, d_agg = _f64(Y), _f64(d_agg)
    coll, tgt = torch.as_tensor(coll).cpu().long(), torch.as_tensor(tgt).cpu().long()
    Hk = Y.numel() // (Y.shape[0] * K)
    y = Y.reshape(Y.shape[0], K, Hk)[coll]
    g = d_agg.reshape(d_agg.shape[0], K, Hk)[tgt]
    return (y * g).sum(-1), (y.abs() * g.abs()).sum(-1)


def scores_backward(ds_src, ds_tgt, alpha, dY0, L, K):
    """-> (dY [V*L, K*Hk], S) with dY = dY0 + ds_src alpha_src + ds_tgt alpha_tgt, the scores broadcast over Hk"""
    ds_src, ds_tgt, alpha, dY0 = _f64(ds_src), _f64(ds_tgt), _f64(alpha), _f64(dY0)
    rows, Hk = _shapes(dY0, L, K)
    a = alpha.reshape(L, K, 2 * Hk)
    a_src, a_tgt = a[None, :, :, :Hk], a[None, :, :, Hk:]
    s = ds_src.reshape(rows // L, L, K, 1)
    t = ds_tgt.reshape(rows // L, L, K, 1)
    d0 = dY0.reshape(rows // L, L, K, Hk)
    out = d0 + s * a_src + t * a_tgt
    mag = d0.abs() + s.abs() * a_src.abs() + t.abs() * a_tgt.abs()
    return out.reshape(rows, K * Hk), mag.reshape(rows, K * Hk)


def alpha_grad(ds_src, ds_tgt, Y, L, K):
    """-> (d_alpha [L, K, 2*Hk], S): d_alpha[l, k, :Hk] = sum_v ds_src[(v,l), k] Y[(v,l), k, :], the target half with ds_tgt"""
    ds_src, ds_tgt, Y = _f64(ds_src), _f64(ds_tgt), _f64(Y)
    rows, Hk = _shapes(Y, L, K)
    Y = Y.reshape(rows // L, L, K, Hk)
    s = ds_src.reshape(rows // L, L, K, 1)
    t = ds_tgt.reshape(rows // L, L, K, 1)
    out = torch.cat([(s * Y).sum(0), (t * Y).sum(0)], dim=-1)
    mag = torch.cat([(s.abs() * Y.abs()).sum(0), (t.abs() * Y.abs()).sum(0)], dim=-1)
    return out, mag
