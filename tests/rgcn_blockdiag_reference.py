"""Float64 references of the R-GCN block-diagonal decomposition (include/tfgnn.h "R-GCN block-diagonal decomposition"), at two
levels that share no formulation.

OP LEVEL (numpy): plain loops over the edges, one edge's terms at a time, for what tfgnn_blockdiag_forward / _backward define, on
the banded blocks Qb [L, di, H] (di = D / C, ho = H / C, c(h) = h // ho, c(d) = d // di):
    pre[v, h]    = m_v * sum over the edges e = (u -> v) of type l of  s[v, l] * sum_i X[u, c(h)*di + i] * Qb[l, i, h]
    dX[u, d]     = sum over the edges e = (u -> v) of type l of  s'[v, l] * sum_j dPre[v, c(d)*ho + j] * Qb[l, d % di, c(d)*ho + j]
    dQb[l, i, h] = sum over the edges e = (u -> v) of type l of  m_v * s[v, l] * X[u, c(h)*di + i] * dPre[v, h]
with the scales of tfgnn_graph_scales as INPUTS (fp32 values: s and s' depend on the edge through (target, type) only, so they
are [V, L] tables here; None = 1).  Every value comes with a bound DERIVED from the sum order the header states.  With
U = 2^-24 the unit roundoff of float32: a sum of products of fp32 factors in which no term passes through more than k roundings
is within  gamma_k sum |terms|,  gamma_k = k U / (1 - k U).  A fused multiply-add rounds once; adding an empty partial sum (an
exact 0) is exact, so every count below is an upper limit.
  pre   a term (one edge, one i) of a row with n in-edges of T distinct types passes
          * the run sum of its segment, r = fma(s_e, x, r): at most the segment's length - 32 for a short row, and
            ceil(512 / G) <= 128 (G >= 4 lane groups per item) for an item's segment - so min(n, 128) roundings;
          * the block apply of its segment, acc = fma(r, Qb, acc), one chain over every run of the segment (a type has at most
            one run per segment) and the di rows of the block: at most T * di;
          * for a long row (n > 32) the joins: at most G - 1 <= 15 segment sums and ceil(n / 512) - 1 item sums;
          * the multiplication by m_v: 1.
        k = min(n, 128) + T * di + [n > 32] (15 + ceil(n / 512) - 1) + 1.
  dX    the same walk by source with the roles swapped (n, T: the out-edges of u; the block apply runs over ho columns) and no
        final multiplication:  k = min(n, 128) + T * ho + [n > 32] (15 + ceil(n / 512) - 1).
  dQb   a term (one edge of type l, E_l of them) passes the two roundings of t = (m_v * s_e) * dPre, its wave's chain
        p = fma(x, t, p) over at most ceil(256 / 4) = 64 edges of a chunk, the 3 wave sums, and the ceil(E_l / 256) chunk sums
        of stage 2:  k = 2 + min(E_l, 64) + 3 + ceil(E_l / 256).
A bound of 0 (no term, or only zero terms) demands an exact 0.

LAYER LEVEL (torch): the layer is RGCN with dense kernels W_l composed from the blocks.  ``layer_reference`` composes them,
calls oracle.tf2gnn_oracle.message_passing_call("rgcn", ...) - one message per edge, the reference's own order - in float64
under torch autograd with the W_l as leaves, and maps their gradients back by  dQb[l, i, c*ho + j] = dW_l[c*di + i, c*ho + j].
It never sums a run or applies a block, so it is independent of the formulation the kernels (and the op-level loops) use."""
import numpy as np
import torch

from oracle import tf2gnn_oracle as orc
from tests.rgcn_basis_reference import rgcn_params, scales_tables  # noqa: F401  (the same scales, the same layer parameters)

U = 2.0 ** -24
CHUNK = 256  # csrc/blockdiag.hip DQ_CHUNK


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _table(t, V, L):
    return np.ones((V, L)) if t is None else _f64(t).reshape(V, L)


def _gamma(k):
    k = _f64(k)
    return k * U / (1.0 - k * U)


def _walk_depth(n, T, block):
    """k of the two walks for rows of n edges of T distinct types (arrays), without the final multiplication"""
    joins = np.where(n > 32, 15 + np.ceil(n / 512.0) - 1, 0.0)
    return np.minimum(n, 128) + T * block + joins


def forward(adjs, V, Qb, X, C, s=None, m=None):
    """-> (pre [V, H] float64, bound [V, H]).  adjs: per type an int array [E_l, 2] of (source, target)."""
    Qb, X = _f64(Qb), _f64(X)
    L, di, H = Qb.shape
    ho = H // C
    s = _table(s, V, L)
    m = np.ones(V) if m is None else _f64(m).reshape(V)
    pre, A = np.zeros((V, H)), np.zeros((V, H))
    n, types = np.zeros(V), [set() for _ in range(V)]
    cols = (np.arange(H) // ho)[None, :] * di + np.arange(di)[:, None]  # [di, H]: the X column of term (i, h)
    for l, adj in enumerate(adjs):
        for u, v in np.asarray(adj, dtype=np.int64).reshape(-1, 2):
            terms = m[v] * s[v, l] * X[u][cols] * Qb[l]  # [di, H]
            pre[v] += terms.sum(axis=0)
            A[v] += np.abs(terms).sum(axis=0)
            n[v] += 1
            types[v].add(l)
    T = np.array([len(t) for t in types], dtype=np.float64)
    return pre, _gamma(_walk_depth(n, T, di) + 1)[:, None] * A


def backward_dx(adjs, V, Qb, dPre, C, s_src=None):
    """-> (dX [V, D], bound).  s_src [V, L] indexed by (TARGET, type): the by-source edge weight, which carries m_target."""
    Qb, dPre = _f64(Qb), _f64(dPre)
    L, di, H = Qb.shape
    ho, D = H // C, C * di
    s = _table(s_src, V, L)
    dX, A = np.zeros((V, D)), np.zeros((V, D))
    n, types = np.zeros(V), [set() for _ in range(V)]
    cols = (np.arange(D) // di)[None, :] * ho + np.arange(ho)[:, None]  # [ho, D]: the dPre / Qb column of term (j, d)
    rows = np.broadcast_to((np.arange(D) % di)[None, :], (ho, D))      # the Qb row of term (j, d)
    for l, adj in enumerate(adjs):
        Qt = Qb[l][rows, cols]  # [ho, D]
        for u, v in np.asarray(adj, dtype=np.int64).reshape(-1, 2):
            terms = s[v, l] * dPre[v][cols] * Qt
            dX[u] += terms.sum(axis=0)
            A[u] += np.abs(terms).sum(axis=0)
            n[u] += 1
            types[u].add(l)
    T = np.array([len(t) for t in types], dtype=np.float64)
    return dX, _gamma(_walk_depth(n, T, ho))[:, None] * A


def backward_dq(adjs, V, C, D, H, X, dPre, s=None, m=None):
    """-> (dQb [L, di, H], bound)."""
    X, dPre = _f64(X), _f64(dPre)
    L, di, ho = len(adjs), D // C, H // C
    s = _table(s, V, L)
    m = np.ones(V) if m is None else _f64(m).reshape(V)
    dq, A = np.zeros((L, di, H)), np.zeros((L, di, H))
    k = np.zeros(L)
    cols = (np.arange(H) // ho)[None, :] * di + np.arange(di)[:, None]  # [di, H]: the X column of term (i, h)
    for l, adj in enumerate(adjs):
        adj = np.asarray(adj, dtype=np.int64).reshape(-1, 2)
        for u, v in adj:
            terms = m[v] * s[v, l] * X[u][cols] * dPre[v][None, :]  # [di, H]
            dq[l] += terms
            A[l] += np.abs(terms)
        E_l = adj.shape[0]
        k[l] = 2 + min(E_l, 64) + 3 + -(-E_l // CHUNK)
    return dq, _gamma(k)[:, None, None] * A


# ---- layer level ------------------------------------------------------------------------------------------------------------
def compose_kernels(Qb, C):
    """W_l[c*di + i, c*ho + j] = Qb[l, i, c*ho + j], zero elsewhere -> tensor [L, D, H].  Qb [L, di, H] (torch, any float dtype)."""
    L, di, H = Qb.shape
    ho = H // C
    W = Qb.new_zeros((L, C * di, H))
    for l in range(L):
        for c in range(C):
            for i in range(di):
                for j in range(ho):
                    W[l, c * di + i, c * ho + j] = Qb[l, i, c * ho + j]
    return W


def band_gradient(dW, C):
    """dQb[l, i, c*ho + j] = dW_l[c*di + i, c*ho + j]; dW [L, D, H] -> [L, di, H]"""
    L, D, H = dW.shape
    di, ho = D // C, H // C
    dQ = dW.new_zeros((L, di, H))
    for c in range(C):
        dQ[:, :, c * ho:(c + 1) * ho] = dW[:, c * di:(c + 1) * di, c * ho:(c + 1) * ho]
    return dQ


def layer_reference(params, Qb, C, X, adjs, dOut=None, dtype=torch.float64):
    """out = RGCN(W_l = blockdiag of Qb[l])(X) through the per-edge oracle in ``dtype``; with dOut also the gradients
    -> (out, dX, dQb [L, di, H]) (the last two None without dOut)."""
    Qb = torch.as_tensor(Qb).detach().to(dtype)
    X = torch.as_tensor(X).detach().to(dtype).clone().requires_grad_(dOut is not None)
    adj_t = [torch.as_tensor(np.ascontiguousarray(a)) for a in adjs]
    W = [w.detach().clone().requires_grad_(dOut is not None) for w in compose_kernels(Qb, C)]
    out = orc.message_passing_call("rgcn", params, {"edge_mlps": [[w] for w in W], "aggr_mlp": None}, X, adj_t)
    if dOut is None:
        return out.detach(), None, None
    grads = torch.autograd.grad((out * torch.as_tensor(dOut).to(dtype)).sum(), [X] + W, allow_unused=True)
    dW = torch.stack([g if g is not None else torch.zeros_like(w) for g, w in zip(grads[1:], W)])
    return out.detach(), grads[0], band_gradient(dW, C)
