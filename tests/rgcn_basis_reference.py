"""Float64 references of the R-GCN basis decomposition (include/tfgnn.h "R-GCN basis decomposition"), at two levels that
share no formulation.

OP LEVEL (numpy): plain loops over the edges for what tfgnn_basis_gather_forward / _backward define,
    Z[v, b, :]   = m_v * sum over the edges e = (u -> v) of type l of  s[v, l] * a[l, b] * X[u, :]
    dX[u, :]     = sum over the edges e = (u -> v) of type l of  s'[v, l] * sum_b a[l, b] * dZ[v, b, :]
    dcoeff[l, b] = sum over the nodes v of  m_v * < dZ[v, b, :], sum over the edges (u -> v) of type l of s[v, l] X[u, :] >
with the scales of tfgnn_graph_scales as INPUTS (fp32 values: s and s' depend on the edge through (target, type) only, so they
are [V, L] tables here; None = 1).  Every value comes with the bound an fp32 evaluation in ANY order is held to.  With
U = 2^-24 the unit roundoff of float32: a sum of n products of fp32 factors in which no term passes through more than k
roundings is within  gamma_k sum |terms|,  gamma_k = k U / (1 - k U) <= (k + 1) U  for k U < 2^-10.
  Z       n = the in-degree of v terms per element.  A term passes the fused multiply-adds of its run (at most the run's length),
          the folds / additions that join the (sub-)runs (at most their number; adding an empty partial sum is exact) and the
          multiplication by m_v: run length + number of runs <= n + 1, so k <= n + 2 and the bound is (n + 3) U sum |terms|.
  dX      n = out-degree of u times B terms.  k <= B (the chain over b) + out-degree <= n + 1: (n + 3) U sum |terms|.
  dcoeff  n = E_l D terms (E_l edges of type l).  A term passes its run (<= E_l), the dot product over the columns including the
          butterfly (<= D; run + dot <= E_l D + 1), the multiplication by m_v, and the ordered reduce: at most E_l table rows
          added in stage 1, 3 wave sums, ceil(V / 1024) chunk sums = the ordered-reduce depth.
          (n + 3 + E_l + 3 + ceil(V / 1024)) U sum |terms|.
A bound of 0 (no term, or only zero terms) demands an exact 0.

LAYER LEVEL (torch): the layer is RGCN with composed kernels W_l = sum_b a[l, b] V_b.  ``layer_reference`` composes them, calls
oracle.tf2gnn_oracle.message_passing_call("rgcn", ...) - one message per edge, the reference's own order - in float64 under
torch autograd with the W_l as leaves, and maps their gradients back by the chain rule,
    dV_b = sum_l a[l, b] dW_l,     da[l, b] = < dW_l, V_b >.
It never forms Z, so it is independent of the aggregate-first formulation the kernels (and the op-level loops) use."""
import numpy as np
import torch

from oracle import tf2gnn_oracle as orc

U = 2.0 ** -24
REDUCE_CHUNK_NODES = 1024  # csrc/basis.hip RED_NODES


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _table(t, V, L):
    return np.ones((V, L)) if t is None else _f64(t).reshape(V, L)


def gather_forward(adjs, V, coeff, X, s=None, m=None):
    """-> (Z [V, B*D] float64, bound [V, B*D]).  adjs: per type an int array [E_l, 2] of (source, target)."""
    coeff, X = _f64(coeff), _f64(X)
    L, B = coeff.shape
    D = X.shape[1]
    s = _table(s, V, L)
    m = np.ones(V) if m is None else _f64(m).reshape(V)
    Z, A = np.zeros((V, B, D)), np.zeros((V, B, D))
    n = np.zeros(V)
    for l, adj in enumerate(adjs):
        for u, v in np.asarray(adj, dtype=np.int64).reshape(-1, 2):
            term = m[v] * s[v, l] * coeff[l][:, None] * X[u][None, :]
            Z[v] += term
            A[v] += np.abs(term)
            n[v] += 1
    return Z.reshape(V, B * D), ((n[:, None, None] + 3) * U * A).reshape(V, B * D)


def gather_backward_dx(adjs, V, coeff, dZ, s_src=None):
    """-> (dX [V, D], bound).  s_src [V, L] indexed by (TARGET, type): the by-source edge weight, which carries m_target."""
    coeff, dZ = _f64(coeff), _f64(dZ)
    L, B = coeff.shape
    D = dZ.shape[1] // B
    dZ = dZ.reshape(V, B, D)
    s = _table(s_src, V, L)
    dX, A = np.zeros((V, D)), np.zeros((V, D))
    n = np.zeros(V)
    for l, adj in enumerate(adjs):
        for u, v in np.asarray(adj, dtype=np.int64).reshape(-1, 2):
            terms = s[v, l] * coeff[l][:, None] * dZ[v]  # [B, D]
            dX[u] += terms.sum(axis=0)
            A[u] += np.abs(terms).sum(axis=0)
            n[u] += B
    return dX, (n[:, None] + 3) * U * A


def gather_backward_dcoeff(adjs, V, coeff_shape, X, dZ, s=None, m=None):
    """-> (dcoeff [L, B], bound)."""
    L, B = coeff_shape
    X, dZ = _f64(X), _f64(dZ)
    D = X.shape[1]
    dZ = dZ.reshape(V, B, D)
    s = _table(s, V, L)
    m = np.ones(V) if m is None else _f64(m).reshape(V)
    dc, A = np.zeros((L, B)), np.zeros((L, B))
    k = np.zeros(L)
    chunks = max(1, -(-V // REDUCE_CHUNK_NODES))
    for l, adj in enumerate(adjs):
        adj = np.asarray(adj, dtype=np.int64).reshape(-1, 2)
        for u, v in adj:
            terms = m[v] * s[v, l] * X[u][None, :] * dZ[v]  # [B, D]
            dc[l] += terms.sum(axis=1)
            A[l] += np.abs(terms).sum(axis=1)
        E_l = adj.shape[0]
        k[l] = E_l * D + 3 + E_l + 3 + chunks
    return dc, k[:, None] * U * A


# ---- layer level ------------------------------------------------------------------------------------------------------------
def rgcn_params(hidden_dim, aggregation_function="sum", message_activation_function="relu", normalize_by_num_incoming=True):
    return {
        "hidden_dim": int(hidden_dim), "aggregation_function": aggregation_function,
        "message_activation_function": message_activation_function, "message_activation_before_aggregation": False,
        "use_target_state_as_input": False, "normalize_by_num_incoming": bool(normalize_by_num_incoming),
        "num_edge_MLP_hidden_layers": 0,
    }


def compose_kernels(coeff, bases):
    """W_l = sum_b a[l, b] V_b -> list of L tensors [D, H].  coeff [L, B], bases [B, D, H] (torch, any float dtype)."""
    return [torch.einsum("b,bdh->dh", coeff[l], bases) for l in range(coeff.shape[0])]


def layer_reference(params, coeff, bases, X, adjs, dOut=None, dtype=torch.float64):
    """out = RGCN(W_l = sum_b a[l,b] V_b)(X) through the per-edge oracle in ``dtype``; with dOut also the gradients
    -> (out, dX, dbases [B, D, H], dcoeff [L, B]) (the last three None without dOut)."""
    coeff = torch.as_tensor(coeff).detach().to(dtype)
    bases = torch.as_tensor(bases).detach().to(dtype)
    X = torch.as_tensor(X).detach().to(dtype).clone().requires_grad_(dOut is not None)
    adj_t = [torch.as_tensor(np.ascontiguousarray(a)) for a in adjs]
    W = [w.detach().clone().requires_grad_(dOut is not None) for w in compose_kernels(coeff, bases)]
    out = orc.message_passing_call("rgcn", params, {"edge_mlps": [[w] for w in W], "aggr_mlp": None}, X, adj_t)
    if dOut is None:
        return out.detach(), None, None, None
    grads = torch.autograd.grad((out * torch.as_tensor(dOut).to(dtype)).sum(), [X] + W, allow_unused=True)
    dW = torch.stack([g if g is not None else torch.zeros_like(w) for g, w in zip(grads[1:], W)]) if W else bases.new_zeros((0,) + tuple(bases.shape[1:]))
    dbases = torch.einsum("lb,ldh->bdh", coeff, dW)      # dV_b = sum_l a[l,b] dW_l
    dcoeff = torch.einsum("ldh,bdh->lb", dW, bases)      # da[l,b] = <dW_l, V_b>
    return out.detach(), grads[0], dbases, dcoeff


def scales_tables(adjs, V, normalize, aggregation, small=1e-7):
    """The scales of tfgnn_graph_scales in float64 from their definition (include/tfgnn.h): s [V, L] (by target), m [V],
    s' = s * m [V, L] (by source, indexed by target)."""
    L = len(adjs)
    c = np.zeros((V, L))
    for l, adj in enumerate(adjs):
        np.add.at(c[:, l], np.asarray(adj, dtype=np.int64).reshape(-1, 2)[:, 1], 1.0)
    s = 1.0 / (c + small) if normalize else np.ones((V, L))
    N = np.maximum(c.sum(axis=1), 1.0)
    m = {"sum": np.ones(V), "mean": 1.0 / N, "sqrt_n": 1.0 / np.sqrt(N)}[aggregation]
    return s, m, s * m[:, None]
