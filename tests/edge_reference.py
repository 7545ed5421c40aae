"""fp64 host references of the per-edge, FiLM and graph-scale kernels (csrc/edge.hip: tfgnn_edge_pair_combine,
tfgnn_graph_original_order, tfgnn_film_edge_forward / _backward, tfgnn_film_combine_forward / _backward; csrc/graph.hip:
tfgnn_graph_scales, tfgnn_graph_target_multiplier and the per-edge arrays of the handle).  Plain torch / numpy on the CPU, no
device code.  Layouts are the library's:
    film   rows [gamma | beta] of width 2 * width          bucket row r = v * L + l
Every float function returns its result AND the magnitude sum S of the same expression (every factor replaced by its absolute
value), the S of ``rgat_reference.gamma_bound``.  The second half of the file is the checker of the device tests (guarded
buffers, ``compare``): it is importable without a device, and tests/test_edge_reference_host.py pins both halves."""
from __future__ import annotations

import numpy as np
import torch

from oracle import adjacency_oracle as ao
from oracle import tf2gnn_oracle as orc
from tests.rgat_reference import U32, gamma_bound  # noqa: F401 - the bound of the device tests is this one

SMALL_NUMBER = np.float32(1e-7)  # gnn_edge_mlp.py:102-106, added to the in-degree in fp32


def _f64(t):
    return torch.as_tensor(t).detach().cpu().double()


def _idx(t):
    return torch.as_tensor(t).detach().cpu().long()


def activation(name, x):
    """the fp64 activation ``name`` (any name of ops.act_id; None / "none": identity) of x"""
    x = _f64(x)
    if name is None or name == "none":
        return x
    return orc.get_activation_function_by_name(name)(x)


# ---- csrc/edge.hip ------------------------------------------------------------------------------------------------------------
def pair_combine(ia, ib, P, Q, act=None):
    """out[e] = act(P[ia[e]] + Q[ib[e]]) -> (out, S, s32); s32 is the fp32 pre-activation sum, one correctly rounded add, so
    the host's bits are the device's"""
    ia, ib = _idx(ia), _idx(ib)
    P32, Q32 = torch.as_tensor(P).detach().cpu().float(), torch.as_tensor(Q).detach().cpu().float()
    s32 = P32[ia] + Q32[ib]
    P, Q = P32.double(), Q32.double()
    return activation(act, P[ia] + Q[ib]), P[ia].abs() + Q[ib].abs(), s32


def _film_edge_operands(msg, mrow, film, frow, w):
    msg, film = _f64(msg), _f64(film)
    E, width = _idx(frow).numel(), film.shape[1] // 2
    assert film.shape[1] == 2 * width and msg.shape[1] == width
    m = msg[_idx(mrow)] if mrow is not None else msg[:E]
    f = film[_idx(frow)]
    we = _f64(w).reshape(E, 1) if w is not None else torch.ones((E, 1), dtype=torch.float64)
    assert m.shape[0] == E
    return m, f[:, :width], f[:, width:], we


def film_edge_forward(msg, mrow, film, frow, w):
    """out[e] = gamma[frow[e]] * (w[e] * msg[mrow[e]]) + beta[frow[e]] -> (out, S); mrow None: identity, w None: 1"""
    m, gamma, beta, we = _film_edge_operands(msg, mrow, film, frow, w)
    return gamma * (we * m) + beta, gamma.abs() * (we.abs() * m.abs()) + beta.abs()


def film_edge_backward(d, msg, mrow, film, frow, w):
    """per edge: d_msg[e] = d[e] * gamma * w[e], d_film[e] = [d[e] * (w[e] * msg) | d[e]] -> (d_msg, d_film, S_msg, S_film)"""
    m, gamma, _, we = _film_edge_operands(msg, mrow, film, frow, w)
    d = _f64(d)
    return (d * gamma * we, torch.cat([d * (we * m), d], dim=1),
            d.abs() * gamma.abs() * we.abs(), torch.cat([d.abs() * (we.abs() * m.abs()), d.abs()], dim=1))


def _film_combine_operands(Z, film, rowptr, node_scale):
    Z = _f64(Z)
    assert Z.dim() == 3, "Z is [V, L, H]"
    V, L, H = Z.shape
    film = _f64(film).reshape(V, L, 2 * H)
    rp = _idx(rowptr)
    cnt = (rp[1:] - rp[:-1])[:V * L].double().reshape(V, L, 1)
    ns = _f64(node_scale).reshape(V, 1) if node_scale is not None else torch.ones((V, 1), dtype=torch.float64)
    return Z, film[:, :, :H], film[:, :, H:], cnt, ns


def film_combine_forward(Z, film, rowptr, node_scale, act=None):
    """pre[v] = node_scale[v] * sum_l (gamma[v,l] * Z[v,l] + cnt[v,l] * beta[v,l]), out = act(pre) -> (pre, out, S), each [V, H];
    Z [V, L, H] (L = 0: pre = 0), film [V*L, 2H], rowptr [V*L + 1], node_scale [V] or None"""
    Z, gamma, beta, cnt, ns = _film_combine_operands(Z, film, rowptr, node_scale)
    pre = ns * (gamma * Z + cnt * beta).sum(1)
    S = ns.abs() * (gamma.abs() * Z.abs() + cnt * beta.abs()).sum(1)
    return pre, activation(act, pre), S


def film_combine_backward(d_pre, Z, film, rowptr, node_scale):
    """g = d_pre[v] * node_scale[v]: dZ[v,l] = gamma[v,l] * g, dfilm[v,l] = [Z[v,l] * g | cnt[v,l] * g]
    -> (dZ [V*L, H], dfilm [V*L, 2H], S_Z, S_film)"""
    Z, gamma, _, cnt, ns = _film_combine_operands(Z, film, rowptr, node_scale)
    V, L, H = Z.shape
    d_pre = _f64(d_pre).reshape(V, H)
    g = (d_pre * ns).reshape(V, 1, H)
    ga = (d_pre.abs() * ns.abs()).reshape(V, 1, H)
    dZ, dfilm = gamma * g, torch.cat([Z * g, cnt * g], dim=2)
    S_Z, S_film = gamma.abs() * ga, torch.cat([Z.abs() * ga, cnt * ga], dim=2)
    return dZ.reshape(V * L, H), dfilm.reshape(V * L, 2 * H), S_Z.reshape(V * L, H), S_film.reshape(V * L, 2 * H)


# ---- the graph: edge orders, scales, derived arrays ---------------------------------------------------------------------------
def _concat(adjs):
    """(src, dst, type) of every edge in the order of the concatenated adjacency lists, int64"""
    L = len(adjs)
    lists = [np.asarray(a, dtype=np.int64).reshape(-1, 2) for a in adjs]
    src = np.concatenate([a[:, 0] for a in lists]) if L else np.zeros(0, np.int64)
    dst = np.concatenate([a[:, 1] for a in lists]) if L else np.zeros(0, np.int64)
    typ = np.concatenate([np.full(a.shape[0], l, dtype=np.int64) for l, a in enumerate(lists)]) if L else np.zeros(0, np.int64)
    return src, dst, typ


def invdeg(rowptr_by_dst):
    """fp32 [V*L]: 1 / (c + 1e-7) evaluated in fp32 like the reference (tests/test_gpu_graph.py), 0 for empty buckets"""
    c = np.diff(np.asarray(rowptr_by_dst).astype(np.int64)).astype(np.float32)
    with np.errstate(divide="ignore"):
        return np.where(c > 0, np.float32(1.0) / (c + SMALL_NUMBER), np.float32(0)).astype(np.float32)


def row_of_position(rowptr):
    """int64 [E]: the bucket row of every position of a CSR"""
    rp = np.asarray(rowptr).astype(np.int64)
    return np.repeat(np.arange(rp.shape[0] - 1, dtype=np.int64), np.diff(rp))


def host_buckets(adjs, V):
    """(rowptr_by_dst, rowptr_by_src, col_by_src, type_by_src) of oracle.adjacency_oracle.bucket_edges: the two sorts that the
    functions below need, to be taken once for a large graph and handed to them as ``buckets``"""
    rp_d, _, _ = ao.bucket_edges(adjs, V, by="dst")
    rp_s, col_s, typ_s = ao.bucket_edges(adjs, V, by="src")
    return rp_d, rp_s, col_s, typ_s


def per_edge_derived(adjs, V, buckets=None):
    """-> (invdeg_edge_by_src fp32 [E], invdeg_edge_by_dst fp32 [E], target_by_dst int32 [E], pattern_by_src int64 [V]):
    1 / (in-degree of the edge's (target, type) bucket + 1e-7) in both edge orders, the target of every edge in by-dst order, and
    per node the emptiness pattern of its by-SOURCE buckets, sum_l 2^l [bucket (v, l) holds an edge] (L <= 8, else None)"""
    L = len(adjs)
    rp_d, rp_s, col_s, typ_s = buckets if buckets is not None else host_buckets(adjs, V)
    inv = invdeg(rp_d)
    rows_d = row_of_position(rp_d)
    by_dst = inv[rows_d] if rows_d.size else np.zeros(0, np.float32)
    by_src = inv[col_s.astype(np.int64) * L + typ_s] if col_s.size else np.zeros(0, np.float32)
    target = (rows_d // max(L, 1)).astype(np.int32)
    pattern = None
    if L <= 8:
        nonempty = (np.diff(rp_s.astype(np.int64)) > 0).reshape(V, L) if L else np.zeros((V, 0), bool)
        pattern = (nonempty * (1 << np.arange(L, dtype=np.int64))).sum(axis=1)
    return by_src.astype(np.float32), by_dst.astype(np.float32), target, pattern


def graph_scales(adjs, V, normalize, mode, buckets=None):
    """include/tfgnn.h tfgnn_graph_scales -> (row_scale [V*L], node_scale [V], ew_by_src [E], ew_by_dst [E]) in fp64.
    mode 0 = sum, 1 = mean, 2 = sqrt_n: m_v = 1, 1 / max(N_v, 1), 1 / sqrt(max(N_v, 1)), N_v = all in-edges of v.  The
    normaliser 1 / (c + 1e-7) is the fp32 value (what the handle stores); everything after it is fp64."""
    assert mode in (0, 1, 2)
    L = len(adjs)
    buckets = buckets if buckets is not None else host_buckets(adjs, V)
    rp_d, _, col_s, _ = buckets
    c = np.diff(rp_d.astype(np.int64)).reshape(V, L) if L else np.zeros((V, 0), np.int64)
    n = np.maximum(c.sum(axis=1), 1).astype(np.float64)
    m = np.ones(V) if mode == 0 else 1.0 / n if mode == 1 else 1.0 / np.sqrt(n)
    by_src, by_dst, _, _ = per_edge_derived(adjs, V, buckets)
    inv = invdeg(rp_d).astype(np.float64).reshape(V, L) if normalize else np.ones((V, L))
    row_scale = (inv * m[:, None]).reshape(V * L)
    ew_src = (by_src.astype(np.float64) if normalize else np.ones(col_s.shape[0])) * m[col_s.astype(np.int64)]
    ew_dst = by_dst.astype(np.float64) if normalize else np.ones(col_s.shape[0])
    return row_scale, m, ew_src, ew_dst


def target_multiplier(rowptr, row_scale, L):
    """-> (k fp32 [R], ident_ptr int32 [R + 1], node_of_row int32 [R]): k = float(c) * row_scale, ONE fp32 product of the fp32
    operands (bit-equal to the device's), or float(c) with row_scale None"""
    rp = np.asarray(rowptr).astype(np.int64)
    R = rp.shape[0] - 1
    c = np.diff(rp).astype(np.float32)
    k = c if row_scale is None else (c * np.asarray(row_scale, dtype=np.float32)).astype(np.float32)
    return k, np.arange(R + 1, dtype=np.int32), (np.arange(R, dtype=np.int64) // max(L, 1)).astype(np.int32)


def original_order(adjs, V, weight_by_dst, eid_by_dst):
    """include/tfgnn.h tfgnn_graph_original_order, straight from the concatenated lists: edge g of type l is (src, tgt) ->
    src_l = src * L + l, tgt_l = tgt * L + l, tgt_node = tgt, w = weight_by_dst[position of g in by-dst order] (ones when
    weight_by_dst is None).  ``eid_by_dst`` [E] names the edge at every by-dst position."""
    L = len(adjs)
    src, dst, typ = _concat(adjs)
    E = src.shape[0]
    w = np.ones(E, dtype=np.float32)
    if weight_by_dst is not None:
        eid = np.asarray(eid_by_dst).astype(np.int64)
        assert eid.shape[0] == E and np.array_equal(np.sort(eid), np.arange(E))
        pos = np.empty(E, dtype=np.int64)
        pos[eid] = np.arange(E)
        w = np.asarray(weight_by_dst, dtype=np.float32)[pos]
    return (src * L + typ).astype(np.int32), (dst * L + typ).astype(np.int32), dst.astype(np.int32), w


def eid_orders_the_edges_by_bucket(adjs, V, eid, rowptr, by="dst"):
    """True when ``eid`` is a permutation of the edges and the edge at every position of the CSR ``rowptr`` lies in that
    position's bucket (the defining property of TFGNN_G_EID_BY_DST / _SRC; the order inside a bucket is not looked at)"""
    src, dst, typ = _concat(adjs)
    eid = np.asarray(eid).astype(np.int64)
    E = src.shape[0]
    if eid.shape[0] != E or not np.array_equal(np.sort(eid), np.arange(E)):
        return False
    node = dst if by == "dst" else src
    return bool(np.array_equal((node * len(adjs) + typ)[eid], row_of_position(rowptr)))


# ---- the checker of the device tests ------------------------------------------------------------------------------------------
SENTINEL = -12345.5
SENTINEL_INT = -12345
KINDS = ("exact", "normal")


def sentinel_of(dtype):
    return SENTINEL if dtype.is_floating_point else SENTINEL_INT


def guarded(rows, cols, device, init=None, dtype=torch.float32):
    """[rows + 1, cols] filled with the sentinel: the output rows and ONE guard row behind them"""
    buf = torch.full((rows + 1, cols), sentinel_of(dtype), dtype=dtype, device=device)
    if init is not None:
        buf[:rows] = torch.as_tensor(init).to(device=device, dtype=dtype).reshape(rows, cols)
    return buf


def guard_untouched(buf, what):
    assert bool((buf[-1] == sentinel_of(buf.dtype)).all()), f"{what}: the guard row behind the last row was written"


def untouched(buf, what):
    assert bool((buf == sentinel_of(buf.dtype)).all()), f"{what} was written"


def draw(kind, shape, gen, scale_rows=False):
    """exact: integers of {-3..3} as fp32; normal: standard normal draws, with ``scale_rows`` one row times 1e4, one times 1e-4"""
    if kind == "exact":
        return torch.randint(-3, 4, shape, generator=gen).float()
    x = torch.randn(shape, generator=gen)
    if scale_rows and shape[0] >= 1:
        x[shape[0] // 3] *= 1e4
        if shape[0] >= 2:
            x[(2 * shape[0]) // 3 if shape[0] > 2 else 1] *= 1e-4
    return x


def draw_scale(kind, n, gen):
    """edge weights / node scales: exact: of {0.5, 1, 2} (products stay multiples of 2^-3); normal: uniform in [0.25, 1.25)"""
    if kind == "exact":
        return torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (n,), generator=gen)]
    return torch.rand((n,), generator=gen) + 0.25


def compare(entry, what, kind, got, want, S, n, record=None):
    """exact: equality with the fp64 reference; normal: |got - want| <= 1.01 n 2^-24 S per element (where S = 0 the result is an
    exact 0).  No element is left out.  -> the worst error / bound (0 for exact); ``record(entry, worst)`` is called before the
    assertion so that a failing figure is logged too."""
    want = _f64(want)
    got = _f64(got).reshape(want.shape)
    assert bool(torch.isfinite(got).all()), f"{entry} {what}: non-finite output"
    if kind == "exact":
        bad = int((got != want).sum())
        assert bad == 0, f"{entry} {what}: {bad} of {want.numel()} elements differ from the exact result"
        return 0.0
    assert kind == "normal", kind
    err = (got - want).abs()
    bound = gamma_bound(n, _f64(S).reshape(want.shape))
    off_zero = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), off_zero)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{entry} {what}: max error / bound = {worst:.3e} (n = {n})")
    if record is not None:
        record(entry, worst)
    assert worst <= 1.0, f"{entry} {what}: error {worst:.3f} x the bound 1.01 n 2^-24 S at element {int(ratio.argmax())}"
    return worst


def compare_equal(entry, what, got, want):
    """bit-for-value equality of arrays of any dtype (index arrays, copies)"""
    got = torch.as_tensor(got).detach().cpu()
    want = torch.as_tensor(want).detach().cpu().reshape(got.shape).to(got.dtype)
    bad = int((got != want).sum())
    first = int((got != want).reshape(-1).nonzero()[0]) if bad else -1
    assert bad == 0, f"{entry} {what}: {bad} of {want.numel()} elements differ, the first at {first}"
