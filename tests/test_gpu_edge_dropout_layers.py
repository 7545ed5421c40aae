"""Edge dropout in RGCN_Basis and RGCN_BlockDiag on the device.

Parity.  The op-level fp64 loops of tests/rgcn_basis_reference.py and tests/rgcn_blockdiag_reference.py take ONE weight per
(target, type) bucket (their [V, L] tables), so they cannot be handed a per-edge array with zeros at the dropped edges.  The
parity check is therefore the filtered-graph comparison: the scales a dropped training call kept in ``ctx["scales"]`` are read
back - one value per bucket over the kept edges, equal to the float64 tables of the kept-edge graph to float32 rounding - and
handed as tables to those loops over the KEPT edges, which give the values; the modules' derived bounds come from the same loops
over ALL edges, because the device walks the full rows.  The rate-0 layer with the same weights on the graph made of the kept
edges is held to the same values.  Without the degree normalisation under "sum" no count divides and the dropped step's
messages carry 1 / (1 - p_l): its table holds that factor, the rate-0 layer's none.  On top, both runs go through product and
activation against the per-edge fp64 oracle with the bound of the two layer test modules (_module_bounds); where the
un-normalised sum meets the 2100-edge hub the dropped run's gradients also get what that forward bound allows them.

Then: inference and rate 0 are the layer as it was (bits and launches), the seeds of a stack, a captured LinkPredictionTask
step that redraws per replay, and the torch.autograd route."""
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from tests import dropout_reference as dr
from tests import edge_dropout_reference as eref
from tests import rgcn_basis_reference as bref
from tests import rgcn_blockdiag_reference as dref
from tests.helpers import KernelsUsed, assert_close, scaled_error

pytestmark = pytest.mark.gpu

STRADDLE = (31, 32, 33, 511, 512, 513)
SEED = 0xED6E5EED


def _edges(V, L, hub, rng):
    """per type an int32 [E_l, 2] array of (source, target)"""
    per_type = [[] for _ in range(L)]
    empty = L - 2 if L >= 3 else None
    types = [l for l in range(L) if l != empty]

    def add(src, tgt):
        t = rng.choice(types, size=len(src))
        for l in types:
            sel = t == l
            if sel.any():
                per_type[l].append(np.stack([src[sel], tgt[sel]], axis=1))

    fixed_in, fixed_out = (set(range(10, 16)), set(range(16, 22))) if hub else (set(), set())
    srcs = np.array([v for v in range(V) if v != 9 and v not in fixed_out])
    tgts = np.array([v for v in range(V) if v != 7 and v not in fixed_in])
    n = 3 * V if V > 50 else 600
    s, t = rng.choice(srcs, n), rng.choice(tgts, n)
    add(s, t)
    add(s[:20], t[:20])                               # duplicated edges
    loops = np.array([0, 1, 4, 5]); add(loops, loops)  # self loops
    if hub:
        add(rng.choice(srcs, 2100), np.full(2100, 2))
        add(np.full(2050, 3), rng.choice(tgts, 2050))
        for node, deg in zip(range(10, 16), STRADDLE):
            add(rng.choice(srcs, deg), np.full(deg, node))
        for node, deg in zip(range(16, 22), STRADDLE):
            add(np.full(deg, node), rng.choice(tgts, deg))
    else:
        add(rng.choice(srcs, 700), np.full(700, 2))
        add(np.full(40, 3), rng.choice(tgts, 40))
    return [np.concatenate(p).astype(np.int32) if p else np.zeros((0, 2), np.int32) for p in per_type]


@functools.lru_cache(maxsize=None)
def _graph_case(V, L):
    """V = 50 with hubs (node 2: >= 2000 in-edges, nodes 10 .. 15: in-degrees 31 .. 513) or V = 3001; type L - 2 has no edges,
    node 7 no in-edges"""
    hub = V == 50
    adjs = _edges(V, L, hub, np.random.default_rng(104729 * V + 131 * L + int(hub)))
    indeg = np.zeros(V, dtype=np.int64)
    for a in adjs:
        np.add.at(indeg, a[:, 1], 1)
    assert indeg[7] == 0 and adjs[L - 2].shape[0] == 0 and (not hub or (indeg[2] >= 2000 and tuple(indeg[10:16]) == STRADDLE))
    return adjs


def _rates(L):
    return [0.2] + [0.4] * (L - 1)


def _build(kind, L, D, H, knob, **over):
    import tf2_gnn_amd.layers.message_passing as mp

    cls = mp.RGCN_Basis if kind == "basis" else mp.RGCN_BlockDiag
    p = cls.get_default_hyperparameters()
    p.update({"hidden_dim": H, "num_bases" if kind == "basis" else "num_blocks": knob, "message_activation_function": "tanh"}, **over)
    mp.set_seed(zlib.crc32(repr((kind, L, D, H, knob)).encode()) & 0x7FFFFFFF)  # the same weights whatever the rate
    layer = cls(p)
    layer.build(mp.MessagePassingInput((None, D), tuple((None, 2) for _ in range(L))))
    return layer, p


def _dev_lists(adjs, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in adjs)


def _ctx_scales_by_edge_id(layer):
    """the scales the last call kept in ctx, in edge-id order -> (by_dst, by_src, node_scale) as numpy; a member that cached
    graph_scales leave None (= 1) comes back as None (the edge arrays) or ones (the node scale)"""
    from tf2_gnn_amd import ops

    ctx = layer._ctx
    g, sc = ctx["graph"], ctx["scales"]
    out = []
    for ew, ids in ((sc.edge_weight_by_dst, ops.G_EID_BY_DST), (sc.edge_weight_by_src, ops.G_EID_BY_SRC)):
        if ew is None:
            out.append(None)
            continue
        eid = g.array(ids).cpu().numpy().astype(np.int64)
        a = np.full(eid.shape[0], np.nan, dtype=np.float32)
        a[eid] = ew.cpu().numpy()
        out.append(a)
    m = np.ones(g.num_nodes, dtype=np.float32) if sc.node_scale is None else sc.node_scale.cpu().numpy()
    return out[0], out[1], m


def _keep_of(layer):
    by_dst, by_src, _ = _ctx_scales_by_edge_id(layer)
    assert np.array_equal(by_dst != 0, by_src != 0)
    return by_dst != 0


def _filtered(adjs, keep):
    out, first = [], 0
    for a in adjs:
        out.append(a[keep[first:first + a.shape[0]]])
        first += a.shape[0]
    return out


def _grads(kind, layer, D, H):
    if kind == "basis":
        B = layer._num_bases
        return [torch.stack([v.grad for v in layer._basis_kernels]).reshape(B * D, H), layer._coefficients.grad]
    return [layer._block_kernels.grad.reshape(-1, H)]


def _reference(kind, p, layer, knob, D, H, X, adjs, dOut, factor, dtype):
    """the per-edge oracle on `adjs` with the layer's weights, the kernels of type l scaled by factor[l]
    -> [out, dX, weight gradients in _grads' shapes] with the chain rule back through the factor"""
    f = torch.as_tensor(np.asarray(factor, dtype=np.float64))
    if kind == "basis":
        po = bref.rgcn_params(p["hidden_dim"], p["aggregation_function"], p["message_activation_function"], p["normalize_by_num_incoming"])
        coeff = layer._coeff.detach().cpu().double() * f[:, None]
        bases = layer._bases.detach().cpu().clone().view(knob, D, H)
        out, dX, dbases, dcoeff = bref.layer_reference(po, coeff, bases, X, adjs, dOut, dtype=dtype)
        return [out, dX, dbases.reshape(knob * D, H), dcoeff * f[:, None].to(dcoeff.dtype)]
    po = dref.rgcn_params(p["hidden_dim"], p["aggregation_function"], p["message_activation_function"], p["normalize_by_num_incoming"])
    Qb = layer._qb.detach().cpu().double() * f[:, None, None]
    out, dX, dQ = dref.layer_reference(po, Qb, knob, X, adjs, dOut, dtype=dtype)
    return [out, dX, (dQ * f[:, None, None].to(dQ.dtype)).reshape(-1, H)]


def _module_bounds(kind, norm, r64, r32):
    """The bound of the two layer test modules per output -> [(name, scale, tol)]: 1e-5 relative to max(1, the largest entry) -
    of the row for an un-normalised forward result -, or, where the reference's own operation order evaluated in fp32 is
    already further from fp64 than that, twice its error (un-normalised sums: four times), as tests/test_gpu_rgcn_basis_layer.py
    states it; the reference's own fp32 error bounds the block-diagonal layer's outputs for the same reason."""
    names = ["fwd", "dX"] + (["dbases", "dcoeff"] if kind == "basis" else ["dQb"])
    res = []
    for name, b64, b32 in zip(names, r64, r32):
        per_row = name == "fwd" and not norm
        scale = b64.abs().amax(dim=1, keepdim=True).clamp(min=1.0) if per_row else max(1.0, float(b64.abs().max()))
        res.append((name, scale, max(1e-5, (2 if norm else 4) * scaled_error(b32.double() / scale, b64 / scale))))
    return res


def _hold(kind, what, norm, got, r64, r32):
    for (name, scale, tol), a, b64 in zip(_module_bounds(kind, norm, r64, r32), got, r64):
        err = scaled_error(a.cpu().double() / scale, b64 / scale)
        print(f"edge dropout {kind} {what} {name}: scaled error {err:.3e}, bound {tol:.3e}")
        assert_close(a.cpu().double() / scale, b64 / scale, tol=tol, what=f"edge dropout {kind} {what} {name}")


def _ratio(err, bound):
    """the largest error / bound; an error where the bound is 0 must be 0"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.all(err[bound == 0] == 0), "an error where the bound is exactly 0"
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def _op_results(kind, layer, knob, X, dOut, dZ):
    """the layer's gather / walk calls on the scales its last training call kept in ctx -> {name: numpy}"""
    from tf2_gnn_amd import ops

    ctx = layer._ctx
    g, sc = ctx["graph"], ctx["scales"]
    kw = dict(edge_weight_by_dst=sc.edge_weight_by_dst, edge_weight_by_src=sc.edge_weight_by_src, node_scale=sc.node_scale)
    if kind == "basis":
        dX, dc = ops.basis_gather_backward(g, layer._coeff, dZ, X, **kw)
        return {"Z": ctx["Z"].cpu().numpy(), "dX": dX.cpu().numpy(), "dcoeff": dc.cpu().numpy()}
    pre = ops.blockdiag_forward(g, layer._qb, X, knob, edge_weight=sc.edge_weight_by_dst, node_scale=sc.node_scale)
    dX, dQ = ops.blockdiag_backward(g, layer._qb, dOut, X, knob, **kw)
    return {"pre": pre.cpu().numpy(), "dX": dX.cpu().numpy(), "dQb": dQ.cpu().numpy()}


def _op_reference(kind, layer, knob, adjs, V, X, dOut, dZ, s, m, s_src):
    """the op-level fp64 loops of the two reference modules on `adjs` with [V, L] scale tables -> {name: (value, bound)}"""
    X, dOut, dZ = X.cpu().numpy(), dOut.cpu().numpy(), dZ.cpu().numpy()
    if kind == "basis":
        coeff = layer._coeff.detach().cpu().numpy()
        return {"Z": bref.gather_forward(adjs, V, coeff, X, s, m), "dX": bref.gather_backward_dx(adjs, V, coeff, dZ, s_src),
                "dcoeff": bref.gather_backward_dcoeff(adjs, V, coeff.shape, X, dZ, s, m)}
    Qb = layer._qb.detach().cpu().numpy()
    D, H = X.shape[1], Qb.shape[2]
    return {"pre": dref.forward(adjs, V, Qb, X, knob, s, m), "dX": dref.backward_dx(adjs, V, Qb, dOut, knob, s_src),
            "dQb": dref.backward_dq(adjs, V, knob, D, H, X, dOut, s, m)}


def _hold_ops(what, got, values, bounds):
    for name in got:
        ratio = _ratio(np.abs(got[name].astype(np.float64) - values[name][0]), bounds[name][1])
        print(f"edge dropout {what} {name}: max error / bound {ratio:.3f}")
        assert ratio <= 1.0, (what, name, ratio)


def _gradient_allowances(kind, layer, knob, kept, V, X, dOut, s, m, s_src, out, e_out):
    """What an error of at most e_out [V, H] in the layer's (tanh) output may do to its gradients, to first order and with no
    cancellation assumed: d_pre = dOut (1 - out^2) moves by at most e_d = |dOut| (2 |out| e_out + e_out^2), every gradient is
    linear in d_pre, and the image of e_d under that map with absolute coefficients comes from the reference modules' op-level
    loops over the kept edges on absolute inputs (|Z|^T e_d and e_d |W|^T for the basis layer's two products).
    -> one array per gradient, in the order of the layer's outputs after out."""
    X, dOut = np.abs(X.cpu().numpy().astype(np.float64)), np.abs(dOut.cpu().numpy().astype(np.float64))
    e_d = dOut * (2.0 * np.abs(out) * e_out + e_out * e_out)
    if kind == "blockdiag":
        aQ = np.abs(layer._qb.detach().cpu().numpy().astype(np.float64))
        D, H = X.shape[1], aQ.shape[2]
        return [dref.backward_dx(kept, V, aQ, e_d, knob, s_src)[0], dref.backward_dq(kept, V, knob, D, H, X, e_d, s, m)[0].reshape(-1, H)]
    ac = np.abs(layer._coeff.detach().cpu().numpy().astype(np.float64))
    aW = np.abs(layer._bases.detach().cpu().numpy().astype(np.float64))  # [B*D, H]
    aZ = bref.gather_forward(kept, V, ac, X, s, m)[0]  # >= |Z|
    e_dZ = e_d @ aW.T
    return [bref.gather_backward_dx(kept, V, ac, e_dZ, s_src)[0], aZ.T @ e_d, bref.gather_backward_dcoeff(kept, V, ac.shape, X, e_dZ, s, m)[0]]


def _hold_with_allowances(kind, what, norm, got, r64, r32, allowances_of):
    """_hold, with every gradient's bound widened by what the forward bound itself allows (allowances_of(out64, e_out))"""
    rows = _module_bounds(kind, norm, r64, r32)
    _, scale, tol = rows[0]
    out64 = r64[0].numpy()
    e_out = tol * np.broadcast_to(np.asarray(scale, dtype=np.float64), out64.shape)
    extra = [0.0] + allowances_of(out64, e_out)
    for (name, scale, tol), a, b64, more in zip(rows, got, r64, extra):
        value = b64.numpy()
        bound = tol * np.broadcast_to(np.asarray(scale, dtype=np.float64), value.shape) * np.maximum(1.0, np.abs(value) / np.asarray(scale, dtype=np.float64)) + more
        ratio = _ratio(np.abs(a.cpu().numpy().astype(np.float64).reshape(value.shape) - value), bound)
        print(f"edge dropout {kind} {what} {name}: max error / bound {ratio:.3f} (module bound {tol:.3e}; largest bound / largest "
              f"entry {float(np.max(bound)) / max(1.0, float(np.abs(value).max())):.2e})")
        assert ratio <= 1.0, (kind, what, name, ratio)


_COMBOS = [(True, "sum"), (False, "sum"), (True, "mean"), (False, "sqrt_n"), (False, "mean"), (True, "sqrt_n"), (False, "sum"), (True, "sum")]
# kind, knob (num_bases / num_blocks), D = H, V, L; every (normalize, aggregation) combination met by both layers
PARITY_CASES = [("basis", 8 if W == 64 else 2, W, V, L) for W in (64, 320) for V in (50, 3001) for L in (4, 37)] + \
               [("blockdiag", C, 64, V, L) for C in (4, 16) for V in (50, 3001) for L in (4, 37)]
PARITY_CASES = [c + _COMBOS[i % 8] for i, c in enumerate(PARITY_CASES)]


@pytest.mark.parametrize("kind,knob,W,V,L,norm,agg", PARITY_CASES,
                         ids=[f"{c[0]}{c[1]}-{c[2]}-V{c[3]}-L{c[4]}-{'norm' if c[5] else 'raw'}-{c[6]}" for c in PARITY_CASES])
def test_dropped_step_is_the_layer_on_the_kept_edges(dev, kind, knob, W, V, L, norm, agg):
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers import MessagePassingInput

    D = H = W
    adjs = _graph_case(V, L)
    per = [a.shape[0] for a in adjs]
    rates = _rates(L)
    over = {"aggregation_function": agg, "normalize_by_num_incoming": norm}
    layer, p = _build(kind, L, D, H, knob, edge_dropout_rate=rates, **over)
    twin, _ = _build(kind, L, D, H, knob, **over)
    for a, b in zip(layer.trainable_variables, twin.trainable_variables):
        assert torch.equal(a.value, b.value), a.name
    gen = torch.Generator().manual_seed(11)
    X, dOut = torch.randn((V, D), generator=gen), torch.randn((V, H), generator=gen)
    what = f"{knob} {W} V{V} L{L} {agg} {'norm' if norm else 'raw'}"

    # the dropped step on the full graph
    layer.edge_dropout_seed = SEED
    epoch = ops.dropout_epoch()
    before = ops.edge_dropout_launch_counts()["edge_dropout_scales"]
    out = layer(MessagePassingInput(X.to(dev), _dev_lists(adjs, dev)), training=True)
    assert ops.edge_dropout_launch_counts()["edge_dropout_scales"] == before + 1
    by_dst, by_src, m_dev = _ctx_scales_by_edge_id(layer)
    dX = layer.backward(dOut.to(dev))
    assert layer._ctx["scales"].row_scale is None
    assert not any(isinstance(k, tuple) and k[0] == "scales" for k in layer._ctx["graph"]._cache)  # a draw is never cached
    got = [out, dX] + _grads(kind, layer, D, H)
    keep = eref.keep_edges(per, rates, SEED, epoch)
    assert np.array_equal(by_dst != 0, keep) and np.array_equal(by_src != 0, keep) and not keep.all()
    kept = _filtered(adjs, keep)

    # its scales, read back: one value per bucket over the kept edges = the reference's tables of the filtered graph
    t, tgt = eref.edge_types(adjs)[keep], eref.edge_targets(adjs)[keep]
    mode = {"sum": 0, "mean": 1, "sqrt_n": 2}[agg]
    raw_sum = not norm and mode == 0
    factor = np.array([dr.scale(r) for r in rates], dtype=np.float32) if raw_sum else np.ones(L, dtype=np.float32)
    s64, m64, ssrc64 = bref.scales_tables(kept, V, norm, agg)
    want_s = s64[tgt, t] * factor[t].astype(np.float64)
    assert np.allclose(by_dst[keep], want_s, rtol=2.0 ** -22, atol=0) and np.allclose(m_dev, m64, rtol=2.0 ** -22, atol=0)
    assert np.allclose(by_src[keep], ssrc64[tgt, t] * factor[t], rtol=2.0 ** -21, atol=0)
    table = np.zeros((V, L), dtype=np.float32)
    table[tgt, t] = by_dst[keep]
    assert np.array_equal(table[tgt, t], by_dst[keep]), "a kept weight that is not constant over its (target, type) bucket"

    # PARITY, op level: the calls the layer makes, on the scales it kept, against the reference modules' fp64 loops with their
    # own derived bounds.  Values: the loops over the kept edges.  Bounds of the dropped step: the same loops over ALL edges
    # with the same tables - the device walks the full rows (a dropped edge is a term that is exactly 0, a kept one the
    # table's value), so row lengths, run counts and joins are the full graph's, and every term is at most the full loop's.
    dZ = torch.randn((V, knob * D), generator=gen) if kind == "basis" else torch.zeros((V, 1))
    Xd, dOutd, dZd = X.to(dev), dOut.to(dev), dZ.to(dev)
    s_tab, ssrc_tab = table, np.zeros((V, L), dtype=np.float32)
    ssrc_tab[tgt, t] = by_src[keep]
    got_ops = _op_results(kind, layer, knob, Xd, dOutd, dZd)
    values = _op_reference(kind, layer, knob, kept, V, X, dOut, dZ, s_tab, m_dev, ssrc_tab)
    bounds = _op_reference(kind, layer, knob, adjs, V, X, dOut, dZ, s_tab, m_dev, ssrc_tab)
    _hold_ops("dropped " + kind + " " + what, got_ops, values, bounds)

    # the rate-0 layer on the graph of the kept edges: the same values (un-normalised sums: without the 1 / (1 - p) its messages
    # do not carry), its scales the dropped step's on the kept edges bit for bit
    out2 = twin(MessagePassingInput(Xd, _dev_lists(kept, dev)), training=True)
    dX2 = twin.backward(dOutd)
    got2 = [out2, dX2] + _grads(kind, twin, D, H)
    sc2 = twin._ctx["scales"]
    if raw_sum:
        assert sc2.edge_weight_by_dst is None and sc2.edge_weight_by_src is None and sc2.node_scale is None
        tables2 = (None, None, None)
        values2 = _op_reference(kind, twin, knob, kept, V, X, dOut, dZ, *tables2)
    else:
        d2, s2, m2 = _ctx_scales_by_edge_id(twin)
        assert (d2 is None or np.array_equal(d2.view(np.uint32), by_dst[keep].view(np.uint32)))
        assert np.array_equal(s2.view(np.uint32), by_src[keep].view(np.uint32)) and np.array_equal(m2.view(np.uint32), m_dev.view(np.uint32))
        values2 = values
    _hold_ops("kept-edge graph " + kind + " " + what, _op_results(kind, twin, knob, Xd, dOutd, dZd), values2, values2)

    # layer level, through the product and the activation: the layer's own out, dX and weight gradients of both runs against
    # the per-edge fp64 oracle on the kept edges with the layer test modules' bound (_module_bounds).  Where the un-normalised
    # sum meets the 2100-edge hub of the V = 50 graph, the dropped run's kept messages carry 1 / (1 - p), a row's entries
    # reach 160 and cancel to below 0.1 where tanh' is 1, and the oracle's own order in fp32 is 2e-5 from fp64 on the output:
    # the forward result is held to the modules' bound as everywhere, and each gradient to that bound plus what the forward
    # bound itself allows (_gradient_allowances) - the basis layer's dbases multiplies the hub row's output error by
    # |Z[hub]| = 120, more than the gradient's own largest entry, so its 1e-5 does not follow from the output's.  The walks
    # themselves are pinned by the op-level bounds above; NOTEBOOK section 40 has the measured decomposition.
    r64 = _reference(kind, p, layer, knob, D, H, X, kept, dOut, factor, torch.float64)
    r32 = _reference(kind, p, layer, knob, D, H, X, kept, dOut, factor, torch.float32)
    if raw_sum and V == 50:
        _hold_with_allowances(kind, "dropped " + what, norm, got, r64, r32, lambda out64, e_out: _gradient_allowances(
            kind, layer, knob, kept, V, X, dOut, s_tab, m_dev, ssrc_tab, out64, e_out))
    else:
        _hold(kind, "dropped " + what, norm, got, r64, r32)
    if raw_sum:  # the rate-0 layer on the kept edges sums unscaled messages
        ones = np.ones(L, dtype=np.float32)
        r64 = _reference(kind, p, twin, knob, D, H, X, kept, dOut, ones, torch.float64)
        r32 = _reference(kind, p, twin, knob, D, H, X, kept, dOut, ones, torch.float32)
    _hold(kind, "kept-edge graph " + what, norm, got2, r64, r32)
    assert not out.cpu()[7].any() and not out2.cpu()[7].any()  # the node without in-edges


@pytest.mark.parametrize("kind,knob", [("basis", 8), ("blockdiag", 4)])
def test_inference_and_rate_zero_are_the_layer_as_it_was(dev, kind, knob):
    """training=False with a non-zero rate, and training=True with rate 0: the bits, the cached scales and the launches of a layer
    built without the hyper-parameter; the new kernel does not run"""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers import MessagePassingInput
    from tf2_gnn_amd.layers.graph_scales import graph_scales

    V, L, D = 50, 4, 64
    adjs = _graph_case(V, L)
    lists = _dev_lists(adjs, dev)
    over = {"aggregation_function": "mean"}
    plain, p = _build(kind, L, D, D, knob, **over)
    assert "edge_dropout_rate" not in p  # the defaults are what they were: a params dict from before the hyper-parameter
    bare = plain
    plain, _ = _build(kind, L, D, D, knob, edge_dropout_rate=0.0, **over)
    dropping, _ = _build(kind, L, D, D, knob, edge_dropout_rate=_rates(L), **over)
    zeros, _ = _build(kind, L, D, D, knob, edge_dropout_rate=[0.0] * L, **over)
    gen = torch.Generator().manual_seed(5)
    X, dOut = torch.randn((V, D), generator=gen).to(dev), torch.randn((V, D), generator=gen).to(dev)

    def run(layer, training):
        c0 = (ops.basis_launch_counts(), ops.blockdiag_launch_counts(), ops.edge_dropout_launch_counts())
        with KernelsUsed() as used:
            out = layer(MessagePassingInput(X, lists), training=training)
            dX = layer.backward(dOut)
        c1 = (ops.basis_launch_counts(), ops.blockdiag_launch_counts(), ops.edge_dropout_launch_counts())
        launches = dict(used.delta)
        for a, b in zip(c0, c1):
            launches.update({k: b[k] - a[k] for k in b})
        res = [out, dX] + _grads(kind, layer, D, D)
        return [x.clone() for x in res], launches, layer._ctx["scales"]

    want, want_launches, want_scales = run(bare, True)
    assert want_launches["edge_dropout_scales"] == 0 and sum(want_launches.values()) > 0
    g = bare._ctx["graph"]
    assert want_scales is graph_scales(g, True, "mean")
    for name, layer, training in (("rate 0, training", plain, True), ("rates [0] * L, training", zeros, True),
                                  ("rate > 0, inference", dropping, False)):
        got, launches, scales = run(layer, training)
        assert launches == want_launches, (name, launches, want_launches)
        assert scales is want_scales, name  # the cached scales of the graph
        for a, b in zip(got, want):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    got, launches, scales = run(dropping, True)
    assert launches == dict(want_launches, edge_dropout_scales=1)  # one launch more, the walks unchanged
    assert scales is not want_scales and not torch.equal(got[0], want[0])


def _stack(dev, rate, seed, input_dropout=0.0, V=50, L=4):
    from tf2_gnn_amd.layers import GNN, GNNInput
    from tf2_gnn_amd.layers.message_passing import set_seed

    params = GNN.get_default_hyperparameters("rgcn_blockdiag")
    params.update({"hidden_dim": 64, "num_layers": 2, "num_blocks": 4, "global_exchange_every_num_layers": 10000,
                   "layer_input_dropout_rate": input_dropout, "edge_dropout_rate": rate, "message_activation_function": "tanh"})
    set_seed(17)
    gnn = GNN(params)
    gnn.dropout_seed = seed
    adjs = _graph_case(V, L)
    X = torch.randn((V, 16), generator=torch.Generator().manual_seed(2))
    inp = GNNInput(X.to(dev), _dev_lists(adjs, dev), torch.zeros(V, dtype=torch.int32, device=dev), 1)
    return gnn, inp, adjs


def test_a_stack_hands_every_layer_and_every_call_a_seed_of_its_own(dev):
    from tf2_gnn_amd import ops

    rates = _rates(4)
    gnn, inp, adjs = _stack(dev, rates, seed=5)
    per = [a.shape[0] for a in adjs]
    epoch = ops.dropout_epoch()

    def patterns(g):
        out = g(inp, training=True)
        ks = [_keep_of(m) for m in g._mp_layers]
        for m, k in zip(g._mp_layers, ks):  # each is the reference's draw for the seed the stack handed the layer
            assert np.array_equal(k, eref.keep_edges(per, rates, m.edge_dropout_seed, epoch))
        return out.clone(), ks, [m.edge_dropout_seed for m in g._mp_layers]

    out1, first, seeds1 = patterns(gnn)
    assert gnn.graph_parts(50, per) & ops.G_PART_EDGE_MAPS and gnn._ctx["graph"].parts & ops.G_PART_EDGE_MAPS
    out2, second, seeds2 = patterns(gnn)
    assert len(set(seeds1 + seeds2)) == 4
    assert not np.array_equal(first[0], first[1]) and not np.array_equal(first[0], second[0]) and not np.array_equal(first[1], second[1])
    assert not torch.equal(out1, out2)
    again, _, _ = _stack(dev, rates, seed=5)
    out3, third, seeds3 = patterns(again)
    assert seeds3 == seeds1 and all(np.array_equal(a, b) for a, b in zip(first, third))
    assert torch.equal(out1.view(torch.int32), out3.view(torch.int32))
    other, _, _ = _stack(dev, rates, seed=6)
    assert not np.array_equal(patterns(other)[1][0], first[0])
    # inference draws nothing and moves no count
    calls = gnn._edge_dropout_calls
    gnn(inp, training=False)
    assert gnn._edge_dropout_calls == calls == 4
    # the seeds of the layer-input dropout are what they are without the feature
    a, _, _ = _stack(dev, rates, seed=5, input_dropout=0.2)
    b, _, _ = _stack(dev, 0.0, seed=5, input_dropout=0.2)
    a(inp, training=True), b(inp, training=True)
    assert a._dropout_calls == b._dropout_calls == 2 and b._edge_dropout_calls == 0 and a._edge_dropout_calls == 2
    ma, mb = a.dropout_masks(), b.dropout_masks()
    assert len(ma) == len(mb) and all((x is None and y is None) or torch.equal(x, y) for x, y in zip(ma, mb))


def test_layers_without_support_refuse_the_rate_in_a_stack(dev):
    from tf2_gnn_amd.layers import GNN, GNNInput

    shapes = GNNInput((None, 16), tuple((None, 2) for _ in range(4)), (None,), ())
    for name in ("rgcn", "rgat"):
        params = GNN.get_default_hyperparameters(name)
        params.update({"hidden_dim": 66, "num_layers": 1})  # (RGAT: 3 heads)
        GNN(dict(params)).build(shapes)  # rate 0: as before
        with pytest.raises(ValueError, match="RGCN_Basis and RGCN_BlockDiag"):
            GNN(dict(params, edge_dropout_rate=0.4)).build(shapes)


def _link_dataset():
    """V = 200, two relations untied: 2 forward + 2 backward types + the self loops as type 0 = 5 edge types"""
    from tf2_gnn_amd.data import LinkPredictionDataset

    rng = np.random.default_rng(33)
    V = 200
    parity = np.arange(V) % 2
    feats = (0.1 * rng.standard_normal((V, 8))).astype(np.float32)
    feats[:, 0] += parity
    pairs = rng.permutation(V * V)[:4000]
    u, v = pairs // V, pairs % V
    rel = (parity[u] + parity[v]) % 2
    train = [np.stack([u[rel == t], v[rel == t]], axis=1)[:600] for t in range(2)]
    params = LinkPredictionDataset.get_default_hyperparameters()
    params["num_negatives_per_positive"] = 2
    ds = LinkPredictionDataset(params)
    ds.load_data_from_arrays(feats, train)
    assert ds.num_relations == 2 and ds.num_edge_types == 5
    return ds


def test_a_captured_link_prediction_step_redraws_on_every_replay(dev):
    from tf2_gnn_amd import CapturedStep, ops
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import LinkPredictionTask

    ds = _link_dataset()
    np.random.seed(3)
    (batch,) = list(ds.get_batches(DataFold.TRAIN, dev))
    feats, labels = batch
    rates = [0.2, 0.4, 0.4, 0.4, 0.4]
    set_seed(4)
    params = LinkPredictionTask.get_default_hyperparameters("rgcn_blockdiag")
    assert "gnn_edge_dropout_rate" not in params  # absent = 0.0
    params.update({"gnn_hidden_dim": 64, "gnn_num_layers": 2, "gnn_global_exchange_every_num_layers": 10000,
                   "gnn_layer_input_dropout_rate": 0.0, "gnn_edge_dropout_rate": rates, "optimizer": "Adam", "learning_rate": 0.01})
    model = LinkPredictionTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    first = model._gnn._mp_layers[0]
    assert type(first).__name__ == "RGCN_BlockDiag" and first._edge_dropout_rates.tolist() == pytest.approx(rates)
    try:
        cap = CapturedStep(lambda: model._run_step(feats, labels, training=True)["loss"])
        cap.capture()  # the eager warm-up steps built the graph with the part the dropped step needs
        g = first._ctx["graph"]
        assert g.parts & ops.G_PART_EDGE_MAPS and g.num_edge_types == 5
        per = list(g.edges_per_type)
        assert per[0] == 200  # the self loops are edge type 0: they take the first rate
        seen, epochs = [], []
        for _ in range(3):
            loss = cap.replay()
            torch.cuda.synchronize()
            epoch = ops.dropout_epoch()
            keep = _keep_of(first)
            assert np.array_equal(keep, eref.keep_edges(per, rates, first.edge_dropout_seed, epoch)), epoch
            assert math.isfinite(float(loss))
            seen.append(keep), epochs.append(epoch)
        assert epochs[1] == epochs[0] + 1 and epochs[2] == epochs[1] + 1
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
        assert abs(seen[0][:200].mean() - 0.8) < 0.12 and abs(seen[0][200:].mean() - 0.6) < 0.08
    finally:
        ops.dropout_epoch_set(0)  # every other test draws the masks of epoch 0
        torch.cuda.synchronize()


def test_torch_autograd_route_reaches_the_dropped_step(dev):
    from tf2_gnn_amd import TorchMessagePassing, ops
    from tf2_gnn_amd.layers import MessagePassingInput

    V, L, D = 50, 4, 64
    adjs = _graph_case(V, L)
    lists = _dev_lists(adjs, dev)
    layer, _ = _build("basis", L, D, D, 8, edge_dropout_rate=_rates(L))
    layer.edge_dropout_seed = SEED
    X = torch.randn((V, D), generator=torch.Generator().manual_seed(4)).to(dev).requires_grad_(True)
    tm = TorchMessagePassing(layer).train()
    before = ops.edge_dropout_launch_counts()["edge_dropout_scales"]
    out = tm(MessagePassingInput(X, lists))
    assert ops.edge_dropout_launch_counts()["edge_dropout_scales"] == before + 1
    keep = _keep_of(layer)
    assert np.array_equal(keep, eref.keep_edges([a.shape[0] for a in adjs], _rates(L), SEED, ops.dropout_epoch())) and not keep.all()
    out.square().sum().backward()
    got = [p_.grad.clone() for p_ in tm.parameters()]
    h = layer(MessagePassingInput(X.detach(), lists), training=True)  # the same seed and epoch: the same draw
    assert torch.equal(h, out.detach()) and np.array_equal(_keep_of(layer), keep)
    dX = layer.backward((2.0 * h).contiguous())
    assert torch.equal(X.grad, dX)
    for g_, v in zip(got, layer.trainable_variables):
        assert torch.equal(g_, v.grad.reshape(g_.shape)), v.name
    tm.eval()
    assert not torch.equal(tm(MessagePassingInput(X, lists)).detach(), out.detach())  # inference: every edge
