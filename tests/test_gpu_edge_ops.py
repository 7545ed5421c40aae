"""The per-edge and FiLM kernels of csrc/edge.hip, entry by entry against tests/edge_reference.py (fp64 on the host):
tfgnn_edge_pair_combine, tfgnn_film_edge_forward / _backward, tfgnn_film_combine_forward / _backward and
tfgnn_graph_original_order, called with raw pointers as the layers call them.

Which branch a case runs:
  edge_pair_combine  float4 branch: widths 4, 8, 24, 256;  scalar branch (width % 4 != 0): widths 1, 3, 5, 130;  each at
                     E = 1 .. 1027 (one thread .. several blocks, ragged last block), index arrays with repeats and the
                     largest valid row;  the 16-byte alignment requirement (refused at width 8, not asked for at width 5);
                     past the 65 536-block grid: width 4 at E = 2^24 + 300, width 3 at E = 5 592 406 + 100
  film_edge_*        widths 1, 7, 24, 128 x E = 1, 65, 1027 x msg_row / edge_weight NULL or given;  past the grid at width 8,
                     E = 2^21 + 100
  film_combine_*     (V, L, H) from one thread to several blocks, bucket counts 0 .. 700 from a real graph, node_scale and pre
                     NULL or given, every activation, L = 0 and V = 0.  The grid cap of these two entries is 65 535 x 8 blocks
                     (134 M elements): no test of a few seconds reaches it, and none here tries.
  original_order     four graphs (an empty type, a 700-edge hub, one edge type), with and without weights, without EDGE_IDS,
                     without edges

Every output buffer carries one guard row of a sentinel behind its last row; it must be untouched afterwards.

Two kinds of input per case.
  exact : integers of {-3..3} as fp32, edge weights and node scales of {0.5, 1, 2}, bucket counts <= 700.  Every product and
          partial sum is an integer multiple of 2^-3 far below 2^24 (the largest, film_combine at 8 types: 8 (9 + 2100) 2), so
          fp32 arithmetic is exact in any order, fused or not: the device result EQUALS the fp64 reference.
  normal: standard normal draws, one row scaled by 1e4 and one by 1e-4.  Bound per output element 1.01 n 2^-24 S, S the fp64
          magnitude sum of the reference, n the number of fp32 roundings a term goes through: 1 (pair_combine), 3
          (film_edge_forward), 2 (d_msg, d_film, dZ, dfilm), 3 L + 1 (film_combine's pre).  Derived, not measured.  The worst
          error / bound per entry point is printed and recorded in the parity log (``max_error_over_bound``, bound 1).
The beta half of d_film is a copy: equal in both kinds.  An activation's own error is not folded into a bound: the device output
is held to the fp64 activation of the DEVICE's pre-activation (pair_combine: the fp32 sum, bit-equal on the host; film_combine:
the returned ``pre``) at the 2e-6 of test_activation_forward_backward."""
import numpy as np
import pytest
import torch

from oracle import adjacency_oracle as ao
from tests import edge_reference as ref
from tests.edge_reference import KINDS, draw, draw_scale, guard_untouched, guarded, untouched
from tests.helpers import assert_close, random_graph, record_parity, to_dev

pytestmark = pytest.mark.gpu

ACT_NAMES = ("none", "relu", "tanh", "leaky_relu", "elu", "selu", "gelu", "sigmoid")
ACT_TOL = 2e-6


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _record(entry, worst):
    record_parity(entry, max_error_over_bound=worst, bound=1.0)


def _compare(entry, what, kind, got, want, S, n):
    return ref.compare(entry, what, kind, got, want, S, n, record=_record)


def _lib_ops():
    from tf2_gnn_amd import _lib, ops

    return _lib.load(), ops


def _off4(t):
    """the same values (or the same room) 4 bytes into a larger buffer: not 16-byte aligned"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _indices(E, rows, gen):
    """int32 [E] in [0, rows) with repeats (E > 1) and the largest valid row"""
    idx = torch.randint(0, rows, (E,), generator=gen, dtype=torch.int32)
    if E >= 1:
        idx[E // 2] = rows - 1
    if E >= 3:
        idx[0] = idx[E - 1]
    return idx


def test_every_activation_is_covered():
    _, ops = _lib_ops()
    assert set(ACT_NAMES) == set(ops._ACT_BY_NAME)


# =================================================================================================================================
# tfgnn_edge_pair_combine
# =================================================================================================================================
PC_VEC = (4, 8, 24, 256)
PC_SCALAR = (1, 3, 5, 130)
PC_E = (1, 2, 63, 64, 65, 257, 1027)
PC_ROWS_P, PC_ROWS_Q = 37, 23


def _pc_inputs(E, width, kind, rows_p=PC_ROWS_P, rows_q=PC_ROWS_Q):
    g = _gen(11, E, width, kind == "exact")
    P = draw(kind, (rows_p, width), g, scale_rows=True)
    Q = draw(kind, (rows_q, width), g, scale_rows=True)
    return _indices(E, rows_p, g), _indices(E, rows_q, g), P, Q


def _call_pair_combine(dev, ia, ib, P, Q, E, width, act, off=()):
    """-> (rc, out [E + 1, width] with its guard row)"""
    lib, ops = _lib_ops()
    Pd, Qd, iad, ibd = P.to(dev), Q.to(dev), ia.to(dev), ib.to(dev)
    out = guarded(E, width, dev)
    if "P" in off:
        Pd = _off4(Pd)
    if "Q" in off:
        Qd = _off4(Qd)
    if "out" in off:
        out = _off4(out)
    rc = lib.tfgnn_edge_pair_combine(ops._ptr(iad), ops._ptr(ibd), ops._ptr(Pd), ops._ptr(Qd), E, width, ops.act_id(act), ops._ptr(out),
                                     ops._stream())
    torch.cuda.synchronize()
    return rc, out


def _check_pair_combine(dev, E, width, kind, act="none", off=()):
    ia, ib, P, Q = _pc_inputs(E, width, kind)
    rc, out = _call_pair_combine(dev, ia, ib, P, Q, E, width, act, off)
    assert rc == 0, f"tfgnn_edge_pair_combine returned {rc}"
    tag = f"width={width} E={E} {kind} {act}" + (f" {'/'.join(off)} offset" if off else "")
    want, S, s32 = ref.pair_combine(ia, ib, P, Q, act)
    if act == "none":
        _compare("tfgnn_edge_pair_combine", tag, kind, out[:E], want, S, 1)
        assert torch.equal(out[:E].cpu(), s32), f"{tag}: not the correctly rounded fp32 sum"
    else:
        assert_close(out[:E].cpu(), ref.activation(act, s32), tol=ACT_TOL, what=f"tfgnn_edge_pair_combine {act} of the fp32 sum")
        if act == "relu":  # relu rounds nothing
            assert torch.equal(out[:E].cpu(), torch.relu(s32)), tag
            if kind == "exact":
                _compare("tfgnn_edge_pair_combine", tag, kind, out[:E], want, S, 1)
    guard_untouched(out, f"pair_combine out {tag}")
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("E", PC_E)
@pytest.mark.parametrize("width", PC_VEC + PC_SCALAR)
def test_pair_combine(dev, width, E, kind):
    assert all(w % 4 == 0 for w in PC_VEC) and all(w % 4 for w in PC_SCALAR)
    _check_pair_combine(dev, E, width, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("act", ["relu", "tanh", "gelu"])
@pytest.mark.parametrize("width", [24, 5])
def test_pair_combine_activations(dev, width, act, kind):
    _check_pair_combine(dev, 257, width, kind, act)


@pytest.mark.parametrize("E,width", [(0, 8), (5, 0), (0, 0)])
def test_pair_combine_empty(dev, E, width):
    lib, ops = _lib_ops()
    out = guarded(4, 8, dev)
    idx = torch.zeros(8, dtype=torch.int32, device=dev)
    P = torch.zeros((4, 8), device=dev)
    assert lib.tfgnn_edge_pair_combine(ops._ptr(idx), ops._ptr(idx), ops._ptr(P), ops._ptr(P), E, width, 1, ops._ptr(out),
                                       ops._stream()) == 0
    assert lib.tfgnn_edge_pair_combine(None, None, None, None, E, width, 1, None, ops._stream()) == 0
    torch.cuda.synchronize()
    untouched(out, f"out of an empty problem (E = {E}, width = {width})")


@pytest.mark.parametrize("which", ["P", "Q", "out"])
def test_pair_combine_refuses_an_unaligned_operand_at_a_float4_width(dev, which):
    lib, _ = _lib_ops()
    E, width = 65, 8
    ia, ib, P, Q = _pc_inputs(E, width, "normal")
    rc, out = _call_pair_combine(dev, ia, ib, P, Q, E, width, "relu", off=(which,))
    assert rc == -1
    assert "16-byte aligned" in lib.tfgnn_last_error().decode()
    untouched(out, f"refused call ({which} offset): out")


@pytest.mark.parametrize("kind", KINDS)
def test_pair_combine_takes_unaligned_operands_at_a_scalar_width(dev, kind):
    a = _check_pair_combine(dev, 65, 5, kind)
    for off in (("P",), ("Q",), ("out",), ("P", "Q", "out")):
        b = _check_pair_combine(dev, 65, 5, kind, off=off)
        assert torch.equal(a, b)


def _check_in_chunks(E, chunk, check):
    for lo in range(0, E, chunk):
        check(lo, min(E, lo + chunk))


@pytest.mark.parametrize("width,E", [(4, 16777216 + 300), (3, 5592406 + 100)])
def test_pair_combine_past_the_grid(dev, width, E):
    """exact kind only: more work items than 65 536 blocks x 256 threads, the grid-stride loop takes a second trip"""
    assert E * (width // 4 if width % 4 == 0 else width) > 65536 * 256
    rows = 1000
    ia, ib, P, Q = _pc_inputs(E, width, "exact", rows_p=rows, rows_q=rows)
    rc, out = _call_pair_combine(dev, ia, ib, P, Q, E, width, "none")
    assert rc == 0
    got = out.cpu()

    def check(lo, hi):
        want, S, _ = ref.pair_combine(ia[lo:hi], ib[lo:hi], P, Q)
        ref.compare("tfgnn_edge_pair_combine", f"width={width} edges {lo}..{hi} of {E}", "exact", got[lo:hi], want, S, 1)

    _check_in_chunks(E, 1 << 21, check)
    guard_untouched(got, f"pair_combine out width={width} E={E}")


# =================================================================================================================================
# tfgnn_film_edge_forward / _backward
# =================================================================================================================================
FE_WIDTHS = (1, 7, 24, 128)
FE_E = (1, 65, 1027)
FE_MSG_ROWS, FE_BUCKETS = 41, 29


def _fe_inputs(E, width, kind, with_mrow, with_w, msg_rows=FE_MSG_ROWS, buckets=FE_BUCKETS):
    g = _gen(21, E, width, kind == "exact", with_mrow, with_w)
    msg = draw(kind, (msg_rows if with_mrow else E, width), g, scale_rows=True)
    film = draw(kind, (buckets, 2 * width), g, scale_rows=True)
    d = draw(kind, (E, width), g, scale_rows=True)
    mrow = _indices(E, msg_rows, g) if with_mrow else None
    frow = _indices(E, buckets, g)  # repeats and the largest row
    w = draw_scale(kind, E, g) if with_w else None
    return d, msg, mrow, film, frow, w


def _call_film_edge(dev, inputs, E, width):
    """-> (out, d_msg, d_film) with their guard rows"""
    lib, ops = _lib_ops()
    d, msg, mrow, film, frow, w = (None if t is None else t.to(dev) for t in inputs)
    out, d_msg, d_film = guarded(E, width, dev), guarded(E, width, dev), guarded(E, 2 * width, dev)
    rc = lib.tfgnn_film_edge_forward(ops._ptr(msg), ops._ptr(mrow), ops._ptr(film), ops._ptr(frow), ops._ptr(w), E, width, ops._ptr(out),
                                     ops._stream())
    assert rc == 0, f"tfgnn_film_edge_forward returned {rc}"
    rc = lib.tfgnn_film_edge_backward(ops._ptr(d), ops._ptr(msg), ops._ptr(mrow), ops._ptr(film), ops._ptr(frow), ops._ptr(w), E, width,
                                      ops._ptr(d_msg), ops._ptr(d_film), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"tfgnn_film_edge_backward returned {rc}"
    return out, d_msg, d_film


def _check_film_edge(dev, E, width, kind, with_mrow, with_w):
    inputs = _fe_inputs(E, width, kind, with_mrow, with_w)
    d, msg, mrow, film, frow, w = inputs
    out, d_msg, d_film = _call_film_edge(dev, inputs, E, width)
    tag = f"width={width} E={E} {kind} mrow={'given' if with_mrow else 'NULL'} w={'given' if with_w else 'NULL'}"
    want, S = ref.film_edge_forward(msg, mrow, film, frow, w)
    _compare("tfgnn_film_edge_forward", tag, kind, out[:E], want, S, 3)
    want_msg, want_film, S_msg, S_film = ref.film_edge_backward(d, msg, mrow, film, frow, w)
    _compare("tfgnn_film_edge_backward", f"d_msg {tag}", kind, d_msg[:E], want_msg, S_msg, 2)
    _compare("tfgnn_film_edge_backward", f"d_film {tag}", kind, d_film[:E], want_film, S_film, 2)
    assert torch.equal(d_film[:E, width:].cpu(), d), f"{tag}: the beta half of d_film is not a copy of d"
    for buf, what in ((out, "out"), (d_msg, "d_msg"), (d_film, "d_film")):
        guard_untouched(buf, f"film_edge {what} {tag}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_w", [False, True])
@pytest.mark.parametrize("with_mrow", [False, True])
@pytest.mark.parametrize("E", FE_E)
@pytest.mark.parametrize("width", FE_WIDTHS)
def test_film_edge(dev, width, E, with_mrow, with_w, kind):
    _check_film_edge(dev, E, width, kind, with_mrow, with_w)


@pytest.mark.parametrize("E,width", [(0, 8), (5, 0)])
def test_film_edge_empty(dev, E, width):
    lib, ops = _lib_ops()
    bufs = [guarded(4, 16, dev) for _ in range(3)]
    x = torch.zeros((8, 16), device=dev)
    idx = torch.zeros(8, dtype=torch.int32, device=dev)
    assert lib.tfgnn_film_edge_forward(ops._ptr(x), ops._ptr(idx), ops._ptr(x), ops._ptr(idx), None, E, width, ops._ptr(bufs[0]),
                                       ops._stream()) == 0
    assert lib.tfgnn_film_edge_backward(ops._ptr(x), ops._ptr(x), ops._ptr(idx), ops._ptr(x), ops._ptr(idx), None, E, width,
                                        ops._ptr(bufs[1]), ops._ptr(bufs[2]), ops._stream()) == 0
    torch.cuda.synchronize()
    for b in bufs:
        untouched(b, f"an output of an empty problem (E = {E}, width = {width})")


def test_film_edge_past_the_grid(dev):
    """exact kind only: E x width past 65 536 blocks x 256 threads, msg_row and edge_weight given"""
    width, E = 8, 2097152 + 100
    assert E * width > 65536 * 256
    inputs = _fe_inputs(E, width, "exact", True, True, msg_rows=1000, buckets=777)
    d, msg, mrow, film, frow, w = inputs
    out, d_msg, d_film = (t.cpu() for t in _call_film_edge(dev, inputs, E, width))

    def check(lo, hi):
        tag = f"edges {lo}..{hi} of {E}"
        args = (msg, mrow[lo:hi], film, frow[lo:hi], w[lo:hi])
        want, S = ref.film_edge_forward(*args)
        ref.compare("tfgnn_film_edge_forward", tag, "exact", out[lo:hi], want, S, 3)
        want_msg, want_film, S_msg, S_film = ref.film_edge_backward(d[lo:hi], *args)
        ref.compare("tfgnn_film_edge_backward", f"d_msg {tag}", "exact", d_msg[lo:hi], want_msg, S_msg, 2)
        ref.compare("tfgnn_film_edge_backward", f"d_film {tag}", "exact", d_film[lo:hi], want_film, S_film, 2)

    _check_in_chunks(E, 1 << 19, check)
    for buf, what in ((out, "out"), (d_msg, "d_msg"), (d_film, "d_film")):
        guard_untouched(buf, f"film_edge {what} past the grid")


# =================================================================================================================================
# tfgnn_film_combine_forward / _backward
# =================================================================================================================================
FC_SHAPES = [(1, 1, 1), (5, 3, 7), (67, 2, 24), (300, 4, 128), (9, 8, 64)]
HUB_COUNT = 700


def _fc_rowptr(V, L):
    """by-target bucket pointers of a random multigraph: about one edge per bucket (so many are empty) and one bucket of
    exactly 700 edges"""
    adjs = random_graph(V, V * L, L, seed=100 * V + L)
    hub = V // 2
    have = int((adjs[0][:, 1] == hub).sum())
    extra = np.stack([np.arange(HUB_COUNT - have) % V, np.full(HUB_COUNT - have, hub)], axis=1).astype(np.int32)
    adjs[0] = np.concatenate([adjs[0], extra])
    rowptr, _, _ = ao.bucket_edges(adjs, V, by="dst")
    counts = np.diff(rowptr)
    assert counts.max() == HUB_COUNT and counts[hub * L] == HUB_COUNT and (V * L == 1 or counts.min() == 0)
    return torch.from_numpy(rowptr)


def _fc_inputs(V, L, H, kind, with_scale):
    g = _gen(31, V, L, H, kind == "exact", with_scale)
    Z = draw(kind, (V * L, H), g, scale_rows=True)
    film = draw(kind, (V * L, 2 * H), g, scale_rows=True)
    d_pre = draw(kind, (V, H), g, scale_rows=True)
    ns = draw_scale(kind, V, g) if with_scale else None
    rowptr = _fc_rowptr(V, L) if L else torch.zeros(1, dtype=torch.int32)
    return Z, film, rowptr, ns, d_pre


def _call_film_combine_forward(dev, dev_inputs, V, L, H, act, with_pre):
    lib, ops = _lib_ops()
    Z, film, rowptr, ns, _ = dev_inputs
    pre, out = guarded(V, H, dev), guarded(V, H, dev)
    rc = lib.tfgnn_film_combine_forward(ops._ptr(Z), ops._ptr(film), ops._ptr(rowptr), ops._ptr(ns), V, L, H, ops.act_id(act),
                                        ops._ptr(pre) if with_pre else None, ops._ptr(out), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"tfgnn_film_combine_forward returned {rc}"
    return pre, out


def _check_film_combine(dev, V, L, H, kind, with_scale):
    inputs = _fc_inputs(V, L, H, kind, with_scale)
    Z, film, rowptr, ns, d_pre = inputs
    dev_inputs = tuple(None if t is None else t.to(dev) for t in inputs)
    tag = f"(V,L,H)=({V},{L},{H}) {kind} node_scale={'given' if with_scale else 'NULL'}"
    want_pre, _, S = ref.film_combine_forward(Z.reshape(V, L, H), film, rowptr, ns)
    for act in ACT_NAMES:
        pre, out = _call_film_combine_forward(dev, dev_inputs, V, L, H, act, True)
        _compare("tfgnn_film_combine_forward", f"pre {tag} {act}", kind, pre[:V], want_pre, S, 3 * L + 1)
        assert_close(out[:V].cpu(), ref.activation(act, pre[:V].cpu()), tol=ACT_TOL,
                     what=f"tfgnn_film_combine_forward {act} of the returned pre")
        if act in ("none", "relu"):  # they round nothing
            assert torch.equal(out[:V].cpu(), ref.activation(act, pre[:V].cpu()).float()), f"{tag} {act}"
        no_pre, out2 = _call_film_combine_forward(dev, dev_inputs, V, L, H, act, False)
        untouched(no_pre, f"{tag}: a buffer that was not passed")
        assert torch.equal(out2, out), f"{tag} {act}: out depends on whether pre is asked for"
        guard_untouched(pre, f"film_combine pre {tag}")
        guard_untouched(out, f"film_combine out {tag}")
    # backward
    lib, ops = _lib_ops()
    Zd, filmd, rpd, nsd, dpd = dev_inputs
    dZ, dfilm = guarded(V * L, H, dev), guarded(V * L, 2 * H, dev)
    rc = lib.tfgnn_film_combine_backward(ops._ptr(dpd), ops._ptr(Zd), ops._ptr(filmd), ops._ptr(rpd), ops._ptr(nsd), V, L, H, ops._ptr(dZ),
                                         ops._ptr(dfilm), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"tfgnn_film_combine_backward returned {rc}"
    want_Z, want_film, S_Z, S_film = ref.film_combine_backward(d_pre, Z.reshape(V, L, H), film, rowptr, ns)
    _compare("tfgnn_film_combine_backward", f"dZ {tag}", kind, dZ[:V * L], want_Z, S_Z, 2)
    _compare("tfgnn_film_combine_backward", f"dfilm {tag}", kind, dfilm[:V * L], want_film, S_film, 2)
    guard_untouched(dZ, f"film_combine dZ {tag}")
    guard_untouched(dfilm, f"film_combine dfilm {tag}")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("V,L,H", FC_SHAPES)
def test_film_combine(dev, V, L, H, with_scale, kind):
    _check_film_combine(dev, V, L, H, kind, with_scale)


@pytest.mark.parametrize("act", ACT_NAMES)
def test_film_combine_without_edge_types(dev, act):
    """L = 0: out = act(0) (node_scale given or not), pre = 0, and the backward writes nothing"""
    lib, ops = _lib_ops()
    V, H = 5, 7
    ns = draw_scale("normal", V, _gen(41)).to(dev)
    act0 = ref.activation(act, torch.zeros((V, H))).float()
    for scale in (None, ns):
        pre, out = guarded(V, H, dev), guarded(V, H, dev)
        assert lib.tfgnn_film_combine_forward(None, None, None, ops._ptr(scale), V, 0, H, ops.act_id(act), ops._ptr(pre), ops._ptr(out),
                                              ops._stream()) == 0
        torch.cuda.synchronize()
        assert bool((pre[:V] == 0).all())
        assert_close(out[:V].cpu(), act0, tol=ACT_TOL, what=f"tfgnn_film_combine_forward {act} of 0")
        guard_untouched(pre, "film_combine pre L = 0")
        guard_untouched(out, "film_combine out L = 0")
    dZ, dfilm = guarded(4, H, dev), guarded(4, 2 * H, dev)
    d_pre = torch.ones((V, H), device=dev)
    assert lib.tfgnn_film_combine_backward(ops._ptr(d_pre), None, None, None, ops._ptr(ns), V, 0, H, ops._ptr(dZ), ops._ptr(dfilm),
                                           ops._stream()) == 0
    torch.cuda.synchronize()
    untouched(dZ, "dZ at L = 0")
    untouched(dfilm, "dfilm at L = 0")


def test_film_combine_without_nodes(dev):
    lib, ops = _lib_ops()
    L, H = 3, 8
    bufs = [guarded(4, 2 * H, dev) for _ in range(4)]
    x = torch.zeros((12, 2 * H), device=dev)
    rp = torch.zeros(13, dtype=torch.int32, device=dev)
    assert lib.tfgnn_film_combine_forward(ops._ptr(x), ops._ptr(x), ops._ptr(rp), None, 0, L, H, 1, ops._ptr(bufs[0]), ops._ptr(bufs[1]),
                                          ops._stream()) == 0
    assert lib.tfgnn_film_combine_backward(ops._ptr(x), ops._ptr(x), ops._ptr(x), ops._ptr(rp), None, 0, L, H, ops._ptr(bufs[2]),
                                           ops._ptr(bufs[3]), ops._stream()) == 0
    torch.cuda.synchronize()
    for b in bufs:
        untouched(b, "an output of a problem without nodes")


# =================================================================================================================================
# tfgnn_graph_original_order
# =================================================================================================================================
GRAPHS = [(5, 12, 3, {}), (50, 400, 4, {"empty_types": (1,)}), (300, 5000, 3, {"hub": (7, 700)}), (7, 30, 1, {})]


def _call_original_order(dev, g, weight_by_dst, with_weight):
    """-> (rc, src_l, tgt_l, tgt_node, w), each [E + 1, 1] with its guard row"""
    lib, ops = _lib_ops()
    E = g.num_edges
    src_l, tgt_l, tgt_node = (guarded(E, 1, dev, dtype=torch.int32) for _ in range(3))
    w = guarded(E, 1, dev)
    rc = lib.tfgnn_graph_original_order(g._h, ops._ptr(weight_by_dst), ops._ptr(src_l), ops._ptr(tgt_l), ops._ptr(tgt_node),
                                        ops._ptr(w) if with_weight else None, ops._stream())
    torch.cuda.synchronize()
    return rc, src_l, tgt_l, tgt_node, w


@pytest.mark.parametrize("V,E,L,kw", GRAPHS)
def test_original_order(dev, V, E, L, kw):
    _, ops = _lib_ops()
    adjs = random_graph(V, E, L, seed=V + E, **kw)
    g = ops.Graph(to_dev(adjs, dev), V)
    Etot = g.num_edges
    assert Etot == sum(a.shape[0] for a in adjs)
    rowptr, _, _ = ao.bucket_edges(adjs, V, by="dst")
    eid = g.array(ops.G_EID_BY_DST).cpu().numpy()
    assert ref.eid_orders_the_edges_by_bucket(adjs, V, eid, rowptr), "G_EID_BY_DST does not name the edges of its buckets"
    weight = (torch.rand((Etot,), generator=_gen(51, V)) + 0.5)
    tag = f"V={V} E={Etot} L={L}"
    for wbd, with_weight in ((weight, True), (None, True), (weight, False), (None, False)):
        rc, src_l, tgt_l, tgt_node, w = _call_original_order(dev, g, None if wbd is None else wbd.to(dev), with_weight)
        assert rc == 0, f"tfgnn_graph_original_order returned {rc}"
        want = ref.original_order(adjs, V, None if wbd is None else wbd.numpy(), eid)
        case = f"{tag} weight_by_dst={'given' if wbd is not None else 'NULL'} weight={'given' if with_weight else 'NULL'}"
        for got, exp, what in zip((src_l, tgt_l, tgt_node), want[:3], ("src_l", "tgt_l", "tgt_node")):
            ref.compare_equal("tfgnn_graph_original_order", f"{what} {case}", got[:Etot, 0], exp)
            guard_untouched(got, f"original_order {what} {case}")
        if with_weight:
            ref.compare_equal("tfgnn_graph_original_order", f"weight {case}", w[:Etot, 0], want[3])
            guard_untouched(w, f"original_order weight {case}")
        else:
            untouched(w, f"{case}: the weight buffer that was not passed")
    g.close()


def test_original_order_needs_the_edge_ids(dev):
    lib, ops = _lib_ops()
    adjs = random_graph(50, 400, 3, seed=1)
    g = ops.Graph(to_dev(adjs, dev), 50, parts=ops.G_PART_PLAN_TYPED)
    rc, src_l, tgt_l, tgt_node, w = _call_original_order(dev, g, None, True)
    assert rc != 0
    msg = lib.tfgnn_last_error().decode()
    assert "tfgnn_graph_original_order" in msg and "EDGE_IDS" in msg
    for buf in (src_l, tgt_l, tgt_node, w):
        untouched(buf, "refused call: an output")
    g.close()


def test_original_order_without_edges(dev):
    _, ops = _lib_ops()
    adjs = random_graph(10, 0, 2, seed=10, empty_types=(0, 1))
    g = ops.Graph(to_dev(adjs, dev), 10)
    rc, src_l, tgt_l, tgt_node, w = _call_original_order(dev, g, None, True)
    assert rc == 0
    for buf in (src_l, tgt_l, tgt_node, w):
        untouched(buf, "E = 0: an output")
    g.close()
