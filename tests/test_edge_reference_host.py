"""tests/edge_reference.py against torch.autograd in fp64, against its own per-edge form, against the doctest graph of
tests/golden/reference_kats.json and a graph worked out by hand (CPU only): a mistake in the closed-form references of
tests/test_gpu_edge_ops.py / tests/test_gpu_graph_scales.py must not be read as a kernel bug.  Also the checker those files
use: it has to reject one element off by 1 (exact kind), one element off by twice its bound (normal kind) and a written guard
row."""
import numpy as np
import pytest
import torch

from oracle import adjacency_oracle as ao
from tests import edge_reference as ref

CLOSE = dict(rtol=1e-12, atol=1e-12)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, g):
    return torch.randn(shape, generator=g, dtype=torch.float64)


# a graph with empty buckets, multi-edges and self loops: V = 6, L = 2
MULTI = [np.array([[0, 1], [0, 1], [0, 1], [2, 2], [3, 1], [5, 4], [4, 4]], dtype=np.int32),
         np.array([[1, 0], [1, 0], [2, 2], [2, 2], [3, 5]], dtype=np.int32)]
MULTI_V = 6


# ---- the backward references are the gradients of the forward ones -------------------------------------------------------------
@pytest.mark.parametrize("with_mrow", [False, True])
@pytest.mark.parametrize("with_w", [False, True])
def test_film_edge_backward_is_the_gradient_of_the_forward(with_mrow, with_w):
    E, width, rows, buckets = 23, 5, 9, 7
    g = _gen(3 + 2 * with_mrow + with_w)
    mrow = torch.randint(0, rows, (E,), generator=g) if with_mrow else None
    frow = torch.randint(0, buckets, (E,), generator=g)
    msg = _randn((rows if with_mrow else E, width), g)
    film = _randn((buckets, 2 * width), g)
    w = _randn((E,), g) if with_w else None
    d = _randn((E, width), g)
    # the definition, written out independently of the reference
    msg_g, film_g = msg.clone().requires_grad_(True), film.clone().requires_grad_(True)
    m = msg_g[mrow] if with_mrow else msg_g
    if with_w:
        m = w[:, None] * m
    out = film_g[frow][:, :width] * m + film_g[frow][:, width:]
    got, S = ref.film_edge_forward(msg, mrow, film, frow, w)
    torch.testing.assert_close(got, out.detach(), **CLOSE)
    g_msg, g_film = torch.autograd.grad((d * out).sum(), [msg_g, film_g])
    d_msg, d_film, S_msg, S_film = ref.film_edge_backward(d, msg, mrow, film, frow, w)
    assert tuple(d_msg.shape) == (E, width) and tuple(d_film.shape) == (E, 2 * width)
    # per edge -> the shared leaves: d_film over the edges of a bucket, d_msg over the edges sharing a message row
    film_sum = torch.zeros_like(film).index_add_(0, frow, d_film)
    msg_sum = torch.zeros_like(msg).index_add_(0, mrow, d_msg) if with_mrow else d_msg
    torch.testing.assert_close(film_sum, g_film, **CLOSE)
    torch.testing.assert_close(msg_sum, g_msg, **CLOSE)
    assert torch.equal(d_film[:, width:], d)  # the beta half is a copy
    # the magnitude sums: the same expressions on absolute values
    wa = w.abs() if with_w else None
    assert torch.equal(S, ref.film_edge_forward(msg.abs(), mrow, film.abs(), frow, wa)[0])
    am, af, _, _ = ref.film_edge_backward(d.abs(), msg.abs(), mrow, film.abs(), frow, wa)
    assert torch.equal(S_msg, am) and torch.equal(S_film, af)
    assert bool((S >= got.abs() - 1e-12).all())


@pytest.mark.parametrize("with_scale", [False, True])
@pytest.mark.parametrize("V,L,H", [(6, 2, 3), (4, 3, 5), (3, 0, 4)])
def test_film_combine_backward_is_the_gradient_of_the_forward(V, L, H, with_scale):
    g = _gen(10 * V + L + with_scale)
    cnt = torch.randint(0, 5, (V * L,), generator=g)
    rowptr = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(cnt, 0)])
    Z, film = _randn((V, L, H), g), _randn((V * L, 2 * H), g)
    ns = _randn((V,), g) if with_scale else None
    d_pre = _randn((V, H), g)
    Zg, fg = Z.clone().requires_grad_(True), film.clone().requires_grad_(True)
    f3 = fg.reshape(V, L, 2 * H)
    pre = (f3[:, :, :H] * Zg + cnt.double().reshape(V, L, 1) * f3[:, :, H:]).sum(1)
    if with_scale:
        pre = ns[:, None] * pre
    got_pre, got_out, S = ref.film_combine_forward(Z, film, rowptr, ns, "tanh")
    torch.testing.assert_close(got_pre, pre.detach(), **CLOSE)
    torch.testing.assert_close(got_out, torch.tanh(pre.detach()), **CLOSE)
    dZ, dfilm, S_Z, S_film = ref.film_combine_backward(d_pre, Z, film, rowptr, ns)
    assert tuple(dZ.shape) == (V * L, H) and tuple(dfilm.shape) == (V * L, 2 * H)
    if L:
        gZ, gf = torch.autograd.grad((d_pre * pre).sum(), [Zg, fg])
        torch.testing.assert_close(dZ, gZ.reshape(V * L, H), **CLOSE)
        torch.testing.assert_close(dfilm, gf, **CLOSE)
    else:
        assert bool((got_pre == 0).all()) and bool((S == 0).all())
    na = ns.abs() if with_scale else None
    assert torch.equal(S, ref.film_combine_forward(Z.abs(), film.abs(), rowptr, na)[0])
    aZ, af, _, _ = ref.film_combine_backward(d_pre.abs(), Z.abs(), film.abs(), rowptr, na)
    assert torch.equal(S_Z, aZ) and torch.equal(S_film, af)


def test_node_side_film_equals_the_per_edge_form():
    """pre = node_scale * segment sum over targets of the per-edge modulated messages, on a graph with empty buckets,
    multi-edges and self loops: Z is the per-bucket sum of the same messages"""
    V, L, H = MULTI_V, len(MULTI), 4
    rowptr, col, typ = ao.bucket_edges(MULTI, V, by="dst")
    E = col.shape[0]
    counts = np.diff(rowptr)
    assert counts.min() == 0 and counts.max() == 4 and E == 12  # (1, 0) receives 0->1 three times and 3->1
    assert any(int(a[i, 0]) == int(a[i, 1]) for a in MULTI for i in range(a.shape[0]))  # self loops
    g = _gen(7)
    x = _randn((V * L, H), g)      # one message row per (source, type)
    film = _randn((V * L, 2 * H), g)
    ns = _randn((V,), g)
    frow = torch.from_numpy(ref.row_of_position(rowptr))          # bucket of every by-dst position
    mrow = torch.from_numpy(col.astype(np.int64) * L + typ)       # source * L + type
    per_edge, _ = ref.film_edge_forward(x, mrow, film, frow, None)
    target = frow // L
    want = ns[:, None] * torch.zeros((V, H), dtype=torch.float64).index_add_(0, target, per_edge)
    Z = torch.zeros((V * L, H), dtype=torch.float64).index_add_(0, frow, x[mrow]).reshape(V, L, H)
    pre, out, _ = ref.film_combine_forward(Z, film, rowptr, ns, None)
    torch.testing.assert_close(pre, want, **CLOSE)
    assert torch.equal(out, pre)


def test_pair_combine_reference():
    g = _gen(5)
    P, Q = torch.randn((7, 5), generator=g), torch.randn((4, 5), generator=g)
    ia, ib = torch.randint(0, 7, (13,), generator=g, dtype=torch.int32), torch.randint(0, 4, (13,), generator=g, dtype=torch.int32)
    out, S, s32 = ref.pair_combine(ia, ib, P, Q, "relu")
    want = torch.stack([P[int(a)].double() + Q[int(b)].double() for a, b in zip(ia, ib)])
    assert out.dtype == torch.float64 and s32.dtype == torch.float32
    assert torch.equal(out, torch.relu(want)) and torch.equal(S, ref.pair_combine(ia, ib, P.abs(), Q.abs())[0])
    assert torch.equal(s32, want.float())  # one correctly rounded add
    for name in ("none", "relu", "tanh", "leaky_relu", "elu", "selu", "gelu", "sigmoid"):
        y = ref.activation(name, torch.tensor([-2.0, 0.0, 3.0]))
        assert y.dtype == torch.float64 and tuple(y.shape) == (3,)
    assert float(ref.activation("leaky_relu", torch.tensor([-2.0]))) == pytest.approx(-0.4, abs=1e-15)


# ---- the graph references ------------------------------------------------------------------------------------------------------
# 5 nodes, 2 edge types, written out by hand.  In-edges (source -> target):
#   type 0: 0->1, 2->1, 3->1, 4->4, 1->0          type 1: 0->4, 0->4, 3->2
# by-dst buckets r = v*2+l: (0,0)={1->0} (1,0)={0->1,2->1,3->1} (2,1)={3->2} (4,0)={4->4} (4,1)={0->4,0->4}, node 3 has no in-edge
HAND = [np.array([[0, 1], [2, 1], [3, 1], [4, 4], [1, 0]], dtype=np.int32), np.array([[0, 4], [0, 4], [3, 2]], dtype=np.int32)]
HAND_V = 5
_F = np.float32
HAND_INV = {1: _F(1) / (_F(1) + _F(1e-7)), 2: _F(1) / (_F(2) + _F(1e-7)), 3: _F(1) / (_F(3) + _F(1e-7))}


def test_graph_scales_on_the_hand_written_graph():
    i1, i2, i3 = (float(HAND_INV[k]) for k in (1, 2, 3))
    N = [1, 3, 1, 0, 3]                       # all in-edges per node
    inv_rows = [i1, 0, i3, 0, 0, i1, 0, 0, i1, i2]
    # by-src order (source, type | target): (0,0|1) (0,1|4) (0,1|4) (1,0|0) (2,0|1) (3,0|1) (3,1|2) (4,0|4)
    tgt_s = [1, 4, 4, 0, 1, 1, 2, 4]
    inv_s = [i3, i2, i2, i1, i3, i3, i1, i1]
    # by-dst order (target, type | source): (0,0|1) (1,0|0) (1,0|2) (1,0|3) (2,1|3) (4,0|4) (4,1|0) (4,1|0)
    inv_d = [i1, i3, i3, i3, i1, i1, i2, i2]
    for mode in (0, 1, 2):
        m = [1.0 if mode == 0 else 1.0 / max(n, 1) if mode == 1 else 1.0 / np.sqrt(max(n, 1)) for n in N]
        for normalize in (0, 1):
            row, node, ew_s, ew_d = ref.graph_scales(HAND, HAND_V, normalize, mode)
            np.testing.assert_allclose(node, m, rtol=1e-15)
            np.testing.assert_allclose(row, [(inv_rows[r] if normalize else 1.0) * m[r // 2] for r in range(10)], rtol=1e-15)
            np.testing.assert_allclose(ew_s, [(inv_s[p] if normalize else 1.0) * m[tgt_s[p]] for p in range(8)], rtol=1e-15)
            np.testing.assert_allclose(ew_d, [inv_d[p] if normalize else 1.0 for p in range(8)], rtol=1e-15)
    by_src, by_dst, target, pattern = ref.per_edge_derived(HAND, HAND_V)
    assert by_src.dtype == np.float32 and by_dst.dtype == np.float32
    np.testing.assert_array_equal(by_src, np.array(inv_s, dtype=np.float32))
    np.testing.assert_array_equal(by_dst, np.array(inv_d, dtype=np.float32))
    np.testing.assert_array_equal(target, [0, 1, 1, 1, 2, 4, 4, 4])
    np.testing.assert_array_equal(pattern, [3, 1, 1, 3, 1])  # by SOURCE: nodes 0 and 3 send both types
    # 1 / (1 + 1e-7) is not 1 in fp32, 1 / (2 + 1e-7) is 0.5: the sum is taken in fp32
    assert HAND_INV[1] < 1 and HAND_INV[2] == _F(0.5)


def test_original_order_on_the_hand_written_graph():
    rowptr, col, typ = ao.bucket_edges(HAND, HAND_V, by="dst")
    # by-dst positions hold the edges (ids in the concatenated lists): 1->0 = 4; 0->1, 2->1, 3->1 = 0, 1, 2; 3->2 = 7; 4->4 = 3; 0->4 x 2 = 5, 6
    eid = np.array([4, 0, 1, 2, 7, 3, 5, 6])
    assert ref.eid_orders_the_edges_by_bucket(HAND, HAND_V, eid, rowptr)
    assert ref.eid_orders_the_edges_by_bucket(HAND, HAND_V, np.array([4, 2, 0, 1, 7, 3, 6, 5]), rowptr)  # inside a bucket: free
    assert not ref.eid_orders_the_edges_by_bucket(HAND, HAND_V, np.array([0, 4, 1, 2, 7, 3, 5, 6]), rowptr)
    assert not ref.eid_orders_the_edges_by_bucket(HAND, HAND_V, np.array([4, 0, 1, 2, 7, 3, 5, 5]), rowptr)
    w_by_dst = np.arange(10, 18, dtype=np.float32)
    src_l, tgt_l, tgt_node, w = ref.original_order(HAND, HAND_V, w_by_dst, eid)
    np.testing.assert_array_equal(src_l, [0, 4, 6, 8, 2, 1, 1, 7])
    np.testing.assert_array_equal(tgt_l, [2, 2, 2, 8, 0, 9, 9, 5])
    np.testing.assert_array_equal(tgt_node, [1, 1, 1, 4, 0, 4, 4, 2])
    np.testing.assert_array_equal(w, [11, 12, 13, 15, 10, 16, 17, 14])
    assert all(a.dtype == np.int32 for a in (src_l, tgt_l, tgt_node)) and w.dtype == np.float32
    np.testing.assert_array_equal(ref.original_order(HAND, HAND_V, None, None)[3], np.ones(8, dtype=np.float32))
    k, ident, node_of_row = ref.target_multiplier(rowptr, None, 2)
    np.testing.assert_array_equal(k, [1, 0, 3, 0, 0, 1, 0, 0, 1, 2])
    np.testing.assert_array_equal(ident, np.arange(11))
    np.testing.assert_array_equal(node_of_row, [0, 0, 1, 1, 2, 2, 3, 3, 4, 4])
    rs = np.full(10, 1 / 3, dtype=np.float32)
    k3, _, _ = ref.target_multiplier(rowptr, rs, 2)
    assert k3.dtype == np.float32 and k3[2] == np.float32(3) * np.float32(1 / 3) and k3[1] == 0


def test_graph_references_on_the_doctest_graph(kats):
    d = kats["num_incoming_doctest"]
    adjs = [np.array(a, dtype=np.int32) for a in d["adjacency_lists"]]
    V, L = d["num_nodes"], len(adjs)
    counts = np.array(d["expected"])  # [L, V] in-degrees, the reference's own output
    row, node, ew_s, ew_d = ref.graph_scales(adjs, V, 1, 1)
    c32 = counts.T.astype(np.float32)  # [V, L]
    inv = np.where(c32 > 0, np.float32(1) / (c32 + np.float32(1e-7)), np.float32(0)).astype(np.float64)
    m = 1.0 / np.maximum(counts.sum(axis=0), 1)
    np.testing.assert_allclose(node, m, rtol=1e-15)
    np.testing.assert_allclose(row, (inv * m[:, None]).reshape(V * L), rtol=1e-15)
    # per edge, straight from the lists: the edge's own (type, target) count
    src_l, tgt_l, tgt_node, w = ref.original_order(adjs, V, None, None)
    flat = [(s, t, l) for l, a in enumerate(adjs) for s, t in a.tolist()]
    np.testing.assert_array_equal(src_l, [s * L + l for s, t, l in flat])
    np.testing.assert_array_equal(tgt_l, [t * L + l for s, t, l in flat])
    np.testing.assert_array_equal(tgt_node, [t for s, t, l in flat])
    rowptr, col, typ = ao.bucket_edges(adjs, V, by="dst")
    eid = np.argsort(np.array(tgt_l), kind="stable")
    assert ref.eid_orders_the_edges_by_bucket(adjs, V, eid, rowptr)
    _, _, _, w = ref.original_order(adjs, V, ew_d.astype(np.float32), eid)
    np.testing.assert_array_equal(w, [np.float32(inv[t, l]) for s, t, l in flat])
    # by-src order: sorted by (source, type), stable; ew_by_src is the weight of the edge's TARGET
    by_src = sorted(range(len(flat)), key=lambda i: flat[i][0] * L + flat[i][2])
    np.testing.assert_allclose(ew_s, [inv[flat[i][1], flat[i][2]] * m[flat[i][1]] for i in by_src], rtol=1e-15)
    np.testing.assert_allclose(ref.graph_scales(adjs, V, 0, 0)[0], np.ones(V * L))


# ---- the checker ---------------------------------------------------------------------------------------------------------------
def test_checker_rejects_an_exact_output_off_by_one():
    want = torch.arange(24, dtype=torch.float64).reshape(4, 6)
    assert ref.compare("entry", "ok", "exact", want.float(), want, None, 1) == 0.0
    got = want.float().clone()
    got[2, 3] += 1
    with pytest.raises(AssertionError, match="1 of 24 elements differ"):
        ref.compare("entry", "off by one", "exact", got, want, None, 1)


@pytest.mark.parametrize("n", [1, 3, 13])
def test_checker_rejects_a_normal_output_off_by_twice_its_bound(n):
    g = _gen(n)
    want, S = _randn((5, 7), g), _randn((5, 7), g).abs() + 0.5
    bound = ref.gamma_bound(n, S)
    assert torch.equal(bound, 1.01 * n * 2.0 ** -24 * S)
    seen = []
    inside = want + 0.99 * bound * torch.sign(_randn((5, 7), g))
    worst = ref.compare("entry", "inside", "normal", inside, want, S, n, record=lambda e, w: seen.append((e, w)))
    assert 0.98 < worst <= 1.0 and seen == [("entry", worst)]
    got = want.clone()
    got[3, 2] += 2.0 * bound[3, 2]
    with pytest.raises(AssertionError, match=r"error 2\.000 x the bound .* at element 23"):
        ref.compare("entry", "twice the bound", "normal", got, want, S, n, record=lambda e, w: seen.append((e, w)))
    assert seen[-1][1] == pytest.approx(2.0)  # the failing figure is recorded before the assertion
    # S = 0 allows nothing but an exact 0; a non-finite output is refused in both kinds
    zero_S, zero_want = S.clone(), want.clone()
    zero_S[0, 0] = zero_want[0, 0] = 0.0
    assert ref.compare("entry", "S = 0, exact 0", "normal", zero_want, zero_want, zero_S, n) == 0.0
    tiny = zero_want.clone()
    tiny[0, 0] = 1e-30
    with pytest.raises(AssertionError):
        ref.compare("entry", "S = 0", "normal", tiny, zero_want, zero_S, n)
    bad = want.clone()
    bad[0, 0] = float("nan")
    for kind in ref.KINDS:
        with pytest.raises(AssertionError, match="non-finite"):
            ref.compare("entry", "nan", kind, bad, want, S, n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.int32])
def test_checker_rejects_a_written_guard_row(dtype):
    buf = ref.guarded(3, 4, "cpu", dtype=dtype)
    assert tuple(buf.shape) == (4, 4)
    ref.untouched(buf, "fresh buffer")
    buf[:3] = 1
    ref.guard_untouched(buf, "rows written, guard intact")
    with pytest.raises(AssertionError, match="was written"):
        ref.untouched(buf, "rows written")
    buf[3, 1] = 0
    with pytest.raises(AssertionError, match="guard row behind the last row was written"):
        ref.guard_untouched(buf, "guard written")
    init = ref.guarded(2, 3, "cpu", init=torch.arange(6).reshape(2, 3), dtype=dtype)
    assert init[:2].tolist() == [[0, 1, 2], [3, 4, 5]]
    ref.guard_untouched(init, "initialised buffer")
    empty = ref.guarded(0, 4, "cpu", dtype=dtype)
    assert tuple(empty.shape) == (1, 4)
    ref.untouched(empty, "no rows")


def test_checker_compare_equal_and_draws():
    ref.compare_equal("entry", "same", torch.arange(5, dtype=torch.int32), np.arange(5))
    with pytest.raises(AssertionError, match="1 of 5 elements differ, the first at 3"):
        ref.compare_equal("entry", "one off", torch.tensor([0, 1, 2, 4, 4], dtype=torch.int32), np.arange(5))
    g = _gen(1)
    x = ref.draw("exact", (200, 3), g)
    assert x.dtype == torch.float32 and set(x.unique().tolist()) == {-3.0, -2.0, -1.0, 0.0, 1.0, 2.0, 3.0}
    s = ref.draw_scale("exact", 100, g)
    assert set(s.unique().tolist()) == {0.5, 1.0, 2.0}
    n = ref.draw("normal", (9, 2000), _gen(2), scale_rows=True)
    rms = n.pow(2).mean(1).sqrt()
    assert 5e3 < rms[3] < 2e4 and 5e-5 < rms[6] < 2e-4 and 0.9 < rms[0] < 1.1
    # the exact inputs stay exact: the largest film_combine sum of the device tests, 8 types x (9 + 700 * 3) x 2 << 2^24
    assert 8 * (9 + 700 * 3) * 2 < 2 ** 24 // 8
