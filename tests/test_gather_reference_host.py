"""tests/gather_reference.py against the oracle's own segment operations on a small graph (CPU only): a bug in the fp64
reference of tests/test_gpu_graph_gather.py must not be read as a kernel bug."""
import numpy as np
import pytest
import torch

from oracle import adjacency_oracle as ao
from oracle import tf2gnn_oracle as orc
from tests import gather_reference as gr
from tests.helpers import random_graph

V, L, WIDTH = 23, 3, 12


@pytest.fixture(scope="module")
def small():
    adjs = random_graph(V, 120, L, seed=4, empty_types=(1,), hub=(3, 40))
    rowptr, col, _ = ao.bucket_edges(adjs, V, by="dst")
    gen = torch.Generator().manual_seed(9)
    X = torch.randn((V, WIDTH), generator=gen)
    ew = torch.rand(col.shape[0], generator=gen) + 0.5
    rs = torch.rand(V * L, generator=gen) + 0.5
    seg = torch.from_numpy(np.repeat(np.arange(V * L), np.diff(rowptr))).int()
    assert int((np.diff(rowptr) == 0).sum()) > 0  # empty rows are part of the comparison
    return adjs, rowptr, col, X, ew, rs, seg


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("scales", [False, True])
def test_sum_and_max_equal_the_oracle_segment_ops(small, weights, scales):
    _, rowptr, col, X, ew, rs, seg = small
    msgs = X.double()[torch.from_numpy(col).long()]
    if weights:
        msgs = msgs * ew.double().unsqueeze(1)
    kw = dict(edge_weight=ew if weights else None, row_scale=rs if scales else None)
    out, l1, row_len = gr.gather_reference(rowptr, col, X, **kw)
    ref = orc.unsorted_segment_sum(msgs, seg, V * L)
    ref_l1 = orc.unsorted_segment_sum(msgs.abs(), seg, V * L)
    if scales:
        ref, ref_l1 = ref * rs.double().unsqueeze(1), ref_l1 * rs.double().clamp(min=1.0).unsqueeze(1)
    torch.testing.assert_close(out, ref, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(l1, ref_l1, rtol=1e-13, atol=1e-13)
    assert np.array_equal(row_len.numpy(), np.diff(rowptr))
    out, _, _ = gr.gather_reference(rowptr, col, X, reduce="max", **kw)
    ref = orc.unsorted_segment_max(msgs, seg, V * L)
    empty = torch.from_numpy(np.diff(rowptr) == 0)
    assert bool((ref[empty] == torch.finfo(torch.float64).min).all())
    ref[empty] = orc.unsorted_segment_max(msgs.float(), seg, V * L).double()[empty]  # the lowest finite fp32, not scaled
    if scales:
        ref[~empty] = ref[~empty] * rs.double()[~empty].unsqueeze(1)
    assert torch.equal(out, ref)
    assert bool((out[empty] == gr.FLOAT_LOWEST).all())


@pytest.mark.parametrize("name", ["sum", "max", "mean", "sqrt_n"])
def test_aggregation_functions_with_activations(small, name):
    """mean / sqrt_n are sums with a row scale; pre / post activations are the oracle's"""
    _, rowptr, col, X, ew, _, seg = small
    pre, post = orc.get_activation_function("gelu"), orc.get_activation_function("tanh")
    msgs = pre(X.double()[torch.from_numpy(col).long()] * ew.double().unsqueeze(1))
    n = torch.from_numpy(np.diff(rowptr)).double().clamp(min=1.0)
    scale = {"sum": None, "max": None, "mean": 1.0 / n, "sqrt_n": 1.0 / n.sqrt()}[name]
    out, _, _ = gr.gather_reference(rowptr, col, X, edge_weight=ew, row_scale=scale, reduce="max" if name == "max" else "sum",
                                    pre_act="gelu", post_act="tanh")
    ref = orc.get_aggregation_function(name)(msgs, seg, V * L)
    if name == "max":
        ref[torch.from_numpy(np.diff(rowptr) == 0)] = gr.FLOAT_LOWEST
    torch.testing.assert_close(out, post(ref), rtol=1e-13, atol=1e-13)
    for act in ("relu", "leaky_relu", "elu", "selu", "sigmoid"):
        x = torch.linspace(-4, 4, 101, dtype=torch.float64)
        assert torch.equal(gr.activation(act)(x), orc.get_activation_function_by_name(act)(x))


def test_per_head_weights_equal_separate_calls(small):
    _, rowptr, col, X, _, rs, _ = small
    K = 3
    ewk = torch.rand((col.shape[0], K), generator=torch.Generator().manual_seed(2)) + 0.5
    out, l1, _ = gr.gather_reference(rowptr, col, X, edge_weight=ewk, row_scale=rs)
    hw = WIDTH // K
    for k in range(K):
        o, l, _ = gr.gather_reference(rowptr, col, X[:, k * hw:(k + 1) * hw], edge_weight=ewk[:, k], row_scale=rs)
        assert torch.equal(out[:, k * hw:(k + 1) * hw], o) and torch.equal(l1[:, k * hw:(k + 1) * hw], l)


def test_view_rows_follow_the_header(small):
    adjs = small[0]
    for by, typed, node, compact in (("dst", gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE, gr.VIEW_BY_DST_TYPED_COMPACT),
                                     ("src", gr.VIEW_BY_SRC_TYPED, gr.VIEW_BY_SRC_NODE, gr.VIEW_BY_SRC_TYPED_COMPACT)):
        rowptr, col, typ = ao.bucket_edges(adjs, V, by=by)
        rp, c, rows = gr.view_rows(adjs, V, typed)
        assert np.array_equal(rp, rowptr) and np.array_equal(c, col) and rows is None
        # node rows, edge by edge from the lists: node v holds the edges whose row node is v, col = other end * L + type
        rp, c, rows = gr.view_rows(adjs, V, node)
        assert rows is None and rp.shape == (V + 1,)
        k = 0 if by == "src" else 1
        for v in range(V):
            want = sorted(int(a[i, 1 - k]) * L + l for l, a in enumerate(adjs) for i in range(a.shape[0]) if a[i, k] == v)
            assert sorted(c[rp[v]:rp[v + 1]].tolist()) == want
        rp, c, rows = gr.view_rows(adjs, V, compact)
        lens = np.diff(rowptr)
        assert np.array_equal(rp, rowptr) and rows.tolist() == [v * L + l for l in range(L) for v in range(V) if lens[v * L + l] > 0]
    pos = np.random.default_rng(0).permutation(V)
    _, _, rows = gr.view_rows(adjs, V, gr.VIEW_BY_DST_TYPED_PATTERN, pattern_pos=pos)
    for v in (0, 5, V - 1):
        for l in range(L):
            assert rows[pos[v] * L + l] == v * L + l
    with pytest.raises(AssertionError):
        gr.view_rows(adjs, V, gr.VIEW_BY_DST_TYPED_PATTERN, pattern_pos=np.zeros(V, dtype=np.int64))


@pytest.mark.parametrize("pre_act", [None, "tanh", "elu"])
def test_backward_reference_equals_autograd_through_the_oracle(pre_act):
    """continuous random messages: no two edges of a target tie, the max gradient goes to one edge per (target, column)"""
    E, T, W = 90, 11, 5
    gen = torch.Generator().manual_seed(6)
    msg = torch.randn((E, W), generator=gen)
    target = torch.randint(0, T - 1, (E,), generator=gen)  # target T - 1 stays empty
    ew = torch.rand(E, generator=gen) + 0.5
    ns = torch.rand(T, generator=gen) + 0.5
    grad = torch.randn((T, W), generator=gen).double()
    act = gr.activation(pre_act)
    m = msg.double().requires_grad_(True)
    z = act(m * ew.float().double().unsqueeze(1))
    (want,) = torch.autograd.grad((orc.unsorted_segment_sum(z, target, T) * ns.double().unsqueeze(1) * grad).sum(), m)
    got = gr.aggregate_backward_reference(msg, target, grad, num_targets=T, edge_weight=ew, node_scale=ns, pre_act=pre_act)
    torch.testing.assert_close(got, want, rtol=1e-13, atol=1e-13)
    m = msg.double().requires_grad_(True)
    z = act(m * ew.float().double().unsqueeze(1))
    (want,) = torch.autograd.grad((orc.unsorted_segment_max(z, target, T) * grad).sum(), m)
    sel, ties, got, gap = gr.aggregate_backward_reference(msg, target, grad, num_targets=T, edge_weight=ew, pre_act=pre_act,
                                                          reduce="max")
    assert float(gap.min()) > 1e-6 and int(ties.max()) == 1 and bool((ties[T - 1] == 0).all())
    assert bool((sel.sum(dim=0) == T - 1).all())
    torch.testing.assert_close(got, want, rtol=1e-6, atol=1e-9)  # (the reference rounds w * msg to fp32 for the tie decision only)
    assert bool((got[~sel] == 0).all())


def test_backward_reference_splits_exact_ties_evenly():
    msg = torch.tensor([[1.0, -2.0], [0.5, 3.0]])
    msg_row = torch.tensor([0, 1, 0, 0])
    target = torch.tensor([0, 0, 0, 1])
    grad = torch.tensor([[6.0, 8.0], [1.0, 1.0]]).double()
    sel, ties, g, gap = gr.aggregate_backward_reference(msg, target, grad, num_targets=2, msg_row=msg_row, reduce="max")
    assert sel.tolist() == [[True, False], [False, True], [True, False], [True, True]]
    assert ties.tolist() == [[2.0, 1.0], [1.0, 1.0]]
    assert g.tolist() == [[3.0, 0.0], [0.0, 8.0], [3.0, 0.0], [1.0, 1.0]]
    assert gap[0].tolist() == [0.5, 5.0 / 3.0] and bool(torch.isinf(gap[1]).all())
