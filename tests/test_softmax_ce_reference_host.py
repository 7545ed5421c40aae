"""tests/softmax_ce_reference.py - the float64 restatement of the tfgnn_softmax_ce_metrics contract (include/tfgnn.h) that
tests/test_gpu_softmax_ce.py holds the kernel to - pinned on the CPU against torch's float64 ``cross_entropy`` and its
autograd gradient, and on the cases the contract spells out: ignored labels, no counted node, ties, one class."""
import math

import numpy as np
import pytest
import torch

from tests.softmax_ce_reference import counted_nodes, softmax_ce


def _inputs(V, C, seed):
    rng = np.random.default_rng(seed)
    x = (3 * rng.standard_normal((V, C))).astype(np.float32)
    x.reshape(-1)[::11] *= 30
    y = rng.integers(0, C, size=V).astype(np.float32)
    return rng, x, y


def _weights(kind, rng, V):
    if kind == "none":
        return None
    if kind == "mask":
        return (rng.random(V) < 0.5).astype(np.float32)
    w = (2 * rng.random(V)).astype(np.float32)
    w[::5] = 0.0
    return w


@pytest.mark.parametrize("kind", ["none", "mask", "fractional"])
@pytest.mark.parametrize("V,C", [(1, 2), (37, 7), (64, 40), (9, 300)])
def test_reference_equals_torch_cross_entropy_in_float64(V, C, kind):
    """loss = sum_v w_v ce_v / sum_v w_v, which is ``F.cross_entropy(reduction="none")`` weighted by hand; the gradient is
    autograd's.  Both sides are float64 sums of the same terms: 1e-12 relative."""
    rng, x, y = _inputs(V, C, seed=V * 1000 + C)
    w = _weights(kind, rng, V)
    if w is not None:
        w[0] = 1.0  # at least one counted node
    ref = softmax_ce(x, y, w)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    w64 = torch.ones(V, dtype=torch.float64) if w is None else torch.from_numpy(w).double()
    per_node = torch.nn.functional.cross_entropy(x64, torch.from_numpy(y).long(), reduction="none")
    loss = (w64 * per_node).sum() / w64.sum()
    (grad,) = torch.autograd.grad(loss, x64)
    assert ref.W == pytest.approx(float(w64.sum()), rel=1e-15)
    assert ref.loss == pytest.approx(float(loss.detach()), rel=1e-12, abs=1e-12)
    assert np.abs(ref.dlogits - grad.numpy()).max() <= 1e-12 * max(1.0, float(grad.abs().max()))
    pred = x64.detach().argmax(dim=1).numpy()  # no ties in these inputs
    assert np.array_equal(ref.pred, pred)
    keep = w64.numpy() > 0
    assert ref.counted_nodes == int(keep.sum()) and ref.correct == int((pred == y)[keep].sum())
    assert ref.accuracy == ref.correct / ref.counted_nodes
    if w is not None:
        assert np.all(ref.dlogits[~keep] == 0.0)


def test_reference_with_ignore_index_of_torch():
    """a label of -1 with weight 1 is torch's ignore_index with reduction="mean": the mean runs over the others"""
    rng, x, y = _inputs(50, 6, seed=3)
    y[::4] = -1.0
    ref = softmax_ce(x, y, None)
    want = torch.nn.functional.cross_entropy(torch.from_numpy(x).double(), torch.from_numpy(y).long(), ignore_index=-1)
    assert ref.loss == pytest.approx(float(want), rel=1e-12)
    assert ref.counted_nodes == int((y >= 0).sum()) and ref.W == float(ref.counted_nodes)


def test_ignored_labels_and_weights_have_zero_gradient_rows():
    C = 5
    x = np.arange(8 * C, dtype=np.float32).reshape(8, C) % 7
    #             ok   -1    >= C  frac  NaN           ok    ok    ok
    y = np.array([2.0, -1.0, 5.0, 2.5, float("nan"), 1.0, 0.0, 4.0], dtype=np.float32)
    #             ok   ok   ok   ok   ok   zero  negative  NaN
    w = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 0.0, -1.0, float("nan")], dtype=np.float32)
    assert counted_nodes(y, w, C).tolist() == [True] + [False] * 7
    assert counted_nodes(y, None, C).tolist() == [True, False, False, False, False, True, True, True]
    ref = softmax_ce(x, y, w)
    assert ref.counted_nodes == 1 and ref.W == 1.0
    assert np.all(ref.dlogits[1:] == 0.0) and np.any(ref.dlogits[0] != 0.0)
    alone = softmax_ce(x[:1], y[:1], None)
    assert ref.loss == alone.loss and np.array_equal(ref.dlogits[0], alone.dlogits[0])
    assert ref.pred.shape == (8,)  # predictions are there for every node


def test_no_counted_node():
    x = np.random.default_rng(0).standard_normal((4, 3)).astype(np.float32)
    for y, w in ((np.full(4, -1.0), None), (np.zeros(4), np.zeros(4))):
        ref = softmax_ce(x, y, w)
        assert ref.loss == 0.0 and ref.W == 0.0 and ref.counted_nodes == 0 and ref.correct == 0
        assert math.isnan(ref.accuracy) and np.all(ref.dlogits == 0.0)
        assert np.array_equal(ref.pred, x.argmax(axis=1))


def test_ties_take_the_lowest_index():
    x = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, -1.0, 0.0, -2.0], [float("nan"), 1.0, 1.0, 0.0]],
                 dtype=np.float32)
    ref = softmax_ce(x[:3], np.array([1.0, 0.0, 2.0]), None)
    assert ref.pred.tolist() == [1, 0, 0] and ref.correct == 2 and ref.accuracy == 2 / 3
    # a NaN takes part as -inf in the argmax and poisons the loss of a counted row
    with_nan = softmax_ce(x, np.array([1.0, 0.0, 2.0, 1.0]), None)
    assert with_nan.pred.tolist() == [1, 0, 0, 1] and math.isnan(with_nan.loss)
    uncounted = softmax_ce(x, np.array([1.0, 0.0, 2.0, -1.0]), None)
    assert uncounted.loss == ref.loss


def test_single_class():
    x = np.array([[3.0], [-7.0], [1e4]], dtype=np.float32)
    ref = softmax_ce(x, np.zeros(3), np.array([1.0, 0.5, 2.0]))
    assert ref.loss == 0.0 and np.all(ref.dlogits == 0.0) and ref.pred.tolist() == [0, 0, 0]
    assert ref.correct == 3 and ref.accuracy == 1.0 and ref.W == 3.5
