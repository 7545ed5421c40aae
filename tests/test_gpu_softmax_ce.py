"""tfgnn_softmax_ce_metrics on the device against tests/softmax_ce_reference.py, the float64 restatement of its contract
(include/tfgnn.h; pinned against torch in tests/test_softmax_ce_reference_host.py).  Not run per GEMM mode: no product is
involved.

Shapes: the small, odd and multi-workgroup ones, C - 1, C, C + 1 at every width where the main pass changes its lane-group
size or its row strategy (C = 32, 64, 128, 256, 512; include/tfgnn.h), and one with more rows than one sweep of the grid
holds (2048 workgroups x 4 waves x 16 rows at C <= 32), which also fills all 64 partials of the weight pass."""
import math

import numpy as np
import pytest
import torch

from tests.softmax_ce_reference import softmax_ce

pytestmark = pytest.mark.gpu

SWITCHES = (32, 64, 128, 256, 512)
SHAPES = [(1, 1), (1, 2), (3, 3), (64, 63), (64, 64), (64, 65), (257, 40), (300, 129), (37, 1000), (9, 2500), (5000, 40)]
SHAPES += [(33, c + d) for c in SWITCHES for d in (-1, 0, 1) if (33, c + d) not in SHAPES and c != 64]
SHAPES += [(140001, 3)]


def _inputs(V, C, kind):
    """logits 3 * randn, every 11th entry times 30; rows 2 (mod 7) with exact ties at the maximum, row 1 all equal, row 3
    shifted by 1e4; labels uniform, every 13th -1 and one equal to C; weights None, a Bernoulli(0.5) mask, or uniform(0, 2)
    with exact zeros and one negative."""
    g = torch.Generator().manual_seed(1000 * V + C)
    x = torch.randn((V, C), generator=g) * 3
    x.view(-1)[::11] *= 30
    if C > 1:
        for v in range(2, V, 7):
            cols = torch.randperm(C, generator=g)[: min(3, C)]
            x[v, cols] = x[v].max() + 1.0
    if V > 1:
        x[1] = 0.75
    if V > 3:
        x[3] += 1e4
    y = torch.randint(0, C, (V,), generator=g).float()
    y[12::13] = -1.0
    if V > 5:
        y[5] = float(C)
    if kind == "none":
        w = None
    elif kind == "mask":
        w = (torch.rand(V, generator=g) < 0.5).float()
    else:
        w = torch.rand(V, generator=g) * 2
        w[4::9] = 0.0
        if V > 6:
            w[6] = -0.5
    return x, y, w


@pytest.mark.parametrize("kind", ["none", "mask", "fractional"])
@pytest.mark.parametrize("V,C", SHAPES)
def test_softmax_ce_metrics_kernel(dev, V, C, kind):
    """Bounds, the ones tests/test_gpu_tasks.py and tests/test_gpu_binary_task.py hold the task kernels to: counts and pred
    exact (argmax compares the given fp32 values); loss 2e-6 * max(1, |ref|); accuracy 1e-6; max |dlogits - ref| <=
    1e-6 / W + 1e-7 max|ref|; rows of uncounted nodes exactly 0; metrics and counts bit-identical run to run and without the
    optional outputs."""
    from tf2_gnn_amd import ops

    x, y, w = _inputs(V, C, kind)
    ref = softmax_ce(x.numpy(), y.numpy(), None if w is None else w.numpy())
    # strided everything: logits inside a wider array, labels and weights the two columns of one [V, 2], dlogits into a
    # wider array whose other columns must stay as they are
    wide = torch.zeros((V, C + 5))
    wide[:, :C] = x
    yw = torch.stack([y, torch.ones(V) if w is None else w], dim=1).to(dev)
    grad_wide = torch.full((V, C + 3), 7.0, device=dev)
    logits_d = wide.to(dev)[:, :C]
    weights_d = None if w is None else yw[:, 1]
    metrics, counts, grad, pred = ops.softmax_ce_metrics(logits_d, yw[:, 0], weights_d, want_pred=True, out=grad_wide[:, :C])
    assert grad.data_ptr() == grad_wide.data_ptr() and bool((grad_wide[:, C:] == 7.0).all())
    assert counts.dtype == torch.int64 and pred.dtype == torch.int32 and pred.shape == (V,)

    loss, acc = float(metrics[0]), float(metrics[1])
    err_loss = abs(loss - ref.loss)
    got = grad.cpu().double().numpy()
    err_grad = float(np.abs(got - ref.dlogits).max())
    bound_grad = (1e-6 / ref.W if ref.W > 0 else 0.0) + 1e-7 * float(np.abs(ref.dlogits).max())
    print(f"softmax_ce_metrics V={V} C={C} weights={kind}: W {ref.W:.9g} loss {loss:.9g} ref {ref.loss:.9g} |err| {err_loss:.3g} "
          f"(bound {2e-6 * max(1.0, abs(ref.loss)):.3g}); acc {acc:.9g} ref {ref.accuracy:.9g}; dlogits max|err| {err_grad:.3g} "
          f"(bound {bound_grad:.3g})")
    assert counts.cpu().tolist() == [ref.correct, ref.counted_nodes]
    assert np.array_equal(pred.cpu().numpy(), ref.pred)
    assert err_loss <= 2e-6 * max(1.0, abs(ref.loss))
    if ref.counted_nodes:
        assert abs(acc - ref.accuracy) <= 1e-6
    else:
        assert math.isnan(acc) and loss == 0.0
    assert err_grad <= bound_grad
    assert bool((got[~ref.counted] == 0.0).all())

    # a contiguous gradient of the wrapper's own holds the same bits; metrics and counts are reproducible
    metrics2, counts2, grad2, no_pred = ops.softmax_ce_metrics(logits_d, yw[:, 0], weights_d)
    assert no_pred is None and grad2.is_contiguous() and torch.equal(grad2, grad)
    metrics3, counts3, no_grad, no_pred = ops.softmax_ce_metrics(logits_d, yw[:, 0], weights_d, need_grad=False, want_pred=False)
    assert no_grad is None and no_pred is None
    for m, c in ((metrics2, counts2), (metrics3, counts3)):
        assert torch.equal(m.view(torch.int32), metrics.view(torch.int32)) and torch.equal(c, counts)


@pytest.mark.parametrize("V,C", [(50, 7), (20, 600)])
def test_all_zero_weights(dev, V, C):
    """no counted node: loss 0.0, not nan; every gradient entry 0.0; accuracy nan; counts [0, 0]; pred still written"""
    from tf2_gnn_amd import ops

    x, y, _ = _inputs(V, C, "none")
    metrics, counts, grad, pred = ops.softmax_ce_metrics(x.to(dev), y.to(dev), torch.zeros(V, device=dev), want_pred=True)
    assert float(metrics[0]) == 0.0 and math.isnan(float(metrics[1])) and counts.cpu().tolist() == [0, 0]
    assert bool((grad == 0.0).all())
    assert np.array_equal(pred.cpu().numpy(), softmax_ce(x.numpy(), y.numpy()).pred)
    metrics, counts, grad, _ = ops.softmax_ce_metrics(x.to(dev), torch.full((V,), -1.0, device=dev))
    assert float(metrics[0]) == 0.0 and math.isnan(float(metrics[1])) and counts.cpu().tolist() == [0, 0]
    assert bool((grad == 0.0).all())


@pytest.mark.parametrize("V,C", [(50, 7), (40, 200), (20, 600)])
def test_nan_logit_is_not_hidden(dev, V, C):
    from tf2_gnn_amd import ops

    x, y, _ = _inputs(V, C, "none")
    y[8] = 0.0
    x[8, C // 2] = float("nan")
    metrics, counts, grad, _ = ops.softmax_ce_metrics(x.to(dev), y.to(dev))
    assert math.isnan(float(metrics[0])) and int(counts[1]) == softmax_ce(x.numpy(), y.numpy()).counted_nodes
    assert bool(torch.isfinite(grad[:8]).all()) and bool(torch.isfinite(grad[9:]).all())
    w = torch.ones(V)
    w[8] = 0.0
    clean = x.clone()
    clean[8] = 0.0
    ref = softmax_ce(clean.numpy(), y.numpy(), w.numpy())
    for labels, weights in ((y, w), (torch.where(torch.arange(V) == 8, torch.tensor(-1.0), y), None)):
        metrics, counts, grad, _ = ops.softmax_ce_metrics(x.to(dev), labels.to(dev), None if weights is None else weights.to(dev))
        assert abs(float(metrics[0]) - ref.loss) <= 2e-6 * max(1.0, abs(ref.loss))
        assert counts.cpu().tolist() == [ref.correct, ref.counted_nodes]
        assert bool(torch.isfinite(grad).all()) and bool((grad[8] == 0.0).all())


def test_single_class(dev):
    from tf2_gnn_amd import ops

    x = torch.tensor([[3.0], [-7.0], [1e4]], device=dev)
    metrics, counts, grad, pred = ops.softmax_ce_metrics(x, torch.zeros(3, device=dev), want_pred=True)
    assert float(metrics[0]) == 0.0 and float(metrics[1]) == 1.0 and counts.cpu().tolist() == [3, 3]
    assert bool((grad == 0.0).all()) and pred.cpu().tolist() == [0, 0, 0]


def test_softmax_ce_metrics_arguments(dev):
    from tf2_gnn_amd import ops

    with pytest.raises(ValueError, match="empty batch"):
        ops.softmax_ce_metrics(torch.zeros((0, 3), device=dev), torch.zeros(0, device=dev))
    with pytest.raises(ValueError, match="empty batch"):
        ops.softmax_ce_metrics(torch.zeros((3, 0), device=dev), torch.zeros(3, device=dev))
    with pytest.raises(ValueError, match="one value per node"):
        ops.softmax_ce_metrics(torch.zeros((4, 3), device=dev), torch.zeros(5, device=dev))
    with pytest.raises(ValueError, match="one value per node"):
        ops.softmax_ce_metrics(torch.zeros((4, 3), device=dev), torch.zeros((4, 3), device=dev))
    with pytest.raises(ValueError, match="one value per node"):
        ops.softmax_ce_metrics(torch.zeros((4, 3), device=dev), torch.zeros(4, device=dev), torch.zeros(3, device=dev))
    with pytest.raises(ValueError, match="2-D"):
        ops.softmax_ce_metrics(torch.zeros(4, device=dev), torch.zeros(4, device=dev))
    with pytest.raises(ValueError, match="out must be"):
        ops.softmax_ce_metrics(torch.zeros((4, 3), device=dev), torch.zeros(4, device=dev), out=torch.zeros((4, 2), device=dev))
    with pytest.raises(TypeError):
        ops.softmax_ce_metrics(torch.zeros((4, 3), device=dev, dtype=torch.float64), torch.zeros(4, device=dev))
    with pytest.raises(TypeError):
        ops.softmax_ce_metrics(torch.zeros((4, 3), device=dev), torch.zeros(4, device=dev),
                               torch.zeros(4, device=dev, dtype=torch.float64))
    # integer labels are cast once; [V, 1] labels and weights are columns
    x = torch.tensor([[2.0, 0.0, 1.0], [0.0, 0.0, 5.0], [1.0, 4.0, 1.0], [0.5, 0.5, 0.0]], device=dev)
    y = torch.tensor([0, 1, -1, 0], device=dev)
    metrics, counts, grad, pred = ops.softmax_ce_metrics(x, y.view(4, 1), torch.ones((4, 1), device=dev), want_pred=True)
    ref = softmax_ce(x.cpu().numpy(), y.cpu().numpy())
    assert counts.cpu().tolist() == [2, 3] == [ref.correct, ref.counted_nodes] and pred.cpu().tolist() == [0, 2, 1, 0]
    assert abs(float(metrics[0]) - ref.loss) <= 2e-6 * max(1.0, ref.loss) and grad.shape == (4, 3)
