"""The GRUCell gate kernels of csrc/elementwise.hip, op by op, against the fp64 closed form of tests/gru_reference.py:
``ops.gru_gates_forward`` / ``ops.gru_gates_backward`` at production widths, and every template instance of the split-operand
gate-gradient kernel (``ops.gru_gates_backward_sp``: six gate gradients, one power-of-two scale per row, dmx / dmh written ONLY as
SP16 operands, the bias gradients as per-wave column sums, an optional factor of dh_direct) - decoded, and as the products that
consume it read it.

Inputs: mx and mh are N(0, 1) times a per-row factor exp(3 N(0, 1)) (one draw per tensor and row): the row scales of the gate
gradients spread over many binades and part of the gates saturate to exactly 0 or 1 in fp32.  The backward reference takes the
fp32 gates the forward KERNEL stored, cast up: their rounding is not part of the comparison."""
import functools

import numpy as np
import pytest
import torch

from tests import gru_reference as gru
from tests.helpers import assert_close, decode_sp16, record_parity

pytestmark = pytest.mark.gpu

MARKER = 2.0 ** -126           # the scale sp_scale_for_max gives an all-zero row (csrc/sp16.hpp)
SCALE_FLOOR = 2.0 ** -112      # below this row maximum the scale exponent is clamped: mx * s < 2^14
WIDTHS = (64, 128, 192, 256, 320, 384, 448, 512)   # every instance of gru_gates_backward_sp_kernel<UPL>, UPL = H / 64
SMALL_V = (1, 3, 4, 5, 255, 256, 1031)             # V < 4: waves without a row; 1031: 20 waves
SP_CASES = [(257, H) for H in WIDTHS] + [(V, H) for H in (64, 192) for V in SMALL_V]


class Case:
    """Seeded inputs of one (V, H) on the device, the gates the forward kernel stored, and the fp64 references - built once
    and shared; tests clone what they change."""

    def __init__(self, V, H, dev):
        from tf2_gnn_amd import ops

        g = torch.Generator().manual_seed(1000 * H + V)
        self.V, self.H = V, H
        mx = torch.randn((V, 3 * H), generator=g) * torch.exp(torch.randn((V, 1), generator=g) * 3.0)
        mh = torch.randn((V, 3 * H), generator=g) * torch.exp(torch.randn((V, 1), generator=g) * 3.0)
        h = torch.randn((V, H), generator=g)
        dh_new = torch.randn((V, H), generator=g)
        self.cpu = (mx, mh, h, dh_new)
        self.mx, self.mh, self.h, self.dh_new = (t.to(dev) for t in self.cpu)
        self.h_new, self.gates = ops.gru_gates_forward(self.mx, self.mh, self.h)
        self.fwd_ref = gru.gru_forward(mx, mh, h)
        self.bwd_ref = gru.gru_backward(dh_new, self.gates, mh, h)


@functools.lru_cache(maxsize=None)
def _case(V, H, dev):
    return Case(V, H, dev)


def _same_operand(a, b):
    return torch.equal(a.data, b.data) and torch.equal(a.inv_scale, b.inv_scale)


def _rows_equal_except(a, b, row):
    keep = torch.ones(a.rows, dtype=torch.bool, device=a.data.device)
    keep[row] = False
    return torch.equal(a.data[keep], b.data[keep]) and torch.equal(a.inv_scale[keep], b.inv_scale[keep])


# ---- a. the fp32 kernels at real widths ---------------------------------------------------------------------------------
FP32_SHAPES = [(1, 64), (5, 12), (257, 128), (130, 320), (67, 513)]


@pytest.mark.parametrize("V,H", FP32_SHAPES)
def test_forward_matches_fp64(dev, V, H):
    """h' and the stored gates, and the same h' bits without the gates: rows v = i / H at widths above, at and off the 64 lanes"""
    from tf2_gnn_amd import ops

    c = _case(V, H, dev)
    h_ref, gates_ref = c.fwd_ref
    assert_close(c.h_new.cpu(), h_ref, tol=2e-6, what="gru gates fwd h'")
    assert_close(c.gates.cpu(), gates_ref, tol=2e-6, what="gru gates fwd gates")
    sat = c.gates[:, :2 * H]
    if V * H >= 1000:
        assert bool(((sat == 0) | (sat == 1)).any()), "no saturated gate in this draw"
    h_only, none = ops.gru_gates_forward(c.mx, c.mh, c.h, save_gates=False)
    assert none is None and torch.equal(h_only, c.h_new)


@pytest.mark.parametrize("V,H", FP32_SHAPES)
def test_backward_matches_fp64(dev, V, H):
    from tf2_gnn_amd import ops

    c = _case(V, H, dev)
    dmx_ref, dmh_ref, dh_ref, _ = c.bwd_ref
    dmx, dmh, dh = ops.gru_gates_backward(c.dh_new, c.gates, c.mh, c.h)
    assert_close(dmx.cpu(), dmx_ref, tol=5e-6, what="gru gates bwd dmx")
    assert_close(dmh.cpu(), dmh_ref, tol=5e-6, what="gru gates bwd dmh")
    assert_close(dh.cpu(), dh_ref, tol=5e-6, what="gru gates bwd dh")


# ---- b. the split-operand kernel, every instance ------------------------------------------------------------------------
def _check_operand(op, ref, what):
    """decoded values within the fp32 kernel's tolerance plus the format's own bound (test_split_rows_reconstructs); scales are
    powers of two; a row with a finite non-zero maximum is scaled into [2^14, 2^15] (csrc/sp16.hpp sp_scale_for_max; below
    2^-112 the exponent is clamped and the row carries the smallest scale)."""
    V, C = ref.shape
    assert (op.rows, op.cols, op.scale_block) == (V, C, C) and tuple(op.inv_scale.shape) == (V, 1)
    rec = decode_sp16(op)
    ref = ref.numpy()
    rowmax = np.abs(ref).max(axis=1, keepdims=True)
    err = np.abs(rec - ref)
    bound = 5e-6 * np.maximum(1.0, np.abs(ref)) + np.maximum(np.abs(ref) * 2.0 ** -22, rowmax * 2.0 ** -38)
    worst = float((err / bound).max())
    record_parity(f"gru gates bwd sp {what}", max_error_over_bound=worst, bound=1.0)
    assert worst <= 1.0, (what, worst, float(err.max()))
    inv = op.inv_scale.cpu().numpy().astype(np.float64).reshape(V)
    m, _ = np.frexp(inv)
    assert np.all(m == 0.5), "scales must be powers of two"
    scaled = np.abs(rec).max(axis=1) / inv
    normal = rowmax.reshape(V) >= 2 * SCALE_FLOOR
    assert np.all((scaled[normal] >= 2.0 ** 14) & (scaled[normal] <= 2.0 ** 15)), (what, scaled[normal].min(), scaled[normal].max())
    tiny = rowmax.reshape(V) < SCALE_FLOOR / 2
    assert np.all(inv[tiny] == MARKER)


def _check_bias(bias_grad, dmx_ref, dmh_ref, what):
    """the bound of test_colsum_bias_gradient_sums: 2e-6 of sum |x| per column"""
    H3 = dmx_ref.shape[1]
    assert tuple(bias_grad.shape) == (2, H3)
    ref = torch.stack([dmx_ref.sum(dim=0), dmh_ref.sum(dim=0)])
    mag = torch.stack([dmx_ref.abs().sum(dim=0), dmh_ref.abs().sum(dim=0)]).clamp(min=1e-30)
    worst = float(((bias_grad.cpu().double() - ref).abs() / mag).max())
    record_parity(f"gru gates bwd sp bias {what}", max_error_over_sum_abs=worst, bound=2e-6)
    assert worst <= 2e-6, (what, worst)


@pytest.mark.parametrize("V,H", SP_CASES)
def test_split_operand_kernel_matches_fp64(dev, V, H):
    from tf2_gnn_amd import ops

    c = _case(V, H, dev)
    dmx_ref, dmh_ref, dh_ref, _ = c.bwd_ref
    dmx_sp, dmh_sp, dh, bias_grad = ops.gru_gates_backward_sp(c.dh_new, c.gates, c.mh, c.h)
    _check_operand(dmx_sp, dmx_ref, "dmx")
    _check_operand(dmh_sp, dmh_ref, "dmh")
    assert_close(dh.cpu(), dh_ref, tol=5e-6, what="gru gates bwd sp dh")
    _check_bias(bias_grad, dmx_ref, dmh_ref, f"H={H}")
    again = ops.gru_gates_backward_sp(c.dh_new, c.gates, c.mh, c.h)
    assert torch.equal(again[3], bias_grad), "the waves are added in a fixed order"
    assert _same_operand(again[0], dmx_sp) and _same_operand(again[1], dmh_sp) and torch.equal(again[2], dh)


@pytest.mark.parametrize("H", WIDTHS)
def test_c_entry_writes_every_byte_it_returns(dev, H):
    """tfgnn_gru_gates_backward_sp called directly on outputs and a workspace full of NaN: the results of the ``ops`` call, bit for
    bit - nothing that is read afterwards was left as it was found."""
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    V = 257
    c = _case(V, H, dev)
    want = ops.gru_gates_backward_sp(c.dh_new, c.gates, c.mh, c.h)
    nan = float("nan")
    sp = [torch.full((V, 3 * H * 4), 0xFF, dtype=torch.uint8, device=dev) for _ in range(2)]  # fp16 0xffff: a NaN
    inv = [torch.full((V, 1), nan, device=dev) for _ in range(2)]
    dh = torch.full((V, H), nan, device=dev)
    bias_grad = torch.full((2, 3 * H), nan, device=dev)
    ws_bytes = lib.tfgnn_gru_gates_backward_sp_workspace_bytes(V, H)
    assert ws_bytes == 8 * 6 * H * 4  # 257 rows: 8 waves
    ws = torch.full((ws_bytes // 4,), nan, device=dev)
    p = ops._ptr
    _lib.check(lib.tfgnn_gru_gates_backward_sp(p(c.dh_new), p(c.gates), p(c.mh), p(c.h), p(sp[0]), p(inv[0]), p(sp[1]), p(inv[1]), p(dh),
                                               None, p(bias_grad), V, H, p(ws), ws_bytes, ops._stream()))
    torch.cuda.synchronize()
    for k in range(2):
        assert torch.equal(sp[k], want[k].data) and torch.equal(inv[k], want[k].inv_scale), k
    assert torch.equal(dh, want[2]) and torch.equal(bias_grad, want[3])
    assert bool(torch.isfinite(ws).all())
    # a workspace one float short is refused before anything is launched
    assert lib.tfgnn_gru_gates_backward_sp(p(c.dh_new), p(c.gates), p(c.mh), p(c.h), p(sp[0]), p(inv[0]), p(sp[1]), p(inv[1]), p(dh),
                                           None, p(bias_grad), V, H, p(ws), ws_bytes - 4, ops._stream()) == -1


# ---- c. the factor of dh_direct -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,H", [(257, 64), (257, 192)])
def test_factor_of_dh_direct(dev, V, H):
    """A stored mask and a DropoutSpec (the mask recomputed from (rate, seed, epoch)) multiply dh_direct alone."""
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    c = _case(V, H, dev)
    rate, seed = 0.25, 77
    args = (c.dh_new, c.gates, c.mh, c.h)
    base = ops.gru_gates_backward_sp(*args)
    masks = []
    try:
        for epoch in (0, 5):
            ops.dropout_epoch_set(epoch)
            mask = ops.dropout_mask((V, H), rate, seed, dev)
            masks.append(mask)
            kept = float((mask != 0).float().mean())
            assert abs(kept - (1 - rate)) < 0.05 and bool(((mask == 0) | ((mask - 1 / (1 - rate)).abs() < 1e-6)).all())
            for out_mul in (mask, ops.DropoutSpec(rate, seed, (V, H), dev)):
                got = ops.gru_gates_backward_sp(*args, out_mul=out_mul)
                assert torch.equal(got[2], base[2] * mask), (epoch, type(out_mul).__name__)
                assert _same_operand(got[0], base[0]) and _same_operand(got[1], base[1]) and torch.equal(got[3], base[3])
        assert not torch.equal(masks[0], masks[1]), "the epoch is part of the mask"
        # the mask stored at epoch 0 stays what it is at epoch 5
        got = ops.gru_gates_backward_sp(*args, out_mul=masks[0])
        assert torch.equal(got[2], base[2] * masks[0])
    finally:
        ops.dropout_epoch_set(0)
    with pytest.raises(ValueError):
        ops.gru_gates_backward_sp(*args, out_mul=ops.DropoutSpec(rate, seed, (V, H + 64), dev))
    with pytest.raises(ValueError):
        ops.gru_gates_backward_sp(*args, out_mul=ops.DropoutSpec(rate, seed, (V + 1, H), dev))
    # The C entries: a stored mask goes to tfgnn_gru_gates_backward_sp, which takes no rate, a rate to ..._sp_dropout, which takes no
    # mask - the two cannot meet in one call; what the entry with a rate can be handed wrongly is a rate outside [0, 1)
    p = ops._ptr
    out = ops.gru_gates_backward_sp(*args)
    ws_bytes = lib.tfgnn_gru_gates_backward_sp_workspace_bytes(V, H)
    ws = torch.empty(ws_bytes // 4, device=dev)
    for bad in (1.0, -0.5):
        rc = lib.tfgnn_gru_gates_backward_sp_dropout(p(c.dh_new), p(c.gates), p(c.mh), p(c.h), p(out[0].data), p(out[0].inv_scale),
                                                     p(out[1].data), p(out[1].inv_scale), p(out[2]), bad, seed, p(out[3]), V, H, p(ws),
                                                     ws_bytes, ops._stream())
        assert rc == -1, bad
    torch.cuda.synchronize()
    assert _same_operand(out[0], base[0]) and torch.equal(out[2], base[2]) and torch.equal(out[3], base[3])  # nothing was launched


# ---- d. edges -----------------------------------------------------------------------------------------------------------
def test_widths_without_a_kernel_and_no_rows(dev):
    from tf2_gnn_amd import ops

    for H in (96, 576):
        z = torch.zeros((4, H), device=dev)
        assert ops.gru_gates_backward_sp(z, torch.zeros((4, 3 * H), device=dev), torch.zeros((4, 3 * H), device=dev), z) is None
    for H in (64, 320):
        e, e3 = torch.empty((0, H), device=dev), torch.empty((0, 3 * H), device=dev)
        dmx_sp, dmh_sp, dh, bias_grad = ops.gru_gates_backward_sp(e, e3, e3, e)
        assert dmx_sp.rows == dmh_sp.rows == 0 and tuple(dh.shape) == (0, H)
        assert tuple(bias_grad.shape) == (2, 3 * H) and not bool(bias_grad.any())


@pytest.mark.parametrize("H", [64, 192])
def test_row_without_gradient_carries_the_marker_scale(dev, H):
    """dh_new == 0 in one row: zeros under the scale of an all-zero row (what sp_split_rows gives one), nothing in the bias
    gradient - whatever that row's state and gates are"""
    from tf2_gnn_amd import ops

    V, row = 257, 37
    c = _case(V, H, dev)
    dh_new = c.dh_new.clone()
    dh_new[row] = 0.0
    dmx_sp, dmh_sp, dh, bias_grad = ops.gru_gates_backward_sp(dh_new, c.gates, c.mh, c.h)
    marker = ops.sp_split_rows(torch.zeros((1, 3 * H), device=dev)).inv_scale.view(-1)
    assert float(marker) == MARKER
    for op in (dmx_sp, dmh_sp):
        assert torch.equal(op.inv_scale[row], marker)
        assert not bool(decode_sp16(op)[row].any())
    assert not bool(dh[row].any())
    dmx_ref, dmh_ref, _, _ = gru.gru_backward(dh_new, c.gates, c.mh, c.h)
    _check_operand(dmx_sp, dmx_ref, "dmx, zero row")
    _check_operand(dmh_sp, dmh_ref, "dmh, zero row")
    _check_bias(bias_grad, dmx_ref, dmh_ref, f"zero row H={H}")
    # other gates, candidate pre-activation and state in that row: adding its zeros changes no bit of the sums
    gates, mh, h = c.gates.clone(), c.mh.clone(), c.h.clone()
    gates[row], mh[row], h[row] = 0.5, 3.0, -2.0
    other = ops.gru_gates_backward_sp(dh_new, gates, mh, h)
    assert torch.equal(other[3], bias_grad)
    for a, b in ((other[0], dmx_sp), (other[1], dmh_sp)):  # (the zeros of the row may differ in sign)
        assert _rows_equal_except(a, b, row) and torch.equal(a.inv_scale, b.inv_scale) and not bool(decode_sp16(a)[row].any())


@pytest.mark.parametrize("H", [64, 192])
def test_special_values_in_the_incoming_gradient(dev, H):
    """A row of +inf: scale 1 and non-finite entries in that row only.  One NaN element: NaN exactly where the fp32 kernel has
    NaN.  A row of NaN (every row of a diverged step): scale 1 - NOT the marker of an all-zero row, which would make the
    weight-gradient product skip the row and return finite gradients - and NaN entries."""
    from tf2_gnn_amd import ops

    V, row = 257, 100
    c = _case(V, H, dev)
    base = ops.gru_gates_backward_sp(c.dh_new, c.gates, c.mh, c.h)
    one = torch.ones(1, device=dev)

    dh_new = c.dh_new.clone()
    dh_new[row] = float("inf")
    got = ops.gru_gates_backward_sp(dh_new, c.gates, c.mh, c.h)
    for k in range(2):
        assert torch.equal(got[k].inv_scale[row], one)
        rec = decode_sp16(got[k])
        assert not np.isfinite(rec[row]).any()
        assert _rows_equal_except(got[k], base[k], row) and np.isfinite(np.delete(rec, row, axis=0)).all()

    dh_new = c.dh_new.clone()
    dh_new[row, 5] = float("nan")
    got = ops.gru_gates_backward_sp(dh_new, c.gates, c.mh, c.h)
    dmx, dmh, dh = ops.gru_gates_backward(dh_new, c.gates, c.mh, c.h)
    assert int(torch.isnan(dmx).sum()) == 3 and int(torch.isnan(dmh).sum()) == 3
    for k, ref in ((0, dmx), (1, dmh)):
        assert np.array_equal(np.isnan(decode_sp16(got[k])), torch.isnan(ref).cpu().numpy())
        assert _rows_equal_except(got[k], base[k], row)
    assert torch.equal(torch.isnan(got[2]), torch.isnan(dh))
    assert torch.equal(torch.isnan(got[3]), torch.stack([torch.isnan(dmx).any(dim=0), torch.isnan(dmh).any(dim=0)]))

    dh_new = c.dh_new.clone()
    dh_new[row] = float("nan")
    got = ops.gru_gates_backward_sp(dh_new, c.gates, c.mh, c.h)
    for k in range(2):
        assert _rows_equal_except(got[k], base[k], row)
        assert np.isnan(decode_sp16(got[k])[row]).all()
        assert float(got[k].inv_scale[row]) == 1.0, "an all-NaN row must not carry the scale of an all-zero row"
    assert bool(torch.isnan(got[3]).all())


# ---- e. what the consumers read -----------------------------------------------------------------------------------------
def _product_error(got, ref, mag, floor=0.0):
    """largest |got - ref| - floor, relative to mag = sum |a||b| of the entry (an entry without magnitude must be within floor)"""
    return float((((got.cpu().double() - ref).abs() - floor).clamp(min=0.0) / mag.clamp(min=1e-300)).max())


def _column_ranges(N, tile_width):
    """(first column, count) ranges of a width the TN product tiles that together cover N columns: the whole operand where it
    tiles N itself (what the layer hands it), else overlapping 128- or 256-column ranges through ``b_cols``"""
    if tile_width(N):
        return [(0, N)]
    w = 128 if N < 256 else 256
    return [(c0, w) for c0 in range(0, N - w + 1, w)] + [(N - w, w)]


def _tn_by_ranges(ops, a_sp, b_sp):
    N = b_sp.cols
    out = torch.empty((a_sp.cols, N), device=a_sp.data.device)
    for c0, n in _column_ranges(N, ops.sp_tile_width):
        out[:, c0:c0 + n] = ops.sp_gemm_tn(a_sp, b_sp, b_cols=(c0, n))
    return out


@pytest.mark.parametrize("V,H", [(300, 64), (300, 192), (300, 128), (300, 320)])
def test_products_fed_with_the_kernel_operands(dev, V, H):
    """The two products GGNN._backward_f16x2 runs on the kernel's operands against the fp64 products of the reference gradients:
        d kernel = agg^T dmx                         tfgnn_sp_gemm_tn, K = V rows
        d h      = dh_direct + (dmh W_r^T) * mask    tfgnn_sp_gemm_nt accumulating, the mask recomputed in both kernels
    Bounds, relative to sum |a||b| per entry (plus |dh_direct| for the accumulating one), from tests/test_gpu_gemm_sp.py: 6e-7 for a
    TN product over rows on different scales (test_gemm_tn_matches_fp64, test_gemm_tn_row_count_not_a_multiple_of_the_tile), 4e-7
    for an NT product (test_gemm_nt_same_error_class_as_fp32_mfma, K = 1280 >= 3H).  Where one does not hold, the same product fed
    with sp_split_rows of the fp32 kernel's outputs is measured and twice its error allowed; both numbers are recorded.

    The products tile their N output columns in 128 / 256 / 320 (``ops.sp_tile_width``), and the layer takes this route only at
    widths they tile (``_f16x2_eligible``).  H = 64 and 192 are not such widths: the TN product then reads all 3H columns of dmx_sp
    through overlapping column ranges it does tile, and the NT product (N = H) must refuse - a missing kernel is an error, not
    another route.  H = 128 and 320 (the benchmark's) run both products exactly as the layer calls them."""
    from tf2_gnn_amd import _lib, ops

    c = _case(V, H, dev)
    g = torch.Generator().manual_seed(V + H)
    agg = torch.randn((V, H), generator=g) * torch.exp(torch.randn((V, 1), generator=g))
    Wr = torch.randn((H, 3 * H), generator=g) * 0.1
    agg_d, Wr_d = agg.to(dev), Wr.to(dev)
    rate, seed = 0.2, 5
    spec = ops.DropoutSpec(rate, seed, (V, H), dev)
    prev = ops.set_gemm_mode("f16x2")
    try:
        mask = ops.dropout_mask((V, H), rate, seed, dev)
        dmx_sp, dmh_sp, dh_direct, _ = ops.gru_gates_backward_sp(c.dh_new, c.gates, c.mh, c.h, out_mul=spec)
        dmx_ref, dmh_ref, dh_ref, _ = gru.gru_backward(c.dh_new, c.gates, c.mh, c.h, factor=mask)
        dmx32, dmh32, dh32 = ops.gru_gates_backward(c.dh_new, c.gates, c.mh, c.h)
        agg_sp, wr_sp = ops.sp_split_rows(agg_d), ops.sp_split_rows(Wr_d)

        # the weight gradient
        dW = _tn_by_ranges(ops, agg_sp, dmx_sp)
        ref = agg.double().t() @ dmx_ref
        mag = agg.double().abs().t() @ dmx_ref.abs()
        e = _product_error(dW, ref, mag)
        e_route = _product_error(_tn_by_ranges(ops, agg_sp, ops.sp_split_rows(dmx32)), ref, mag)
        record_parity(f"gru gates sp -> tn product H={H}", max_error_over_sum_abs=e, max_reference_route=e_route, bound=6e-7)
        print(f"tn H={H}: kernel operands {e:.3e}, split of the fp32 gradients {e_route:.3e} (of sum |a||b|)")
        assert e <= 6e-7 or e <= 2 * e_route, (e, e_route)

        # the state gradient
        if ops.sp_tile_width(H):
            dX = ops.sp_gemm_nt(dmh_sp, wr_sp, out=dh_direct.clone(), accumulate=True, out_mul=spec)
            m64 = mask.cpu().double()
            ref = dh_ref + (dmh_ref @ Wr.double().t()) * m64
            mag = dh_ref.abs() + (dmh_ref.abs() @ Wr.double().abs().t()) * m64
            # Saturated rows of these inputs have gate gradients down to fp32 subnormals (row maxima of 1e-38 .. 1e-43), and where z
            # is exactly 0 nothing else is added to their products.  Such entries have no relative precision to compare: a row whose
            # maximum is below 2^-112 is below the format's smallest scale and may drop out whole (csrc/sp16.hpp), and a result
            # below the smallest normal fp32 is rounded absolutely.  Both are absolute floors, from the formats alone.
            floor = 2.0 ** -112 * Wr.double().abs().sum(dim=1).unsqueeze(0) + 2.0 ** -126
            e = _product_error(dX, ref, mag, floor)
            route = ops.sp_gemm_nt(ops.sp_split_rows(dmh32), wr_sp, out=ops.mul(dh32, mask), accumulate=True, out_mul=spec)
            e_route = _product_error(route, ref, mag, floor)
            record_parity(f"gru gates sp -> nt product H={H}", max_error_over_sum_abs=e, max_reference_route=e_route, bound=4e-7)
            print(f"nt H={H}: kernel operands {e:.3e}, split of the fp32 gradients {e_route:.3e} (of sum |a||b| + |dh_direct|)")
            assert e <= 4e-7 or e <= 2 * e_route, (e, e_route)
        else:
            keep = dh_direct.clone()
            with pytest.raises(_lib.TfgnnError, match="status -4"):
                ops.sp_gemm_nt(dmh_sp, wr_sp, out=dh_direct, accumulate=True, out_mul=spec)
            torch.cuda.synchronize()
            assert torch.equal(dh_direct, keep)

        # a diverged row: the weight gradient says so, as the fp32 route does
        dh_new = c.dh_new.clone()
        dh_new[123] = float("nan")
        dmx_nan, _, _, _ = ops.gru_gates_backward_sp(dh_new, c.gates, c.mh, c.h)
        dmx32_nan, _, _ = ops.gru_gates_backward(dh_new, c.gates, c.mh, c.h)
        assert bool(torch.isnan(ops.gemm(agg_d, dmx32_nan, trans_a=True)).any())
        for c0, n in _column_ranges(3 * H, ops.sp_tile_width):
            assert bool(torch.isnan(ops.sp_gemm_tn(agg_sp, dmx_nan, b_cols=(c0, n))).any()), (c0, n)
    finally:
        ops.set_gemm_mode("f16x2")  # (clears a raised spread flag)
        ops.set_gemm_mode(prev)
