"""Every kernel that draws a dropout mask against tests/dropout_reference.py - the numpy restatement of the generator text in
include/tfgnn.h - BIT FOR BIT: the flat kernel (``ops.dropout_forward``, ``ops.dropout_mask``, ``DropoutSpec.mask()``),
tfgnn_dropout_forward_sp at all four instantiations, the epoch word, and one case per consumer that recomputes the mask (the NT
product's epilogue in a forward and in a gradient product, tfgnn_gru_gates_backward_sp_dropout), so that each chain ends at the
host reference and not at another kernel.  No tolerances: ``np.array_equal`` / ``torch.equal`` throughout (values that hold a
NaN are compared as bit patterns of the non-NaN elements plus the NaN positions).

Not reached on the device: the high-word term of the hash (groups >= 2^32, tensors of more than 2^34 elements).  No entry takes
an index offset, and a tensor of that size is no test; tests/test_dropout_reference_host.py pins that term on the reference.

The NT product tiles N in 128, 256 or 320 columns and refuses every other width, so its four-wave family is taken at its
smallest width, N = 128, and the eight-wave family at N = 320."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dropout_reference as ref
from tests import gru_reference as gru
from tests import sp16_reference as sp16
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
STACK = 7 * 1000003
TOP_RATE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))  # 1 - 2^-24
GRID_CAP = 4096 * 256  # threads of the flat kernel's largest grid


@pytest.fixture(autouse=True)
def epoch_zero_and_mode_back_afterwards():
    from tf2_gnn_amd import ops

    mode = ops.get_gemm_mode()
    ops.dropout_epoch_set(0)  # (tests that replayed a captured step before this file leave it advanced)
    yield
    ops.dropout_epoch_set(0)  # every other test draws the masks of epoch 0
    torch.cuda.synchronize()
    assert ops.dropout_epoch() == 0
    ops.set_gemm_mode(mode)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want, what=""):
    """bit patterns equal; where ``want`` is a NaN, ``got`` is one (payload and sign of a NaN are the multiplier's business)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), what


def _times(x, m):
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return (np.asarray(x, dtype=np.float32) * np.asarray(m, dtype=np.float32)).astype(np.float32)


# ---- the flat kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, GRID_CAP + 7])
def test_flat_kernel_sizes(dev, n):
    """up to a ragged last group, and the smallest size with a second grid-stride trip (and a ragged group behind it)"""
    from tf2_gnn_amd import ops

    rate, seed = 0.1, STACK + 3
    want = ref.mask(n, rate, seed)
    x = torch.from_numpy(np.random.default_rng(n).standard_normal(n).astype(np.float32)).to(dev)
    y, mask = ops.dropout_forward(x, rate, seed)
    assert np.array_equal(_bits(mask.cpu().numpy()), _bits(want))
    _same_bits(y.cpu().numpy(), _times(x.cpu().numpy(), want))
    assert np.array_equal(_bits(ops.dropout_mask((n,), rate, seed, dev).cpu().numpy()), _bits(want))
    if n > GRID_CAP:
        assert not np.array_equal(want[:7], want[GRID_CAP:GRID_CAP + 7]), "the second trip has masks of its own"


FLAT_CASES = [  # (rate, seed, epoch): every rate, seed and epoch of tests/test_dropout_reference_host.py, the edges of each
    (0.003, 0, 0), (0.05, 1, 1), (0.1, 2, 2), (0.2, 1000003, 3), (0.5, 1000004, 7), (0.9, 1 << 63, M32), (0.1, M64, 0),
    (0.25, STACK + 1, 0), (0.125, STACK + 2, 1), (0.1, STACK + 1, 0), (0.1, STACK + 2, 0), (0.1, 0, M32), (0.2, 1, 0),
    (0.9, 2, 1), (0.5, M64, M32), (0.003, 1 << 63, 7), (2.0 ** -24, 5, 0), (2.0 ** -24, 5, 3), (0.0, 5, 0), (0.0, M64, 2),
    (TOP_RATE, 5, 0), (TOP_RATE, 11, M32)]


@pytest.mark.parametrize("rate,seed,epoch", FLAT_CASES)
def test_flat_kernel_argument_cases(dev, rate, seed, epoch):
    from tf2_gnn_amd import ops

    n = 64 * 1024 + 3
    want = ref.mask(n, rate, seed, epoch)
    ops.dropout_epoch_set(epoch)
    got = ops.dropout_mask((n,), rate, seed, dev).cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    # exactly 0 or the float32 scale
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
    assert set(np.unique(_bits(got)).tolist()) <= {0, int(_bits(scale).reshape(-1)[0])}
    if rate == 0.0:
        assert (got == 1.0).all()
    if rate == TOP_RATE:
        assert float(scale) == 2.0 ** 24
    spec = ops.DropoutSpec(rate, seed, (n // 4, 4), dev)
    assert np.array_equal(_bits(spec.mask().cpu().numpy().reshape(-1)), _bits(want[:4 * (n // 4)]))


def _special_x(n):
    x = np.random.default_rng(3).standard_normal(n).astype(np.float32)
    x[0:64:4] = -0.0
    x[1:64:4] = np.float32(1e-41)  # a denormal
    x[2:64:8] = np.inf
    x[6:64:8] = -np.inf
    x[3:64:4] = np.nan
    return x


def test_flat_kernel_call_forms(dev):
    from tf2_gnn_amd import _lib, ops

    n, rate, seed = 1031, 0.2, 77
    want = ref.mask(n, rate, seed)
    xh = _special_x(n)
    inf = np.isinf(xh)
    assert (want[inf] == 0).any() and (want[inf] != 0).any(), "the case must drop an inf and keep one"
    x = torch.from_numpy(xh).to(dev)
    y, mask = ops.dropout_forward(x, rate, seed)
    yh = y.cpu().numpy()
    assert np.array_equal(_bits(mask.cpu().numpy()), _bits(want))
    _same_bits(yh, _times(xh, want), "y = x * mask")
    assert np.isnan(yh[inf & (want == 0)]).all() and np.isinf(yh[inf & (want != 0)]).all()  # a dropped inf is NaN: tf.nn.dropout
    # the denormal is scaled, not flushed; a dropped -0 stays -0
    den = np.flatnonzero((xh == np.float32(1e-41)) & (want != 0))
    assert den.size and (yh[den] != 0).all()
    # without the mask, and the mask alone
    y2, none = ops.dropout_forward(x, rate, seed, want_mask=False)
    assert none is None and np.array_equal(_bits(y2.cpu().numpy()), _bits(yh))
    assert np.array_equal(_bits(ops.dropout_mask((n,), rate, seed, dev).cpu().numpy()), _bits(want))
    # a view whose pointers are not 16-byte aligned: the index is the element's position in the CALL
    m = n - 1
    want_v = ref.mask(m, rate, seed)
    yv, mv = ops.dropout_forward(x[1:], rate, seed)
    assert x[1:].data_ptr() % 16 == 4
    assert np.array_equal(_bits(mv.cpu().numpy()), _bits(want_v))
    _same_bits(yv.cpu().numpy(), _times(xh[1:], want_v), "view")
    ybuf, mbuf = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    p = ops._ptr
    _lib.check(_lib.load().tfgnn_dropout_forward(p(x[1:]), p(ybuf[1:]), p(mbuf[1:]), m, rate, seed, ops._stream()))
    assert np.array_equal(_bits(mbuf[1:].cpu().numpy()), _bits(want_v)) and float(mbuf[0]) == 7.0 and float(ybuf[0]) == 7.0
    _same_bits(ybuf[1:].cpu().numpy(), _times(xh[1:], want_v), "view, all three pointers")


# ---- tfgnn_dropout_forward_sp -------------------------------------------------------------------------------------------
def _sp_direct(dev, x, rate, seed, want_mask=True):
    """tfgnn_dropout_forward_sp through ctypes -> (y, mask | None, SP16 bytes [rows, 4 cols], inverse scales [rows])"""
    from tf2_gnn_amd import _lib, ops

    rows, cols = x.shape
    y = torch.full_like(x, 7.0)
    mask = torch.full_like(x, 7.0) if want_mask else None
    data = torch.full((rows, 4 * cols), 0xEE, dtype=torch.uint8, device=dev)
    inv = torch.full((rows,), 7.0, device=dev)
    p = ops._ptr
    _lib.check(_lib.load().tfgnn_dropout_forward_sp(p(x), p(y), p(mask), rows, cols, rate, seed, p(data), 4 * cols, p(inv), ops._stream()))
    return y, mask, data, inv


def _check_sp(xh, rate, seed, epoch, y, mask, data, inv, what):
    rows, cols = xh.shape
    want = ref.mask((rows, cols), rate, seed, epoch)
    if mask is not None:
        assert np.array_equal(_bits(mask.cpu().numpy()), _bits(want)), what
    yh = y.cpu().numpy()
    _same_bits(yh, _times(xh, want), what)
    h, l, inv_ref = sp16.encode(yh, cols)  # one scale per row
    assert np.array_equal(_bits(inv.cpu().numpy().reshape(rows)), _bits(inv_ref.reshape(rows))), what
    # byte for byte, but for the sign of a zero: y holds -0 wherever a negative x was dropped, and the format leaves the sign of
    # a zero h or l open (tests/sp16_reference.py: the device writes h = +0, l = -0 there, the model h = -0, l = +0)
    got_bytes = data.cpu().numpy()[:, :4 * cols]
    assert np.array_equal(sp16.without_zero_signs(got_bytes), sp16.without_zero_signs(sp16.pack(h, l))), what
    return want, yh, inv_ref.reshape(rows)


SP_COLS = [16, 32, 128, 144, 256, 320, 336, 512]  # VPL 2, 2, 2, 4 (dead slots), 4, 5, 8 (dead slots), 8
SP_ROWS = [1, 16, 17, 33]


@pytest.mark.parametrize("cols", SP_COLS)
def test_sp_kernel_y_mask_and_operand(dev, cols):
    from tf2_gnn_amd import ops

    ops.set_gemm_mode("f16x2")
    rate, seed = 0.2, STACK + 5
    for rows in SP_ROWS:
        xh = (np.random.default_rng(cols + rows).standard_normal((rows, cols)) * np.exp(
            3.0 * np.random.default_rng(rows).standard_normal((rows, 1)))).astype(np.float32)
        x = torch.from_numpy(xh).to(dev)
        if cols == 16:  # ``ops.dropout_forward`` takes this width to the flat kernel
            y, mask, data, inv = _sp_direct(dev, x, rate, seed)
        else:
            y, mask = ops.dropout_forward(x, rate, seed)
            hit = ops._sp_rows_memo.get(id(y))
            assert hit is not None and hit[0]() is y, "the dropout kernel wrote no operand"
            op = hit[2]
            assert (op.rows, op.cols, op.scale_block) == (rows, cols, cols)
            data, inv = op.data, op.inv_scale
        _check_sp(xh, rate, seed, 0, y, mask, data, inv, (rows, cols))


def test_sp_kernel_without_a_mask_at_an_epoch_and_special_rows(dev):
    """NULL mask; epoch 3; a row that drops to all zeros (inverse scale 2^-126, the marker of an all-zero row), a row of zeros, a
    row holding a NaN and one holding a dropped inf (scale 1, as tests/sp16_reference.py states the rule)"""
    from tf2_gnn_amd import ops

    rows, cols, rate, seed = 17, 144, 0.5, 4242
    want = ref.mask((rows, cols), rate, seed, 3)
    xh = np.random.default_rng(8).standard_normal((rows, cols)).astype(np.float32)
    xh[2] = np.where(want[2] == 0, xh[2], 0.0)      # what is kept of row 2 is zero
    xh[4] = 0.0
    xh[6, 9] = np.nan
    drop9 = int(np.flatnonzero(want[9] == 0)[0])
    xh[9, drop9] = np.inf
    assert np.abs(xh[2]).max() > 0
    x = torch.from_numpy(xh).to(dev)
    ops.dropout_epoch_set(3)
    y, none, data, inv = _sp_direct(dev, x, rate, seed, want_mask=False)
    assert none is None
    _, yh, inv_ref = _check_sp(xh, rate, seed, 3, y, None, data, inv, "special rows")
    assert (yh[2] == 0).all() and (yh[4] == 0).all() and inv_ref[2] == inv_ref[4] == np.float32(2.0 ** -126)
    assert np.isnan(yh[9, drop9]) and inv_ref[6] == inv_ref[9] == 1.0
    y2, mask2, data2, inv2 = _sp_direct(dev, x, rate, seed)  # the stored mask changes nothing else
    assert np.array_equal(_bits(mask2.cpu().numpy()), _bits(want))
    assert torch.equal(data2, data) and torch.equal(inv2, inv)
    _same_bits(y2.cpu().numpy(), yh)
    # everything dropped: every row carries the marker
    yz, _, dz, iz = _sp_direct(dev, torch.from_numpy(np.abs(xh[:5, :32]) + 1).to(dev).contiguous(), TOP_RATE, 1)
    assert ref.mask((5, 32), TOP_RATE, 1, 3).max() == 0
    assert not bool(yz.any()) and not bool(dz.any()) and bool((iz == 2.0 ** -126).all())


# ---- the epoch ----------------------------------------------------------------------------------------------------------
def test_epoch_set_advance_get_and_wrap(dev):
    from tf2_gnn_amd import ops

    shape, rate, seed = (33, 20), 0.1, STACK + 1
    ops.dropout_epoch_set(0)
    assert ops.dropout_epoch() == 0
    ops.dropout_epoch_advance()
    assert ops.dropout_epoch() == 1
    assert np.array_equal(_bits(ops.dropout_mask(shape, rate, seed, dev).cpu().numpy()), _bits(ref.mask(shape, rate, seed, 1)))
    ops.dropout_epoch_set(6)
    ops.dropout_epoch_advance()
    assert ops.dropout_epoch() == 7
    m7 = ops.dropout_mask(shape, rate, seed, dev).cpu().numpy()
    assert np.array_equal(_bits(m7), _bits(ref.mask(shape, rate, seed, 7)))
    ops.dropout_epoch_set(M32)
    assert ops.dropout_epoch() == M32
    assert np.array_equal(_bits(ops.dropout_mask(shape, rate, seed, dev).cpu().numpy()), _bits(ref.mask(shape, rate, seed, M32)))
    ops.dropout_epoch_advance()
    assert ops.dropout_epoch() == 0
    m0 = ops.dropout_mask(shape, rate, seed, dev).cpu().numpy()
    assert np.array_equal(_bits(m0), _bits(ref.mask(shape, rate, seed, 0))) and not np.array_equal(m0, m7)


# ---- the consumers ------------------------------------------------------------------------------------------------------
def _operands(dev, M, N, K, seed):
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(seed)
    a = ops.sp_split_rows(torch.randn((M, K), generator=g).to(dev))
    b = ops.sp_split_cols((torch.randn((K, N), generator=g) * 0.2).to(dev))
    return a, b


def _dev_mask(dev, shape, rate, seed, epoch=0):
    return torch.from_numpy(ref.mask(shape, rate, seed, epoch)).to(dev)


@pytest.mark.parametrize("N", [128, 320])
def test_nt_product_epilogue_forward(dev, N):
    """plain, through a permuting row map (the mask follows the OUTPUT row), and at epoch 3"""
    from tf2_gnn_amd import ops

    M, K, rate, seed = 130, 64, 0.2, 77
    a, b = _operands(dev, M, N, K, N)
    plain = ops.sp_gemm_nt(a, b, act="relu")
    assert 0.2 < float((plain > 0).float().mean()) < 0.8
    got = ops.sp_gemm_nt(a, b, act="relu", dropout=(rate, seed))
    assert torch.equal(got, plain * _dev_mask(dev, (M, N), rate, seed))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(M).astype(np.int32)).to(dev)
    plain_p = ops.sp_gemm_nt(a, b, act="relu", row_map=perm)
    assert torch.equal(plain_p[perm.long()], plain) and not torch.equal(plain_p, plain)
    got_p = ops.sp_gemm_nt(a, b, act="relu", dropout=(rate, seed), row_map=perm)
    assert torch.equal(got_p, plain_p * _dev_mask(dev, (M, N), rate, seed))
    ops.dropout_epoch_set(3)
    got_3 = ops.sp_gemm_nt(a, b, act="relu", dropout=(rate, seed))
    assert torch.equal(got_3, plain * _dev_mask(dev, (M, N), rate, seed, 3)) and not torch.equal(got_3, got)


def test_nt_product_refuses_a_width_it_does_not_tile(dev):
    from tf2_gnn_amd import _lib, ops

    a, b = _operands(dev, 130, 64, 64, 1)
    with pytest.raises(_lib.TfgnnError):
        ops.sp_gemm_nt(a, b, act="relu", dropout=(0.2, 77))


@pytest.mark.parametrize("N", [128, 320])
def test_nt_product_epilogue_gradient(dev, N):
    """a gradient product recomputes the forward mask: act'(saved) first, then the mask"""
    from tf2_gnn_amd import ops

    M, K, rate, seed = 130, 64, 0.25, 9
    a, b = _operands(dev, M, N, K, N + 1)
    saved = torch.randn((M, N), generator=torch.Generator().manual_seed(4)).to(dev)
    plain = ops.sp_gemm_nt(a, b, act_grad=("relu", saved))
    assert torch.equal(plain != 0, (saved > 0) & (ops.sp_gemm_nt(a, b) != 0))
    got = ops.sp_gemm_nt(a, b, act_grad=("relu", saved), dropout=(rate, seed))
    assert torch.equal(got, plain * _dev_mask(dev, (M, N), rate, seed))
    assert torch.equal(got != 0, (plain != 0) & (_dev_mask(dev, (M, N), rate, seed) != 0))


def test_gru_gate_gradient_recomputes_the_mask(dev):
    from tf2_gnn_amd import ops

    V, H, rate, seed = 33, 64, 0.25, STACK + 2
    g = torch.Generator().manual_seed(12)
    mx, mh = torch.randn((V, 3 * H), generator=g), torch.randn((V, 3 * H), generator=g)
    h, dh_new = torch.randn((V, H), generator=g), torch.randn((V, H), generator=g)
    args = [t.to(dev) for t in (mx, mh, h, dh_new)]
    _, gates = ops.gru_gates_forward(args[0], args[1], args[2])
    call = (args[3], gates, args[1], args[2])
    base = ops.gru_gates_backward_sp(*call)
    assert bool((base[2] != 0).all())
    for epoch in (0, 3):
        ops.dropout_epoch_set(epoch)
        want = ref.mask((V, H), rate, seed, epoch)
        got = ops.gru_gates_backward_sp(*call, out_mul=ops.DropoutSpec(rate, seed, (V, H), dev))
        dh = got[2]
        assert np.array_equal(dh.cpu().numpy() == 0, want == 0), epoch                    # the zero pattern
        assert torch.equal(dh, base[2] * torch.from_numpy(want).to(dev)), epoch              # and the factor where it is not zero
        assert_close(dh.cpu(), gru.gru_backward(dh_new, gates, mh, h, factor=torch.from_numpy(want))[2], tol=5e-6,
                     what="gru gates bwd sp dh, reference mask")
        assert torch.equal(got[0].data, base[0].data) and torch.equal(got[1].data, base[1].data) and torch.equal(got[3], base[3])
