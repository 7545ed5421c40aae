"""RGAT's node-side kernels (csrc/rgat.hip), op by op against tests/rgat_reference.py (fp64 on the host): the five C entries
tfgnn_rgat_node_scores, _edge_dot, _scores_backward, _scores_backward_sp and _alpha_grad, called with raw pointers as the layer
calls them.  No graph object: ``coll`` is random int32 in [0, V*L), ``tgt`` random int32 in [0, V).

Which kernel a case runs (the dispatch of the entry points, restated in ``_vec_shape`` / ``_vec4`` below and asserted per list):
  node_scores  vec  : NODE_VEC (lpe = 1, lph = 1, a 16-lane and a full-wave reduction, 64 heads) at V = 1, 5, 67
               scalar: NODE_SCALAR at V = 67; the 4-byte-offset operand of (3,1,64); past the 16 384-block grid at V = 70 000
  edge_dot     vec  : EDGE_VEC x every residue of the 4-edge unroll and a ragged last lane group (E = 1 .. 1027)
               scalar: EDGE_SCALAR at E = 1027; the offset operand; past the grid at E = 70 000
  scores_bwd   vec  : SB_VEC;  scalar: SB_SCALAR, the offset operand, past the grid at V = 70 000
  scores_bwd_sp     : SP_SHAPES (C = 16 .. 2048, dead lanes at C = 2000) x V = 1 .. 67, the wrapped row loop at V = 32 800
  alpha_grad   partial vec: AG_VEC (LH = 1536: the column loop iterates);  partial scalar: AG_SCALAR and the offset workspace;
               final: every case - one block of nodes (V <= 16), parts that start past nblocks (V = 17 .. 1000), the 1024-block
               cap with and without empty trailing slices (V = 16 384 .. 20 000)

Every output buffer, the alpha-grad workspace, the SP16 data and the row scales carry one guard row of a sentinel behind their
last row; it must be untouched afterwards.

Two kinds of input per case.
  exact : integers of {-3..3} as fp32.  Every product and partial sum is an integer below 2^24 (9 n < 2^24 for the longest
          sum here, n = 70 000), so fp32 arithmetic is exact in any order, fused or not: the device result EQUALS the fp64
          reference.  A dropped, doubled or misplaced term at a tail, a block boundary or a lane-group edge shows here.
  normal: standard normal draws, one row scaled by 1e4 and one by 1e-4.  Bound per output element 1.01 n 2^-24 S, the gamma_n
          bound of an n-term fp32 sum in any order (n < 2^17), n = Hk (node_scores, edge_dot), V (alpha_grad), 3
          (scores_backward), S the fp64 magnitude sum of the reference.  Derived, not measured.  The worst error / bound per
          entry point is printed and recorded in the parity log (``max_error_over_bound``, bound 1)."""
import numpy as np
import pytest
import torch

from tests import rgat_reference as ref
from tests.helpers import record_parity
from tests.test_gpu_layers import check_rgat_backward

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5
SENTINEL_BYTE = 0xA5
KINDS = ("exact", "normal")
MARKER = 1.1754943508222875e-38  # 2^-126: the scale of an all-zero row (csrc/sp16.hpp)


# ---- the dispatch of the entry points, restated --------------------------------------------------------------------------------
def _vec_shape(K, H):
    """rgat_vec_shape: the lane-group kernels of node_scores / edge_dot"""
    if H % K or (H // K) % 4 or H % 4:
        return False
    lph, lpe = H // K // 4, H // 4
    return lph & (lph - 1) == 0 and lpe & (lpe - 1) == 0 and lpe <= 64


def _vec4(K, H):
    """the float4 forms of scores_backward and of alpha_grad's partial kernel"""
    return (H // K) % 4 == 0


# ---- inputs and buffers ---------------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _draw(kind, shape, gen, scale_rows=False):
    if kind == "exact":
        return torch.randint(-3, 4, shape, generator=gen).float()
    x = torch.randn(shape, generator=gen)
    if scale_rows and shape[0] >= 1:
        x[shape[0] // 3] *= 1e4
        if shape[0] >= 2:
            x[(2 * shape[0]) // 3 if shape[0] > 2 else 1] *= 1e-4
    return x


def _guarded(rows, cols, dev, init=None):
    buf = torch.full((rows + 1, cols), SENTINEL, dtype=torch.float32, device=dev)
    if init is not None:
        buf[:rows] = init.to(dev).reshape(rows, cols)
    return buf


def _off4(t):
    """the same values 4 bytes into a larger buffer: not 16-byte aligned"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _guard_untouched(buf, what):
    assert bool((buf[-1] == SENTINEL).all()), f"{what}: the guard row behind the last row was written"


def _untouched(buf, what):
    assert bool((buf == (SENTINEL_BYTE if buf.dtype == torch.uint8 else SENTINEL)).all()), f"{what} was written"


def _compare(entry, what, kind, got, want, S, n):
    """exact: equality with the fp64 reference; normal: error <= 1.01 n 2^-24 S per element, worst ratio printed and recorded"""
    got = got.detach().cpu().double().reshape(want.shape)
    assert bool(torch.isfinite(got).all()), f"{entry} {what}: non-finite output"
    if kind == "exact":
        bad = int((got != want).sum())
        assert torch.equal(got, want), f"{entry} {what}: {bad} of {want.numel()} elements differ from the exact result"
        return 0.0
    err = (got - want).abs()
    bound = ref.gamma_bound(n, S.reshape(want.shape))
    off_zero = torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err))  # S = 0: the result is an exact 0
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), off_zero)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{entry} {what}: max error / bound = {worst:.3e} (n = {n})")
    record_parity(entry, max_error_over_bound=worst, bound=1.0)
    assert worst <= 1.0, f"{entry} {what}: error {worst:.3f} x the bound 1.01 n 2^-24 S at element {int(ratio.argmax())}"
    return worst


def _lib_ops():
    from tf2_gnn_amd import _lib, ops

    return _lib.load(), ops


# =================================================================================================================================
# tfgnn_rgat_node_scores
# =================================================================================================================================
NODE_VEC = [(3, 1, 4), (2, 2, 8), (3, 1, 64), (2, 1, 256), (4, 8, 256), (1, 64, 256), (3, 8, 32)]
NODE_SCALAR = [(3, 3, 24), (3, 4, 24), (2, 1, 7), (2, 5, 40), (1, 64, 64), (2, 2, 512), (3, 8, 96)]


def test_case_lists_take_the_kernels_they_name():
    assert all(_vec_shape(K, H) for _, K, H in NODE_VEC) and not any(_vec_shape(K, H) for _, K, H in NODE_SCALAR)
    assert all(_vec_shape(K, H) for K, H in EDGE_VEC) and not any(_vec_shape(K, H) for K, H in EDGE_SCALAR)
    assert all(_vec4(K, H) for _, K, H in SB_VEC + AG_VEC + SP_SHAPES) and not any(_vec4(K, H) for _, K, H in SB_SCALAR + AG_SCALAR)
    # lane-group extremes of the node_scores list: lpe = 1, lph = 1, a full wave per row
    assert (3, 1, 4) in NODE_VEC and (2, 2, 8) in NODE_VEC and (2, 1, 256) in NODE_VEC
    assert 9 * 70000 < 2 ** 24  # the exact inputs stay exact at the longest sum


def _run_node_scores(dev, V, L, K, H, kind, off=None):
    lib, ops = _lib_ops()
    rows, Hk = V * L, H // K
    g = _gen(1, V, L, K, H, kind == "exact")
    Y = _draw(kind, (rows, H), g, scale_rows=True)
    alpha = _draw(kind, (L, K, 2 * Hk), g)
    Yd, ad = Y.to(dev), alpha.to(dev)
    if off == "Y":
        Yd = _off4(Yd)
    if off == "alpha":
        ad = _off4(ad)
    s_src, s_tgt = _guarded(rows, K, dev), _guarded(rows, K, dev)
    rc = lib.tfgnn_rgat_node_scores(ops._ptr(Yd), ops._ptr(ad), V, L, K, H, ops._ptr(s_src), ops._ptr(s_tgt), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"tfgnn_rgat_node_scores returned {rc}"
    return Y, alpha, s_src, s_tgt


def _check_node_scores(dev, V, L, K, H, kind, off=None):
    Y, alpha, s_src, s_tgt = _run_node_scores(dev, V, L, K, H, kind, off)
    rows = V * L
    want_s, want_t, S_s, S_t = ref.node_scores(Y, alpha, L, K)
    tag = f"(L,K,H)=({L},{K},{H}) V={V} {kind}" + (f" {off} offset" if off else "")
    _compare("tfgnn_rgat_node_scores", f"s_src {tag}", kind, s_src[:rows], want_s, S_s, H // K)
    _compare("tfgnn_rgat_node_scores", f"s_tgt {tag}", kind, s_tgt[:rows], want_t, S_t, H // K)
    _guard_untouched(s_src, f"node_scores s_src {tag}")
    _guard_untouched(s_tgt, f"node_scores s_tgt {tag}")
    return s_src, s_tgt


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", [1, 5, 67])
@pytest.mark.parametrize("L,K,H", NODE_VEC)
def test_node_scores_vec(dev, L, K, H, V, kind):
    _check_node_scores(dev, V, L, K, H, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,K,H", NODE_SCALAR)
def test_node_scores_scalar(dev, L, K, H, kind):
    _check_node_scores(dev, 67, L, K, H, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_node_scores_alignment_fallback(dev, kind):
    """Y (or alpha) 4 bytes into a buffer: the scalar kernel.  Both offsets run the same kernel on the same values: bit-equal."""
    L, K, H, V = 3, 1, 64, 67
    _check_node_scores(dev, V, L, K, H, kind)
    a_src, a_tgt = _check_node_scores(dev, V, L, K, H, kind, off="Y")
    b_src, b_tgt = _check_node_scores(dev, V, L, K, H, kind, off="alpha")
    assert torch.equal(a_src, b_src) and torch.equal(a_tgt, b_tgt)


@pytest.mark.parametrize("kind", KINDS)
def test_node_scores_past_the_grid(dev, kind):
    V, L, K, H = 70000, 1, 64, 64
    assert V * L * K > 16384 * 256  # the grid-stride loop wraps
    _check_node_scores(dev, V, L, K, H, kind)


@pytest.mark.parametrize("V,L", [(0, 3), (5, 0)])
def test_node_scores_empty(dev, V, L):
    lib, ops = _lib_ops()
    Y = torch.zeros((4, 8), device=dev)
    alpha = torch.zeros((max(L, 1), 2, 8), device=dev)
    s_src, s_tgt = _guarded(0, 2, dev), _guarded(0, 2, dev)
    assert lib.tfgnn_rgat_node_scores(ops._ptr(Y), ops._ptr(alpha), V, L, 2, 8, ops._ptr(s_src), ops._ptr(s_tgt), ops._stream()) == 0
    torch.cuda.synchronize()
    _untouched(s_src, "s_src of an empty problem")
    _untouched(s_tgt, "s_tgt of an empty problem")


# =================================================================================================================================
# tfgnn_rgat_edge_dot
# =================================================================================================================================
EDGE_VEC = [(1, 4), (1, 16), (1, 64), (1, 256), (2, 8), (8, 256)]
EDGE_SCALAR = [(3, 24), (4, 24), (1, 7), (8, 96), (64, 64)]
EDGE_V, EDGE_L = 50, 2


def _check_edge_dot(dev, E, K, H, kind, off=None):
    lib, ops = _lib_ops()
    V, L = EDGE_V, EDGE_L
    g = _gen(2, E, K, H, kind == "exact")
    Y = _draw(kind, (V * L, H), g, scale_rows=True)
    d_agg = _draw(kind, (V, H), g, scale_rows=True)
    coll = torch.randint(0, V * L, (E,), generator=g, dtype=torch.int32)
    tgt = torch.randint(0, V, (E,), generator=g, dtype=torch.int32)
    Yd, gd = Y.to(dev), d_agg.to(dev)
    if off == "Y":
        Yd = _off4(Yd)
    if off == "d_agg":
        gd = _off4(gd)
    cd, td = coll.to(dev), tgt.to(dev)
    da = _guarded(E, K, dev)
    rc = lib.tfgnn_rgat_edge_dot(ops._ptr(cd), ops._ptr(td), ops._ptr(Yd), ops._ptr(gd), E, K, H, ops._ptr(da), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"tfgnn_rgat_edge_dot returned {rc}"
    tag = f"(K,H)=({K},{H}) E={E} {kind}" + (f" {off} offset" if off else "")
    if E:
        want, S = ref.edge_dot(coll, tgt, Y, d_agg, K)
        _compare("tfgnn_rgat_edge_dot", tag, kind, da[:E], want, S, H // K)
    _guard_untouched(da, f"edge_dot da {tag}")  # (a store from a clamped tail edge lands here)
    return da


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("E", [1, 2, 3, 4, 5, 63, 64, 65, 1027])
@pytest.mark.parametrize("K,H", EDGE_VEC)
def test_edge_dot_vec(dev, K, H, E, kind):
    _check_edge_dot(dev, E, K, H, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,H", EDGE_SCALAR)
def test_edge_dot_scalar(dev, K, H, kind):
    _check_edge_dot(dev, 1027, K, H, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_edge_dot_past_the_grid(dev, kind):
    E, K, H = 70000, 64, 64
    assert E * K > 16384 * 256
    _check_edge_dot(dev, E, K, H, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_edge_dot_alignment_fallback(dev, kind):
    E, K, H = 1027, 1, 64
    _check_edge_dot(dev, E, K, H, kind)
    a = _check_edge_dot(dev, E, K, H, kind, off="Y")
    b = _check_edge_dot(dev, E, K, H, kind, off="d_agg")
    assert torch.equal(a, b)


def test_edge_dot_empty(dev):
    _check_edge_dot(dev, 0, 2, 8, "exact")


# =================================================================================================================================
# tfgnn_rgat_scores_backward (in place: dY holds dY0 on entry)
# =================================================================================================================================
SB_VEC = [(3, 3, 24), (3, 8, 96), (2, 2, 512), (3, 1, 4), (4, 8, 256)]
SB_SCALAR = [(3, 4, 24), (2, 1, 7), (1, 64, 64)]


def _sb_inputs(V, L, K, H, kind, salt=3):
    rows, Hk = V * L, H // K
    g = _gen(salt, V, L, K, H, kind == "exact")
    ds_src = _draw(kind, (rows, K), g, scale_rows=True)
    ds_tgt = _draw(kind, (rows, K), g, scale_rows=True)
    alpha = _draw(kind, (L, K, 2 * Hk), g)
    dY0 = _draw(kind, (rows, H), g, scale_rows=True)
    return ds_src, ds_tgt, alpha, dY0


def _check_scores_backward(dev, V, L, K, H, kind, off=None):
    lib, ops = _lib_ops()
    rows = V * L
    ds_src, ds_tgt, alpha, dY0 = _sb_inputs(V, L, K, H, kind)
    sd, td, ad = ds_src.to(dev), ds_tgt.to(dev), alpha.to(dev)
    dY = _guarded(rows, H, dev, init=dY0)
    if off == "dY":
        dY = _off4(dY)
    if off == "alpha":
        ad = _off4(ad)
    rc = lib.tfgnn_rgat_scores_backward(ops._ptr(sd), ops._ptr(td), ops._ptr(ad), V, L, K, H, ops._ptr(dY), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"tfgnn_rgat_scores_backward returned {rc}"
    want, S = ref.scores_backward(ds_src, ds_tgt, alpha, dY0, L, K)
    tag = f"(L,K,H)=({L},{K},{H}) V={V} {kind}" + (f" {off} offset" if off else "")
    _compare("tfgnn_rgat_scores_backward", tag, kind, dY[:rows], want, S, 3)
    _guard_untouched(dY, f"scores_backward dY {tag}")
    return dY


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("L,K,H", SB_VEC + SB_SCALAR)
def test_scores_backward(dev, L, K, H, kind):
    _check_scores_backward(dev, 67, L, K, H, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_scores_backward_past_the_grid(dev, kind):
    V, L, K, H = 70000, 1, 64, 64
    assert V * L * H > 16384 * 256
    _check_scores_backward(dev, V, L, K, H, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_scores_backward_alignment_fallback(dev, kind):
    L, K, H = 3, 8, 96
    _check_scores_backward(dev, 67, L, K, H, kind)
    a = _check_scores_backward(dev, 67, L, K, H, kind, off="dY")
    b = _check_scores_backward(dev, 67, L, K, H, kind, off="alpha")
    assert torch.equal(a, b)


# =================================================================================================================================
# tfgnn_rgat_scores_backward_sp
# =================================================================================================================================
SP_SHAPES = [(1, 1, 16), (2, 3, 24), (3, 3, 48), (5, 5, 400), (4, 8, 512), (4, 8, 256)]
SP_UNSUPPORTED = [(2, 4, 24), (1, 3, 24), (5, 8, 512)]  # Hk % 4 != 0 ; C % 16 != 0 ; C > 2048


def _sp_buffers(V, C, dev, dY0):
    dY = _guarded(V, C, dev, init=dY0)
    data = torch.full((V + 1, 4 * C), SENTINEL_BYTE, dtype=torch.uint8, device=dev)
    inv = torch.full((V + 1, 1), SENTINEL, dtype=torch.float32, device=dev)
    return dY, data, inv


def _call_sp(dev, inputs, V, L, K, H, update, dY_off=False):
    """-> (rc, dY, data, inv), guard rows included"""
    lib, ops = _lib_ops()
    ds_src, ds_tgt, alpha, dY0 = inputs
    sd, td, ad = ds_src.to(dev), ds_tgt.to(dev), alpha.to(dev)
    dY, data, inv = _sp_buffers(V, L * H, dev, dY0)
    if dY_off:
        dY = _off4(dY)
    rc = lib.tfgnn_rgat_scores_backward_sp(ops._ptr(sd), ops._ptr(td), ops._ptr(ad), ops._ptr(dY), update, V, L, K, H, ops._ptr(data),
                                           ops._ptr(inv), ops._stream())
    torch.cuda.synchronize()
    return rc, dY, data, inv


def _check_sp_against_split(dev, inputs, V, L, K, H, tag):
    """update_fp32 = 1 and 0 on the same inputs; the split operand against a split pass over the updated fp32 values"""
    _, ops = _lib_ops()
    C = L * H
    rc, dY, data, inv = _call_sp(dev, inputs, V, L, K, H, 1)
    assert rc == 0, f"tfgnn_rgat_scores_backward_sp returned {rc} at {tag}"
    op = ops.sp_split_rows(dY[:V], scale_block=0)
    torch.cuda.synchronize()
    assert tuple(op.data.shape) == (V, 4 * C) and tuple(op.inv_scale.shape) == (V, 1)
    assert torch.equal(inv[:V], op.inv_scale), f"{tag}: row scales differ from a split pass over the updated dY"
    assert torch.equal(data[:V], op.data), f"{tag}: SP16 bytes differ from a split pass over the updated dY"
    rc0, dY_kept, data0, inv0 = _call_sp(dev, inputs, V, L, K, H, 0)
    assert rc0 == 0
    assert torch.equal(dY_kept[:V].cpu().view(torch.int32), inputs[3].reshape(V, C).view(torch.int32)), f"{tag}: update_fp32 = 0 wrote dY"
    assert torch.equal(data0, data) and torch.equal(inv0, inv), f"{tag}: update_fp32 = 0 gives another split operand"
    for buf, what in ((dY, "dY"), (inv, "inv_scale"), (dY_kept, "dY (update_fp32 = 0)")):
        _guard_untouched(buf, f"scores_backward_sp {what} {tag}")
    assert bool((data[-1] == SENTINEL_BYTE).all()), f"scores_backward_sp {tag}: the guard row behind the SP16 data was written"
    return dY, data, inv


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", [1, 3, 4, 5, 67])
@pytest.mark.parametrize("L,K,H", SP_SHAPES)
def test_scores_backward_sp(dev, L, K, H, V, kind):
    inputs = _sb_inputs(V, L, K, H, kind, salt=4)
    tag = f"(L,K,H)=({L},{K},{H}) V={V} {kind}"
    dY, _, _ = _check_sp_against_split(dev, inputs, V, L, K, H, tag)
    want, S = ref.scores_backward(*inputs, L, K)
    _compare("tfgnn_rgat_scores_backward_sp", tag, kind, dY[:V], want, S, 3)


@pytest.mark.parametrize("kind", KINDS)
def test_scores_backward_sp_row_loop_wraps(dev, kind):
    V, L, K, H = 32800, 1, 1, 16
    assert -(-V // 4) > 8192  # more row groups than blocks
    inputs = _sb_inputs(V, L, K, H, kind, salt=4)
    dY, _, _ = _check_sp_against_split(dev, inputs, V, L, K, H, f"V={V} {kind}")
    want, S = ref.scores_backward(*inputs, L, K)
    _compare("tfgnn_rgat_scores_backward_sp", f"V={V} {kind}", kind, dY[:V], want, S, 3)


def test_scores_backward_sp_zero_and_inf_rows(dev):
    """A row that is all zero after the update carries the marker scale 2^-126 and all-zero fragments; a row with an inf gets
    scale 1 and no NaN in its l plane (inf - inf).  Both still equal the split pass bit for bit."""
    V, L, K, H = 5, 2, 3, 24
    C = L * H
    ds_src, ds_tgt, alpha, dY0 = _sb_inputs(V, L, K, H, "normal", salt=5)
    ds_src[1 * L:2 * L] = 0.0
    ds_tgt[1 * L:2 * L] = 0.0
    dY0 = dY0.reshape(V, C)
    dY0[1] = 0.0
    dY0[3, 5] = float("inf")
    dY0 = dY0.reshape(V * L, H)
    dY, data, inv = _check_sp_against_split(dev, (ds_src, ds_tgt, alpha, dY0), V, L, K, H, "zero / inf rows")
    assert bool((dY[1] == 0).all()) and float(inv[1]) == MARKER and bool((data[1] == 0).all())
    assert float(inv[3]) == 1.0 and float(dY[3, 5]) == float("inf")
    planes = data[3].cpu().numpy().reshape(C // 16, 2, 32).copy().view(np.float16).reshape(C // 16, 2, 16)
    assert not np.isnan(planes[:, 1, :]).any(), "NaN in the l plane of the row with an inf"
    assert np.isinf(planes[0, 0, 5]) and planes[0, 1, 5] == 0


def test_scores_backward_sp_refuses_an_unaligned_dY(dev):
    V, L, K, H = 5, 2, 3, 24
    inputs = _sb_inputs(V, L, K, H, "normal", salt=6)
    rc, dY, data, inv = _call_sp(dev, inputs, V, L, K, H, 1, dY_off=True)
    assert rc == -1
    assert torch.equal(dY[:V].cpu(), inputs[3].reshape(V, L * H))
    _guard_untouched(dY, "refused call: dY")
    _untouched(data, "refused call: SP16 data")
    _untouched(inv, "refused call: inv_scale")


@pytest.mark.parametrize("L,K,H", SP_UNSUPPORTED)
def test_scores_backward_sp_refuses_unsupported_shapes(dev, L, K, H):
    """the shapes of tests/test_rgat_reference_host.py with real operands: -4 (the caller takes the fp32 route), nothing written"""
    V = 3
    inputs = _sb_inputs(V, L, K, H, "normal", salt=7)
    for update in (1, 0):
        rc, dY, data, inv = _call_sp(dev, inputs, V, L, K, H, update)
        assert rc == -4
        assert torch.equal(dY[:V].cpu(), inputs[3].reshape(V, L * H))
        _guard_untouched(dY, "refused call: dY")
        _untouched(data, "refused call: SP16 data")
        _untouched(inv, "refused call: inv_scale")


# =================================================================================================================================
# tfgnn_rgat_alpha_grad
# =================================================================================================================================
AG_VEC = [(3, 3, 24), (1, 1, 4), (2, 8, 256), (3, 2, 512)]  # (3, 2, 512): L H = 1536 > 1024 columns per pass
AG_SCALAR = [(3, 4, 24), (2, 1, 7), (1, 64, 64)]
AG_CAP = [(1, 1, 8), (2, 3, 24)]


def _call_alpha_grad(dev, dev_inputs, V, L, K, H, ws_off=False, shrink=0):
    """-> (rc, d_alpha [L*K + 1, 2 Hk], workspace [nblocks + 1, 2 L H]), guard rows included"""
    lib, ops = _lib_ops()
    sd, td, Yd = dev_inputs
    nbytes = int(lib.tfgnn_rgat_alpha_grad_workspace_bytes(V, L, H))
    assert nbytes % (2 * L * H * 4) == 0 and nbytes // (2 * L * H * 4) == min(1024, -(-V // 16))
    ws = _guarded(nbytes // (2 * L * H * 4), 2 * L * H, dev)
    if ws_off:
        ws = _off4(ws)
    d_alpha = _guarded(L * K, 2 * (H // K), dev)
    rc = lib.tfgnn_rgat_alpha_grad(ops._ptr(sd), ops._ptr(td), ops._ptr(Yd), V, L, K, H, ops._ptr(d_alpha), ops._ptr(ws), nbytes - shrink,
                                   ops._stream())
    torch.cuda.synchronize()
    return rc, d_alpha, ws


def _ag_inputs(V, L, K, H, kind):
    g = _gen(8, V, L, K, H, kind == "exact")
    ds_src = _draw(kind, (V * L, K), g)
    ds_tgt = _draw(kind, (V * L, K), g)
    Y = _draw(kind, (V * L, H), g, scale_rows=True)
    return ds_src, ds_tgt, Y


def _check_alpha_grad(dev, V, L, K, H, kind):
    inputs = _ag_inputs(V, L, K, H, kind)
    dev_inputs = tuple(t.to(dev) for t in inputs)
    tag = f"(L,K,H)=({L},{K},{H}) V={V} {kind}"
    rc, d_alpha, ws = _call_alpha_grad(dev, dev_inputs, V, L, K, H)
    assert rc == 0, f"tfgnn_rgat_alpha_grad returned {rc} at {tag}"
    want, S = ref.alpha_grad(*inputs, L, K)
    _compare("tfgnn_rgat_alpha_grad", tag, kind, d_alpha[:L * K], want, S, V)
    _guard_untouched(d_alpha, f"alpha_grad d_alpha {tag}")
    _guard_untouched(ws, f"alpha_grad workspace {tag}")
    # node slices past V are empty: their blocks write zeros
    nb = ws.shape[0] - 1
    per = -(-V // nb)
    first_empty = -(-V // per)
    assert bool((ws[first_empty:nb] == 0).all()), f"{tag}: blocks {first_empty} .. {nb - 1} own no node and must write zeros"
    # the same call again, and with the workspace 4 bytes into a buffer (the scalar partial kernel): the same bits
    rc2, again, _ = _call_alpha_grad(dev, dev_inputs, V, L, K, H)
    rc3, shifted, ws3 = _call_alpha_grad(dev, dev_inputs, V, L, K, H, ws_off=True)
    assert rc2 == 0 and rc3 == 0
    assert torch.equal(again, d_alpha), f"{tag}: two calls on the same inputs differ"
    assert torch.equal(shifted, d_alpha), f"{tag}: the scalar partial kernel (offset workspace) adds in another order"
    _guard_untouched(ws3, f"alpha_grad offset workspace {tag}")
    return first_empty, nb


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", [1, 15, 16, 17, 100, 1000])
@pytest.mark.parametrize("L,K,H", AG_VEC + AG_SCALAR)
def test_alpha_grad(dev, L, K, H, V, kind):
    _check_alpha_grad(dev, V, L, K, H, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", [16384, 16385, 16400, 20000])
@pytest.mark.parametrize("L,K,H", AG_CAP)
def test_alpha_grad_at_the_block_cap(dev, L, K, H, V, kind):
    first_empty, nb = _check_alpha_grad(dev, V, L, K, H, kind)
    assert nb == 1024
    assert (first_empty < nb) == (V != 16384)  # past 16 384 nodes a slice holds 17+ nodes and the trailing blocks none


def test_alpha_grad_without_nodes_zero_fills(dev):
    lib, ops = _lib_ops()
    L, K, H = 2, 3, 24
    d_alpha = _guarded(L * K, 2 * (H // K), dev)
    assert lib.tfgnn_rgat_alpha_grad(None, None, None, 0, L, K, H, ops._ptr(d_alpha), None, 0, ops._stream()) == 0
    torch.cuda.synchronize()
    assert bool((d_alpha[:L * K] == 0).all())
    _guard_untouched(d_alpha, "alpha_grad V = 0")


def test_alpha_grad_refuses_a_short_workspace(dev):
    V, L, K, H = 100, 2, 3, 24
    dev_inputs = tuple(t.to(dev) for t in _ag_inputs(V, L, K, H, "normal"))
    rc, d_alpha, ws = _call_alpha_grad(dev, dev_inputs, V, L, K, H, shrink=1)
    assert rc == -1
    _untouched(d_alpha, "refused call: d_alpha")
    _untouched(ws, "refused call: workspace")


# =================================================================================================================================
# the layer at one head
# =================================================================================================================================
@pytest.mark.parametrize("H", [16, 24])
def test_rgat_layer_backward_parity_at_one_head(dev, H):
    """H = 16: the lane-group kernels (tfgnn_rgat_edge_dot's vec form runs only at one head); H = 24: the scalar route"""
    check_rgat_backward(dev, 1, "tanh", V=90, E=900, L=3, H=H)


@pytest.mark.gemm_modes
def test_rgat_layer_backward_parity_at_one_head_in_every_mode(dev, gemm_mode):
    """f16x2 reaches tfgnn_rgat_scores_backward_sp with K = 1 (C = 192)"""
    check_rgat_backward(dev, 1, "tanh", V=90, E=900, L=3, H=64)


def test_layer_takes_edge_dot_at_one_head():
    """the layer calls tfgnn_rgat_edge_dot only where the gather cannot fuse the dot product; one head of 16 is such a shape"""
    from tf2_gnn_amd import ops

    assert not ops.graph_gather_dot_supported(16, 1) and not ops.graph_gather_dot_supported(24, 1)
    assert _vec_shape(1, 16) and not _vec_shape(1, 24)
