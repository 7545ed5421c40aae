"""The planned graph gather that writes its sums as an SP16 split operand (csrc/spmm.hip tfgnn_graph_gather_reduce_sp, kernel
family gather_sp, ``ops.graph_gather_sp``) on the planned graphs of tests/test_gpu_graph_gather.py: short rows at both sides of
the threshold, whole-row items, rows of two and three items whose last item holds one edge, and the in-wave combine.

Every call goes to the C entry with buffers of the test's own: one sentinel operand row behind the last SP16 row, one sentinel
element behind the last scale, one sentinel row behind the partial slots and - with one operand row per view row - 64 bytes of
padding between the rows (ld_out_sp_bytes = 4 * width + 64).  The [V, L * width] fold (rows_per_operand_row = L) is the same
call with ld_out_sp_bytes = 4 * width, read back as that operand; ``ops.graph_gather_sp`` itself is held to the same bytes in
test_wrapper_writes_the_bytes_of_the_c_entry.

(a) against fp64 (tests/gather_reference.py):  |decode - ref| <= SUM_TOL * l1 + format_bound(ref, block maximum of ref)
    SUM_TOL = 2e-6 is the fp32 gather's bound, format_bound = max(|ref| * 2^-22, block maximum * 2^-37) the format's
    (tests/sp16_reference.py).  Rows without edges: zero bytes and the marker 2^-126.
(b) against the fp32 gather of the same call, bit for bit: inverse scales and h / l (as fp16 values, +0 == -0) equal
    sp16_reference.encode applied on the host to the device result of ``ops.graph_gather`` with the same arguments - the SP
    paths add in the order of the fp32 paths and then multiply by the row scale."""
import ctypes

import numpy as np
import pytest
import torch

from tests import gather_reference as gr
from tests import sp16_reference as sp
from tests.helpers import decode_sp16, record_parity
from tests.test_gpu_graph_gather import (ALL_VIEWS, NODE_DEGREES, NUM_NODES, PARTIAL_SLOTS, SENTINEL, SUM_TOL, TYPED_LENGTHS, Spec,
                                         _Case)

pytestmark = pytest.mark.gpu

# one width per SP instantiation of gather_dispatch, and the dead tails: 8 x 1 (16: half the lanes dead, 32), 16 x 1 (48: dead
# tail, 64), 16 x 2 (96: dead tail, 128), 16 x 4 (256), 16 x 5 (320), 32 x 4 (336: dead tail, 512)
SP_WIDTHS = (16, 32, 48, 64, 96, 128, 256, 320, 336, 512)
SHARED_WIDTHS = (64, 320)  # the fp64 references of these widths are kept for the tests that share them
PLAIN = Spec()
WEIGHTED = Spec(ew=1, rs=True)  # [E] edge weights and row scales (the SP16 gather writes plain sums: no activation)
TYPED_FOLD_VIEWS = (gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_SRC_TYPED, gr.VIEW_BY_DST_TYPED_PATTERN)
BYTE_SENTINEL = 0xA5
MARKER = float(sp.MARKER_INV)
ERR_UNSUPPORTED = -4  # include/tfgnn.h TFGNN_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def case(dev):
    return _Case(dev)


def _reference(case, view, width, spec):
    """case.reference as numpy arrays; only the shared widths stay in the case's cache"""
    ref, l1 = case.reference(view, width, spec)
    if width not in SHARED_WIDTHS:
        case._refs.pop((view, width, spec), None)
    return ref.numpy(), l1.numpy()


def _row_lengths(case, view):
    """edges of every output row of the view"""
    rowptr, _, out_rows = case.host(view)
    lens = np.diff(rowptr)
    return lens if out_rows is None else lens[out_rows]


class _Result:
    """what one call wrote, on the host: h, l fp16 [rows, width], inv fp32 [rows] (None with a fixed scale), the raw bytes"""

    def __init__(self, data, inv, width):
        self.data, self.inv, self.width = data, inv, width
        self.h, self.l = sp.unpack(data, width)

    def decode(self, inv=None):
        return sp.decode(self.h, self.l, self.inv if inv is None else np.full(self.h.shape[0], inv), self.width)

    def same_bits(self, other):
        return (np.array_equal(self.data[:, : 4 * self.width], other.data[:, : 4 * self.width])
                and (self.inv is None or np.array_equal(self.inv, other.inv)))


class _Buffers:
    """guarded device buffers of one call: SP16 rows (leading dimension ``ld`` bytes), scales, partial slots"""

    def __init__(self, case, rows, width, ld, scales=True):
        self.rows, self.width, self.ld = rows, width, ld
        self.data = torch.full(((rows + 1) * ld,), BYTE_SENTINEL, dtype=torch.uint8, device=case.dev)
        self.inv = torch.full((rows + 1,), SENTINEL, dtype=torch.float32, device=case.dev) if scales else None
        self.ws = torch.full((PARTIAL_SLOTS + 1, width), SENTINEL, dtype=torch.float32, device=case.dev)
        assert self.data.data_ptr() % 64 == 0

    def untouched(self):
        ok = bool((self.data == BYTE_SENTINEL).all()) and bool((self.ws == SENTINEL).all())
        return ok and (self.inv is None or bool((self.inv == SENTINEL).all()))

    def check_guards(self, what):
        grid = self.data.view(self.rows + 1, self.ld)
        assert bool((grid[-1] == BYTE_SENTINEL).all()), f"{what}: the operand row behind the last SP16 row was written"
        assert bool((grid[:, 4 * self.width:] == BYTE_SENTINEL).all()), f"{what}: the padding between the SP16 rows was written"
        assert bool((self.ws[-1] == SENTINEL).all()), f"{what}: the row behind the partial slots was written"
        if self.inv is not None:
            assert float(self.inv[-1]) == SENTINEL, f"{what}: the element behind the last scale was written"

    def result(self):
        grid = self.data.view(self.rows + 1, self.ld)[:-1].cpu().numpy()
        return _Result(grid, None if self.inv is None else self.inv[:-1].cpu().numpy(), self.width)


def _call(case, view, width, buf, *, entry="tfgnn_graph_gather_reduce_sp", inp, col=None, ew=None, rs=None, fixed=None, data_ptr=None,
          ld=None, inv="own", ws_bytes=None, job=None):
    """one call of the C entry on ``buf`` -> its return code"""
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    g = case.handle(view)
    g.wait()
    g.ensure(ops._VIEW_PARTS[view])
    nbytes = int(lib.tfgnn_graph_gather_workspace_bytes(g._h, view, width)) if ws_bytes is None else ws_bytes
    assert nbytes <= (buf.ws.numel() - width) * 4
    inv_ptr = ops._ptr(buf.inv) if inv == "own" else inv
    args = [g._h, view, ops._ptr(col), ops._ptr(ew), ops._ptr(rs), ops._ptr(inp), inp.stride(0), width,
            ctypes.c_void_p(buf.data.data_ptr() if data_ptr is None else data_ptr), buf.ld if ld is None else ld, inv_ptr,
            ops._ptr(fixed), ops._ptr(buf.ws), nbytes]
    if job is not None:
        args.append(ctypes.cast(ctypes.pointer(job), ctypes.c_void_p))
    rc = getattr(lib, entry)(*args, ops._stream())
    torch.cuda.synchronize()
    return rc


def _run(case, view, width, spec=PLAIN, *, fold=False, fixed=None, inp=None, col=None, what=""):
    """tfgnn_graph_gather_reduce_sp over the view with the case's inputs -> _Result (guards checked)"""
    from tf2_gnn_amd import _lib

    X, ew, rs = case.inputs(view, width)
    rows = case.num_out_rows(view)
    buf = _Buffers(case, rows, width, 4 * width + (0 if fold else 64), scales=fixed is None)
    rc = _call(case, view, width, buf, inp=X.to(case.dev) if inp is None else inp, col=col, ew=ew.to(case.dev) if spec.ew else None,
               rs=rs.to(case.dev) if spec.rs else None, fixed=fixed)
    assert rc == 0, _lib.load().tfgnn_last_error().decode()
    buf.check_guards(f"{what} view {view} width {width}")
    res = buf.result()
    if fold:  # the same bytes read as the [V, L * width] operand with one scale block per edge type
        L = len(case.host_lists(view))
        assert rows == NUM_NODES * L
        from tf2_gnn_amd import ops

        op = ops.SplitOperand(buf.data[: rows * 4 * width].view(NUM_NODES, L * 4 * width),
                              (buf.inv[:-1] if fixed is None else fixed.expand(rows)).reshape(NUM_NODES, L).contiguous(), NUM_NODES,
                              L * width, width)
        res.folded = decode_sp16(op).reshape(rows, width)
    return res


def _fp32(case, view, width, spec=PLAIN, **kw):
    """the fp32 gather of the same call (ops.graph_gather) -> numpy [rows, width]"""
    return case.run(view, width, spec, **kw).numpy()


def _check_fp64(dec, ref, l1, lens, block_max, what, group):
    """(a) of the module docstring; the worst error-to-bound ratio goes to the parity log under ``group``"""
    assert dec.shape == ref.shape, f"{what}: shape {dec.shape} vs {ref.shape}"
    assert np.all(np.isfinite(dec)), f"{what}: non-finite operand"
    bound = SUM_TOL * l1 + sp.format_bound(ref, block_max)
    err = np.abs(dec - ref)
    empty = lens == 0
    assert np.all(dec[empty] == 0), f"{what}: a row without edges does not decode to exactly zero"
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if ratio.size else 0.0
    record_parity(group, max_error_to_bound=worst, bound=1.0)
    print(f"{what}: worst error / bound {worst:.3e}")
    if worst > 1.0:
        r, c = np.unravel_index(int(ratio.argmax()), ratio.shape)
        raise AssertionError(f"{what}: error {err[r, c]:.3e} is {worst:.3e} of its bound {bound[r, c]:.3e} at output row {r} "
                             f"({int(lens[r])} edges), column {c}")


def _check_empty_rows(res, lens, what):
    """rows without edges: zero bytes and the marker scale"""
    empty = lens == 0
    assert not res.data[empty][:, : 4 * res.width].any(), f"{what}: a row without edges has non-zero bytes"
    if res.inv is not None:
        bad = np.flatnonzero(empty & (res.inv != sp.MARKER_INV))
        assert bad.size == 0, f"{what}: row {bad[:1]} without edges has inverse scale {res.inv[bad[:1]]}, not the marker 2^-126"


def _check_bits(res, fp32, lens, what, fixed_inv=None):
    """(b) of the module docstring"""
    h, l, inv = sp.encode(fp32, res.width, fixed_inv=fixed_inv)
    if res.inv is not None:
        bad = np.flatnonzero(res.inv != inv[:, 0])
        assert bad.size == 0, (f"{what}: inverse scale of output row {bad[0]} ({int(lens[bad[0]])} edges) is {res.inv[bad[0]]}, the "
                               f"fp32 gather's row encodes with {inv[bad[0], 0]} ({bad.size} rows differ)")
    for name, got, want in (("h", res.h, h), ("l", res.l, l)):
        diff = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        if diff.any():
            r, c = np.argwhere(diff)[0]
            raise AssertionError(f"{what}: {name} of output row {r} ({int(lens[r])} edges), column {c} is {got[r, c]!r}, the fp32 "
                                 f"gather's sum {fp32[r, c]!r} encodes to {want[r, c]!r} ({int(diff.sum())} entries in "
                                 f"{np.unique(np.argwhere(diff)[:, 0]).size} rows differ)")


def _check_all(case, res, view, width, spec, what, group, fp32=None):
    lens = _row_lengths(case, view)
    ref, l1 = _reference(case, view, width, spec)
    _check_fp64(res.decode(), ref, l1, lens, sp.blockmax(ref, width), what, group)
    _check_empty_rows(res, lens, what)
    _check_bits(res, _fp32(case, view, width, spec) if fp32 is None else fp32, lens, what)


# ---- the plan ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", ALL_VIEWS)
def test_plan_has_ten_partial_slots_at_the_sp_widths(case, view):
    """513 -> 2, 1024 -> 2, 1025 -> 3, 1100 -> 3 items: if the plan constants move, this fails instead of the tests below
    quietly no longer reaching the item and combine paths"""
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    lens = _row_lengths(case, view)
    planned = NODE_DEGREES if _Case.kind(view) == "node" else TYPED_LENGTHS
    compact = view in (gr.VIEW_BY_DST_TYPED_COMPACT, gr.VIEW_BY_SRC_TYPED_COMPACT)  # (no rows for the empty buckets)
    assert set(n for n in planned if n or not compact) <= set(int(x) for x in lens)
    for w in SP_WIDTHS:
        assert lib.tfgnn_graph_gather_workspace_bytes(case.handle(view)._h, view, w) == PARTIAL_SLOTS * w * 4


# ---- forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", SP_WIDTHS)
@pytest.mark.parametrize("view", ALL_VIEWS)
def test_plain_sums_both_walks_and_folds(case, monkeypatch, view, width):
    """every view at every SP instantiation: one row per lane group (TFGNN_GATHER_MULTI = 1) and two (21) write the same bits;
    typed and pattern views also as the [V, L * width] operand"""
    what = f"plain view {view} width {width}"
    monkeypatch.setenv("TFGNN_GATHER_MULTI", "1")
    one = _run(case, view, width, what=what)
    fp32 = _fp32(case, view, width)
    _check_all(case, one, view, width, PLAIN, what, "graph_gather_sp views plain sum", fp32=fp32)
    monkeypatch.setenv("TFGNN_GATHER_MULTI", "21")
    two = _run(case, view, width, what=what + " walk 21")
    assert one.same_bits(two), f"{what}: the two walks differ"
    assert np.array_equal(fp32, _fp32(case, view, width))
    if view in TYPED_FOLD_VIEWS:
        ref, l1 = _reference(case, view, width, PLAIN)
        for walk in ("1", "21"):
            monkeypatch.setenv("TFGNN_GATHER_MULTI", walk)
            folded = _run(case, view, width, fold=True, what=what + f" folded walk {walk}")
            assert one.same_bits(folded), f"{what}: the folded operand differs (walk {walk})"
            _check_fp64(folded.folded, ref, l1, _row_lengths(case, view), sp.blockmax(ref, width), what + " folded",
                        "graph_gather_sp views plain sum")


@pytest.mark.parametrize("width", SP_WIDTHS)
@pytest.mark.parametrize("view", ALL_VIEWS)
def test_edge_weights_and_row_scales(case, view, width):
    """[E] edge weights and row scales, the walk chosen by the library (typed views: two rows per lane group)"""
    what = f"weighted view {view} width {width}"
    res = _run(case, view, width, WEIGHTED, what=what)
    _check_all(case, res, view, width, WEIGHTED, what, "graph_gather_sp views weights + scales")
    if view in TYPED_FOLD_VIEWS:
        assert res.same_bits(_run(case, view, width, WEIGHTED, fold=True, what=what + " folded"))


FIXED_CASES = [(v, w) for v in (gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE) for w in SP_WIDTHS] + \
              [(v, 64) for v in ALL_VIEWS if v not in (gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE)]


@pytest.mark.parametrize("view,width", FIXED_CASES)
def test_fixed_inverse_scale(case, view, width):
    """one caller-chosen scale for the tensor, from twice the fp32 result's largest magnitude: no scale is written, and the block
    maximum of the format's bound is that tensor bound (as in test_gather_sp_matches_fp32_gather)"""
    from tf2_gnn_amd import ops

    what = f"fixed scale view {view} width {width}"
    lens = _row_lengths(case, view)
    for spec in (PLAIN, WEIGHTED):
        fp32 = _fp32(case, view, width, spec)
        bound = ops.absmax(torch.from_numpy(fp32).to(case.dev), scale=2.0)
        fixed = ops.tensor_inv_scale(bound)
        inv = float(fixed.cpu())
        assert float(bound.cpu()) == 2.0 * float(np.abs(fp32).max()) and sp.SCALED_LO <= float(bound.cpu()) / inv < sp.SCALED_HI
        res = _run(case, view, width, spec, fixed=fixed, what=what)
        assert res.inv is None
        ref, l1 = _reference(case, view, width, spec)
        _check_fp64(res.decode(inv), ref, l1, lens, float(bound.cpu()), what, "graph_gather_sp fixed scale")
        _check_empty_rows(res, lens, what)
        _check_bits(res, fp32, lens, what, fixed_inv=np.float32(inv))
        if view in TYPED_FOLD_VIEWS:
            folded = _run(case, view, width, spec, fixed=fixed, fold=True, what=what + " folded")
            assert res.same_bits(folded)
            _check_fp64(folded.folded, ref, l1, lens, float(bound.cpu()), what + " folded", "graph_gather_sp fixed scale")


@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_input_as_a_column_slice(case, view):
    """ld_in > width at a 16-byte aligned offset; an offset of one float has no float4 path and is refused with nothing written"""
    from tf2_gnn_amd import _lib

    width = 64
    X = case.inputs(view, width)[0]
    wide = torch.full((X.shape[0], width + 8), 3.25)
    wide[:, 4:4 + width] = X
    wide = wide.to(case.dev)
    what = f"input slice view {view}"
    res = _run(case, view, width, inp=wide[:, 4:4 + width], what=what)
    _check_all(case, res, view, width, PLAIN, what, "graph_gather_sp operands")
    buf = _Buffers(case, case.num_out_rows(view), width, 4 * width + 64)
    assert _call(case, view, width, buf, inp=wide[:, 1:1 + width]) != 0
    assert "16-byte aligned" in _lib.load().tfgnn_last_error().decode()
    assert buf.untouched()


@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_SRC_NODE])
def test_column_override_with_per_edge_rows(case, view):
    """col = the identity over [E, width] per-edge rows (the per-edge message forms)"""
    width = 64
    rowptr, _, out_rows = case.host(view)
    assert out_rows is None
    E = case.num_edges(view)
    msgs = torch.randn((E, width), generator=torch.Generator().manual_seed(50 + view))
    ident = torch.arange(E, dtype=torch.int32, device=case.dev)
    what = f"col override view {view}"
    res = _run(case, view, width, inp=msgs.to(case.dev), col=ident, what=what)
    ref, l1, lens = gr.gather_reference(rowptr, np.arange(E), msgs)
    ref, l1, lens = ref.numpy(), l1.numpy(), lens.numpy()
    _check_fp64(res.decode(), ref, l1, lens, sp.blockmax(ref, width), what, "graph_gather_sp operands")
    _check_empty_rows(res, lens, what)
    _check_bits(res, _fp32(case, view, width, inp=msgs.to(case.dev), col=ident), lens, what)


@pytest.mark.parametrize("spec", [PLAIN, WEIGHTED], ids=["plain", "weighted"])
@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE, gr.VIEW_BY_SRC_TYPED_COMPACT])
def test_same_call_twice_same_bits(case, view, spec):
    assert _run(case, view, 320, spec).same_bits(_run(case, view, 320, spec))


def test_wrapper_writes_the_bytes_of_the_c_entry(case):
    """ops.graph_gather_sp (which allocates its own operand): shapes per view and rows_per_operand_row, bytes and scales"""
    from tf2_gnn_amd import ops

    width = 64
    for view in ALL_VIEWS:
        X, ew, rs = case.inputs(view, width)
        L = len(case.host_lists(view))
        rows = case.num_out_rows(view)
        want = _run(case, view, width, WEIGHTED)
        for R in (1, L) if view in TYPED_FOLD_VIEWS else (1,):
            op = ops.graph_gather_sp(case.handle(view), view, X.to(case.dev), edge_weight=ew.to(case.dev), row_scale=rs.to(case.dev),
                                     rows_per_operand_row=R)
            assert (op.rows, op.cols, op.scale_block) == (rows // R, R * width, width)
            assert tuple(op.data.shape) == (rows // R, R * width * 4) and tuple(op.inv_scale.shape) == (rows // R, R)
            assert np.array_equal(op.data.cpu().numpy().reshape(rows, 4 * width), want.data[:, : 4 * width])
            assert np.array_equal(op.inv_scale.cpu().numpy().reshape(rows), want.inv)


# ---- special values on the planned rows ------------------------------------------------------------------------------------------
def _row_of_length(case, view, n):
    """the output row that holds the planned row of ``n`` edges"""
    planned = NODE_DEGREES if _Case.kind(view) == "node" else TYPED_LENGTHS
    L = 1 if _Case.kind(view) == "node" else len(case.host_lists(view))
    row = planned.index(n) * L
    assert int(_row_lengths(case, view)[row]) == n
    return row


@pytest.mark.parametrize("view,width", [(gr.VIEW_BY_DST_TYPED, 64), (gr.VIEW_BY_DST_TYPED, 320), (gr.VIEW_BY_DST_NODE, 64)])
def test_inf_and_nan_land_in_the_rows_that_gather_them(case, view, width):
    """an input row with one inf (gathered by the 49-edge row: a whole-row item), one with one nan (by the second item of the
    1025-edge row) and one of nothing but nan (by the 3-edge row).  Every row that gathers one of them takes the inf / nan
    branch of the scale rule: inverse scale 1, the class in h, l = 0 there; every other row keeps its bits."""
    rowptr, col, out_rows = case.host(view)
    assert out_rows is None
    lens = _row_lengths(case, view)
    long_n, short_n = (49, 3) if _Case.kind(view) == "typed" else (33, 3)
    src_inf = int(col[rowptr[_row_of_length(case, view, long_n)] + 5])
    src_nan = int(col[rowptr[_row_of_length(case, view, 1025)] + 600])
    src_all = int(col[rowptr[_row_of_length(case, view, short_n)] + 1])
    assert len({src_inf, src_nan, src_all}) == 3
    X = case.inputs(view, width)[0].clone()
    X[src_inf, 3] = float("inf")
    X[src_nan, 7] = float("nan")
    X[src_all, :] = float("nan")
    what = f"inf / nan view {view} width {width}"
    clean = _run(case, view, width, what=what)
    res = _run(case, view, width, inp=X.to(case.dev), what=what)
    ref, _, _ = gr.gather_reference(rowptr, col, X)
    ref = ref.numpy()
    hit = ~np.isfinite(ref).all(axis=1)
    rows_hit = set(np.flatnonzero(hit))
    assert {_row_of_length(case, view, long_n), _row_of_length(case, view, 1025), _row_of_length(case, view, short_n)} <= rows_hit
    assert 3 <= len(rows_hit) < 40  # the rows that gather one of the three input rows, not the graph
    # the neighbouring rows are unchanged
    assert np.array_equal(res.data[~hit], clean.data[~hit]) and np.array_equal(res.inv[~hit], clean.inv[~hit])
    bad = [int(r) for r in np.flatnonzero(hit) if res.inv[r] != 1.0]
    assert not bad, (f"{what}: output rows {bad} ({[int(lens[r]) for r in bad]} edges) gather an inf or nan and carry inverse scale "
                     f"{[float(res.inv[r]) for r in bad]}, not 1")
    nonfinite = ~np.isfinite(ref)
    assert np.array_equal(np.isnan(res.h), np.isnan(ref)), f"{what}: nan entries"
    assert np.array_equal(np.isposinf(res.h[nonfinite]), np.isposinf(ref[nonfinite])), f"{what}: inf entries"
    assert np.all(res.l[nonfinite] == 0), f"{what}: l of a non-finite entry is not zero"
    _check_bits(res, _fp32(case, view, width, inp=X.to(case.dev)), lens, what)


@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_subnormal_input_row_feeding_a_one_edge_row(case, view):
    """1e-42 is 714 * 2^-149: the row scales by the capped 2^126 (inverse scale 2^-126, the marker's value, with non-zero
    bytes) and h holds it exactly"""
    width = 64
    rowptr, col, _ = case.host(view)
    row = _row_of_length(case, view, 1)
    src = int(col[rowptr[row]])
    X = case.inputs(view, width)[0].clone()
    X[src, :] = 1e-42
    what = f"subnormal view {view}"
    res = _run(case, view, width, inp=X.to(case.dev), what=what)
    assert res.inv[row] == sp.MARKER_INV and res.data[row, : 4 * width].any()
    assert np.all(res.decode()[row] == float(np.float32(1e-42))) and np.all(res.l[row] == 0)
    lens = _row_lengths(case, view)
    ref, l1, _ = gr.gather_reference(rowptr, col, X)
    ref, l1 = ref.numpy(), l1.numpy()
    _check_fp64(res.decode(), ref, l1, lens, sp.blockmax(ref, width), what, "graph_gather_sp special values")
    _check_bits(res, _fp32(case, view, width, inp=X.to(case.dev)), lens, what)


@pytest.mark.parametrize("view", [gr.VIEW_BY_DST_TYPED, gr.VIEW_BY_DST_NODE])
def test_long_rows_that_cancel_to_zero_carry_the_marker(case, view):
    """per-edge rows of small integers (every fp32 sum of them is exact, in any order) in pairs +x, -x along the rows of 64 and
    512 edges (whole-row items), 1024 (two items) and 1100 (three): zero bytes and the marker, as for a row without edges -
    what the weight-gradient product's spread guard reads (csrc/sp16.hpp sp_row_holds)"""
    width = 64
    rowptr, _, _ = case.host(view)
    E = case.num_edges(view)
    gen = torch.Generator().manual_seed(70 + view)
    msgs = torch.randint(-8, 9, (E, width), generator=gen).float()
    rows = [_row_of_length(case, view, n) for n in (64, 512, 1024, 1100)]
    for row in rows:
        b, e = int(rowptr[row]), int(rowptr[row + 1])
        msgs[b + 1:e:2] = -msgs[b:e:2]
    ident = torch.arange(E, dtype=torch.int32, device=case.dev)
    what = f"cancelling rows view {view}"
    res = _run(case, view, width, inp=msgs.to(case.dev), col=ident, what=what)
    ref, l1, lens = gr.gather_reference(rowptr, np.arange(E), msgs)
    ref, lens = ref.numpy(), lens.numpy()
    assert all(np.all(ref[row] == 0) for row in rows)
    for row in rows:
        assert res.inv[row] == sp.MARKER_INV, f"{what}: the row of {int(lens[row])} edges has inverse scale {res.inv[row]}"
        assert np.all(res.h[row] == 0) and np.all(res.l[row] == 0), f"{what}: the row of {int(lens[row])} edges is not zero"
    assert np.array_equal(res.decode(), ref)  # integers below 2^11 * 8: the operand holds every sum exactly
    others = (lens > 0) & (np.abs(ref).max(axis=1) > 0)
    assert np.all(res.inv[others] != sp.MARKER_INV)


# ---- the C entry's argument checks -----------------------------------------------------------------------------------------------
def test_c_entry_argument_checks(case):
    """each refused call returns an error and writes nothing"""
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    view, width = gr.VIEW_BY_DST_TYPED, 64
    rows = case.num_out_rows(view)
    X = case.inputs(view, width)[0].to(case.dev)
    buf = _Buffers(case, rows, width, 4 * width + 64)

    def refused(message, **kw):
        rc = _call(case, view, kw.pop("width", width), buf, **{"inp": X, **kw})
        assert rc != 0 and message in lib.tfgnn_last_error().decode(), (rc, lib.tfgnn_last_error().decode())
        assert buf.untouched(), f"a refused call ({message}) wrote to its buffers"
        return rc

    refused("NULL output", inv=None)  # d_inv_scale and d_fixed_inv_scale both NULL
    refused("leading dimension / alignment", ld=4 * width + 32)  # not a multiple of 64
    refused("leading dimension / alignment", ld=4 * width - 64)  # below 4 * width
    refused("leading dimension / alignment", data_ptr=buf.data.data_ptr() + 16)  # misaligned d_out_sp
    X24 = torch.randn((NUM_NODES, 24), generator=torch.Generator().manual_seed(24)).to(case.dev)
    refused("width % 16 == 0", width=24, inp=X24, ld=128, ws_bytes=PARTIAL_SLOTS * 24 * 4)
    wide = _Buffers(case, rows, 1024, 4 * 1024)
    X1024 = torch.randn((NUM_NODES, 1024), generator=torch.Generator().manual_seed(1024)).to(case.dev)
    rc = _call(case, view, 1024, wide, inp=X1024)
    assert rc == ERR_UNSUPPORTED and "one feature window" in lib.tfgnn_last_error().decode()
    assert wide.untouched()
    # the same buffers take an accepted call afterwards
    assert _call(case, view, width, buf, inp=X) == 0
    buf.check_guards("after the refused calls")
    assert buf.result().same_bits(_run(case, view, width))


def test_deferred_entry_writes_the_same_operand_and_an_empty_job(case):
    """tfgnn_graph_gather_reduce_sp_deferred (kept for C callers): the gather combines its long rows itself, the job that used
    to carry the combine pass comes back with kind 0"""
    from tf2_gnn_amd import _lib

    view, width = gr.VIEW_BY_DST_TYPED, 64
    X, ew, rs = case.inputs(view, width)
    buf = _Buffers(case, case.num_out_rows(view), width, 4 * width + 64)
    job = _lib.AuxJob()
    ctypes.memset(ctypes.byref(job), 0xFF, ctypes.sizeof(job))
    rc = _call(case, view, width, buf, entry="tfgnn_graph_gather_reduce_sp_deferred", inp=X.to(case.dev), ew=ew.to(case.dev),
               rs=rs.to(case.dev), job=job)
    assert rc == 0, _lib.load().tfgnn_last_error().decode()
    buf.check_guards("deferred entry")
    assert job.kind == 0 and job.num_blocks == 0
    assert buf.result().same_bits(_run(case, view, width, WEIGHTED))
