"""Split-operand ("f16x2") Dense products (include/tfgnn.h tfgnn_sp_*, csrc/gemm_sp.hip) against the fp64 product and
against the fp32-MFMA kernel on the same data: the SP16 conversion (exact h + l reconstruction bound, power-of-two
scales), every tile width, ragged M, K tails (K % 64 != 0), the epilogues, per-block scales and special values."""
import numpy as np
import pytest
import torch

from tests.helpers import assert_close, decode_sp16

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,C,sb", [(37, 320, 0), (64, 1280, 320), (5, 64, 16), (300, 336, 0)])
def test_split_rows_reconstructs(dev, R, C, sb):
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(R + C)
    x = torch.randn((R, C), generator=g) * torch.exp(torch.randn((R, 1), generator=g) * 6.0)
    x[0, :] = 0.0                      # an all-zero row: scale 1
    x[1, 3] = 1e-30                    # a tiny entry beside O(1) values
    if R > 4:
        x[4, :] = x[4, :] * 1e-38      # subnormal-range row
    op = ops.sp_split_rows(x.to(dev), scale_block=sb)
    rec = decode_sp16(op)
    ref = x.double().numpy()
    blk = op.scale_block
    bmax = np.abs(ref).reshape(R, C // blk, blk).max(axis=2, keepdims=True)
    bmax = np.repeat(bmax, blk, axis=2).reshape(R, C)
    bound = np.maximum(np.abs(ref) * 2.0 ** -22, bmax * 2.0 ** -38)
    assert np.all(np.abs(rec - ref) <= bound), float(np.max(np.abs(rec - ref) / np.maximum(bound, 1e-300)))
    inv = op.inv_scale.cpu().numpy()
    m, _ = np.frexp(inv)
    assert np.all(m == 0.5), "scales must be powers of two"


def test_split_cols_and_segments(dev):
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(3)
    W = torch.randn((4, 80, 128), generator=g) * 0.1  # stacked kernels [L, D, H]
    Wd = W.to(dev)
    # [K = L*D, N = H] -> rows n, cols (l, d)
    op = ops.sp_split_cols(Wd.reshape(320, 128))
    np.testing.assert_allclose(decode_sp16(op), W.reshape(320, 128).t().double().numpy(), rtol=2.0 ** -21, atol=1e-12)
    # rows d, cols (l, h): [W_0[d,:] | W_1[d,:] | ...]
    op2 = ops.sp_split_rows(Wd[0], segments=(128, 80 * 128, 4 * 128))
    ref2 = W.permute(1, 0, 2).reshape(80, 512).double().numpy()
    np.testing.assert_allclose(decode_sp16(op2), ref2, rtol=2.0 ** -21, atol=1e-12)


def _run(dev, M, N, K, sb=0, bias=False, act=None, acc=False, grad=False, seed=0, a_gen=None):
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(seed + M + N + K)
    A = torch.randn((M, K), generator=g) if a_gen is None else a_gen(g)
    Bt = torch.randn((N, K), generator=g) * 0.05
    bias_t = torch.randn(N, generator=g) if bias else None
    C0 = torch.randn((M, N), generator=g) if acc else None
    mul = (torch.rand((M, N), generator=g) > 0.2).float() * 1.25 if grad else None
    saved = torch.tanh(torch.randn((M, N), generator=g)) if grad else None
    ref = A.double() @ Bt.double().t()
    if bias:
        ref = ref + bias_t.double()
    if act:
        ref = torch.tanh(ref)
    if grad:
        ref = ref * mul.double() * (1.0 - saved.double() ** 2)
    if acc:
        ref = ref + C0.double()
    a_op = ops.sp_split_rows(A.to(dev), scale_block=sb)
    b_op = ops.sp_split_rows(Bt.to(dev))
    out = C0.to(dev).clone() if acc else None
    res = ops.sp_gemm_nt(a_op, b_op, bias=None if bias_t is None else bias_t.to(dev), act=act, out=out, accumulate=acc,
                         out_mul=None if mul is None else mul.to(dev),
                         act_grad=None if saved is None else ("tanh", saved.to(dev)))
    torch.cuda.synchronize()
    return res.cpu(), ref, A, Bt


@pytest.mark.parametrize("M,N,K", [(300, 320, 1280), (129, 128, 64), (1000, 256, 336), (64, 640, 16), (2050, 320, 320),
                                   (5, 384, 48), (128, 1280, 320)])
def test_gemm_nt_matches_fp64(dev, M, N, K):
    res, ref, _, _ = _run(dev, M, N, K)
    scale = max(1.0, 0.05 * float(K) ** 0.5)
    assert_close(res / scale, (ref / scale).float(), tol=1e-5, what=f"sp nt {M}x{N}x{K}")


@pytest.mark.parametrize("epi", ["bias_act", "accumulate", "grad", "all"])
def test_gemm_nt_epilogues(dev, epi):
    kw = dict(bias=epi in ("bias_act", "all"), act="tanh" if epi in ("bias_act", "all") else None,
              acc=epi in ("accumulate", "all"), grad=epi in ("grad", "all"))
    res, ref, _, _ = _run(dev, 333, 320, 640, **kw)
    assert_close(res, ref.float(), tol=2e-5, what=f"sp nt epilogue {epi}")


def test_gemm_nt_same_error_class_as_fp32_mfma(dev):
    """Accumulation error against fp64 on N(0,1), relu-sparse and positive operands (K = 1280): below 4e-7 of sum |a||b|
    per output - the class of the fp32 kernels (tools/mfma_acc_probe.hip measures, for one unsplit K = 1280 chain, rms
    7.0e-7 for this path, 1.14e-6 for the fp32-MFMA chain and 9.8e-7 for bf16x3).  The fp32-MFMA kernel's error on the same
    data is printed beside it (it splits K at this size, which shortens its chains)."""
    from tf2_gnn_amd import ops

    M, N, K = 1024, 320, 1280
    gens = {
        "normal": lambda g: torch.randn((M, K), generator=g),
        "relu": lambda g: torch.relu(torch.randn((M, K), generator=g)),
        "positive": lambda g: torch.rand((M, K), generator=g),
    }
    prev = ops.set_gemm_mode("fp32")
    try:
        for name, gen in gens.items():
            res, ref, A, Bt = _run(dev, M, N, K, a_gen=gen, seed=7)
            mag = A.double().abs() @ Bt.double().abs().t()
            e_sp = (res.double() - ref).abs()
            r32 = ops.gemm(A.to(dev), Bt.to(dev), trans_b=True).cpu()
            e_32 = (r32.double() - ref).abs()
            print(f"{name}: max |err| f16x2 {float(e_sp.max()):.3e} fp32-MFMA {float(e_32.max()):.3e}; "
                  f"max err / sum|a||b| f16x2 {float((e_sp / mag).max()):.3e} fp32-MFMA {float((e_32 / mag).max()):.3e}")
            assert float((e_sp / mag).max()) <= 4e-7, name
            assert float(e_sp.max()) <= 1e-5 * max(1.0, float(ref.abs().max())), name
    finally:
        ops.set_gemm_mode(prev)


def test_gemm_nt_block_scales_wide_dynamic_range(dev):
    """Four scale blocks per row whose magnitudes differ by up to 1e+-30 (and rows that differ by as much): every
    output is within fp32 rounding of the fp64 product relative to the largest block contribution of its row."""
    M, N, K, sb = 200, 320, 1280, 320

    def gen(g):
        a = torch.randn((M, K), generator=g)
        blk = torch.tensor([1.0, 1e-6, 1e4, 1e-30]).repeat_interleave(sb)
        rowscale = torch.exp(torch.randn((M, 1), generator=g) * 20.0).clamp(1e-30, 1e30)
        a = a * blk * rowscale
        a[3, :sb] = 0.0
        a[5, :] = 0.0
        return a

    res, ref, A, Bt = _run(dev, M, N, K, sb=sb, a_gen=gen, seed=11)
    rowmag = (A.double().abs() @ Bt.double().abs().t())  # sum |a||b|: the scale fp32 accumulation error is relative to
    err = (res.double() - ref).abs()
    assert torch.isfinite(res).all()
    assert float((err / rowmag.clamp(min=1e-300)).max()) <= 2e-6


def test_gemm_nt_special_values(dev):
    """inf / nan / +-FLT_MAX rows give the result class of the fp32 product; ordinary rows beside them stay exact."""
    from tf2_gnn_amd import ops

    M, N, K = 130, 128, 64
    g = torch.Generator().manual_seed(5)
    A = torch.randn((M, K), generator=g)
    Bt = torch.randn((N, K), generator=g) * 0.1
    fmax = torch.finfo(torch.float32).max
    A[1, 7] = float("inf")
    A[2, 9] = float("nan")
    A[3, :] = -fmax           # empty-segment rows of a max aggregation (reference edge case)
    A[4, 11] = fmax
    A[6, :] = 1e-42           # subnormals
    ref = A.double() @ Bt.double().t()
    a_op, b_op = ops.sp_split_rows(A.to(dev)), ops.sp_split_rows(Bt.to(dev))
    res = ops.sp_gemm_nt(a_op, b_op).cpu()
    assert torch.isnan(res[2]).all()
    assert (torch.isinf(res[1]) | torch.isnan(res[1])).all()
    ok = torch.ones(M, dtype=torch.bool)
    ok[[1, 2, 3, 4]] = False
    assert_close(res[ok], ref[ok].float(), tol=1e-5, what="ordinary rows beside special rows")
    # +-FLT_MAX rows: the fp32 product saturates to +-inf or stays finite and huge; same sign and class as fp64 clipped
    big = res[[3, 4]]
    refb = ref[[3, 4]]
    assert torch.equal(torch.sign(big[torch.isfinite(big)].double()), torch.sign(refb[torch.isfinite(big)]))
    fin = torch.isfinite(big) & (refb.abs() < 1e38)
    mag = (A.double().abs() @ Bt.double().abs().t())[[3, 4]]  # these rows cancel heavily: error relative to sum |a||b|
    assert float(((big.double() - refb)[fin].abs() / mag[fin]).max()) <= 1e-6


# ---- weight-gradient (TN) product and the producers of tensor-scaled operands --------------------------------------
@pytest.mark.parametrize("K,M,N,a0,b0", [(3000, 128, 320, 0, 0), (1000, 256, 128, 64, 16), (77, 128, 256, 0, 0),
                                         (5003, 1280, 320, 0, 0)])
def test_gemm_tn_matches_fp64(dev, K, M, N, a0, b0):
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(K + M + N)
    X = torch.randn((K, a0 + M + 32), generator=g)
    G = torch.randn((K, b0 + N + 16), generator=g) * 1e-4     # gradients are small
    G[::7] *= 30.0
    rows = torch.randn((K, 1), generator=g)
    for spread, bound in ((2.0, 6e-7), (4.0, 3e-5)):
        # rows (= k) on different scales: the per-k factors at work.  exp(2 N(0,1)): rows spread over 2^+-9 - every term
        # keeps its 22 bits; exp(4 N(0,1)) (with the x30 rows of G): 2^+-20 - rows more than 2^13 below the largest
        # scale product lose low bits gracefully, rows 2^24 below drop out: the documented limit of the format
        # (csrc/gemm_sp.hip sp_tn_factors_kernel), not reached by the node states / gradients of one batch
        Xs = X * torch.exp(rows * spread)
        xs = ops.sp_split_rows(Xs.to(dev), scale_block=32)  # up to four scale blocks per 128-column tile
        gs = ops.sp_split_rows(G.to(dev))
        out = ops.sp_gemm_tn(xs, gs, a_cols=(a0, M), b_cols=(b0, N)).cpu()
        ref = Xs[:, a0:a0 + M].double().t() @ G[:, b0:b0 + N].double()
        mag = Xs[:, a0:a0 + M].double().abs().t() @ G[:, b0:b0 + N].double().abs()
        e = float(((out.double() - ref).abs() / mag).max())
        print(f"tn {K}x{M}x{N} row spread exp({spread} N): max err / sum|a||b| = {e:.2e}")
        assert e <= bound, (spread, e)
    scale = float(ref.abs().max())
    assert_close(out / scale, (ref / scale).float(), tol=1e-5, what=f"sp tn {K}x{M}x{N}")


def test_gemm_tn_scatter_layout_and_accumulate(dev):
    """dW of stacked kernels [L, D, H] from m = (l, h), n = d, and accumulation into an existing gradient."""
    from tf2_gnn_amd import ops

    L, D, H, V = 4, 128, 64, 900
    g = torch.Generator().manual_seed(9)
    X = torch.randn((V, D), generator=g)
    G = torch.randn((V, L * H), generator=g) * 0.01
    ref = torch.einsum("vd,vlh->ldh", X.double(), G.double().view(V, L, H))
    xs = ops.sp_split_rows(X.to(dev))
    gs = ops.sp_split_rows(G.to(dev), scale_block=H)
    dW = torch.zeros((L, D, H), device=dev)
    ops.sp_gemm_tn(gs, xs, out=dW, scatter=(H, D * H, 1, H))
    assert_close(dW.cpu(), ref.float(), tol=1e-5, what="dW [L, D, H]")
    ops.sp_gemm_tn(gs, xs, out=dW, scatter=(H, D * H, 1, H), accumulate=True)
    assert_close(dW.cpu(), (2 * ref).float(), tol=1e-5, what="dW accumulated")


@pytest.mark.parametrize("width", [32, 64, 128, 256, 320, 512])
@pytest.mark.parametrize("fixed", [False, True])
def test_gather_sp_matches_fp32_gather(dev, width, fixed):
    """The SP16-writing gather against the fp32 gather of the same view: identical sums (same kernel, same order), so
    the decoded operand must equal the fp32 result to the format's 2^-22, scales being powers of two; hubs (item and
    multi-item rows) and empty buckets included."""
    from tests.helpers import random_graph, to_dev
    from tf2_gnn_amd import ops

    V, L = 700, 3
    adjs = random_graph(V, 9000, L, seed=width, hub=(5, 2500))
    gr = ops.Graph(to_dev(adjs, dev), V)
    g = torch.Generator().manual_seed(width)
    X = (torch.randn((V, width), generator=g) * torch.exp(torch.randn((V, 1), generator=g) * 3)).to(dev)
    rs = gr.array(ops.G_INVDEG_BY_DST)
    XL = (torch.randn((V * L, width), generator=g) * torch.exp(torch.randn((V * L, 1), generator=g) * 3)).to(dev)
    for view, scale in ((ops.VIEW_BY_DST_TYPED, rs), (ops.VIEW_BY_SRC_TYPED, None), (ops.VIEW_BY_DST_NODE, None)):
        inp = XL if view == ops.VIEW_BY_DST_NODE else X  # node views gather rows (source, type) of a [V * L, .] tensor
        ref = ops.graph_gather(gr, view, inp, row_scale=scale).cpu().double().numpy()
        fixed_inv = ops.tensor_inv_scale(ops.absmax(torch.from_numpy(ref).float().to(dev), scale=2.0)) if fixed else None
        R = L if view != ops.VIEW_BY_DST_NODE else 1
        op = ops.graph_gather_sp(gr, view, inp, row_scale=scale, fixed_inv_scale=fixed_inv, rows_per_operand_row=R)
        if fixed:
            op = ops.SplitOperand(op.data, op.inv_scale.expand(op.rows, 1).contiguous(), op.rows, op.cols, op.cols)
        rec = decode_sp16(op).reshape(ref.shape)
        rowmax = np.abs(ref).max(axis=1, keepdims=True) if not fixed else np.full((ref.shape[0], 1), np.abs(ref).max() * 2)
        bound = np.maximum(np.abs(ref) * 2.0 ** -22, rowmax * 2.0 ** -37)
        assert np.all(np.abs(rec - ref) <= bound), (view, float(np.max(np.abs(rec - ref) / np.maximum(bound, 1e-300))))


@pytest.mark.parametrize("width", [64, 128, 512])
def test_gather_sp_compact_views_equal_a_split_pass_over_the_fp32_gather(dev, width):
    """Compact views (one row per NON-EMPTY bucket, type-major) written as a split operand - RGIN's d(MLP outputs) at configs[4]:
    the same bytes and scales as sp_split_rows over the fp32 gather of the view (same sums in the same order, same scale rule);
    edge weights, hub buckets (item and multi-item rows), empty buckets."""
    from tests.helpers import random_graph, to_dev
    from tf2_gnn_amd import ops

    V, L = 900, 6
    adjs = random_graph(V, 7000, L, seed=width, hub=(3, 3000))
    gr = ops.Graph(to_dev(adjs, dev), V, parts=ops.G_PARTS_DEFAULT)
    g = torch.Generator().manual_seed(width)
    X = (torch.randn((V, width), generator=g) * torch.exp(torch.randn((V, 1), generator=g) * 3)).to(dev)
    ew = torch.rand(gr.num_edges, generator=g).to(dev)
    for view, by_src in ((ops.VIEW_BY_SRC_TYPED_COMPACT, True), (ops.VIEW_BY_DST_TYPED_COMPACT, False)):
        nz = int(gr.nonempty_offsets(by_src)[-1])
        assert 0 < nz < V * L
        for w in (None, ew):
            ref32 = ops.graph_gather(gr, view, X, edge_weight=w)
            assert tuple(ref32.shape) == (nz, width)
            ref = ops.sp_split_rows(ref32)
            op = ops.graph_gather_sp(gr, view, X, edge_weight=w)
            assert (op.rows, op.cols, op.scale_block) == (nz, width, width)
            assert torch.equal(op.inv_scale.view(-1), ref.inv_scale.view(-1))
            assert torch.equal(op.data.view(torch.float16).float(), ref.data.view(torch.float16).float())  # (+0 == -0)
    with pytest.raises(ValueError):
        ops.graph_gather_sp(gr, ops.VIEW_BY_SRC_TYPED_COMPACT, X, rows_per_operand_row=L)


def test_absmax(dev):
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(1)
    for n in (1, 3, 1000, 123457):
        x = torch.randn(n, generator=g) * 5
        assert float(ops.absmax(x.to(dev)).cpu()) == float(x.abs().max())
        assert float(ops.absmax(x.to(dev), scale=2.0).cpu()) == float(2.0 * x.abs().max())


def test_dropout_writes_the_same_split_operand_as_a_split_pass(dev):
    """ops.dropout_forward in f16x2 mode: y and mask bit-equal to the flat kernel, SP16 bytes and scales bit-equal to
    sp_split_rows(y); the memo hands the operand out for that tensor only while its version is unchanged.  The narrow and odd
    shapes end in a partial group of 16 rows and stop inside a template instance's width (the ``c < cols`` guard): 32 and 48
    columns in the two-float4 instance, 272 in the five-, 336 in the eight-float4 one."""
    from tf2_gnn_amd import ops

    for rows, cols in ((1000, 320), (37, 64), (513, 512), (5, 128), (17, 32), (19, 48), (33, 272), (21, 336)):
        x = torch.randn((rows, cols), device=dev)
        x[0] = 0.0
        ops.set_gemm_mode("bf16x3")
        y0, m0 = ops.dropout_forward(x, 0.1, 1234)
        ops.set_gemm_mode("f16x2")
        try:
            y1, m1 = ops.dropout_forward(x, 0.1, 1234)
            op = ops.sp_rows_of(y1)
            ref = ops.sp_split_rows(y1)
            assert torch.equal(y0, y1) and torch.equal(m0, m1)
            # the pieces of a dropped negative element are (-0, +0) here and (+0, -0) from the split pass: compare values
            assert op is not ref and torch.equal(op.inv_scale.view(-1), ref.inv_scale.view(-1))
            assert np.array_equal(decode_sp16(op), decode_sp16(ref))
            assert ops.sp_rows_of(y1) is op
            y1.mul_(2.0)  # version bump: the remembered operand is stale
            assert ops.sp_rows_of(y1) is not op
        finally:
            ops.set_gemm_mode("bf16x3")
    keep = float((m0 != 0).float().mean())
    assert abs(keep - 0.9) < 0.05


@pytest.mark.parametrize("M,N,K,grad,want_fp32", [(300, 320, 1280, False, True), (1000, 320, 320, True, False), (129, 128, 64, True, True),
                                                  (2050, 256, 336, False, False), (64, 320, 16, True, True)])
def test_gemm_nt_split_result_equals_a_split_pass_over_the_fp32_result(dev, M, N, K, grad, want_fp32):
    """tfgnn_sp_gemm_nt_sp: the epilogue writes the result as an SP16 operand (one scale per row over all N columns -
    two waves exchange their half-row maxima).  It must be the split of exactly the values the fp32 epilogue stores."""
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn((M, K), generator=g)
    A[3] = 0.0  # a zero row: smallest-normal scale, zero pieces
    A[5] *= 1e-20
    Bt = torch.randn((N, K), generator=g) * 0.05
    mul = ((torch.rand((M, N), generator=g) > 0.2).float() * 1.25).to(dev) if grad else None
    saved = torch.tanh(torch.randn((M, N), generator=g)).to(dev) if grad else None
    a_op, b_op = ops.sp_split_rows(A.to(dev)), ops.sp_split_rows(Bt.to(dev))
    kw = dict(act=None if grad else "relu", out_mul=mul, act_grad=None if saved is None else ("tanh", saved))
    plain = ops.sp_gemm_nt(a_op, b_op, **kw)
    out, op = ops.sp_gemm_nt_split(a_op, b_op, want_fp32=want_fp32, **kw)
    ref = ops.sp_split_rows(plain)
    if want_fp32:
        assert torch.equal(out, plain)
        assert ops.sp_rows_of(out) is op
    else:
        assert out is None
    assert op.scale_block == N and torch.equal(op.inv_scale.view(-1), ref.inv_scale.view(-1))
    assert np.array_equal(decode_sp16(op), decode_sp16(ref))


def test_both_nt_front_ends_hand_the_kernel_the_same_arguments(dev):
    """``sp_gemm_nt`` and ``sp_gemm_nt_split`` are front ends of one call of tfgnn_sp_gemm_nt_rows: with an activation AND a
    multiplier in the epilogue, over one full 128-row tile plus a ragged one, the fp32 results are the same bits, and the
    fp32 tensor of the split front end remembers its split form."""
    from tf2_gnn_amd import ops

    M, K, N = 130, 64, 128
    g = torch.Generator().manual_seed(130)
    a_op = ops.sp_split_rows(torch.randn((M, K), generator=g).to(dev))
    b_op = ops.sp_split_rows((torch.randn((N, K), generator=g) * 0.05).to(dev))
    mul = ((torch.rand((M, N), generator=g) > 0.2).float() * 1.25).to(dev)
    plain = ops.sp_gemm_nt(a_op, b_op, act="relu", out_mul=mul)
    out, op = ops.sp_gemm_nt_split(a_op, b_op, act="relu", out_mul=mul, want_fp32=True)
    assert tuple(plain.shape) == (M, N) and bool((plain > 0).any())
    assert torch.equal(out, plain)
    assert ops.sp_rows_of(out) is op


def test_gemm_nt_split_result_over_several_column_tiles_carries_one_scale_per_tile(dev):
    """Round 5: N = 512 = two column tiles of 256 - the split form of the result has scale blocks of 256 columns and equals a
    split pass over the fp32 result with that block size; it feeds the next product as an operand with per-block scales."""
    from tf2_gnn_amd import ops

    gen = torch.Generator().manual_seed(4)
    A = torch.randn((700, 512), generator=gen).to(dev)
    W = (torch.randn((512, 512), generator=gen) * 0.05).to(dev)
    out, op = ops.sp_gemm_nt_split(ops.sp_split_rows(A), ops.sp_split_rows(W), act="relu")
    assert op.scale_block == 256 and tuple(op.inv_scale.shape) == (700, 2)
    ref = ops.sp_split_rows(out, scale_block=256)
    assert torch.equal(op.data, ref.data) and torch.equal(op.inv_scale, ref.inv_scale)
    nxt = ops.sp_gemm_nt(op, ops.sp_split_rows(W))
    exact = torch.relu(A.double() @ W.double().t()) @ W.double().t()
    assert float((nxt.double() - exact).abs().max()) <= 1e-5 * max(1.0, float(exact.abs().max()))


@pytest.mark.parametrize("sizes", [[300, 5, 128, 0, 1000, 129], [4000], [1, 1, 1]])
@pytest.mark.parametrize("H", [512, 128])
def test_grouped_products_on_split_operands(dev, sizes, H):
    """tfgnn_sp_gemm_nt_grouped (configs[4]: the per-relation MLP of RGIN over the non-empty (source, type) rows): every group
    multiplies its own weight operand; rows read through a row -> node index; relu + split-form output of the hidden layer,
    the second layer on that operand, the input-gradient product with relu' of the saved hidden activations - against fp64,
    and the grouped form equals the per-group calls of the plain product bit for bit."""
    from tf2_gnn_amd import ops

    G = len(sizes)
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    R, V = off[-1], 900
    gen = torch.Generator().manual_seed(R + H)
    X = torch.randn((V, H), generator=gen)
    node = torch.randint(0, V, (R,), generator=gen).int()
    W1 = torch.randn((G, H, H), generator=gen) * 0.06
    W2 = torch.randn((G, H, H), generator=gen) * 0.06
    groups = ops.RowGroups(off, dev)
    assert groups.num_tiles == sum((n + 127) // 128 for n in sizes)
    x_sp = ops.sp_split_rows(X.to(dev))
    w1t = ops.sp_split_rows(W1.transpose(1, 2).contiguous().view(G * H, H).to(dev))  # group g: W1_g^T [out, in]
    w2t = ops.sp_split_rows(W2.transpose(1, 2).contiguous().view(G * H, H).to(dev))
    hid32, hid_sp = ops.sp_gemm_nt_grouped(x_sp, w1t, groups, a_rows=node.to(dev), act="relu", want_split=True)
    # the weight operand as column blocks of ONE transposed split of the stacked kernels (one launch; scales shared by groups)
    w1c = ops.sp_split_cols(W1.contiguous().view(G * H, H).to(dev))
    hid32_c, _ = ops.sp_gemm_nt_grouped(x_sp, w1c, groups, a_rows=node.to(dev), act="relu", b_column_blocks=True)
    y32, _ = ops.sp_gemm_nt_grouped(hid_sp, w2t, groups)
    Xc = X.double()[node.long()]
    hid_ref = torch.cat([torch.relu(Xc[off[g]:off[g + 1]] @ W1[g].double()) for g in range(G)])
    y_ref = torch.cat([hid_ref[off[g]:off[g + 1]] @ W2[g].double() for g in range(G)])
    assert_close(hid32.cpu(), hid_ref.float(), tol=1e-5, what="grouped sp nt hidden")
    assert_close(hid32_c.cpu(), hid_ref.float(), tol=1e-5, what="grouped sp nt hidden (column-block weights)")
    assert_close(y32.cpu(), y_ref.float(), tol=2e-5, what="grouped sp nt output")
    bn = ops.sp_tile_width(H)
    ref_sp = ops.sp_split_rows(hid32, scale_block=bn)
    assert torch.equal(hid_sp.data, ref_sp.data) and torch.equal(hid_sp.inv_scale, ref_sp.inv_scale)
    # input gradient of the second layer with relu'(hidden): dH = (dY @ W2_g^T) * (hidden > 0), split form only
    dY = torch.randn((R, H), generator=gen)
    w2r = ops.sp_split_rows(W2.contiguous().view(G * H, H).to(dev))  # group g: W2_g [in, out] = the [N = in, K = out] operand
    _, dh_sp_only = ops.sp_gemm_nt_grouped(ops.sp_split_rows(dY.to(dev)), w2r, groups, act_grad=("relu", hid32), want_fp32=False,
                                           want_split=True)
    dh32, dh_sp = ops.sp_gemm_nt_grouped(ops.sp_split_rows(dY.to(dev)), w2r, groups, act_grad=("relu", hid32), want_split=True)
    assert torch.equal(dh_sp_only.data, dh_sp.data) and torch.equal(dh_sp_only.inv_scale, dh_sp.inv_scale)
    dh_ref = torch.cat([(dY.double()[off[g]:off[g + 1]] @ W2[g].double().t()) for g in range(G)]) * (hid_ref > 0)
    flips = (hid32.cpu() > 0) != (hid_ref > 0)  # (units at the relu kink may decide differently in fp32)
    err = ((dh32.cpu().double() - dh_ref).abs() / dh_ref.abs().clamp(min=1.0))[~flips]
    assert float(err.max()) <= 1e-5 if err.numel() else True
    ref_sp = ops.sp_split_rows(dh32, scale_block=bn)
    # (relu' makes exact zeros with either sign - (negative) x 0 - and the two kernels round the low piece of a -0 to different
    # zeros: compare the fp16 VALUES)
    assert torch.equal(dh_sp.data.view(torch.float16).float(), ref_sp.data.view(torch.float16).float())
    assert torch.equal(dh_sp.inv_scale, ref_sp.inv_scale)
    # the kernel gradients of all groups in one launch (tfgnn_sp_gemm_tn_grouped): dW1_g = Xc_g^T dH_g, dW2_g = hidden_g^T dY_g
    xc_sp = ops.sp_gather_rows(x_sp, node.to(dev))
    dY_sp = ops.sp_split_rows(dY.to(dev))
    dW2 = ops.sp_gemm_tn_grouped(hid_sp, dY_sp, groups, torch.empty((G, H, H), device=dev)).cpu()
    dW1 = ops.sp_gemm_tn_grouped(dh_sp, xc_sp, groups, torch.empty((G, H, H), device=dev), transposed=True).cpu()
    # (against the fp32 values the operands were split from: in a group of one row an entry of the product is ONE a * b, and the
    # fp32 rounding of a nearly cancelled hidden unit is not small relative to that unit)
    dh_val, hid_val = dh32.cpu().double(), hid32.cpu().double()
    for g in range(G):
        sl = slice(off[g], off[g + 1])
        for got, ref, mag in ((dW2[g], hid_val[sl].t() @ dY.double()[sl], hid_val[sl].abs().t() @ dY.double()[sl].abs()),
                              (dW1[g], Xc[sl].t() @ dh_val[sl], Xc[sl].abs().t() @ dh_val[sl].abs())):
            if sizes[g] == 0:
                assert not bool(got.any())
            else:
                assert float(((got.double() - ref).abs() / mag.clamp(min=1e-30)).max()) <= 3e-6, g
    # group by group with the plain product: the same bits
    assert torch.equal(xc_sp.data, x_sp.data[node.long().to(dev)]) and torch.equal(xc_sp.inv_scale, x_sp.inv_scale[node.long().to(dev)])
    for g in range(G):
        if sizes[g] == 0:
            continue
        sl = slice(off[g], off[g + 1])
        part = ops.SplitOperand(xc_sp.data[sl], xc_sp.inv_scale[sl], sizes[g], H, xc_sp.scale_block)
        wg = ops.SplitOperand(w1t.data[g * H:(g + 1) * H], w1t.inv_scale[g * H:(g + 1) * H], H, H, H)
        try:
            ops.sp_gemm_nt_splitk(False)  # (a stand-alone product of few tiles would split K in its launch)
            assert torch.equal(ops.sp_gemm_nt(part, wg, act="relu"), hid32[sl])
        finally:
            ops.sp_gemm_nt_splitk(True)


@pytest.mark.parametrize("K,M,N,sb", [(3000, 320, 320, 0), (777, 64, 128, 0), (5000, 512, 512, 256), (29999, 128, 128, 0), (2016 * 3 + 5, 512, 256, 128)])
def test_gemm_tn_wide_range_form(dev, K, M, N, sb):
    """tfgnn_sp_gemm_tn_wide (round 5): per-k factors on BOTH operands' fragments.  Same numbers as the one-factor product on
    ordinary operands; with each operand's row scales spread over 2^18 (their products over 2^36 - the one-factor form flags
    that and loses the small rows) or one operand's alone over 2^36 (round 6: the two factors share a pair's deficit) the
    result stays within 2e-6 of sum |a||b| per entry and the guard stays quiet; a row 2^60 below the rest of its operand
    still trips it.  Also transposed scatter and accumulation."""
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    ops.set_gemm_mode("f16x2")
    gen = torch.Generator().manual_seed(K + M)
    a = torch.randn((K, M), generator=gen)
    b = torch.randn((K, N), generator=gen)

    def run(a_, b_, **kw):
        return ops.sp_gemm_tn(ops.sp_split_rows(a_.to(dev), scale_block=sb), ops.sp_split_rows(b_.to(dev)), wide=True, **kw).cpu()

    def rel(got, a_, b_):
        ref = a_.double().t() @ b_.double()
        mag = a_.double().abs().t() @ b_.double().abs()
        return float(((got.double() - ref).abs() / mag.clamp(min=1e-300)).max())

    assert rel(run(a, b), a, b) <= 2e-6
    plain = ops.sp_gemm_tn(ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev))).cpu()
    assert float((run(a, b) - plain).abs().max()) <= 1e-5 * float(plain.abs().max())
    torch.cuda.synchronize()
    assert lib.tfgnn_sp_spread_flag(0) == 0
    # rows spread over 2^18 in EACH operand, independently
    sa = torch.exp2(torch.randint(-18, 1, (K, 1), generator=gen).float())
    sb_ = torch.exp2(torch.randint(-18, 1, (K, 1), generator=gen).float())
    a2, b2 = a * sa, b * sb_
    a2[::7] = 0.0
    b2[3::11] = 0.0
    assert rel(run(a2, b2), a2, b2) <= 2e-6
    torch.cuda.synchronize()
    assert lib.tfgnn_sp_spread_flag(0) == 0 and ops.get_gemm_mode() == ops.GEMM_F16X2
    out = torch.randn((N, M), generator=gen).to(dev)  # transposed, accumulating
    base = out.clone()
    got = ops.sp_gemm_tn(ops.sp_split_rows(a2.to(dev), scale_block=sb), ops.sp_split_rows(b2.to(dev)), wide=True, out=out,
                         scatter=(M, 0, 1, M), accumulate=True)
    ref = (a2.double().t() @ b2.double()).t() + base.cpu().double()
    mag = (a2.double().abs().t() @ b2.double().abs()).t() + base.cpu().double().abs()
    assert float(((got.cpu().double() - ref).abs() / mag).max()) <= 2e-6
    # operands longer than one launch covers (512 K ranges: 10^6 node rows) run as consecutive row ranges adding into out
    if K > 2500:
        out2 = base.clone().to(dev)
        try:
            ops.TN_WIDE_MAX_ROWS, keep = 2016, ops.TN_WIDE_MAX_ROWS
            ops.sp_gemm_tn(ops.sp_split_rows(a2.to(dev), scale_block=sb), ops.sp_split_rows(b2.to(dev)), wide=True, out=out2,
                           scatter=(M, 0, 1, M), accumulate=True)
        finally:
            ops.TN_WIDE_MAX_ROWS = keep
        assert float(((out2.cpu().double() - ref).abs() / mag).max()) <= 2e-6
    # ONE operand's rows spread over 2^36, the other's over 2^4 (attention-pooled gradients against node states: configs[2] /
    # configs[3]): the deficit of a pair of rows is split between the two factors (round 6), nothing is lost, the guard is quiet
    sa36 = torch.exp2(torch.randint(-36, 1, (K, 1), generator=gen).float())
    a4, b4 = a * sa36, b * torch.exp2(torch.randint(-4, 1, (K, 1), generator=gen).float())
    a4[2::9] = 0.0
    assert rel(run(a4, b4), a4, b4) <= 2e-6
    a5, b5 = a * torch.exp2(torch.randint(-4, 1, (K, 1), generator=gen).float()), b * sa36  # ... and the other way round
    b5[1::13] = 0.0
    assert rel(run(a5, b5), a5, b5) <= 2e-6
    torch.cuda.synchronize()
    assert lib.tfgnn_sp_spread_flag(0) == 0 and ops.get_gemm_mode() == ops.GEMM_F16X2
    # a row 2^30 below its neighbours is carried by both factors (2^15 each): still quiet; 2^60 below: reported
    a3 = a.clone()
    a3[5] *= 2.0 ** -30
    assert rel(run(a3, b), a3, b) <= 2e-6
    torch.cuda.synchronize()
    assert lib.tfgnn_sp_spread_flag(0) == 0
    a3[5] *= 2.0 ** -30
    run(a3, b)
    torch.cuda.synchronize()
    assert lib.tfgnn_sp_spread_flag(0) == 1
    ops.set_gemm_mode("f16x2")  # re-arm


@pytest.mark.parametrize("K,M,N", [(3000, 320, 320), (777, 64, 128), (2000, 336, 256), (30000, 320, 320), (29999, 128, 128)])
def test_gemm_tn_row_count_not_a_multiple_of_the_tile(dev, K, M, N):
    """M % 128 != 0 (dW of a 320 x 320 Dense kernel): the last row tile runs past M and its surplus rows stay in the
    workspace; both operands with one scale per row, as the product epilogues write them."""
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(K + M)
    X = torch.randn((K, M), generator=g) * torch.exp(torch.randn((K, 1), generator=g))
    G = torch.randn((K, N), generator=g) * 1e-3
    out = ops.sp_gemm_tn(ops.sp_split_rows(X.to(dev)), ops.sp_split_rows(G.to(dev))).cpu()
    ref = X.double().t() @ G.double()
    mag = X.double().abs().t() @ G.double().abs()
    e = float(((out.double() - ref).abs() / mag).max())
    assert out.shape == (M, N) and e <= 6e-7, e
    # into a strided destination (the [in, out] kernel of a Dense layer from dW^T = G^T X)
    dW = torch.zeros((N, M), device=dev)
    ops.sp_gemm_tn(ops.sp_split_rows(X.to(dev)), ops.sp_split_rows(G.to(dev)), out=dW, scatter=(M, 0, 1, M))
    assert torch.equal(dW.cpu().t(), out)


@pytest.mark.parametrize("C", [64, 128, 256])
def test_narrow_row_split_equals_the_general_kernel(dev, C):
    """rows of 64 / 128 / 256 columns take a one-pass kernel from 4096 rows on: same bytes and scales as the general kernel
    (run here on chunks below that size), padded source rows, special values included."""
    from tf2_gnn_amd import ops

    R = 9001
    g = torch.Generator().manual_seed(C)
    full = torch.randn((R, C + 8), generator=g) * torch.exp(torch.randn((R, 1), generator=g) * 4)
    full[5] = 0.0
    full[6, 3] = float("inf")
    full[7, 9] = float("nan")
    x = full.to(dev)[:, :C]
    whole = ops.sp_split_rows(x)
    for r0 in range(0, R, 4000):
        part = ops.sp_split_rows(x[r0 : r0 + 4000])
        assert torch.equal(whole.data[r0 : r0 + 4000], part.data)
        assert torch.equal(whole.inv_scale[r0 : r0 + 4000].view(-1), part.inv_scale.view(-1))


def test_small_passes_sharing_one_launch_equal_their_stand_alone_kernels(dev, monkeypatch):
    """tfgnn_aux_launch (round 4): weight splits built as jobs and launched together in ONE launch (``ops.aux_flush``) give
    bit-identical results to the kernels of their own - the operands, and everything the products around them compute."""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import make_synthetic_batch

    g = torch.Generator().manual_seed(11)
    W = (torch.randn((4, 320, 320), generator=g) * 0.1).to(dev)
    V, E, L, H = 4000, 120000, 4, 320
    feats, adjs = make_synthetic_batch(V, E, L, H, seed=2)
    X = torch.from_numpy(feats).to(dev)
    graph = ops.Graph(tuple(torch.from_numpy(a).to(dev) for a in adjs), V)
    dY = torch.randn((V, H), generator=g).to(dev)

    def run(shared_launch):
        if shared_launch:
            cj = ops.sp_split_cols_jobs(W.view(4 * 320, 320))
            rj = ops.sp_split_rows_jobs(W[0], segments=(320, 320 * 320, 4 * 320))
            ops.aux_flush([cj, rj])
            cols, rows = cj.operand, rj.operand
        else:
            cols = ops.sp_split_cols(W.view(4 * 320, 320))
            rows = ops.sp_split_rows(W[0], segments=(320, 320 * 320, 4 * 320))
        A = ops.graph_gather_sp(graph, ops.VIEW_BY_DST_TYPED, X, rows_per_operand_row=L)  # long buckets
        Y = ops.sp_gemm_nt(A, cols, act="relu")
        G = ops.graph_gather_sp(graph, ops.VIEW_BY_SRC_TYPED, dY, rows_per_operand_row=L)
        dW = torch.empty_like(W)
        ops.sp_gemm_tn(G, ops.sp_split_rows(X), out=dW, scatter=(H, 320 * H, 1, H))
        dX = ops.sp_gemm_nt(G, rows)
        return [cols.data, cols.inv_scale, rows.data, rows.inv_scale, A.data, A.inv_scale, Y, G.data, G.inv_scale, dW, dX]

    ref = [t.clone() for t in run(False)]
    got = [t.clone() for t in run(True)]
    names = ["W^T sp", "W^T inv", "W rows sp", "W rows inv", "A sp", "A inv", "Y", "G sp", "G inv", "dW", "dX"]
    for n, a, b in zip(names, got, ref):
        assert torch.equal(a, b), n
    graph.close()


def test_two_pass_weight_split_launches_on_the_stream_it_was_deferred_for(dev, monkeypatch):
    """A long-K weight split launched under a side stream: exactly two launches (the column maxima, then the split), both on
    that stream, and the operand is the one-pass split's, bit for bit.  Nothing is left behind: a library call on the main
    stream afterwards launches no small pass.  (The jobs used to wait in a queue that a call from ANOTHER stream could flush;
    they are launched where they are built now, so that cannot happen.)"""
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    K, N = 40 * 64, 256
    assert lib.tfgnn_sp_split_cols_two_pass_bytes(K, N) > 0
    g = torch.Generator().manual_seed(17)
    w = (torch.randn((K, N), generator=g) * torch.exp(torch.randn((1, N), generator=g) * 3)).to(dev)
    ref = ops.sp_split_cols(w)
    torch.cuda.synchronize()
    launches = []
    real = lib.tfgnn_aux_launch

    def spy(jobs, n, stream):
        launches.append((getattr(stream, "value", stream), [int(jobs[i].kind) for i in range(n)]))
        return real(jobs, n, stream)

    monkeypatch.setattr(lib, "tfgnn_aux_launch", spy)
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    side.wait_stream(main)
    with torch.cuda.stream(side):
        jobs = ops.sp_split_cols_jobs(w)
        assert not launches  # building the jobs launches nothing
        ops.aux_flush([jobs])
    op = jobs.operand
    assert side.cuda_stream != main.cuda_stream
    assert [st for st, _ in launches] == [side.cuda_stream, side.cuda_stream], (launches, main.cuda_stream, side.cuda_stream)
    assert [kinds for _, kinds in launches] == [[6], [2]], launches  # AUX_COL_ABSMAX, then AUX_SPLIT_COLS (csrc/aux_jobs.hpp)
    main.wait_stream(side)
    del launches[:]
    ops.absmax(w)  # a library call on the main stream: there is nothing left for it to launch
    torch.cuda.synchronize()
    assert not launches, launches
    assert torch.equal(op.data, ref.data) and torch.equal(op.inv_scale, ref.inv_scale)


def test_layer_backward_after_a_rejected_call_builds_the_weight_operand(dev):
    """ops.mp_backward that raises on its argument checks (no split form of the layer input) must not leave an unbuilt weight
    operand in the cache: the next call with the same (never split) kernels builds it and gives dX and dW bit-equal to a
    run with an empty cache."""
    from tests.helpers import random_graph, to_dev
    from tf2_gnn_amd import ops

    V, E, L, D, H = 1200, 15000, 3, 128, 128
    g = torch.Generator().manual_seed(29)
    W = (torch.randn((L, D, H), generator=g) * 0.07).to(dev)
    X = torch.randn((V, D), generator=g).to(dev)
    d_pre = torch.randn((V, H), generator=g).to(dev)
    graph = ops.Graph(to_dev(random_graph(V, E, L, seed=29), dev), V)
    x_sp = ops.sp_split_rows(X)
    ops.clear_weight_operand_cache()
    with pytest.raises(ValueError):
        ops.mp_backward(graph, d_pre, W, None)
    dX, _, dW = ops.mp_backward(graph, d_pre, W, x_sp)
    got = (dX.clone(), dW.clone())
    ops.clear_weight_operand_cache()
    dX, _, dW = ops.mp_backward(graph, d_pre, W, x_sp)
    torch.cuda.synchronize()
    assert torch.equal(got[0], dX) and torch.equal(got[1], dW)
    graph.close()


@pytest.mark.parametrize("V,E,L,D,H", [(3000, 5000, 4, 128, 128), (1500, 2500, 8, 64, 320), (700, 20000, 3, 320, 256), (130, 90, 2, 16, 128)])
def test_product_over_pattern_ordered_rows_skipping_empty_blocks_equals_the_plain_product(dev, V, E, L, D, H):
    """tfgnn_sp_gemm_nt_dropout d_tile_kmask / d_row_map with TFGNN_VIEW_BY_DST_TYPED_PATTERN (round 4): the gather writes
    bucket (v, l) at row pos[v] of the operand, bit-identical to its row in node order; the product that skips the all-zero type
    blocks of a row tile and writes its rows back through the row map equals the product over the node-ordered operand BIT
    FOR BIT - plain, with bias + activation + dropout, and with the split-form output.  (Sparse batches: most buckets are empty;
    the dense one has a single pattern and nothing to skip; the last has a ragged single tile.)"""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import make_synthetic_batch

    feats, adjs = make_synthetic_batch(V, E, L, D, seed=V + L)
    g = ops.Graph([torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in adjs], V)
    X = torch.from_numpy(feats).to(dev)
    a_node = ops.graph_gather_sp(g, ops.VIEW_BY_DST_TYPED, X, rows_per_operand_row=L)
    a_pat = ops.graph_gather_sp(g, ops.VIEW_BY_DST_TYPED_PATTERN, X, rows_per_operand_row=L)
    node_at = g.array(ops.G_PATTERN_NODE_BY_DST)
    pos = g.array(ops.G_PATTERN_POS_BY_DST)
    kmask = g.array(ops.G_PATTERN_TILEMASK_BY_DST)
    assert kmask.dtype == torch.uint8 and kmask.numel() == (V + 127) // 128
    idx = node_at.long()
    assert torch.equal(torch.sort(idx).values, torch.arange(V, device=dev))
    assert torch.equal(pos.long()[idx], torch.arange(V, device=dev))
    assert torch.equal(a_pat.data, a_node.data[idx]) and torch.equal(a_pat.inv_scale, a_node.inv_scale[idx])
    gen = torch.Generator().manual_seed(5)
    W = (torch.randn((L * D, H), generator=gen) * 0.2).to(dev)
    w_sp = ops.sp_split_cols(W)
    bias = torch.randn(H, generator=gen).to(dev)
    ref = ops.sp_gemm_nt(a_node, w_sp)
    assert torch.equal(ops.sp_gemm_nt(a_pat, w_sp, row_map=node_at), ref)               # the row map alone
    assert torch.equal(ops.sp_gemm_nt(a_pat, w_sp, tile_kmask=kmask, row_map=node_at), ref)
    ref = ops.sp_gemm_nt(a_node, w_sp, bias=bias, act="relu", dropout=(0.2, 77))
    got = ops.sp_gemm_nt(a_pat, w_sp, bias=bias, act="relu", dropout=(0.2, 77), tile_kmask=kmask, row_map=node_at)
    assert torch.equal(got, ref)
    ref32, ref_op = ops.sp_gemm_nt_split(a_node, w_sp, act="tanh", dropout=(0.1, 3))
    got32, got_op = ops.sp_gemm_nt_split(a_pat, w_sp, act="tanh", dropout=(0.1, 3), tile_kmask=kmask, row_map=node_at)
    assert torch.equal(got32, ref32) and torch.equal(got_op.data, ref_op.data) and torch.equal(got_op.inv_scale, ref_op.inv_scale)
    # the mask really describes the operand: a cleared bit = an all-zero block in every row of the tile
    blocks = a_pat.data.view(V, L, D * 4)
    for t in range(kmask.numel()):
        m = int(kmask[t])
        rows = blocks[t * 128:(t + 1) * 128]
        for l in range(L):
            if not (m >> l) & 1:
                assert not bool(rows[:, l].any()), (t, l)
    g.close()


@pytest.mark.parametrize("V,E,L,H,D", [(3000, 5000, 4, 128, 128), (1500, 2500, 8, 64, 320), (20000, 60000, 4, 320, 320), (130, 90, 2, 16, 128)])
def test_input_gradient_product_reading_its_rows_in_by_source_pattern_order_equals_the_plain_product(dev, V, E, L, H, D):
    """Round 5 (tfgnn_sp_gemm_nt_rows): the by-source sums [G_0|..|G_{L-1}] stay in node order; the product reads its rows through
    TFGNN_G_PATTERN_NODE_BY_SRC, skips the all-zero type blocks of a row tile (TFGNN_G_PATTERN_TILEMASK_BY_SRC) and writes node
    order again - BIT-EQUAL to the plain product: alone, with the gradient epilogue (mask x act'(saved)), accumulating, with
    dropout recomputed, and with the split-form output.  (Small cases also split K inside the launch, both ways alike.)"""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import make_synthetic_batch

    _, adjs = make_synthetic_batch(V, E, L, 16, seed=V + L + 1)
    g = ops.Graph([torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in adjs], V, parts=ops.G_PARTS_ALL)
    gen = torch.Generator().manual_seed(11)
    d_agg = torch.randn((V, H), generator=gen).to(dev)
    G_sp = ops.graph_gather_sp(g, ops.VIEW_BY_SRC_TYPED, d_agg, rows_per_operand_row=L)
    node_at = g.array(ops.G_PATTERN_NODE_BY_SRC)
    kmask = g.array(ops.G_PATTERN_TILEMASK_BY_SRC)
    assert torch.equal(torch.sort(node_at.long()).values, torch.arange(V, device=dev))
    assert kmask.dtype == torch.uint8 and kmask.numel() == (V + 127) // 128
    # the mask describes the operand rows the tile reads: a cleared bit = an all-zero block in every one of them
    blocks = G_sp.data.view(V, L, H * 4)[node_at.long()]
    for t in range(min(kmask.numel(), 40)):
        m = int(kmask[t])
        for l in range(L):
            if not (m >> l) & 1:
                assert not bool(blocks[t * 128:(t + 1) * 128, l].any()), (t, l)
    if V >= 1000:
        assert int((kmask.int() != (1 << L) - 1).sum()) > 0, "nothing to skip in this batch"
    W = (torch.randn((D, L * H), generator=gen) * 0.1).to(dev)
    w_sp = ops.sp_split_rows(W)
    skip = dict(tile_kmask=kmask, a_rows=node_at, row_map=node_at)
    mul = ((torch.rand((V, D), generator=gen) > 0.2).float() * 1.25).to(dev)
    saved = torch.tanh(torch.randn((V, D), generator=gen)).to(dev)
    base = torch.randn((V, D), generator=gen).to(dev)
    forms = [dict(), dict(out_mul=mul, act_grad=("tanh", saved)), dict(accumulate=True, out_mul=mul),
             dict(act_grad=("relu", saved), dropout=(0.25, 9))]

    def run(kw, **extra):
        kw = dict(kw, **extra)
        if kw.get("accumulate"):
            kw["out"] = base.clone()
        return ops.sp_gemm_nt(G_sp, w_sp, **kw)

    # bit for bit
    try:
        ops.sp_gemm_nt_splitk(False)
        assert torch.equal(run({}, a_rows=node_at, row_map=node_at), run({}))  # the index alone
        for kw in forms:
            assert torch.equal(run(kw, **skip), run(kw)), kw.keys()
        if D in (128, 256, 320):
            ref32, ref_op = ops.sp_gemm_nt_split(G_sp, w_sp, out_mul=mul, act_grad=("tanh", saved))
            got32, got_op = ops.sp_gemm_nt_split(G_sp, w_sp, out_mul=mul, act_grad=("tanh", saved), **skip)
            assert torch.equal(got32, ref32) and torch.equal(got_op.data, ref_op.data) and torch.equal(got_op.inv_scale, ref_op.inv_scale)
        plain = [run(kw) for kw in forms]
    finally:
        ops.sp_gemm_nt_splitk(True)
    g.close()


@pytest.mark.parametrize("M,N,K,sb", [(7110, 320, 960, 320), (300, 320, 1280, 0), (129, 128, 512, 0), (1000, 256, 1280, 320), (700, 640, 960, 0),
                                      (14000, 320, 480, 0)])
def test_gemm_nt_k_split_inside_the_launch(dev, M, N, K, sb):
    """Round 5: products over few row tiles split K inside their launch (include/tfgnn.h
    tfgnn_sp_gemm_nt_set_splitk_workspace): splits 1.. hand their accumulators to split 0, which adds them in split order.
    Same bound against fp64 as the unsplit product, within fp32 rounding of it, bit-reproducible over launches (the flags go
    back to zero), no reducer ever timed out - with every epilogue form."""
    from tf2_gnn_amd import ops

    def products(**kw):
        return _run(dev, M, N, K, sb=sb, **kw)

    ops.sp_gemm_nt_splitk(True)
    _, _, before = ops.sp_gemm_nt_splitk()
    res, ref, _, _ = products()
    on, timed_out, after = ops.sp_gemm_nt_splitk()
    assert on and not timed_out and after == before + 1, "the product under test did not split"
    scale = max(1.0, 0.05 * float(K) ** 0.5)
    assert_close(res / scale, (ref / scale).float(), tol=1e-5, what=f"sp nt k-split {M}x{N}x{K}")
    for _ in range(3):
        again, _, _, _ = products()
        assert torch.equal(again, res)
    full = dict(bias=True, act="tanh", acc=True, grad=True)
    res_e, ref_e, _, _ = products(**full)
    assert_close(res_e, ref_e.float(), tol=2e-5, what=f"sp nt k-split epilogue {M}x{N}x{K}")
    try:
        ops.sp_gemm_nt_splitk(False)
        plain, _, _, _ = products()
        plain_e, _, _, _ = products(**full)
        assert ops.sp_gemm_nt_splitk()[2] == after + 4  # (3 repeats + the epilogue run; none since the switch)
    finally:
        ops.sp_gemm_nt_splitk(True)
    assert float((res.double() - plain.double()).abs().max()) <= 2e-6 * scale * max(1.0, float(ref.abs().max()) / scale)
    assert float((res_e.double() - plain_e.double()).abs().max()) <= 4e-6 * max(1.0, float(ref_e.abs().max()))
    assert not ops.sp_gemm_nt_splitk()[1]


def test_tile_mask_needs_block_scales_that_tile_k(dev):
    from tf2_gnn_amd import ops

    x = torch.randn((256, 256), device=dev)
    a = ops.sp_split_rows(x)  # one scale per row: no blocks to skip
    w = ops.sp_split_cols(torch.randn((256, 128), device=dev))
    mask = torch.full((2,), 255, dtype=torch.uint8, device=dev)
    ops.sp_gemm_nt(a, w, tile_kmask=mask)  # a single block: the mask can only say "run it"
    a9 = ops.sp_split_rows(torch.randn((256, 9 * 16), device=dev), scale_block=16)
    w9 = ops.sp_split_cols(torch.randn((9 * 16, 128), device=dev))
    with pytest.raises(ValueError, match="tile mask"):
        ops.sp_gemm_nt(a9, w9, tile_kmask=mask)
    with pytest.raises(ValueError, match="tile_kmask"):
        ops.sp_gemm_nt(a, w, tile_kmask=mask[:1])
    with pytest.raises(ValueError, match="row_map"):
        ops.sp_gemm_nt(a, w, row_map=torch.zeros(5, dtype=torch.int32, device=dev))


@pytest.mark.parametrize("K,N", [(4096, 512), (20480, 512), (2560, 320), (1296, 128), (1280, 256)])
def test_two_pass_split_of_a_long_kernel_stack_equals_the_one_pass_split(dev, K, N):
    """Round 6 (BASELINE configs[4]): the transposed split of a long [K, N] stack of kernels as jobs takes its column maxima in a
    pass of its own (a job of one shared launch) and converts in the next launch - every byte read once instead of once per K
    slice.  The operand and its scales must be the one-pass split's, bit for bit; K <= 1280 keeps the one-pass job."""
    from tf2_gnn_amd import _lib, ops

    gen = torch.Generator().manual_seed(K + N)
    w = (torch.randn((K, N), generator=gen) * torch.logspace(-3, 2, N).unsqueeze(0)).to(dev)
    w[5::7, 3] = 0.0
    w[:, 8] = 0.0  # an all-zero column: the marker scale
    assert (_lib.load().tfgnn_sp_split_cols_two_pass_bytes(K, N) > 0) == (K > 1280)
    ref = ops.sp_split_cols(w)
    jobs = ops.sp_split_cols_jobs(w)
    assert bool(jobs.stage1) == (K > 1280)
    ops.aux_flush([jobs])
    got = jobs.operand
    torch.cuda.synchronize()
    assert torch.equal(got.inv_scale, ref.inv_scale) and torch.equal(got.data, ref.data)
    # and as a consumer meets it: the product right behind the split that ``sp_weight_operand`` launches
    a = ops.sp_split_rows(torch.randn((300, K), generator=gen).to(dev))
    out_ref = ops.sp_gemm_nt(a, ref)
    ops.clear_weight_operand_cache()
    out = ops.sp_gemm_nt(a, ops.sp_weight_operand(w, "cols", lambda: ops.sp_split_cols_jobs(w)))
    assert torch.equal(out, out_ref)


def test_xcd_aware_tile_order_of_products_over_several_column_tiles_is_bit_identical(dev):
    """Round 6 (csrc/gemm_sp.hip, SpArgs::xcd_per): products over two or four column tiles (configs[4] N = 512, rgat N = 1024)
    hand their tiles to the XCDs in whole row tiles - a row tile's column tiles run on ONE XCD instead of each fetching the
    row tile's A rows over the fabric.  Same tiles, same arithmetic: the result does not depend on the order
    (TFGNN_SP_NT_XCD=0 restores the old one; the switch is read once per process, hence the two child processes)."""
    import hashlib
    import os
    import subprocess
    import sys

    code = (
        "import hashlib, torch\n"
        "from tf2_gnn_amd import ops\n"
        "dev = torch.device('cuda', 0)\n"
        "g = torch.Generator().manual_seed(11)\n"
        "h = hashlib.sha256()\n"
        "for M, N, K in ((3000, 512, 512), (2500, 1024, 256), (130, 512, 96), (4000, 256, 320)):\n"
        "    a = ops.sp_split_rows(torch.randn((M, K), generator=g).to(dev))\n"
        "    b = ops.sp_split_rows((torch.randn((N, K), generator=g) * 0.05).to(dev))\n"
        "    h.update(ops.sp_gemm_nt(a, b, act='relu').cpu().numpy().tobytes())\n"
        "sizes = [300, 0, 129, 1000, 77]\n"
        "off = [0]\n"
        "for n in sizes: off.append(off[-1] + n)\n"
        "H = 512\n"
        "X = torch.randn((off[-1], H), generator=g)\n"
        "W = torch.randn((len(sizes), H, H), generator=g) * 0.05\n"
        "groups = ops.RowGroups(off, dev)\n"
        "wt = ops.sp_split_rows(W.transpose(1, 2).contiguous().view(len(sizes) * H, H).to(dev))\n"
        "y, y_sp = ops.sp_gemm_nt_grouped(ops.sp_split_rows(X.to(dev)), wt, groups, act='relu', want_split=True)\n"
        "h.update(y.cpu().numpy().tobytes()); h.update(y_sp.data.cpu().numpy().tobytes()); h.update(y_sp.inv_scale.cpu().numpy().tobytes())\n"
        "print('DIGEST', h.hexdigest())\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    digests = []
    for knob in ("0", "1"):
        env = dict(os.environ, TFGNN_SP_NT_XCD=knob, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
        res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=root)
        assert res.returncode == 0, res.stderr[-2000:]
        digests.append([ln for ln in res.stdout.splitlines() if ln.startswith("DIGEST")][-1])
    assert digests[0] == digests[1]
    assert hashlib.sha256(b"").hexdigest() not in digests[0]
