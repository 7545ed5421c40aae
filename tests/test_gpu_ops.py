"""HIP primitives against plain fp32/fp64 references (run through the C ABI via ctypes)."""
import numpy as np
import pytest
import torch

from oracle import adjacency_oracle as ao
from oracle import tf2gnn_oracle as orc
from tests.helpers import assert_close, random_graph, to_dev

pytestmark = pytest.mark.gpu

ACTS = ["relu", "tanh", "leaky_relu", "elu", "selu", "gelu", "sigmoid"]


def _ref_act(name):
    return torch.sigmoid if name == "sigmoid" else orc.get_activation_function(name)


@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
@pytest.mark.parametrize(
    "M,N,K",
    [(64, 64, 32), (130, 320, 96), (257, 128, 1280), (33, 7, 50), (5, 121, 3), (1, 1, 1), (300, 640, 64), (100, 12, 17)],
)
def test_gemm_matches_fp64(dev, ta, tb, M, N, K):
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    B = torch.randn((N, K) if tb else (K, N), generator=g)
    ref = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    out = ops.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb)
    scale = max(1.0, float(K) ** 0.5)
    assert_close(out.cpu() / scale, (ref / scale).float(), tol=2e-6, what=f"gemm {M}x{N}x{K} ta={ta} tb={tb}")


@pytest.fixture
def gemm_mode():
    from tf2_gnn_amd import ops

    prev = ops.get_gemm_mode()
    yield ops.set_gemm_mode
    ops.set_gemm_mode(prev)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16x3_9"])
@pytest.mark.parametrize(
    "ta,tb,M,N,K",
    [
        (False, False, 1000, 320, 1280),  # forward: [V, L*D] @ [L*D, H]
        (False, True, 1000, 320, 1280),   # dX:  G_cat @ Wh^T
        (True, False, 320, 1280, 5000),   # dW:  X^T @ G_cat (split-K)
        (False, False, 129, 640, 68),     # ragged M tile, K tail
        (True, False, 324, 320, 100),     # ragged M with K-major A, K tail
        (False, True, 7, 320, 64),
        # 128 x 256 and 128 x 128 tiles (hidden sizes 128 / 256 / 512, GRU 3H = 384)
        (False, False, 900, 256, 640),
        (False, True, 515, 512, 256),
        (True, False, 256, 1024, 3000),
        (False, False, 777, 128, 640),
        (False, True, 300, 384, 128),
        (True, False, 128, 384, 2100),
        (True, False, 132, 128, 70),
    ],
)
def test_gemm_bf16x3_matches_fp64(dev, gemm_mode, mode, ta, tb, M, N, K):
    """fp32 GEMM on the bf16 matrix cores via exact operand splitting (csrc/gemm_x3.hip): same 1e-5-class
    bound against fp64 as the fp32-MFMA kernel, on operands that use all 24 significand bits."""
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn((K, M) if ta else (M, K), generator=g)
    B = torch.randn((N, K) if tb else (K, N), generator=g)
    ref = (A.double().t() if ta else A.double()) @ (B.double().t() if tb else B.double())
    gemm_mode("fp32")
    out32 = ops.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb)
    gemm_mode(mode)
    out = ops.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb)
    out_b = ops.gemm(A.to(dev), B.to(dev), trans_a=ta, trans_b=tb)
    assert torch.equal(out, out_b)
    # fp32 accumulation of K N(0,1) products: rounding noise ~ eps * sqrt(K) * sqrt(K) / sqrt(3) per output (1 sigma),
    # the maximum over 1e5 outputs sits at ~4.5 sigma -> 4e-6 * sqrt(K) absolute; and never worse than the fp32 kernel
    scale = max(1.0, float(K) ** 0.5)
    assert_close(out.cpu() / scale, (ref / scale).float(), tol=4e-6, what=f"x3 gemm {M}x{N}x{K} ta={ta} tb={tb}")
    e32 = (out32.cpu().double() - ref).abs().max().item()
    e3 = (out.cpu().double() - ref).abs().max().item()
    print(f"max|err| vs fp64: fp32-mfma {e32:.3e}  {mode} {e3:.3e}")
    assert e3 <= 1.5 * e32 + 1e-6


@pytest.mark.parametrize("mode", ["bf16x3", "bf16x3_9"])
def test_gemm_bf16x3_epilogue_and_exactness(dev, gemm_mode, mode):
    from tf2_gnn_amd import ops

    gemm_mode(mode)
    # integers: every piece product and every partial sum is exact -> bit-exact result, transposes detected
    g = torch.Generator().manual_seed(11)
    # (|a b| K < 2^24; 9-bit values exercise the h and m planes)
    A = torch.randint(-400, 400, (200, 96), generator=g).float()
    B = torch.randint(-400, 400, (96, 320), generator=g).float()
    ref = (A.double() @ B.double())
    out = ops.gemm(A.to(dev), B.to(dev))
    assert torch.equal(out.cpu().double(), ref)
    outT = ops.gemm(A.t().contiguous().to(dev), B.to(dev), trans_a=True)
    outBT = ops.gemm(A.to(dev), B.t().contiguous().to(dev), trans_b=True)
    assert torch.equal(out, outT) and torch.equal(out, outBT)
    # bias + activation + accumulate into a strided output
    bias = torch.randn(320, generator=g)
    A = torch.randn((200, 96), generator=g)
    B = torch.randn((96, 320), generator=g)
    wide = torch.ones((200, 400), device=dev)
    ops.gemm(A.to(dev), B.to(dev), bias=bias.to(dev), act="relu", out=wide[:, 40:360], accumulate=True)
    ref = torch.relu(A.double() @ B.double() + bias.double()) + 1.0
    assert_close(wide[:, 40:360].cpu(), ref.float(), tol=5e-6, what="x3 epilogue")
    assert torch.all(wide[:, :40] == 1) and torch.all(wide[:, 360:] == 1)


@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 64, 32), (4, 320, 320), (2, 33, 100), (1, 1280, 320)])
def test_transpose_batched(dev, shape):
    from tf2_gnn_amd import ops

    x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
    out = ops.transpose_batched(x.to(dev))
    assert torch.equal(out.cpu(), x.transpose(1, 2).contiguous())
    assert torch.equal(ops.transpose_batched(x[0].to(dev)).cpu(), x[0].t().contiguous())


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("act", ["relu", "tanh", "gelu", None])
@pytest.mark.parametrize("with_mask", [True, False])
def test_gemm_grad_epilogue(dev, gemm_mode, mode, act, with_mask):
    """C = (A @ B^T) * mask * act'(saved): fused into the split-operand kernel's epilogue in bf16x3 mode
    (tfgnn_gemm_grad_epilogue), separate kernels otherwise - same result either way.  Without a factor it is the plain
    product (ops.gemm)."""
    from tf2_gnn_amd import ops

    gemm_mode(mode)
    M, N, K = 1000, 320, 640
    g = torch.Generator().manual_seed(M + (7 if with_mask else 0))
    A = torch.randn((M, K), generator=g)
    B = torch.randn((N, K), generator=g) * 0.1
    mask = ((torch.rand((M, N), generator=g) > 0.1).float() / 0.9) if with_mask else None
    pre = torch.randn((M, N), generator=g)
    saved = None
    ref = A.double() @ B.double().t()
    if with_mask:
        ref = ref * mask.double()
    if act is not None:
        p64 = pre.double().requires_grad_(True)
        y = _ref_act(act)(p64)
        (dact,) = torch.autograd.grad(y.sum(), p64)
        ref = ref * dact
        saved = pre if act == "gelu" else y.detach().float()
    out = ops.gemm_grad(A.to(dev), B.to(dev), trans_b=True, out_mul=None if mask is None else mask.to(dev),
                        act_grad=None if act is None else (act, saved.to(dev)))
    scale = float(K) ** 0.5
    assert_close(out.cpu() / scale, (ref / scale).float(), tol=2e-6, what=f"gemm_grad {mode} {act} mask={with_mask}")
    # in-place form
    buf = torch.empty((M, N), device=dev)
    out2 = ops.gemm_grad(A.to(dev), B.to(dev), trans_b=True, out=buf, out_mul=None if mask is None else mask.to(dev),
                         act_grad=None if act is None else (act, saved.to(dev)))
    assert torch.equal(out2, out)
    # accumulating form: a second term of the same gradient added into the first one's result
    C0 = torch.randn((M, N), generator=g)
    buf3 = C0.to(dev)
    out3 = ops.gemm_grad(A.to(dev), B.to(dev), trans_b=True, out=buf3, accumulate=True, out_mul=None if mask is None else mask.to(dev),
                         act_grad=None if act is None else (act, saved.to(dev)))
    assert out3.data_ptr() == buf3.data_ptr()
    assert_close(out3.cpu() / scale, ((ref + C0.double()) / scale).float(), tol=2e-6, what=f"gemm_grad accumulate {mode} {act} mask={with_mask}")


@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("N,K", [(128, 128), (256, 192), (320, 64), (512, 512)])
def test_grouped_gemms_match_fp64(dev, gemm_mode, mode, N, K):
    """tfgnn_gemm_grouped_rows / _k (the per-relation multiplies over compact rows) against per-group fp64 products;
    ragged groups, an empty one, a group smaller than one tile; both GEMM modes."""
    from tf2_gnn_amd import ops

    gemm_mode(mode)
    sizes = [300, 0, 5, 777, 130, 64]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    G, R = len(sizes), int(off[-1])
    g = torch.Generator().manual_seed(N + K)
    A = torch.randn((R, K), generator=g)
    W = torch.randn((G, K, N), generator=g) * 0.1
    off_dev = torch.from_numpy(off).to(dev)
    off_h = [int(x) for x in off]
    out = ops.gemm_grouped_rows(A.to(dev), off_dev, off_h, W.to(dev), act="relu")
    Gr = torch.randn((R, N), generator=g)
    outT = ops.gemm_grouped_rows(Gr.to(dev), off_dev, off_h, W.to(dev), trans_b=True)
    dW = ops.gemm_grouped_k(A.to(dev), Gr.to(dev), off_dev, off_h, G)
    dW2 = ops.gemm_grouped_k(A.to(dev), Gr.to(dev), off_dev, off_h, G)
    assert torch.equal(dW, dW2)
    for i in range(G):
        sl = slice(off_h[i], off_h[i + 1])
        ref = torch.relu(A[sl].double() @ W[i].double())
        assert_close(out[sl].cpu(), ref.float(), tol=2e-5, what=f"grouped rows g{i}")
        refT = Gr[sl].double() @ W[i].double().t()
        assert_close(outT[sl].cpu(), refT.float(), tol=2e-5, what=f"grouped rows^T g{i}")
        refW = A[sl].double().t() @ Gr[sl].double()
        scale = max(1.0, float(refW.abs().max()))
        assert_close(dW[i].cpu() / scale, (refW / scale).float(), tol=1e-5, what=f"grouped k g{i}")
    # the input-gradient form with the derivative of the hidden activation below in the epilogue (tfgnn_gemm_grouped_rows_grad;
    # a separate pass where the kernel has no such epilogue): the same bits as the product followed by activation_backward
    saved = torch.relu(torch.randn((R, K), generator=g)).to(dev)
    fused = ops.gemm_grouped_rows(Gr.to(dev), off_dev, off_h, W.to(dev), trans_b=True, act_grad=("relu", saved))
    assert torch.equal(fused, ops.activation_backward("relu", outT, saved))
    saved_t = torch.tanh(torch.randn((R, K), generator=g)).to(dev)
    fused = ops.gemm_grouped_rows(Gr.to(dev), off_dev, off_h, W.to(dev), trans_b=True, act_grad=("tanh", saved_t))
    assert torch.equal(fused, ops.activation_backward("tanh", outT, saved_t))


def test_gemm_asymmetric_identity(dev):
    """transpose-detecting check (A = I, asymmetric B)."""
    from tf2_gnn_amd import ops

    n = 96
    B = torch.arange(n * 80, dtype=torch.float32).reshape(n, 80) / 7.0
    out = ops.gemm(torch.eye(n).to(dev), B.to(dev))
    assert torch.equal(out.cpu(), B)


@pytest.mark.parametrize("act", [None] + ACTS)
def test_gemm_epilogue_bias_act_accumulate_strided(dev, act):
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(3)
    A = torch.randn((70, 48), generator=g)
    B = torch.randn((48, 36), generator=g)
    bias = torch.randn(36, generator=g)
    ref = A.double() @ B.double() + bias.double()
    if act is not None:
        ref = _ref_act(act)(ref)
    # strided output (a column block of a wider matrix) + accumulate
    wide = torch.ones((70, 100), device=dev)
    ops.gemm(A.to(dev), B.to(dev), bias=bias.to(dev), act=act, out=wide[:, 10:46], accumulate=True)
    assert_close(wide[:, 10:46].cpu(), (ref + 1.0).float(), tol=5e-6, what=f"epilogue {act}")
    assert torch.all(wide[:, :10] == 1) and torch.all(wide[:, 46:] == 1)


def test_gemm_split_k_weight_gradient_shape(dev):
    """dW = X^T G with K = number of nodes: split-K path, deterministic."""
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(5)
    X = torch.randn((20000, 64), generator=g)
    G = torch.randn((20000, 96), generator=g)
    ref = X.double().t() @ G.double()
    o1 = ops.gemm(X.to(dev), G.to(dev), trans_a=True)
    o2 = ops.gemm(X.to(dev), G.to(dev), trans_a=True)
    assert torch.equal(o1, o2)
    assert_close(o1.cpu() / 141.0, (ref / 141.0).float(), tol=3e-6, what="split-k")


@pytest.mark.parametrize("width", [3, 4, 7, 8, 12, 32, 64, 128, 256, 320, 512, 1280])
@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_gather_reduce_matches_oracle(dev, width, reduce):
    """The plan-less entry only (tfgnn_csr_gather_reduce: no items, no length-ordered short rows, no combine pass, no output
    row map).  The planned entry the layers call, tfgnn_graph_gather_reduce, is held to the same bound on every work unit of
    its plan in tests/test_gpu_graph_gather.py."""
    from tf2_gnn_amd import ops

    V, L = 200, 3
    adjs = random_graph(V, 3000, L, seed=width, empty_types=(2,), hub=(5, 300))
    rowptr, col, _ = ao.bucket_edges(adjs, V, by="dst")
    g = torch.Generator().manual_seed(width)
    X = torch.randn((V, width), generator=g)
    ew = torch.rand(col.shape[0], generator=g) + 0.5
    rs = torch.rand(V * L, generator=g) + 0.5
    seg = torch.from_numpy(np.repeat(np.arange(V * L), np.diff(rowptr))).int()
    msgs = X.double()[torch.from_numpy(col).long()] * ew.double().unsqueeze(-1)
    if reduce == "sum":
        ref = orc.unsorted_segment_sum(msgs, seg, V * L) * rs.double().unsqueeze(-1)
    else:
        ref = orc.unsorted_segment_max(msgs.float(), seg, V * L).double()
        nonempty = torch.from_numpy(np.diff(rowptr) > 0)
        ref[nonempty] = ref[nonempty] * rs.double()[nonempty].unsqueeze(-1)
    out = ops.gather_reduce(
        torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), X.to(dev),
        edge_weight=ew.to(dev), row_scale=rs.to(dev),
        reduce=ops.REDUCE_MAX if reduce == "max" else ops.REDUCE_SUM,
    )
    # fp32 summation error is bounded by (row length) * eps * sum|terms|: compare relative to the
    # L1 mass of each row (hub rows hold 300+ terms)
    l1 = orc.unsorted_segment_sum(msgs.abs(), seg, V * L).clamp(min=1.0) * rs.double().unsqueeze(-1).clamp(min=1.0)
    err = ((out.cpu().double() - ref).abs() / (l1 if reduce == "sum" else ref.abs().clamp(min=1.0))).max()
    assert float(err) <= 2e-6, f"gather {reduce} w={width}: {float(err):.3e}"


def test_gather_reduce_pre_post_activation_and_strides(dev):
    from tf2_gnn_amd import ops

    V = 64
    adjs = random_graph(V, 500, 1, seed=1)
    rowptr, col, _ = ao.bucket_edges(adjs, V, by="dst")
    X = torch.randn((V, 40))
    wide_in = torch.zeros((V, 64))
    wide_in[:, 8:48] = X
    seg = torch.from_numpy(np.repeat(np.arange(V), np.diff(rowptr))).int()
    ref = torch.tanh(orc.unsorted_segment_sum(torch.relu(X.double()[torch.from_numpy(col).long()]), seg, V))
    out_wide = torch.full((V, 100), 9.0, device=dev)
    ops.gather_reduce(torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev), wide_in.to(dev)[:, 8:48],
                      pre_act="relu", post_act="tanh", out=out_wide[:, 20:60])
    assert_close(out_wide[:, 20:60].cpu(), ref.float(), tol=2e-6, what="pre/post act")
    assert torch.all(out_wide[:, :20] == 9) and torch.all(out_wide[:, 60:] == 9)


@pytest.mark.parametrize("name", ["sum", "max", "mean", "sqrt_n"])
def test_aggregation_function_semantics(dev, name):
    """get_aggregation_function(name)(data, segment_ids, num_segments) == tf.math.unsorted_segment_*"""
    from tf2_gnn_amd.utils import get_aggregation_function

    g = torch.Generator().manual_seed(2)
    data = torch.randn((37, 5), generator=g)
    ids = torch.randint(0, 9, (37,), generator=g).int()
    ids[ids == 4] = 3  # segment 4 is empty
    ref = orc.get_aggregation_function(name)(data, ids, 11)
    out = get_aggregation_function(name)(data=data.to(dev), segment_ids=ids.to(dev), num_segments=11)
    assert_close(out.cpu(), ref, tol=2e-6, what=name)


def test_tanh_relative_accuracy(dev):
    """VERDICT r4 weak 1a / ADVICE r4: the device tanh (common.hpp fast_tanh: every tanh activation, product epilogue and both
    GELU passes) must be RELATIVELY accurate like TensorFlow's - log-spaced inputs from 1e-7 to 10, both signs, <= 4 ulp of the
    fp64 tanh rounded to fp32; tiny inputs come back unchanged (tanh(x) = x to fp32 below 2e-4)."""
    from tf2_gnn_amd import ops

    mag = torch.logspace(-7, 1, 200001, dtype=torch.float64).float()
    x = torch.cat([mag, -mag, torch.tensor([0.0, 0.625, -0.625, 0.6249999, 88.0, -88.0, 1e-20, -1e-30])])
    ref = torch.tanh(x.double())
    y = ops.activation_forward("tanh", x.to(dev)).cpu()
    ref32 = ref.float()
    ulp = (torch.nextafter(ref32.abs(), torch.tensor(float("inf"))) - ref32.abs()).double()
    err = ((y.double() - ref).abs() / ulp).max().item()
    assert err <= 4.0, f"device tanh is {err:.2f} ulp off"
    tiny = x.abs() < 1e-4
    assert torch.equal(y[tiny], x[tiny])
    assert torch.equal(y[x.abs() >= 20.0], torch.sign(x[x.abs() >= 20.0]))
    # the derivative the backward pass takes from the saved output, relative to 1 - tanh^2 where that is not itself cancelling
    keep = x.abs() < 2.0
    d = ops.activation_backward("tanh", torch.ones_like(x).to(dev), y.to(dev)).cpu()
    dref = 1.0 - ref**2
    assert float(((d.double() - dref).abs() / dref)[keep].max()) <= 2e-6
    # gelu (utils/activation.py:7-14) goes through the same tanh: relative to the fp64 value over 1e-6 .. 10
    xg = torch.cat([torch.logspace(-6, 1, 20001, dtype=torch.float64).float(), -torch.logspace(-6, 0.0, 20001, dtype=torch.float64).float()])  # (below -1 the formula itself cancels in 1 + tanh)
    gref = _ref_act("gelu")(xg.double())
    gy = ops.activation_forward("gelu", xg.to(dev)).cpu()
    assert float(((gy.double() - gref).abs() / gref.abs().clamp(min=1e-30)).max()) <= 2e-6


@pytest.mark.parametrize("act", ACTS)
def test_activation_forward_backward(dev, act):
    from tf2_gnn_amd import ops

    x = torch.linspace(-6, 6, 1003, dtype=torch.float64).requires_grad_(True)
    y = _ref_act(act)(x)
    (gx,) = torch.autograd.grad(y.sum(), x)
    xd = x.detach().float().to(dev)
    yd = ops.activation_forward(act, xd)
    assert_close(yd.cpu(), y.detach().float(), tol=2e-6, what=f"{act} fwd")
    dy = torch.ones_like(xd)
    saved = xd if act == "gelu" else yd
    dx = ops.activation_backward(act, dy, saved)
    assert_close(dx.cpu(), gx.float(), tol=5e-6, what=f"{act} bwd")
    # with the dropout mask of the layer input in the same pass (tfgnn_activation_backward_mul): the bits of the two passes
    g = torch.randn(xd.shape, generator=torch.Generator().manual_seed(2)).to(dev)
    m = ((torch.rand(xd.shape, generator=torch.Generator().manual_seed(3)) > 0.2).float() / 0.8).to(dev)
    assert torch.equal(ops.activation_backward(act, g, saved, mul=m), ops.activation_backward(act, ops.mul(g, m), saved))
    assert torch.equal(ops.activation_backward(act, g[1:], saved[1:], mul=m[1:]), ops.activation_backward(act, ops.mul(g, m), saved)[1:])


def test_gru_gates_forward_backward(dev):
    from tf2_gnn_amd import ops

    V, H = 50, 12
    g = torch.Generator().manual_seed(0)
    mx = torch.randn((V, 3 * H), generator=g, dtype=torch.float64).requires_grad_(True)
    mh = torch.randn((V, 3 * H), generator=g, dtype=torch.float64).requires_grad_(True)
    h = torch.randn((V, H), generator=g, dtype=torch.float64).requires_grad_(True)
    z = torch.sigmoid(mx[:, :H] + mh[:, :H])
    r = torch.sigmoid(mx[:, H:2 * H] + mh[:, H:2 * H])
    c = torch.tanh(mx[:, 2 * H:] + r * mh[:, 2 * H:])
    out = z * h + (1 - z) * c
    dout = torch.randn((V, H), generator=g, dtype=torch.float64)
    gmx, gmh, gh = torch.autograd.grad((out * dout).sum(), [mx, mh, h])
    f = lambda t: t.detach().float().to(dev)
    h_new, gates = ops.gru_gates_forward(f(mx), f(mh), f(h))
    assert_close(h_new.cpu(), out.detach().float(), tol=2e-6, what="gru fwd")
    dmx, dmh, dh = ops.gru_gates_backward(f(dout), gates, f(mh), f(h))
    assert_close(dmx.cpu(), gmx.float(), tol=5e-6, what="gru dmx")
    assert_close(dmh.cpu(), gmh.float(), tol=5e-6, what="gru dmh")
    assert_close(dh.cpu(), gh.float(), tol=5e-6, what="gru dh")


def _layernorm_case(rows, H, seed=1):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, H), generator=g, dtype=torch.float64)
    gamma = torch.randn(H, generator=g, dtype=torch.float64)
    beta = torch.randn(H, generator=g, dtype=torch.float64)
    dy = torch.randn((rows, H), generator=g, dtype=torch.float64)
    return x, gamma, beta, dy


def _layernorm_reference(x, gamma, beta, dy):
    x, gamma, beta = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y = orc.layer_norm(x, gamma, beta, 1e-3)
    return (y.detach(),) + torch.autograd.grad((y * dy).sum(), [x, gamma, beta])


@pytest.mark.parametrize("rows,H", [(1, 1), (3, 63), (4, 64), (5, 65), (33, 70), (257, 320)])
def test_layernorm_forward_backward(dev, rows, H):
    """One wave per row, four rows per workgroup, lane j owns columns j, j + 64, ...: row counts that are no multiple of four, a
    last workgroup of one row, and one, two and five strides per lane with a ragged last stride."""
    from tf2_gnn_amd import ops

    x, gamma, beta, dy = _layernorm_case(rows, H)
    y, gx, gg, gb = _layernorm_reference(x, gamma, beta, dy)
    f = lambda t: t.detach().float().to(dev)
    yd, mean, rstd = ops.layernorm_forward(f(x), f(gamma), f(beta), 1e-3)
    assert_close(yd.cpu(), y.float(), tol=5e-6, what="ln fwd")
    assert_close(mean.cpu(), x.mean(dim=1).float(), tol=5e-6, what="ln mean")
    dx, dgam, dbet = ops.layernorm_backward(f(dy), f(x), f(gamma), mean, rstd)
    assert_close(dx.cpu(), gx.float(), tol=1e-5, what="ln dx")
    assert_close(dgam.cpu(), gg.float(), tol=1e-5, what="ln dgamma")
    assert_close(dbet.cpu(), gb.float(), tol=1e-5, what="ln dbeta")


def test_layernorm_constant_row(dev):
    """A row of one value: the variance is 0, rstd = 1 / sqrt(eps), y = beta, and dx = rstd * gamma-weighted dy less its mean."""
    from tf2_gnn_amd import ops

    x, gamma, beta, dy = _layernorm_case(6, 70, seed=2)
    x[2] = 3.25
    y, gx, gg, gb = _layernorm_reference(x, gamma, beta, dy)
    f = lambda t: t.detach().float().to(dev)
    yd, mean, rstd = ops.layernorm_forward(f(x), f(gamma), f(beta), 1e-3)
    assert float(mean[2]) == 3.25
    assert abs(float(rstd[2]) * 1e-3 ** 0.5 - 1.0) <= 2e-6
    assert torch.equal(yd[2].cpu(), beta.float())
    assert_close(yd.cpu(), y.float(), tol=5e-6, what="ln fwd, constant row")
    dx, dgam, dbet = ops.layernorm_backward(f(dy), f(x), f(gamma), mean, rstd)
    assert_close(dx.cpu(), gx.float(), tol=1e-5, what="ln dx, constant row")
    assert_close(dgam.cpu(), gg.float(), tol=1e-5, what="ln dgamma, constant row")
    assert_close(dbet.cpu(), gb.float(), tol=1e-5, what="ln dbeta, constant row")


def test_layernorm_large_row_mean(dev):
    """Rows offset by +-1e3 from a unit spread: what the two-pass variance is for.  The fp32 input is the common starting point
    (the reference takes it cast up).  Tolerances are those of test_layernorm_forward_backward plus the conditioning of x - mean in
    fp32: one rounding of a 1e3-sized mean, delta = 1e3 * 2^-24 in units of x, is delta * rstd in xhat = (x - mean) * rstd, and
    reaches the outputs through their first derivatives with respect to xhat:
        y = xhat gamma + beta                          -> delta rstd |gamma|
        dx = rstd (g - mean(g) - xhat mean(g xhat))    -> delta rstd^2 (|mean(g xhat)| + |xhat| mean|g|),  g = dy gamma
        dgamma = sum_rows dy xhat                      -> sum_rows |dy| delta rstd
    (dbeta does not depend on x).  The bound comes from the number format, not from what the kernel gives."""
    from tf2_gnn_amd import ops

    rows, H = 33, 70
    x, gamma, beta, dy = _layernorm_case(rows, H, seed=3)
    offset = torch.where(torch.arange(rows) % 2 == 0, 1e3, -1e3).double().unsqueeze(1)
    x = (x + offset).float().double()
    y, gx, gg, gb = _layernorm_reference(x, gamma, beta, dy)
    f = lambda t: t.detach().float().to(dev)
    yd, mean, rstd = ops.layernorm_forward(f(x), f(gamma), f(beta), 1e-3)
    dx, dgam, dbet = ops.layernorm_backward(f(dy), f(x), f(gamma), mean, rstd)
    delta = 1e3 * 2.0 ** -24
    mu = x.mean(dim=1, keepdim=True)
    rs = 1.0 / torch.sqrt(((x - mu) ** 2).mean(dim=1, keepdim=True) + 1e-3)
    xhat = (x - mu) * rs
    g = dy * gamma
    extra_y = delta * rs * gamma.abs()
    extra_dx = delta * rs * rs * ((g * xhat).mean(dim=1, keepdim=True).abs() + xhat.abs() * g.abs().mean(dim=1, keepdim=True))
    extra_dgamma = (dy.abs() * delta * rs).sum(dim=0)
    for what, got, ref, tol, extra in (("y", yd, y, 5e-6, extra_y), ("dx", dx, gx, 1e-5, extra_dx), ("dgamma", dgam, gg, 1e-5, extra_dgamma),
                                       ("dbeta", dbet, gb, 1e-5, torch.zeros(H, dtype=torch.float64))):
        err = (got.cpu().double() - ref).abs()
        bound = tol * ref.abs().clamp(min=1.0) + extra
        worst = float((err / bound).max())
        print(f"ln large mean {what}: max error {float(err.max()):.3e}, worst error / bound {worst:.3f}")
        assert worst <= 1.0, (what, worst)
    assert float((mean.cpu().double() - mu.view(-1)).abs().max()) <= delta


@pytest.mark.parametrize("bounds", [(-0.5, 0.75), (-0.5, None), (None, 0.75), (None, None)], ids=["both", "lower", "upper", "none"])
def test_clip_at_nan_inf_and_the_bounds(dev, bounds):
    """tfgnn_clip / tfgnn_clip_backward against torch.clamp on the CPU: a NaN stays a NaN (tf.maximum / tf.minimum propagate
    it; fmaxf / fminf would return the bound), +-inf clips to a finite bound and stays without one, values exactly on a
    bound pass the gradient.  Exact: a clip rounds nothing."""
    from tf2_gnn_amd import ops

    lo, hi = bounds
    g = torch.Generator().manual_seed(2)
    x = torch.round(4 * torch.randn(1000, generator=g)) / 8  # a grid of eighths: many values exactly on the bounds
    x[::97] = float("nan")
    x[1::97] = float("inf")
    x[2::97] = float("-inf")
    assert int((x == -0.5).sum()) > 20 and int((x == 0.75).sum()) > 20
    dy = torch.randn(1000, generator=g)
    want = x if lo is None and hi is None else torch.clamp(x, min=lo, max=hi)
    y = ops.clip(x.to(dev), lo, hi).cpu()
    assert torch.equal(torch.isnan(y), torch.isnan(x)) and int(torch.isnan(y).sum()) == 11
    zero = torch.zeros_like(x)
    assert torch.equal(torch.where(torch.isnan(y), zero, y), torch.where(torch.isnan(want), zero, want))  # +-inf included
    keep = torch.ones_like(x, dtype=torch.bool)
    if lo is not None:
        keep &= x >= lo
    if hi is not None:
        keep &= x <= hi
    if lo is None and hi is None:  # ops.clip_backward compares with -inf / +inf: all pass but a NaN
        keep &= ~torch.isnan(x)
    dx = ops.clip_backward(dy.to(dev), x.to(dev), lo, hi).cpu()
    assert torch.equal(dx, torch.where(keep, dy, torch.zeros_like(dy)))


@pytest.mark.parametrize("M", [1, 200, 256, 257, 4097, 7110, 150001])
@pytest.mark.parametrize("N", [7, 121, 320])
def test_colsum_bias_gradient_sums(dev, M, N):
    """tfgnn_colsum (Dense / GRUCell bias gradients, the sums of LayerNorm's d gamma / d beta): both kernels (16-byte rows and
    odd widths), one slab and many, a ragged last slab, rows of a wider matrix - against the fp64 sum, relative to sum |x|; the
    same call twice gives the same bits (fixed slab order)."""
    from tf2_gnn_amd import ops

    g = torch.Generator().manual_seed(M + N)
    wide = torch.randn((M, N + 5), generator=g).to(dev)
    for x in (wide[:, :N].contiguous(), wide[:, 1:N + 1]):
        got = ops.colsum(x)
        ref = x.double().sum(dim=0)
        mag = x.double().abs().sum(dim=0).clamp(min=1e-30)
        assert float(((got.double() - ref).abs() / mag).max()) <= 2e-6
        assert torch.equal(got, ops.colsum(x))


def test_dropout_mask_statistics_and_scaling(dev):
    from tf2_gnn_amd import ops

    x = torch.ones(200000, device=dev)
    y, mask = ops.dropout_forward(x, 0.1, seed=7)
    kept = (mask > 0).float().mean().item()
    assert abs(kept - 0.9) < 0.01
    vals = torch.unique(mask).cpu()
    assert vals.numel() == 2 and vals[0] == 0 and abs(float(vals[1]) - 1 / 0.9) < 1e-6
    assert torch.equal(y, mask)
    y2, mask2 = ops.dropout_forward(x, 0.1, seed=7)
    assert torch.equal(mask, mask2)
    _, mask3 = ops.dropout_forward(x, 0.1, seed=8)
    assert not torch.equal(mask, mask3)
    # and they are the masks include/tfgnn.h writes out (tests/dropout_reference.py), bit for bit - at the epoch in force: tests
    # that replayed a captured step before this one have advanced it
    from tests import dropout_reference

    epoch = ops.dropout_epoch()
    assert np.array_equal(mask.cpu().numpy(), dropout_reference.mask(200000, 0.1, 7, epoch))
    assert np.array_equal(mask3.cpu().numpy(), dropout_reference.mask(200000, 0.1, 8, epoch))
    with pytest.raises(ValueError):
        ops.dropout_forward(x, 1.0, seed=0)


def test_compact_bucket_arrays_and_grouped_gemm(dev):
    """Non-empty buckets in type-major order (graph.hip) + the grouped GEMMs that run over them."""
    from tf2_gnn_amd import ops

    V, L, D, H = 300, 3, 16, 24
    adjs = random_graph(V, 500, L, seed=13, empty_types=(1,), hub=(4, 90))
    g = ops.Graph(to_dev(adjs, dev), V)
    for by, (ids, view) in {"dst": ((ops.G_NZ_CPOS_BY_DST, ops.G_NZ_ROW_BY_DST, ops.G_NZ_NODE_BY_DST, ops.G_NZ_OFF_BY_DST,
                                      ops.G_NZ_NODEPTR_BY_DST, ops.G_NZ_COL_BY_DST), ops.VIEW_BY_DST_TYPED_COMPACT),
                            "src": ((ops.G_NZ_CPOS_BY_SRC, ops.G_NZ_ROW_BY_SRC, ops.G_NZ_NODE_BY_SRC, ops.G_NZ_OFF_BY_SRC,
                                      ops.G_NZ_NODEPTR_BY_SRC, ops.G_NZ_COL_BY_SRC), ops.VIEW_BY_SRC_TYPED_COMPACT)}.items():
        rowptr, col, _ = ao.bucket_edges(adjs, V, by=by)
        lens = np.diff(rowptr).reshape(V, L)
        nzmask = lens > 0
        # type-major enumeration of the non-empty buckets
        exp_rows = [v * L + l for l in range(L) for v in range(V) if nzmask[v, l]]
        off_h = g.nonempty_offsets(by == "src")
        assert off_h == [int(nzmask[:, :l].sum()) for l in range(L)] + [int(nzmask.sum())]
        np.testing.assert_array_equal(g.array(ids[1]).cpu().numpy(), np.array(exp_rows, dtype=np.int32))
        np.testing.assert_array_equal(g.array(ids[2]).cpu().numpy(), np.array(exp_rows) // L)
        cpos = g.array(ids[0]).cpu().numpy()
        exp_cpos = np.full(V * L, -1)
        exp_cpos[exp_rows] = np.arange(len(exp_rows))
        np.testing.assert_array_equal(cpos, exp_cpos)
        np.testing.assert_array_equal(g.array(ids[3]).cpu().numpy(), np.array(off_h))
        nptr = g.array(ids[4]).cpu().numpy()
        np.testing.assert_array_equal(nptr, np.concatenate([[0], np.cumsum(nzmask.sum(1))]))
        cols = g.array(ids[5]).cpu().numpy()
        for v in (0, 4, V - 1):
            np.testing.assert_array_equal(cols[nptr[v]:nptr[v + 1]], [exp_cpos[v * L + l] for l in range(L) if nzmask[v, l]])
        # compact gather == rows of the dense gather
        X = torch.randn((V, D), generator=torch.Generator().manual_seed(1)).to(dev)
        dense = ops.graph_gather(g, view - 4 if view == 4 else 2, X)
        comp = ops.graph_gather(g, view, X)
        assert comp.shape == (len(exp_rows), D)
        assert torch.equal(comp.cpu(), dense.cpu()[exp_rows])
        # grouped GEMMs vs per-group fp64
        W = torch.randn((L, D, H), generator=torch.Generator().manual_seed(2))
        out = ops.gemm_grouped_rows(comp, g.array(ids[3]), off_h, W.to(dev))
        Gc = torch.randn((len(exp_rows), H), generator=torch.Generator().manual_seed(3))
        outT = ops.gemm_grouped_rows(Gc.to(dev), g.array(ids[3]), off_h, W.to(dev), trans_b=True)
        dW = ops.gemm_grouped_k(comp, Gc.to(dev), g.array(ids[3]), off_h, L)
        for l in range(L):
            sl = slice(off_h[l], off_h[l + 1])
            assert_close(out[sl].cpu(), (comp[sl].cpu().double() @ W[l].double()).float(), tol=5e-6, what="grouped rows")
            assert_close(outT[sl].cpu(), (Gc[sl].double() @ W[l].double().t()).float(), tol=5e-6, what="grouped rows T")
            assert_close(dW[l].cpu() / 10, (comp[sl].cpu().double().t() @ Gc[sl].double()).float() / 10, tol=5e-6, what="grouped k")
    g.close()
