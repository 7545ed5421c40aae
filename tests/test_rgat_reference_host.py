"""tests/rgat_reference.py against torch.autograd in fp64 and against the oracle's RGAT logits (CPU only): a bug in the
closed-form reference of tests/test_gpu_rgat_node_ops.py must not be read as a kernel bug.  Also the decisions the node-side
entry points of csrc/rgat.hip take on the host, before any HIP call: return codes and the workspace size."""
import pytest
import torch

from oracle import tf2gnn_oracle as orc
from tests import rgat_reference as ref


def _draw(V, L, K, Hk, seed):
    g = torch.Generator().manual_seed(seed)
    Y = torch.randn((V * L, K, Hk), generator=g, dtype=torch.float64)
    alpha = torch.randn((L, K, 2 * Hk), generator=g, dtype=torch.float64)
    ds_src, ds_tgt = (torch.randn((V * L, K), generator=g, dtype=torch.float64) for _ in range(2))
    return Y, alpha, ds_src, ds_tgt


@pytest.mark.parametrize("V,L,K,Hk", [(7, 3, 3, 8), (11, 2, 1, 5)])
def test_backward_references_are_the_gradients_of_node_scores(V, L, K, Hk):
    Y, alpha, ds_src, ds_tgt = _draw(V, L, K, Hk, 100 * V + Hk)
    Yg, ag = Y.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
    # the definition, written out independently of the reference: one einsum per half
    Y4 = Yg.reshape(V, L, K, Hk)
    s_src = torch.einsum("vlki,lki->vlk", Y4, ag[:, :, :Hk]).reshape(V * L, K)
    s_tgt = torch.einsum("vlki,lki->vlk", Y4, ag[:, :, Hk:]).reshape(V * L, K)
    got = ref.node_scores(Y, alpha, L, K)
    torch.testing.assert_close(got[0], s_src.detach(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got[1], s_tgt.detach(), rtol=1e-12, atol=1e-12)
    gY, ga = torch.autograd.grad((ds_src * s_src + ds_tgt * s_tgt).sum(), [Yg, ag])
    dY0 = torch.randn((V * L, K * Hk), generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    dY, S = ref.scores_backward(ds_src, ds_tgt, alpha, dY0, L, K)
    torch.testing.assert_close(dY, dY0 + gY.reshape(V * L, K * Hk), rtol=1e-12, atol=1e-12)
    d_alpha, Sa = ref.alpha_grad(ds_src, ds_tgt, Y, L, K)
    assert tuple(d_alpha.shape) == (L, K, 2 * Hk)
    torch.testing.assert_close(d_alpha, ga, rtol=1e-12, atol=1e-12)
    # the magnitude sums: the same expressions on absolute values, never below the result's own magnitude
    assert bool((S >= dY.abs() - 1e-12).all()) and bool((Sa >= d_alpha.abs() - 1e-12).all())
    dYa, _ = ref.scores_backward(ds_src.abs(), ds_tgt.abs(), alpha.abs(), dY0.abs(), L, K)
    da_abs, _ = ref.alpha_grad(ds_src.abs(), ds_tgt.abs(), Y.abs(), L, K)
    assert torch.equal(S, dYa) and torch.equal(Sa, da_abs)
    abs_scores = ref.node_scores(Y.abs(), alpha.abs(), L, K)
    assert torch.equal(got[2], abs_scores[0]) and torch.equal(got[3], abs_scores[1])


def test_node_scores_are_the_oracles_logits():
    """oracle/tf2gnn_oracle.py _rgat_message: leaky_relu(<[Ys | Yt], alpha_l>) per edge and head; with the identity as the
    kernel, Ys / Yt are rows of Y"""
    V, L, K, Hk, E = 9, 2, 3, 4, 40
    H = K * Hk
    Y, alpha, _, _ = _draw(V, L, K, Hk, 3)
    s_src, s_tgt, _, _ = ref.node_scores(Y, alpha, L, K)
    g = torch.Generator().manual_seed(8)
    src, tgt = (torch.randint(0, V, (E,), generator=g) for _ in range(2))
    Yv = Y.reshape(V, L, H)
    for l in range(L):
        _, scores = orc._rgat_message({"num_heads": K, "hidden_dim": H}, torch.eye(H, dtype=torch.float64), alpha[l],
                                      Yv[src, l], Yv[tgt, l])
        z = s_src[src * L + l] + s_tgt[tgt * L + l]
        torch.testing.assert_close(torch.nn.functional.leaky_relu(z, 0.2), scores, rtol=1e-12, atol=1e-12)


def test_edge_dot_reference_and_fp32_inputs_are_cast_up():
    V, L, K, Hk, E = 6, 2, 2, 3, 25
    Y, _, _, _ = _draw(V, L, K, Hk, 4)
    g = torch.Generator().manual_seed(9)
    d_agg = torch.randn((V, K, Hk), generator=g, dtype=torch.float64)
    coll, tgt = torch.randint(0, V * L, (E,), generator=g, dtype=torch.int32), torch.randint(0, V, (E,), generator=g, dtype=torch.int32)
    da, S = ref.edge_dot(coll, tgt, Y, d_agg, K)
    want = torch.stack([torch.stack([Y[int(c), k] @ d_agg[int(t), k] for k in range(K)]) for c, t in zip(coll, tgt)])
    torch.testing.assert_close(da, want, rtol=1e-12, atol=1e-12)
    assert bool((S >= da.abs() - 1e-12).all())
    # 2-D operands (the device layout [rows, H]) and fp32 inputs: the fp64 result of exactly those values
    da32, _ = ref.edge_dot(coll, tgt, Y.float().reshape(V * L, K * Hk), d_agg.float().reshape(V, K * Hk), K)
    assert da32.dtype == torch.float64
    assert torch.equal(da32, ref.edge_dot(coll, tgt, Y.float().double(), d_agg.float().double(), K)[0])


def test_exact_inputs_stay_exact_in_fp32():
    """integers in {-3..3}: every product and partial sum of the longest sum the device tests use (70 000 terms, 9 * n < 2^24)
    is an integer fp32 holds exactly, so a sequential fp32 accumulation equals the fp64 sum"""
    n = 70000
    g = torch.Generator().manual_seed(1)
    a = torch.randint(-3, 4, (n,), generator=g).float()
    b = torch.randint(-3, 4, (n,), generator=g).float()
    assert 9 * n < 2 ** 24
    assert float(torch.cumsum(a * b, 0, dtype=torch.float32)[-1]) == float((a.double() * b.double()).sum())


def test_scores_backward_sp_return_codes_without_gpu():
    from tf2_gnn_amd import _lib

    lib = _lib.load()

    def sp(V, L, K, H):
        return lib.tfgnn_rgat_scores_backward_sp(None, None, None, None, 1, V, L, K, H, None, None, None)

    assert sp(8, 2, 4, 24) == -4    # Hk = 6: Hk % 4 != 0
    assert sp(8, 1, 3, 24) == -4    # C = 24: C % 16 != 0
    assert sp(8, 5, 8, 512) == -4   # C = 2560 > 2048
    assert sp(0, 2, 3, 24) == 0     # no rows: a no-op (a supported shape, NULL pointers)
    assert sp(8, 2, 3, 24) == -1    # a supported shape with rows needs its operands
    assert b"NULL" in lib.tfgnn_last_error()
    assert sp(8, 2, 5, 24) == -1 and sp(8, 2, 65, 260) == -1  # the head checks come first


@pytest.mark.parametrize("V", [1, 16, 17, 16384, 16400])
def test_alpha_grad_workspace_bytes(V):
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    for L, H in ((3, 24), (1, 4), (2, 512)):
        assert lib.tfgnn_rgat_alpha_grad_workspace_bytes(V, L, H) == min(1024, -(-V // 16)) * 2 * L * H * 4, (V, L, H)
    assert lib.tfgnn_rgat_alpha_grad_workspace_bytes(0, 3, 24) == 0
    assert lib.tfgnn_rgat_alpha_grad_workspace_bytes(V, 0, 24) == 0
    assert lib.tfgnn_rgat_alpha_grad_workspace_bytes(V, 3, 0) == 0


def test_head_checks_of_the_node_side_entry_points_without_gpu():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    for K, H in ((5, 24), (65, 260)):  # H % K != 0 ; K > 64
        assert lib.tfgnn_rgat_edge_dot(None, None, None, None, 10, K, H, None, None) == -1, (K, H)
        assert lib.tfgnn_rgat_scores_backward(None, None, None, 10, 2, K, H, None, None) == -1, (K, H)
        assert lib.tfgnn_rgat_alpha_grad(None, None, None, 10, 2, K, H, None, None, 0, None) == -1, (K, H)
    assert b"num_heads" in lib.tfgnn_last_error() or b"bad sizes" in lib.tfgnn_last_error()
    # empty problems are no-ops
    assert lib.tfgnn_rgat_edge_dot(None, None, None, None, 0, 2, 8, None, None) == 0
    assert lib.tfgnn_rgat_scores_backward(None, None, None, 0, 2, 2, 8, None, None) == 0
    assert lib.tfgnn_rgat_alpha_grad(None, None, None, 10, 0, 2, 8, None, None, 0, None) == 0
