"""R-GCN block-diagonal decomposition, the part that needs no GPU: the two float64 references
(tests/rgcn_blockdiag_reference.py) agree with each other; the layer is registered, has its defaults and refuses what the
decomposition does not commute with; the new C entries are exported, declared and bound with the ABI number unmoved, and refuse
bad arguments before they touch a device; the host-side chunk table of the weight gradient against a literal restatement."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import rgcn_blockdiag_reference as ref
from tests.helpers import random_graph

ROOT = Path(__file__).resolve().parent.parent
NEW = ["tfgnn_blockdiag_forward", "tfgnn_blockdiag_backward", "tfgnn_blockdiag_workspace_bytes", "tfgnn_blockdiag_launch_counts"]


def _small_graph(seed):
    V, L = 23, 5
    adjs = random_graph(V, 120, L, seed=seed, empty_types=(3,), hub=(2, 40))
    adjs[1] = np.concatenate([adjs[1], adjs[1][:4], np.array([[4, 4], [5, 5]], dtype=np.int32)])  # duplicates, self loops
    adjs = [a[(a[:, 1] != 7) & (a[:, 0] != 9) & (a[:, 0] != 11) & (a[:, 1] != 11)] for a in adjs]
    return adjs, V, L  # type 3 empty, node 7 without in-edges, node 9 without out-edges, node 11 isolated


# (D, H, C): di != ho, C = 1, C = D (diagonal), and a plain one
@pytest.mark.parametrize("D,H,C", [(6, 9, 3), (6, 5, 1), (4, 4, 4), (8, 4, 2)])
@pytest.mark.parametrize("aggregation,normalize", [("sum", True), ("mean", True), ("sqrt_n", False), ("mean", False)])
def test_the_two_references_agree(D, H, C, aggregation, normalize):
    """op-level loops composed to a layer (pre, tanh, and back) == per-edge oracle with composed dense kernels and the band
    map of their gradients, to 1e-12 of each tensor's largest entry"""
    adjs, V, L = _small_graph(3)
    rng = np.random.default_rng(5)
    Qb = rng.standard_normal((L, D // C, H)) / np.sqrt(D // C)
    X, dOut = rng.standard_normal((V, D)), rng.standard_normal((V, H))
    params = ref.rgcn_params(H, aggregation, "tanh", normalize)
    out_l, dX_l, dQb_l = ref.layer_reference(params, Qb, C, X, adjs, dOut)

    s, m, s_src = ref.scales_tables(adjs, V, normalize, aggregation)
    pre, _ = ref.forward(adjs, V, Qb, X, C, s, m)
    out = np.tanh(pre)
    dPre = dOut * (1.0 - out * out)
    dX, _ = ref.backward_dx(adjs, V, Qb, dPre, C, s_src)
    dQb, _ = ref.backward_dq(adjs, V, C, D, H, X, dPre, s, m)
    for name, got, want in (("out", out, out_l), ("dX", dX, dX_l), ("dQb", dQb, dQb_l)):
        want = want.numpy()
        assert got.shape == want.shape, name
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name
    assert np.all(dQb[3] == 0) and np.all(pre[7] == 0) and np.all(dX[9] == 0) and np.all(pre[11] == 0) and np.all(dX[11] == 0)


def test_compose_and_band_are_inverse_on_the_blocks():
    rng = np.random.default_rng(2)
    Qb = torch.from_numpy(rng.standard_normal((3, 2, 12)))  # C = 4: blocks of 2 x 3
    W = ref.compose_kernels(Qb, 4)
    assert W.shape == (3, 8, 12) and torch.equal(ref.band_gradient(W, 4), Qb)
    assert int((W != 0).sum()) == Qb.numel() and float(W[1, 2, 3]) == float(Qb[1, 0, 3]) and float(W[1, 2, 0]) == 0.0


def test_reference_bounds_are_zero_exactly_where_there_is_no_term():
    adjs, V, L = _small_graph(4)
    rng = np.random.default_rng(1)
    C, D, H = 2, 4, 6
    Qb, X, dPre = rng.standard_normal((L, D // C, H)), rng.standard_normal((V, D)), rng.standard_normal((V, H))
    pre, pb = ref.forward(adjs, V, Qb, X, C)
    dX, xb = ref.backward_dx(adjs, V, Qb, dPre, C)
    dq, qb = ref.backward_dq(adjs, V, C, D, H, X, dPre)
    assert np.all(pb[7] == 0) and np.all(xb[9] == 0) and np.all(qb[3] == 0) and np.all(pb[11] == 0) and np.all(xb[11] == 0)
    assert np.all(pb[2] > 0) and pb.shape == pre.shape and xb.shape == dX.shape and qb.shape == dq.shape == (L, D // C, H)


def test_registry_and_default_hyperparameters():
    from tf2_gnn_amd.layers import GNN, RGCN_BlockDiag, get_known_message_passing_classes, get_message_passing_class
    from tf2_gnn_amd.layers.message_passing import MessagePassing
    import tf2_gnn_amd
    from tf2_gnn_amd.layers import message_passing

    assert tf2_gnn_amd.RGCN_BlockDiag is RGCN_BlockDiag and message_passing.RGCN_BlockDiag is RGCN_BlockDiag
    assert get_message_passing_class("rgcn_blockdiag") is RGCN_BlockDiag and get_message_passing_class("RGCN_BlockDiag") is RGCN_BlockDiag
    assert "RGCN_BlockDiag" in set(get_known_message_passing_classes())
    hp = RGCN_BlockDiag.get_default_hyperparameters()
    assert hp["num_blocks"] == 4 and hp["normalize_by_num_incoming"] is True
    assert set(hp) == set(MessagePassing.get_default_hyperparameters()) | {"num_blocks", "normalize_by_num_incoming"}
    g = GNN.get_default_hyperparameters("rgcn_blockdiag")
    assert g["message_calculation_class"] == "rgcn_blockdiag" and g["num_blocks"] == 4
    from tf2_gnn_amd.tasks import LinkPredictionTask

    assert LinkPredictionTask.get_default_hyperparameters("rgcn_blockdiag")["gnn_num_blocks"] == 4


@pytest.mark.parametrize("over", [{"aggregation_function": "max"}, {"message_activation_before_aggregation": True},
                                  {"num_blocks": 0}])
def test_what_does_not_commute_with_the_decomposition_is_refused_at_construction(over):
    from tf2_gnn_amd.layers import RGCN_BlockDiag

    with pytest.raises(ValueError, match="only commutes with sum-like aggregation"):
        RGCN_BlockDiag(dict(RGCN_BlockDiag.get_default_hyperparameters(), **over))


def _built(num_blocks, D, H, L=7):
    from tf2_gnn_amd.layers import MessagePassingInput, RGCN_BlockDiag
    from tf2_gnn_amd.layers.message_passing import set_default_device

    set_default_device("cpu")
    try:
        layer = RGCN_BlockDiag(dict(RGCN_BlockDiag.get_default_hyperparameters(), num_blocks=num_blocks, hidden_dim=H))
        layer.build(MessagePassingInput((None, D), tuple((None, 2) for _ in range(L))))
    finally:
        set_default_device(None)
    return layer


@pytest.mark.parametrize("C,D,H", [(4, 10, 8), (4, 8, 10), (3, 8, 8)])
def test_block_counts_that_do_not_divide_the_widths_are_refused_at_build(C, D, H):
    with pytest.raises(ValueError, match=rf"num_blocks = {C} must divide the input width {D} and the hidden width {H}"):
        _built(C, D, H)


def test_variable_initialisation_and_dense_kernels():
    layer = _built(3, 6, 15)
    assert [(v.name, v.shape) for v in layer.trainable_variables] == [("block_kernels", (7, 2, 15))]
    Qb = layer.trainable_variables[0].value
    limit = (6.0 / (2 + 5)) ** 0.5  # Glorot-uniform per block [di, ho] = [2, 5]
    assert 0.9 * limit < float(Qb.abs().max()) <= limit
    W = layer.dense_kernels()
    assert W.shape == (7, 6, 15) and torch.equal(W, ref.compose_kernels(Qb, 3))
    assert layer.graph_parts(10, [1] * 7, 6) == 1 | 2 | 16  # PLAN_TYPED | PLAN_NODE | EDGE_IDS


def test_new_symbols_are_exported_declared_and_bound_and_the_abi_stays_5():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in text
    for struct, cname in ((_lib.BlockdiagForwardArgs, "tfgnn_blockdiag_forward_args"),
                          (_lib.BlockdiagBackwardArgs, "tfgnn_blockdiag_backward_args")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, flags=re.S).group(1)
        declared = [re.search(r"(\w+)$", part.strip()).group(1) for stmt in body.split(";") if stmt.strip()
                    for part in stmt.split(",")]
        assert declared == [f[0] for f in struct._fields_], cname


def _args(cls, **over):
    a = cls()
    a.struct_size = ctypes.sizeof(a)
    a.C, a.D, a.H = 4, 16, 8
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("cls, entry", [("BlockdiagForwardArgs", "tfgnn_blockdiag_forward"),
                                        ("BlockdiagBackwardArgs", "tfgnn_blockdiag_backward")])
def test_argument_refusals_that_need_no_device(cls, entry):
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    fn, cls = getattr(lib, entry), getattr(_lib, cls)
    err = lib.tfgnn_last_error
    assert fn(None, None) == -1 and b"struct_size" in err()
    assert fn(ctypes.byref(_args(cls, struct_size=8)), None) == -1 and b"struct_size" in err()
    assert fn(ctypes.byref(_args(cls)), None) == -1 and b"graph is NULL" in err()  # NULL handle
    assert fn(ctypes.byref(_args(cls, C=0)), None) == -1 and b"num_blocks >= 1" in err()
    assert fn(ctypes.byref(_args(cls, D=0)), None) == -1 and b"D >= 1" in err()
    assert fn(ctypes.byref(_args(cls, D=18)), None) == -1 and b"num_blocks = 4 must divide D = 18 and H = 8" in err()
    assert fn(ctypes.byref(_args(cls, H=10)), None) == -1 and b"num_blocks = 4 must divide D = 16 and H = 10" in err()
    # the cap of the lane mapping: a block is at most 64 wide on either side; D and H themselves are not capped
    assert fn(ctypes.byref(_args(cls, C=1, D=65, H=8)), None) == -4 and b"D / num_blocks <= 64" in err()
    assert fn(ctypes.byref(_args(cls, C=2, D=16, H=130)), None) == -4 and b"H / num_blocks <= 64" in err()
    assert fn(ctypes.byref(_args(cls, C=64, D=4096, H=4096)), None) == -1 and b"graph is NULL" in err()
    with pytest.raises(ValueError, match="num_blocks"):
        _lib.check(fn(ctypes.byref(_args(cls, C=0)), None))


def test_workspace_query_and_launch_counters_without_a_device():
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    q = lib.tfgnn_blockdiag_workspace_bytes
    assert q(0, 16, 16, 0, 0, 0) == 0 and q(3, 16, 15, 0, 0, 0) == 0 and q(1, 65, 8, 0, 0, 0) == 0 and q(4, 16, 8, -1, 0, 0) == 0
    # backward: dX partial rows of D floats + (sum_l ceil(E_l / 256)) * di * H floats; forward: partial rows of H floats
    assert q(4, 16, 8, 0, 0, 0) == 0
    assert q(4, 16, 8, 0, 5, 3) == 5 * 16 * 4 + 3 * 4 * 8 * 4
    assert q(4, 16, 8, 100, 5, 3) == 100 * 8 * 4
    assert q(7, 7, 7, 1, 1, 1) == max(32, 32 + 32)  # every part rounded up to 16 bytes
    buf = (ctypes.c_int64 * 5)(-1, -1, -1, -1, -1)
    assert lib.tfgnn_blockdiag_launch_counts(buf, 5) == 0 and min(buf[:3]) >= 0 and buf[3] == 0 and buf[4] == 0
    assert set(ops.blockdiag_launch_counts()) == {"fwd", "dx", "dq"}
    assert lib.tfgnn_blockdiag_launch_counts(None, 3) == -1


def test_chunk_table_against_a_literal_restatement():
    """types with 0, 1, 255, 256, 257 and 600 edges: chunks of 256 consecutive list positions, never across a type"""
    from tf2_gnn_amd import ops

    ctype, first, count, ptr = ops.blockdiag_chunk_table([0, 1, 255, 256, 257, 600])
    assert ctype == [1, 2, 3, 4, 4, 5, 5, 5]
    assert first == [0, 1, 256, 512, 768, 769, 1025, 1281]
    assert count == [1, 255, 256, 256, 1, 256, 256, 88]
    assert ptr == [0, 0, 1, 2, 3, 5, 8]
    assert ops.blockdiag_chunk_table([]) == ([], [], [], [0])
    assert ops.blockdiag_chunk_table([0, 0]) == ([], [], [], [0, 0, 0])
    assert ops.blockdiag_chunk_table([512]) == ([0, 0], [0, 256], [256, 256], [0, 2])


def test_ops_wrappers_check_their_arguments_before_the_call():
    from tf2_gnn_amd import ops

    class FakeGraph:
        num_edge_types, num_nodes, num_edges = 4, 10, 30

    with pytest.raises((RuntimeError, TypeError, ValueError)):
        ops.blockdiag_forward(FakeGraph(), torch.zeros(4, 4, 8), torch.zeros(10, 16), 4)  # CPU tensors: no fallback
