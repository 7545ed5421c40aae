"""R-GCN basis decomposition, the part that needs no GPU: the two float64 references (tests/rgcn_basis_reference.py) agree
with each other; the layer is registered, has its defaults and refuses what the decomposition does not commute with; the new
C entries are exported, declared and bound with the ABI number unmoved, and refuse bad arguments before they touch a device."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import rgcn_basis_reference as ref
from tests.helpers import random_graph

ROOT = Path(__file__).resolve().parent.parent
NEW = ["tfgnn_basis_gather_forward", "tfgnn_basis_gather_backward", "tfgnn_basis_workspace_bytes", "tfgnn_basis_launch_counts"]


def _small_graph(seed):
    V, L = 23, 5
    adjs = random_graph(V, 120, L, seed=seed, empty_types=(3,), hub=(2, 40))
    adjs[1] = np.concatenate([adjs[1], adjs[1][:4], np.array([[4, 4], [5, 5]], dtype=np.int32)])  # duplicates, self loops
    adjs = [a[(a[:, 1] != 7) & (a[:, 0] != 9)] for a in adjs]  # node 7 without in-edges, node 9 without out-edges
    return adjs, V, L


@pytest.mark.parametrize("aggregation", ["sum", "mean", "sqrt_n"])
@pytest.mark.parametrize("normalize", [True, False])
def test_the_two_references_agree(aggregation, normalize):
    """op-level loops composed to a layer (Z, product with the stacked bases, tanh, and back) == per-edge oracle with composed
    kernels and the chain rule, to 1e-12 of each tensor's largest entry"""
    adjs, V, L = _small_graph(3)
    B, D, H = 3, 6, 5
    rng = np.random.default_rng(5)
    coeff, bases = rng.standard_normal((L, B)), rng.standard_normal((B, D, H)) / np.sqrt(D)
    X, dOut = rng.standard_normal((V, D)), rng.standard_normal((V, H))
    params = ref.rgcn_params(H, aggregation, "tanh", normalize)
    out_l, dX_l, dbases_l, dcoeff_l = ref.layer_reference(params, coeff, bases, X, adjs, dOut)

    s, m, s_src = ref.scales_tables(adjs, V, normalize, aggregation)
    Z, _ = ref.gather_forward(adjs, V, coeff, X, s, m)
    W = bases.reshape(B * D, H)
    out = np.tanh(Z @ W)
    dPre = dOut * (1.0 - out * out)
    dZ = dPre @ W.T
    dX, _ = ref.gather_backward_dx(adjs, V, coeff, dZ, s_src)
    dcoeff, _ = ref.gather_backward_dcoeff(adjs, V, (L, B), X, dZ, s, m)
    for name, got, want in (("out", out, out_l), ("dX", dX, dX_l), ("dbases", (Z.T @ dPre).reshape(B, D, H), dbases_l),
                            ("dcoeff", dcoeff, dcoeff_l)):
        want = want.numpy()
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), name
    assert np.all(dcoeff[3] == 0) and np.all(Z[7] == 0) and np.all(dX[9] == 0)


def test_reference_bounds_are_zero_exactly_where_there_is_no_term():
    adjs, V, L = _small_graph(4)
    rng = np.random.default_rng(1)
    coeff, X, dZ = rng.standard_normal((L, 2)), rng.standard_normal((V, 3)), rng.standard_normal((V, 6))
    Z, zb = ref.gather_forward(adjs, V, coeff, X)
    dX, xb = ref.gather_backward_dx(adjs, V, coeff, dZ)
    dc, cb = ref.gather_backward_dcoeff(adjs, V, (L, 2), X, dZ)
    assert np.all(zb[7] == 0) and np.all(xb[9] == 0) and np.all(cb[3] == 0)
    assert np.all(zb[2] > 0) and zb.shape == Z.shape and xb.shape == dX.shape and cb.shape == dc.shape


def test_registry_and_default_hyperparameters():
    from tf2_gnn_amd.layers import GNN, RGCN_Basis, get_known_message_passing_classes, get_message_passing_class
    from tf2_gnn_amd.layers.message_passing import MessagePassing

    assert get_message_passing_class("rgcn_basis") is RGCN_Basis and get_message_passing_class("RGCN_Basis") is RGCN_Basis
    assert "RGCN_Basis" in set(get_known_message_passing_classes())
    hp = RGCN_Basis.get_default_hyperparameters()
    assert hp["num_bases"] == 8 and hp["normalize_by_num_incoming"] is True
    assert set(hp) == set(MessagePassing.get_default_hyperparameters()) | {"num_bases", "normalize_by_num_incoming"}
    g = GNN.get_default_hyperparameters("rgcn_basis")
    assert g["message_calculation_class"] == "rgcn_basis" and g["num_bases"] == 8
    from tf2_gnn_amd.tasks import LinkPredictionTask

    assert LinkPredictionTask.get_default_hyperparameters("rgcn_basis")["gnn_num_bases"] == 8


@pytest.mark.parametrize("over", [{"aggregation_function": "max"}, {"message_activation_before_aggregation": True},
                                  {"num_bases": 0}])
def test_what_does_not_commute_with_the_decomposition_is_refused_at_construction(over):
    from tf2_gnn_amd.layers import RGCN_Basis

    with pytest.raises(ValueError, match="only commutes with sum-like aggregation"):
        RGCN_Basis(dict(RGCN_Basis.get_default_hyperparameters(), **over))


def test_variables_and_checkpoint_names():
    from tf2_gnn_amd.layers import MessagePassingInput, RGCN_Basis
    from tf2_gnn_amd.layers.message_passing import set_default_device

    set_default_device("cpu")
    try:
        layer = RGCN_Basis(dict(RGCN_Basis.get_default_hyperparameters(), num_bases=3, hidden_dim=5))
        layer.build(MessagePassingInput((None, 4), tuple((None, 2) for _ in range(7))))
    finally:
        set_default_device(None)
    assert [(v.name, v.shape) for v in layer.trainable_variables] == [
        ("basis_0/kernel", (4, 5)), ("basis_1/kernel", (4, 5)), ("basis_2/kernel", (4, 5)), ("relation_coefficients", (7, 3))]
    # the kernels are views of one [B*D, H] buffer, glorot_uniform((D, H)) each
    assert layer._bases.shape == (12, 5) and layer._basis_kernels[1].value.data_ptr() == layer._bases[4:].data_ptr()
    assert float(layer._bases.abs().max()) <= (6.0 / 9) ** 0.5 and float(layer._coeff.abs().max()) <= (6.0 / 10) ** 0.5
    assert layer.graph_parts(10, [1] * 7, 4) == 3  # PLAN_TYPED | PLAN_NODE


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
    for struct, cname in ((_lib.BasisForwardArgs, "tfgnn_basis_forward_args"), (_lib.BasisBackwardArgs, "tfgnn_basis_backward_args")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, flags=re.S).group(1)
        declared = [re.search(r"(\w+)$", part.strip()).group(1) for stmt in body.split(";") if stmt.strip()
                    for part in stmt.split(",")]
        assert declared == [f[0] for f in struct._fields_], cname


def _fwd(**over):
    from tf2_gnn_amd import _lib

    a = _lib.BasisForwardArgs()
    a.struct_size = ctypes.sizeof(a)
    a.B, a.D = 8, 16
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _bwd(**over):
    from tf2_gnn_amd import _lib

    a = _lib.BasisBackwardArgs()
    a.struct_size = ctypes.sizeof(a)
    a.B, a.D = 8, 16
    for k, v in over.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("make, entry", [(_fwd, "tfgnn_basis_gather_forward"), (_bwd, "tfgnn_basis_gather_backward")])
def test_argument_refusals_that_need_no_device(make, entry):
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    fn = getattr(lib, entry)
    assert fn(None, None) == -1 and b"struct_size" in lib.tfgnn_last_error()
    assert fn(ctypes.byref(make(struct_size=8)), None) == -1 and b"struct_size" in lib.tfgnn_last_error()
    assert fn(ctypes.byref(make()), None) == -1 and b"graph is NULL" in lib.tfgnn_last_error()  # NULL handle
    assert fn(ctypes.byref(make(B=0)), None) == -1 and b"1 <= num_bases <= 64" in lib.tfgnn_last_error()
    assert fn(ctypes.byref(make(B=65)), None) in (-1, -4) and b"1 <= num_bases <= 64" in lib.tfgnn_last_error()
    assert fn(ctypes.byref(make(D=0)), None) == -1 and b"D >= 1" in lib.tfgnn_last_error()
    with pytest.raises(ValueError, match="num_bases"):
        _lib.check(fn(ctypes.byref(make(B=0)), None))


def test_workspace_query_and_launch_counters_without_a_device():
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    q = lib.tfgnn_basis_workspace_bytes
    assert q(100, 1000, 4, 0, 16, 0, 0) == 0 and q(100, 1000, 4, 65, 16, 0, 0) == 0 and q(100, 1000, 4, 8, 0, 0, 0) == 0
    # backward: dX partial rows, the [E, B] table, L * ceil(V / 1024) * B chunk sums; forward: partial rows of B * D floats
    assert q(100, 1000, 4, 8, 16, 0, 0) == 1000 * 8 * 4 + 4 * 1 * 8 * 4
    assert q(3000, 1000, 4, 8, 16, 0, 5) == 5 * 16 * 4 + 1000 * 8 * 4 + 4 * 3 * 8 * 4
    assert q(100, 10, 4, 8, 16, 7, 0) == 7 * 8 * 16 * 4
    assert q(0, 0, 1, 1, 1, 0, 0) == 16
    buf = (ctypes.c_int64 * 5)(-1, -1, -1, -1, -1)
    assert lib.tfgnn_basis_launch_counts(buf, 5) == 0 and min(buf[:3]) >= 0 and buf[3] == 0 and buf[4] == 0
    assert set(ops.basis_launch_counts()) == {"basis_fwd", "basis_dx", "basis_dcoeff"}
    assert lib.tfgnn_basis_launch_counts(None, 3) == -1


def test_ops_wrappers_check_their_arguments_before_the_call():
    from tf2_gnn_amd import ops

    class FakeGraph:
        num_edge_types, num_nodes, num_edges = 4, 10, 30

    with pytest.raises((RuntimeError, TypeError, ValueError)):
        ops.basis_gather_forward(FakeGraph(), torch.zeros(4, 8), torch.zeros(10, 16))  # CPU tensors: no fallback
