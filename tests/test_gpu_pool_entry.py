"""Graph readout in one forward and one backward call (tfgnn_pool_forward / tfgnn_pool_backward, csrc/pool_fused.hip):
parity of WeightedSumGraphRepresentation on the new kernels against the fp64 oracle from 1-node graphs to one graph of
200 000 nodes, the C ABI called directly with non-trivial leading dimensions against the op-level sequence it replaces,
the launch counters, run-to-run and capture determinism, and the error paths."""
import numpy as np
import pytest
import torch

from oracle import tf2gnn_oracle as orc
from tests.helpers import assert_close, record_parity, scaled_error
from tests.pool_abi import _raw_backward, _raw_forward

pytestmark = pytest.mark.gpu

KINDS = ["softmax", "sigmoid", "average", "none"]
BOUNDS = [(None, None), (-0.3, 0.4)]  # tanh outputs lie in (-1, 1): both bounds clip a good part of them, not all


def _chunk():
    from tf2_gnn_amd import _lib

    return _lib.POOL_CHUNK_NODES


def _sizes(case):
    C = _chunk()
    rng = np.random.default_rng(11)
    return {
        "small": [5, 1, 9, 3, 7, 12],
        "empty": [0, 4, 0, 0, 3, 0],
        "many": [int(n) for n in rng.integers(1, 31, size=4096)],
        "chunk_boundary": [C - 1, C, C + 1, 3 * C + 7],
        "huge": [3, 200000, 1, 17],
    }[case]


def _ids(sizes):
    return torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(sizes)] + [torch.zeros(0, dtype=torch.int32)])


def _make_layer(dev, wf, sizes, VD, GD, heads, hidden, bounds, seed=3):
    from tf2_gnn_amd.layers import NodesToGraphRepresentationInput, WeightedSumGraphRepresentation
    from tf2_gnn_amd.layers.message_passing import set_seed

    set_seed(seed)
    g = torch.Generator().manual_seed(seed)
    ids = _ids(sizes)
    X = torch.randn((int(ids.numel()), VD), generator=g)
    layer = WeightedSumGraphRepresentation(GD, heads, weighting_fun=wf, scoring_mlp_layers=[hidden], transformation_mlp_layers=[hidden],
                                           scoring_mlp_use_biases=True, transformation_mlp_activation_fun="tanh",
                                           transformation_mlp_result_lower_bound=bounds[0],
                                           transformation_mlp_result_upper_bound=bounds[1])
    inp = NodesToGraphRepresentationInput(X.to(dev), ids.to(dev), len(sizes))
    layer(inp)  # builds
    for v in layer.trainable_variables:
        if v.name.endswith("bias"):
            v.value.copy_(torch.randn(v.shape, generator=g))
    dOut = torch.randn((len(sizes), GD), generator=g)
    return layer, inp, X, ids, dOut


def _pool_weights(layer):
    def mlp(m):
        return [k.value.cpu().clone() for k in m.kernels], [None if b is None else b.value.cpu().clone() for b in m.biases]

    w = {"transformation": mlp(layer._transformation_mlp)}
    if layer._weighting_fun not in ("none", "average"):
        w["scoring"] = mlp(layer._scoring_mlp)
    return w


def _oracle(layer, wf, X, ids, G, GD, heads, bounds, dOut):
    """-> (out, dX, [gradient per MLP variable in the order of _variables(layer)]) in fp64"""
    cfg = {"graph_representation_size": GD, "num_heads": heads, "weighting_fun": wf, "scoring_mlp_activation_fun": "ReLU",
           "transformation_mlp_activation_fun": "tanh", "transformation_mlp_result_lower_bound": bounds[0],
           "transformation_mlp_result_upper_bound": bounds[1]}
    w = _pool_weights(layer)
    X64 = X.double().requires_grad_(True)
    w64 = {k: ([t.double().requires_grad_(True) for t in ks], [None if b is None else b.double().requires_grad_(True) for b in bs])
           for k, (ks, bs) in w.items()}
    ref = orc.weighted_sum_graph_representation(cfg, w64, X64, ids, G)
    leaves = []
    for key in ("transformation", "scoring"):
        if key in w64:
            leaves += list(w64[key][0]) + [b for b in w64[key][1] if b is not None]
    grads = torch.autograd.grad((ref * dOut.double()).sum(), [X64] + leaves)
    return ref.detach(), grads[0], list(grads[1:])


def _variables(layer):
    out = []
    for mlp in (layer._transformation_mlp, getattr(layer, "_scoring_mlp", None)):
        if mlp is not None:
            out += list(mlp.kernels) + [b for b in mlp.biases if b is not None]
    return out


def _clipped_share(layer, bounds):
    T = layer._ctx["T"]
    return float((T < bounds[0]).float().mean()), float((T > bounds[1]).float().mean())


# ---- the op-level sequence the two calls replace (the parent commit's route), through _lib ---------------------------------
def _op_level_forward(kind, ptr, T, S, heads, lo, hi):
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    G, (V, GD) = ptr.numel() - 1, T.shape
    w = None
    if kind == "sigmoid":
        w = S
    elif kind == "softmax":
        w = torch.empty_like(S)
        _lib.check(lib.tfgnn_segment_softmax(ops._ptr(S), heads, heads, ops._ptr(ptr), G, ops._ptr(w), heads, ops._stream()))
    R = T if lo is None and hi is None else ops.clip(T, lo, hi)
    out = torch.empty((G, GD), dtype=torch.float32, device=T.device)
    _lib.check(lib.tfgnn_segment_weighted_sum(ops._ptr(R), ops._ptr(w), ops._ptr(ptr), G, GD, heads, int(kind == "average"),
                                              ops._ptr(out), ops._stream()))
    return out, w, R


def _op_level_backward(kind, ptr, ids, g, T, R, w, heads, lo, hi):
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    G, (V, GD) = ptr.numel() - 1, T.shape
    dR = torch.empty((V, GD), dtype=torch.float32, device=g.device)
    dW = torch.empty((V, heads), dtype=torch.float32, device=g.device) if w is not None else None
    _lib.check(lib.tfgnn_segment_weighted_sum_backward(ops._ptr(g), ops._ptr(R) if w is not None else None, ops._ptr(w), ops._ptr(ids),
                                                       ops._ptr(ptr), V, GD, heads, int(kind == "average"), ops._ptr(dR), ops._ptr(dW),
                                                       ops._stream()))
    if lo is not None or hi is not None:
        dR = ops.clip_backward(dR, T, lo, hi)
    dS = dW
    if kind == "softmax":
        dS = torch.empty_like(dW)
        _lib.check(lib.tfgnn_segment_softmax_backward(ops._ptr(w), ops._ptr(dW), heads, ops._ptr(ptr), G, ops._ptr(dS), ops._stream()))
    return dR, dS


def _layer_on_op_level_route(layer, inp, dOut_dev, heads, bounds):
    """The layer's forward and backward with the readout tail on the op-level calls -> (out, dX, gradients)."""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers.nodes_to_graph_representation import segment_offsets

    wf = layer._weighting_fun
    X = inp.node_embeddings
    ids = inp.node_to_graph_map
    ptr = segment_offsets(ids, int(inp.num_graphs))
    S = None
    if wf == "sigmoid":
        S = layer._scoring_mlp(X, final_act="sigmoid")
    elif wf == "softmax":
        S = layer._scoring_mlp(X)
    T = layer._transformation_mlp(X, final_act="tanh")
    out, w, R = _op_level_forward(wf, ptr, T, S, heads, *bounds)
    dT, dS = _op_level_backward(wf, ptr, ids, dOut_dev, T, R, w, heads, *bounds)
    dX = layer._transformation_mlp.backward(dT)
    if dS is not None:
        dX = ops.add_scale(dX, layer._scoring_mlp.backward(dS), 1.0)
    return out, dX, [v.grad.clone() for v in _variables(layer)]


def _errors(got, ref):
    """scaled errors of (out, dX, gradients) against the fp64 oracle; gradients relative to max(1, largest |reference|)"""
    out, dX, grads = got
    r_out, r_dX, r_grads = ref
    errs = {"out": scaled_error(out, r_out), "dX": scaled_error(dX, r_dX)}
    for i, (a, r) in enumerate(zip(grads, r_grads)):
        scale = max(1.0, float(r.abs().max()))
        errs[f"grad{i}"] = scaled_error(a.cpu().double() / scale, r / scale)
    return errs


@pytest.mark.parametrize("case, VD, GD, heads", [
    ("small", 20, 16, 4), ("empty", 20, 16, 4), ("small", 20, 20, 4), ("empty", 12, 1, 1), ("many", 20, 128, 8),
    ("chunk_boundary", 20, 16, 4), ("chunk_boundary", 20, 128, 8),
])
@pytest.mark.parametrize("bounds", BOUNDS, ids=["nobounds", "clipped"])
@pytest.mark.parametrize("wf", KINDS)
def test_layer_parity_against_the_fp64_oracle(dev, wf, bounds, case, VD, GD, heads):
    sizes = _sizes(case)
    layer, inp, X, ids, dOut = _make_layer(dev, wf, sizes, VD, GD, heads, 24, bounds)
    out = layer(inp)
    if bounds[0] is not None and layer._ctx["V"] > 20:
        below, above = _clipped_share(layer, bounds)
        assert 0.02 < below < 0.9 and 0.02 < above < 0.9, (below, above)
    dX = layer.backward(dOut.to(dev))
    r_out, r_dX, r_grads = _oracle(layer, wf, X, ids, len(sizes), GD, heads, bounds, dOut)
    tag = f"pool entry {wf} {case} GD{GD} {'clip' if bounds[0] is not None else 'plain'}"
    assert_close(out.cpu(), r_out, tol=1e-5, what=tag + " out")
    assert_close(dX.cpu(), r_dX.float(), tol=1e-5, what=tag + " dX")
    for v, r in zip(_variables(layer), r_grads):
        scale = max(1.0, float(r.abs().max()))
        assert_close(v.grad.cpu() / scale, (r / scale).float(), tol=1e-5, what=tag + f" d{v.name}")


@pytest.mark.parametrize("bounds", BOUNDS, ids=["nobounds", "clipped"])
@pytest.mark.parametrize("wf", KINDS)
def test_one_graph_of_200000_nodes_is_no_worse_than_the_op_level_route(dev, wf, bounds):
    """No bound of our own for sums over 200 000 nodes: the new route's largest error against fp64 must not exceed that of the
    op-level sequence on the same inputs (or pass the 1e-5 of the other cases).  Both are logged."""
    sizes = _sizes("huge")
    GD, heads = 128, 4
    layer, inp, X, ids, dOut = _make_layer(dev, wf, sizes, 20, GD, heads, 24, bounds)
    out = layer(inp)
    dX = layer.backward(dOut.to(dev))
    new = (out.cpu(), dX.cpu(), [v.grad.clone() for v in _variables(layer)])
    old = _layer_on_op_level_route(layer, inp, dOut.to(dev), heads, bounds)
    ref = _oracle(layer, wf, X, ids, len(sizes), GD, heads, bounds, dOut)
    e_new, e_old = _errors(new, ref), _errors(old, ref)
    tag = f"pool entry {wf} huge {'clip' if bounds[0] is not None else 'plain'}"
    for k in e_new:
        print(f"{tag} {k}: new {e_new[k]:.3e} op-level {e_old[k]:.3e}")
        record_parity(f"{tag} {k}", max_scaled_error=e_new[k], max_scaled_error_op_level=e_old[k], bound=max(e_old[k], 1e-5))
    for k in e_new:
        assert e_new[k] <= e_old[k] or e_new[k] <= 1e-5, (k, e_new[k], e_old[k])


def _raw_inputs(dev, sizes, GD, heads, col0, seed=5):
    """T, dT as column slices [col0, col0 + GD) of buffers 12 columns wider; S, w, dS as slices of [V, heads + 3] buffers"""
    from tf2_gnn_amd.layers.nodes_to_graph_representation import segment_offsets

    g = torch.Generator().manual_seed(seed)
    ids = _ids(sizes).to(dev)
    V, G = int(ids.numel()), len(sizes)
    ptr = segment_offsets(ids, G)
    T = torch.randn((V, GD + 12), generator=g).to(dev)[:, col0:col0 + GD]
    S = torch.randn((V, heads + 3), generator=g).to(dev)[:, 1:1 + heads]
    dOut = torch.randn((G, GD), generator=g).to(dev)
    return ids, ptr, T, S, dOut


@pytest.mark.parametrize("col0", [4, 1], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("bounds", [(None, None), (-0.5, 0.7)], ids=["nobounds", "clipped"])
@pytest.mark.parametrize("wf", KINDS)
def test_c_abi_with_leading_dimensions_against_the_op_level_sequence(dev, wf, bounds, col0):
    C = _chunk()
    sizes = [5, 0, 1, 2 * C + 9, 30, 0, C, 7]
    GD, heads = 32, 4
    ids, ptr, T, S, dOut = _raw_inputs(dev, sizes, GD, heads, col0)
    V = T.shape[0]
    if wf == "sigmoid":
        S = torch.sigmoid(S)
    if wf in ("none", "average"):
        S = None
    w_buf = torch.full((V, heads + 5), 7.0, device=dev)
    w = w_buf[:, 2:2 + heads] if wf == "softmax" else None
    out = _raw_forward(wf, ptr, T, S, heads, *bounds, w=w)
    w_used = w if wf == "softmax" else S
    dT_buf = torch.full((V, GD + 12), 7.0, device=dev)
    dT = dT_buf[:, col0:col0 + GD]
    dS_buf = torch.full((V, heads + 2), 7.0, device=dev)
    dS = dS_buf[:, 1:1 + heads] if w_used is not None else None
    _raw_backward(wf, ptr, ids, dOut, T, w_used, heads, *bounds, dT, dS)
    Tc = T.contiguous()
    Sc = None if S is None else S.contiguous()
    o_out, o_w, R = _op_level_forward(wf, ptr, Tc, Sc, heads, *bounds)
    o_dT, o_dS = _op_level_backward(wf, ptr, ids, dOut, Tc, R, o_w, heads, *bounds)
    tag = f"pool abi {wf} {'clip' if bounds[0] is not None else 'plain'} col{col0}"
    assert_close(out, o_out, tol=1e-5, what=tag + " out")
    if wf == "softmax":
        assert_close(w, o_w, tol=1e-5, what=tag + " w")
        # the op-level dT multiplies with ITS weights: bit equality is a statement about the same weights
        o_dT, _ = _op_level_backward(wf, ptr, ids, dOut, Tc, R, w.contiguous(), heads, *bounds)
    assert torch.equal(dT, o_dT), tag + " dT: one multiply per element"
    if dS is not None:
        assert_close(dS, o_dS, tol=1e-5, what=tag + " dS")
    # nothing outside the slices was written
    assert float(dT_buf[:, :col0].min()) == 7.0 and float(dT_buf[:, col0 + GD:].min()) == 7.0
    assert float(dS_buf[:, 0].min()) == 7.0 and float(dS_buf[:, 1 + heads:].min()) == 7.0
    assert float(w_buf[:, :2].min()) == 7.0 and float(w_buf[:, 2 + heads:].min()) == 7.0
    assert not bool(torch.isnan(out).any())


@pytest.mark.parametrize("wf", KINDS)
def test_the_layer_runs_the_fused_kernels(dev, wf):
    from tf2_gnn_amd import ops

    for case in ("small", "chunk_boundary"):
        layer, inp, X, ids, dOut = _make_layer(dev, wf, _sizes(case), 20, 16, 4, 24, (None, None))
        before = ops.pool_launch_counts()
        layer(inp)
        mid = ops.pool_launch_counts()
        layer.backward(dOut.to(dev))
        after = ops.pool_launch_counts()
        assert 1 <= mid["pool_fwd"] - before["pool_fwd"] <= 2 and mid["pool_bwd"] == before["pool_bwd"]
        assert 1 <= after["pool_bwd"] - mid["pool_bwd"] <= 2 and after["pool_fwd"] == mid["pool_fwd"]
        if case == "small":  # fewer nodes than a chunk: nothing to combine
            assert mid["pool_fwd"] - before["pool_fwd"] == 1 and after["pool_bwd"] - mid["pool_bwd"] == 1


@pytest.mark.parametrize("case, heads", [("huge", 4), ("many", 8)])
def test_two_runs_are_bit_equal(dev, case, heads):
    from tf2_gnn_amd import ops

    GD = 128
    ids, ptr, T, S, dOut = _raw_inputs(dev, _sizes(case), GD, heads, 4)
    runs = []
    for _ in range(2):
        out, w = ops.pool_forward("softmax", ptr, T, S, heads, -0.5, 0.7)
        dT, dS = ops.pool_backward("softmax", ptr, ids, dOut, T, w, heads, -0.5, 0.7)
        torch.cuda.synchronize()
        runs.append((out.clone(), w.clone(), dT.clone(), dS.clone()))
        S = S.clone()  # other addresses, and the workspace keeps what the first run left in it
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_captured_pooling_step_replays_bit_equal(dev):
    from tf2_gnn_amd import CapturedStep, ops

    C = _chunk()
    layer, inp, X, ids, dOut = _make_layer(dev, "softmax", [9, 2 * C + 5, 1, 0, 40], 20, 128, 8, 24, (-0.3, 0.4))
    g = dOut.to(dev)

    def step():
        out = layer(inp, training=False)
        dX = layer.backward(g)
        return out, dX, [v.grad for v in _variables(layer)]

    def snapshot(res):
        torch.cuda.synchronize()
        return [res[0].clone(), res[1].clone()] + [t.clone() for t in res[2]]

    try:
        eager = snapshot(step())
        cap = CapturedStep(step)
        cap.capture()
        for _ in range(3):
            replayed = snapshot(cap.replay())
            assert all(torch.equal(a, b) for a, b in zip(eager, replayed))
    finally:
        ops.dropout_epoch_set(0)  # a replay advances the dropout epoch; every other test draws the masks of epoch 0
        torch.cuda.synchronize()


def test_error_paths_launch_nothing(dev):
    from tf2_gnn_amd import ops

    ids, ptr, T, S, dOut = _raw_inputs(dev, [300, 5], 16, 4, 4)
    w = torch.empty((T.shape[0], 4), device=dev)
    before = ops.pool_launch_counts()
    with pytest.raises(ValueError, match="workspace"):
        _raw_forward("softmax", ptr, T, S, 4, None, None, w=w, ws_bytes=16)
    with pytest.raises(ValueError, match="struct_size"):
        _raw_forward("softmax", ptr, T, S, 4, None, None, w=w, struct_size=8)
    with pytest.raises(ValueError, match="lower bound"):
        _raw_forward("softmax", ptr, T, S, 4, 1.0, 0.0, w=w)
    assert ops.pool_launch_counts() == before
