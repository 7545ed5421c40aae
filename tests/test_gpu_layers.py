"""Parity of the HIP layers (through the C ABI) with the CPU oracle on identical inputs.
Tolerance: fp32 node states within 1e-5 (north_star), scaled: |a-b| <= 1e-5 * max(1, |b|)."""
import zlib

import numpy as np
import pytest
import torch

from oracle import tf2gnn_oracle as orc
from tests.helpers import (KINK_MARGIN, assert_close, kink_clearance, mp_weights_from_layer, random_graph, scaled_error,
                           to_dev)

# every test of this module runs in the three GEMM modes (conftest.py: gemm_modes)
pytestmark = [pytest.mark.gpu, pytest.mark.gemm_modes, pytest.mark.usefixtures("gemm_mode")]


def _build(cls_name, params, D, L):
    import tf2_gnn_amd.layers.message_passing as mp

    cls = getattr(mp, cls_name)
    p = cls.get_default_hyperparameters()
    p.update(params)
    # the weights of a test do not depend on which tests ran before it (the initialiser's generator is global)
    mp.set_seed(zlib.crc32(repr((cls_name, sorted(p.items(), key=lambda kv: kv[0]), D, L)).encode()) & 0x7FFFFFFF)
    layer = cls(p)
    layer.build(mp.MessagePassingInput((None, D), tuple((None, 2) for _ in range(L))))
    return layer, p


# ---- the reference's own known-answer vectors, through the generic path on the GPU ---------------
@pytest.mark.parametrize("idx", range(4))
def test_message_passing_kats_on_gpu(dev, kats, idx):
    """tf2_gnn/test/layers/test_message_passing.py:35-84 with a user subclass (PassSourceStates)."""
    from tf2_gnn_amd.layers import MessagePassing, MessagePassingInput

    class PassSourceStates(MessagePassing):
        def __init__(self):
            params = super().get_default_hyperparameters()
            params["message_activation_function"] = "relu"
            params["aggregation_function"] = "sum"
            super().__init__(params)

        def _message_function(self, edge_source_states, edge_target_states, num_incoming_to_node_per_message,
                              edge_type_idx, training):
            return edge_source_states

    k = kats["message_passing_kats"][idx]
    X = torch.tensor(k["node_embeddings"], dtype=torch.float32, device=dev)
    adjs = tuple(torch.tensor(a, dtype=torch.int32, device=dev).reshape(-1, 2) for a in k["adjacency_lists"])
    out = PassSourceStates()(MessagePassingInput(X, adjs), training=False)
    expected = torch.tensor(k["aggregated_states"], dtype=torch.float32)
    assert out.shape == expected.shape
    np.testing.assert_array_almost_equal(out.cpu().numpy(), expected.numpy())


CASES = [
    # name, class, param overrides
    ("rgcn", "RGCN", {}),
    ("rgcn_tanh_mean", "RGCN", {"message_activation_function": "tanh", "aggregation_function": "mean"}),
    ("rgcn_sqrt_n_nonorm", "RGCN", {"aggregation_function": "sqrt_n", "normalize_by_num_incoming": False}),
    ("rgcn_gelu", "RGCN", {"message_activation_function": "gelu"}),
    ("rgcn_max", "RGCN", {"aggregation_function": "max"}),
    ("rgcn_act_before", "RGCN", {"message_activation_before_aggregation": True, "message_activation_function": "elu"}),
    ("rgcn_target", "RGCN", {"use_target_state_as_input": True}),
    ("rgcn_compact_buckets", "RGCN", {"use_compact_buckets": True}),
    ("ggnn_compact_buckets", "GGNN", {"use_compact_buckets": True}),
    ("edge_mlp_ppi", "GNN_Edge_MLP", {"num_edge_MLP_hidden_layers": 0, "message_activation_function": "gelu"}),
    ("edge_mlp_src_only", "GNN_Edge_MLP", {"use_target_state_as_input": False}),
    ("edge_mlp_default", "GNN_Edge_MLP", {}),  # target states + 1 hidden layer: per-edge MLP (path C)
    ("edge_mlp_2hidden_norm_mean", "GNN_Edge_MLP", {"num_edge_MLP_hidden_layers": 2, "normalize_by_num_incoming": True,
                                                    "aggregation_function": "mean", "message_activation_function": "tanh"}),
    ("rgin", "RGIN", {}),
    ("rgin_norm_aggr_mlp", "RGIN", {"normalize_by_num_incoming": True, "num_aggr_MLP_hidden_layers": 1}),
    ("ggnn", "GGNN", {}),
    ("ggnn_nonorm", "GGNN", {"normalize_by_num_incoming": False}),
    ("rgat", "RGAT", {"num_heads": 4}),
    ("rgat_tanh_8", "RGAT", {"num_heads": 8, "message_activation_function": "tanh"}),
]


@pytest.mark.parametrize("name,cls_name,over", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("H", [16, 64])
def test_layer_forward_parity(dev, name, cls_name, over, H):
    check_layer_forward(dev, name, cls_name, over, H, V=150, E=1800, L=3)


def check_layer_forward(dev, name, cls_name, over, H, V, E, L):
    from tf2_gnn_amd.layers import MessagePassingInput

    D = H
    adjs = random_graph(V, E, L, seed=H, empty_types=(1,) if "rgin" in name else (), hub=(3, min(200, V // 2)))
    layer, p = _build(cls_name, dict(over, hidden_dim=H), D, L)
    g = torch.Generator().manual_seed(H)
    X = torch.randn((V, D), generator=g)
    out = layer(MessagePassingInput(X.to(dev), to_dev(adjs, dev)), training=False)
    w = mp_weights_from_layer(layer)
    adj_t = [torch.from_numpy(a) for a in adjs]
    ref32 = orc.message_passing_call(cls_name, p, w, X, adj_t)
    assert out.shape == (V, H)
    # The fp64 oracle is the arbiter: the HIP result must be within 1e-5 of it.  The reference-order
    # fp32 result is held to the same yardstick; where ITS rounding error already exceeds 1e-5 (long
    # un-normalised sums with cancellation) the HIP path may not be worse than twice that.
    w64 = _to64(w)
    ref64 = orc.message_passing_call(cls_name, p, w64, X.double(), adj_t)
    err_ref32 = scaled_error(ref32, ref64)
    err_hip = scaled_error(out.cpu(), ref64)
    if p.get("normalize_by_num_incoming", True) is False and cls_name != "RGAT":
        # un-normalised sums over a 200-edge hub: states reach |x| ~ 30 and small entries are the result
        # of cancellation; the yardstick is then the magnitude of the node's state vector
        scale = ref64.abs().amax(dim=1, keepdim=True).clamp(min=1.0)
        err_hip = float(((out.cpu().double() - ref64).abs() / scale).max())
        err_ref32 = float(((ref32.double() - ref64).abs() / scale).max())
    assert err_hip <= max(1e-5, 2 * err_ref32), f"{name}: HIP vs fp64 {err_hip:.3e}, reference-order fp32 vs fp64 {err_ref32:.3e}"


def draw_inputs_clear_of_kinks(ref_forward, V, H, seed):
    """(X, dOut) ~ N(0,1) such that no relu / leaky_relu unit of the fp64 oracle forward ``ref_forward(X)`` lies within
    KINK_MARGIN of its kink (tests/helpers.py): the gradient comparison is then between the same linear branches.  The
    selection only looks at the oracle, never at HIP results."""
    for attempt in range(60):
        g = torch.Generator().manual_seed(seed + 1000 * attempt)
        X = torch.randn((V, H), generator=g)
        dOut = torch.randn((V, H), generator=g)
        if kink_clearance(lambda: ref_forward(X)) >= KINK_MARGIN:
            return X, dOut
    raise AssertionError("no kink-free input found in 60 draws")


def _to64(w):
    if isinstance(w, dict):
        return {k: _to64(v) for k, v in w.items()}
    if isinstance(w, list):
        return [_to64(v) for v in w]
    if isinstance(w, tuple):
        return tuple(_to64(v) for v in w)
    if isinstance(w, torch.Tensor):
        return w.double()
    return w


def test_rgcn_odd_dims_scalar_paths(dev):
    """hidden_dim 7 / input dim 5 (the reference's default hidden_dim): unaligned kernels."""
    from tf2_gnn_amd.layers import MessagePassingInput

    V, L, D, H = 40, 2, 5, 7
    adjs = random_graph(V, 300, L, seed=9)
    layer, p = _build("RGCN", {"hidden_dim": H}, D, L)
    X = torch.randn((V, D), generator=torch.Generator().manual_seed(9))
    out = layer(MessagePassingInput(X.to(dev), to_dev(adjs, dev)))
    ref = orc.message_passing_call("rgcn", p, mp_weights_from_layer(layer), X, [torch.from_numpy(a) for a in adjs])
    assert_close(out.cpu(), ref, tol=1e-5, what="rgcn odd dims")


def test_layers_on_empty_and_isolated_inputs(dev):
    from tf2_gnn_amd.layers import MessagePassingInput

    H = 8
    layer, p = _build("RGCN", {"hidden_dim": H}, H, 2)
    X = torch.randn((6, H), generator=torch.Generator().manual_seed(0))
    empty = [np.zeros((0, 2), np.int32), np.zeros((0, 2), np.int32)]
    out = layer(MessagePassingInput(X.to(dev), to_dev(empty, dev)))
    assert torch.equal(out.cpu(), torch.zeros((6, H)))
    # max aggregation over nodes without incoming edges: float32 lowest -> activation
    layer, p = _build("RGCN", {"hidden_dim": H, "aggregation_function": "max", "message_activation_function": "tanh"}, H, 1)
    adj = [np.array([[0, 1], [2, 1]], np.int32)]
    out = layer(MessagePassingInput(X.to(dev), to_dev(adj, dev)))
    ref = orc.message_passing_call("rgcn", p, mp_weights_from_layer(layer), X, [torch.from_numpy(adj[0])])
    assert_close(out.cpu(), ref, tol=1e-5, what="max empty segments")
    assert torch.all(out.cpu()[0] == -1.0)


BWD_CASES = [
    ("rgcn", "RGCN", {}),
    ("rgcn_compact_buckets", "RGCN", {"use_compact_buckets": True}),
    ("rgcn_tanh_mean", "RGCN", {"message_activation_function": "tanh", "aggregation_function": "mean"}),
    ("rgcn_gelu_nonorm", "RGCN", {"message_activation_function": "gelu", "normalize_by_num_incoming": False}),
    ("rgcn_target", "RGCN", {"use_target_state_as_input": True}),
    ("edge_mlp_src_only", "GNN_Edge_MLP", {"use_target_state_as_input": False}),
    ("edge_mlp_default", "GNN_Edge_MLP", {}),
    ("edge_mlp_2hidden_norm_mean", "GNN_Edge_MLP", {"num_edge_MLP_hidden_layers": 2, "normalize_by_num_incoming": True,
                                                    "aggregation_function": "mean", "message_activation_function": "tanh"}),
    ("rgin", "RGIN", {}),
    ("rgin_aggr_mlp", "RGIN", {"normalize_by_num_incoming": True, "num_aggr_MLP_hidden_layers": 1}),
    ("ggnn", "GGNN", {}),
    # general aggregations: max (ties share the gradient), activation before aggregation (message_passing.py:169-172)
    ("rgcn_max", "RGCN", {"aggregation_function": "max"}),
    ("rgcn_preact_relu_max", "RGCN", {"aggregation_function": "max", "message_activation_before_aggregation": True}),
    ("rgcn_preact_tanh_sum", "RGCN", {"message_activation_before_aggregation": True, "message_activation_function": "tanh"}),
    ("edge_mlp_max", "GNN_Edge_MLP", {"aggregation_function": "max"}),
    ("edge_mlp_preact_gelu_mean", "GNN_Edge_MLP", {"message_activation_before_aggregation": True,
                                                   "message_activation_function": "gelu", "aggregation_function": "mean",
                                                   "normalize_by_num_incoming": True}),
    ("edge_mlp_src_only_preact_sqrt_n", "GNN_Edge_MLP", {"use_target_state_as_input": False, "aggregation_function": "sqrt_n",
                                                         "message_activation_before_aggregation": True,
                                                         "message_activation_function": "elu"}),
    ("rgin_max", "RGIN", {"aggregation_function": "max"}),
    ("ggnn_max", "GGNN", {"aggregation_function": "max"}),
]


@pytest.mark.parametrize("name,cls_name,over", BWD_CASES, ids=[c[0] for c in BWD_CASES])
def test_layer_backward_parity(dev, name, cls_name, over):
    """explicit HIP backward == torch autograd through the fp64 oracle (stand-in for tf.GradientTape)."""
    check_layer_backward(dev, name, cls_name, over, V=120, E=1500, L=3, H=32)


def check_layer_backward(dev, name, cls_name, over, V, E, L, H, dout_scale=1.0, adjs=None, dout_row_scale=None):
    """dout_scale: the HIP backward pass gets dOut * dout_scale (a real loss gradient is 1e-9, not N(0,1))
    and its gradients are scaled back before the comparison - the reference gradients are linear in dOut, so every bound
    stays relative to the gradient's OWN magnitude.  dout_row_scale [V]: dOut's rows multiplied by it, for both the HIP pass and
    the references (nodes whose gradients are orders of magnitude apart).  Returns the layer."""
    from tf2_gnn_amd.layers import MessagePassingInput

    if adjs is None:
        adjs = random_graph(V, E, L, seed=4, hub=(2, min(150, V // 2)))
    adj_t = [torch.from_numpy(a) for a in adjs]
    layer, p = _build(cls_name, dict(over, hidden_dim=H), H, L)
    w32 = mp_weights_from_layer(layer)
    X, dOut = draw_inputs_clear_of_kinks(lambda x: orc.message_passing_call(cls_name, p, _to64(w32), x.double(), adj_t), V, H, 11)
    if dout_row_scale is not None:
        dOut = dOut * dout_row_scale.unsqueeze(-1)
    out = layer(MessagePassingInput(X.to(dev), to_dev(adjs, dev)), training=True)
    dX = layer.backward((dOut * dout_scale).to(dev)) / dout_scale

    w64 = _to64(w32)
    leaves = []

    def req(t):
        t.requires_grad_(True)
        leaves.append(t)
        return t

    for l in range(L):
        w64["edge_mlps"][l] = [req(k) for k in w64["edge_mlps"][l]]
    if w64.get("aggr_mlp") is not None:
        w64["aggr_mlp"] = [req(k) for k in w64["aggr_mlp"]]
    for k in ("gru_kernel", "gru_recurrent_kernel", "gru_bias"):
        if k in w64:
            w64[k] = req(w64[k])
    X64 = X.double().requires_grad_(True)
    ref = orc.message_passing_call(cls_name, p, w64, X64, adj_t)
    # the reference-order fp32 evaluation of the same step (forward + autograd): where ITS rounding error against fp64
    # already exceeds the bound (un-normalised sums over a hub, 150+ terms with cancellation), the HIP path may not be
    # worse than twice that (hard part 2)
    X32 = X.clone().requires_grad_(True)
    leaves32 = []

    def req32(t):
        t = t.clone().requires_grad_(True)
        leaves32.append(t)
        return t

    w32g = dict(w32)
    w32g["edge_mlps"] = [[req32(k) for k in w32["edge_mlps"][l]] for l in range(L)]
    if w32.get("aggr_mlp") is not None:
        w32g["aggr_mlp"] = [req32(k) for k in w32["aggr_mlp"]]
    for k in ("gru_kernel", "gru_recurrent_kernel", "gru_bias"):
        if k in w32:
            w32g[k] = req32(w32[k])
    ref32 = orc.message_passing_call(cls_name, p, w32g, X32, adj_t)
    g32 = torch.autograd.grad((ref32 * dOut).sum(), [X32] + leaves32)
    dX32 = g32[0]
    ref32_by_id = {id(t): gr for t, gr in zip(leaves, g32[1:])}  # same traversal order as the fp64 leaves
    # un-normalised sums over the 150-edge hub: the aggregate-first product is ONE fp32 chain over L x D = 640 terms at the
    # magnitude of the 150-edge sum (|.| ~ 45), the reference's order a chain over the 150 messages - factor 4 there
    slack = 4 if p.get("normalize_by_num_incoming", True) is False else 2
    if p.get("normalize_by_num_incoming", True) is False and cls_name != "RGAT":
        # un-normalised sums over the hub (states |x| ~ 30 - 100, small entries are the result of cancellation): the yardstick
        # is the magnitude of the node's state vector, as in check_layer_forward
        rs = ref.detach().abs().amax(dim=1, keepdim=True).clamp(min=1.0)
        assert_close(out.cpu().double() / rs, ref.detach() / rs, tol=max(1e-5, slack * scaled_error(ref32.detach().double() / rs, ref.detach() / rs)),
                     what=name + " fwd")
    else:
        assert_close(out.cpu(), ref.detach().float(), tol=max(1e-5, slack * scaled_error(ref32.detach(), ref.detach())), what=name + " fwd")
    grads = torch.autograd.grad((ref * dOut.double()).sum(), [X64] + leaves)
    assert_close(dX.cpu(), grads[0].float(), tol=max(1e-5, slack * scaled_error(dX32, grads[0])), what=name + " dX")
    ref_by_id = {id(t): gr for t, gr in zip(leaves, grads[1:])}
    pairs = []
    for l in range(L):
        for j, v in enumerate(layer._edge_type_mlps.vars[l]):
            pairs.append((v, w64["edge_mlps"][l][j]))
    if w64.get("aggr_mlp") is not None:
        pairs += list(zip(layer._aggregation_mlp_vars, w64["aggr_mlp"]))
    if "gru_kernel" in w64:
        ru = layer._recurrent_unit
        pairs += [(ru["kernel"], w64["gru_kernel"]), (ru["recurrent_kernel"], w64["gru_recurrent_kernel"]),
                  (ru["bias"], w64["gru_bias"])]
    assert len(pairs) == len(layer.trainable_variables) == len(leaves)
    for v, t in pairs:
        rv = ref_by_id[id(t)]
        assert v.grad is not None, v.name
        scale = max(1.0, float(rv.abs().max()))
        # weight gradients are sums over all edges / nodes: 1e-5 of the largest entry, or - where the reference-order fp32
        # evaluation itself is further from fp64 than that - at most `slack` times its error
        err32 = scaled_error(ref32_by_id[id(t)] / scale, rv / scale)
        assert_close(v.grad.cpu() / (scale * dout_scale), (rv / scale).float(), tol=max(1e-5, slack * err32), what=f"{name} d{v.name}")
    return layer


def _gnn_oracle_weights(gnn):
    w = {"initial_projection": gnn._initial_projection_layer.value.cpu().clone(), "mp": [], "dense": {}, "layernorm": []}
    for i, mp in enumerate(gnn._mp_layers):
        w["mp"].append(mp_weights_from_layer(mp))
        if gnn._use_inter_layer_layernorm:
            g_, b_ = gnn._inter_layer_layernorms[i]
            w["layernorm"].append((g_.value.cpu().clone(), b_.value.cpu().clone()))
        if str(i) in gnn._dense_layers:
            w["dense"][i] = gnn._dense_layers[str(i)].value.cpu().clone()
    return w


@pytest.mark.parametrize(
    "mp_style,over",
    [
        ("rgcn", {"dense_every_num_layers": 10000, "residual_every_num_layers": 10000}),  # PPI_RGCN.json shape
        ("rgcn", {"dense_every_num_layers": 2, "residual_every_num_layers": 2, "use_inter_layer_layernorm": True}),
        ("ggnn", {"dense_every_num_layers": 3, "residual_every_num_layers": 1}),
        ("rgin", {"dense_every_num_layers": 1, "residual_every_num_layers": 2, "use_inter_layer_layernorm": True}),
        # per-edge MLP with target states (path C): both input-gradient products carry the next step's factors
        ("gnn_edge_mlp", {"dense_every_num_layers": 10000, "residual_every_num_layers": 10000}),
        ("gnn_edge_mlp", {"dense_every_num_layers": 2, "residual_every_num_layers": 2}),
    ],
)
def test_gnn_stack_forward_backward_parity(dev, mp_style, over):
    """GNN._internal_call (gnn.py:276-329): forward, all representations, and weight gradients."""
    check_gnn_stack(dev, mp_style, over)


def check_gnn_stack(dev, mp_style, over, V=100, E=1200, L=3, Din=10, H=24, num_layers=4, dout_scale=1.0):
    """dout_scale: as in check_layer_backward - the HIP backward pass gets dOut * dout_scale, its gradients are scaled back."""
    from tf2_gnn_amd.layers import GNN, GNNInput

    params = GNN.get_default_hyperparameters(mp_style)
    params.update({"hidden_dim": H, "num_layers": num_layers, "global_exchange_every_num_layers": 10000})
    params.update(over)
    adjs = random_graph(V, E, L, seed=21)
    gnn = GNN(params)
    g = torch.Generator().manual_seed(5)
    X = torch.randn((V, Din), generator=g)
    dOut = torch.randn((V, H), generator=g)
    inp = GNNInput(X.to(dev), to_dev(adjs, dev), torch.zeros(V, dtype=torch.int32, device=dev), 1)
    out, all_reprs = gnn(inp, training=False, return_all_representations=True)
    w = _gnn_oracle_weights(gnn)
    ref, ref_all = orc.gnn_internal_call(params, w, X, [torch.from_numpy(a) for a in adjs])
    assert len(all_reprs) == params["num_layers"] + 1
    if mp_style == "gnn_edge_mlp":
        # four un-normalised per-edge MLP layers: states reach |x| ~ 10^2 and two fp32 evaluation orders differ by more than the
        # elementwise bound; the fp64 oracle is the arbiter, the yardstick the magnitude of a node's state vector, and the HIP
        # path may not be worse than twice the reference-order fp32 evaluation (as in check_layer_forward)
        ref64f, ref_all64 = orc.gnn_internal_call(params, _to64(w), X.double(), [torch.from_numpy(a) for a in adjs])
        for a, b32, b64 in zip(list(all_reprs) + [out], list(ref_all) + [ref], list(ref_all64) + [ref64f]):
            scale = b64.abs().amax(dim=1, keepdim=True).clamp(min=1.0)
            err_hip = float(((a.cpu().double() - b64).abs() / scale).max())
            err_ref32 = float(((b32.double() - b64).abs() / scale).max())
            assert err_hip <= max(1e-5, 2 * err_ref32), f"gnn {mp_style}: HIP vs fp64 {err_hip:.3e}, reference-order fp32 {err_ref32:.3e}"
    else:
        for a, b in zip(all_reprs, ref_all):
            assert_close(a.cpu(), b, tol=1e-5, what="all_node_representations")
        assert_close(out.cpu(), ref, tol=1e-5, what=f"gnn {mp_style}")

    # backward vs autograd through the fp64 oracle
    w64 = _to64(w)
    leaves = []

    def visit(obj):
        if isinstance(obj, torch.Tensor):
            obj.requires_grad_(True)
            leaves.append(obj)
        elif isinstance(obj, dict):
            for k in obj:
                visit(obj[k])
        elif isinstance(obj, (list, tuple)):
            for v in obj:
                visit(v)

    visit(w64)
    ref64, _ = orc.gnn_internal_call(params, w64, X.double(), [torch.from_numpy(a) for a in adjs])
    grads = torch.autograd.grad((ref64 * dOut.double()).sum(), leaves, allow_unused=True)
    ref_by_id = {id(t): gr for t, gr in zip(leaves, grads)}
    # the same backward pass in the reference's order and fp32: where ITS weight gradients are further than the bound from
    # fp64 (four un-normalised edge-MLP layers: states ~ 10^2), the HIP gradients may be at most twice as far
    import copy

    w32g = copy.deepcopy(w)
    leaves64, leaves = leaves, []
    visit(w32g)
    leaves32, leaves = leaves, leaves64
    ref32g, _ = orc.gnn_internal_call(params, w32g, X, [torch.from_numpy(a) for a in adjs])
    grads32 = torch.autograd.grad((ref32g * dOut).sum(), leaves32, allow_unused=True)
    err32_by_id = {}
    for t64, g64, g32 in zip(leaves64, grads, grads32):
        if g64 is not None and g32 is not None:
            sc = max(1.0, float(g64.abs().max()))
            err32_by_id[id(t64)] = scaled_error(g32 / sc, g64 / sc)

    def grad_close(got, leaf, what):
        r = ref_by_id[id(leaf)]
        scale = max(1.0, float(r.abs().max()))  # relative to the largest entry of the gradient
        assert_close(got.cpu() / (scale * dout_scale), (r / scale).float(), tol=max(1e-5, 2 * err32_by_id.get(id(leaf), 0.0)), what=what)

    gnn(inp, training=False)
    gnn.backward((dOut * dout_scale).to(dev))
    grad_close(gnn._initial_projection_layer.grad, w64["initial_projection"], "d initial projection")
    for i, mp in enumerate(gnn._mp_layers):
        ref_k = w64["mp"][i]["edge_mlps"]
        for l in range(L):
            for j, v in enumerate(mp._edge_type_mlps.vars[l]):
                grad_close(v.grad, ref_k[l][j], f"layer {i} {v.name}")
        if str(i) in gnn._dense_layers:
            grad_close(gnn._dense_layers[str(i)].grad, w64["dense"][i], f"dense {i}")
        if params["use_inter_layer_layernorm"]:
            gam, bet = gnn._inter_layer_layernorms[i]
            grad_close(gam.grad, w64["layernorm"][i][0], f"ln gamma {i}")
    return gnn


def test_gnn_training_dropout_matches_oracle_with_same_masks(dev):
    from tf2_gnn_amd.layers import GNN, GNNInput

    V, L, Din, H = 80, 2, 6, 16
    params = GNN.get_default_hyperparameters("rgcn")
    params.update({"hidden_dim": H, "num_layers": 3, "global_exchange_every_num_layers": 10000,
                   "layer_input_dropout_rate": 0.25, "dense_every_num_layers": 2, "residual_every_num_layers": 2})
    adjs = random_graph(V, 600, L, seed=2)
    gnn = GNN(params)
    X = torch.randn((V, Din), generator=torch.Generator().manual_seed(1))
    inp = GNNInput(X.to(dev), to_dev(adjs, dev), torch.zeros(V, dtype=torch.int32, device=dev), 1)
    out = gnn(inp, training=True)
    masks = [m.cpu() for m in gnn.dropout_masks()]
    assert all(0.6 < float((m > 0).float().mean()) < 0.9 for m in masks)
    ref, _ = orc.gnn_internal_call(params, _gnn_oracle_weights(gnn), X, [torch.from_numpy(a) for a in adjs], dropout_masks=masks)
    assert_close(out.cpu(), ref, tol=1e-5, what="gnn training dropout")
    out_eval = gnn(inp, training=False)
    ref_eval, _ = orc.gnn_internal_call(params, _gnn_oracle_weights(gnn), X, [torch.from_numpy(a) for a in adjs])
    assert_close(out_eval.cpu(), ref_eval, tol=1e-5, what="gnn eval")


def _pool_weights(layer):
    def mlp(m):
        return [k.value.cpu().clone() for k in m.kernels], [None if b is None else b.value.cpu().clone() for b in m.biases]

    w = {"transformation": mlp(layer._transformation_mlp)}
    if layer._weighting_fun not in ("none", "average"):
        w["scoring"] = mlp(layer._scoring_mlp)
    return w


@pytest.mark.parametrize("wf", ["softmax", "sigmoid", "average", "none"])
def test_weighted_sum_graph_representation_parity(dev, wf):
    """nodes_to_graph_representation.py:170-229 forward, and backward vs autograd on the oracle."""
    check_weighted_sum(dev, wf, sizes=[5, 1, 9, 3, 7, 12], VD=20, GD=16, heads=4, hidden=24)


def check_weighted_sum(dev, wf, sizes, VD, GD, heads, hidden):
    from tf2_gnn_amd.layers import NodesToGraphRepresentationInput, WeightedSumGraphRepresentation

    g = torch.Generator().manual_seed(3)
    ids = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(sizes)])
    V = int(ids.numel())
    X = torch.randn((V, VD), generator=g)
    layer = WeightedSumGraphRepresentation(GD, heads, weighting_fun=wf, scoring_mlp_layers=[hidden],
                                           transformation_mlp_layers=[hidden], scoring_mlp_use_biases=True,
                                           transformation_mlp_activation_fun="tanh")
    out = layer(NodesToGraphRepresentationInput(X.to(dev), ids.to(dev), len(sizes)))
    for v in layer.trainable_variables:  # make biases non-trivial, then recompute
        if v.name.endswith("bias"):
            v.value.copy_(torch.randn(v.shape, generator=g))
    out = layer(NodesToGraphRepresentationInput(X.to(dev), ids.to(dev), len(sizes)))
    cfg = {"graph_representation_size": GD, "num_heads": heads, "weighting_fun": wf,
           "scoring_mlp_activation_fun": "ReLU", "transformation_mlp_activation_fun": "tanh"}
    w = _pool_weights(layer)
    ref = orc.weighted_sum_graph_representation(cfg, w, X, ids, len(sizes))
    assert_close(out.cpu(), ref, tol=1e-5, what=f"pool {wf}")
    # backward
    dOut = torch.randn((len(sizes), GD), generator=g)
    dX = layer.backward(dOut.to(dev))
    X64 = X.double().requires_grad_(True)
    w64 = {k: ([t.double().requires_grad_(True) for t in ks], [None if b is None else b.double().requires_grad_(True) for b in bs])
           for k, (ks, bs) in w.items()}
    ref64 = orc.weighted_sum_graph_representation(cfg, w64, X64, ids, len(sizes))
    pairs = []  # (HIP variable, fp64 leaf): kernels and biases of the two MLPs
    for key, mlp in (("transformation", layer._transformation_mlp), ("scoring", getattr(layer, "_scoring_mlp", None))):
        if key in w64:
            pairs += [(v, t) for v, t in zip(mlp.kernels, w64[key][0])]
            pairs += [(v, t) for v, t in zip(mlp.biases, w64[key][1]) if v is not None]
    grads = torch.autograd.grad((ref64 * dOut.double()).sum(), [X64] + [t for _, t in pairs])
    assert_close(dX.cpu(), grads[0].float(), tol=1e-5, what=f"pool {wf} dX")
    for (v, _), r in zip(pairs, grads[1:]):
        scale = max(1.0, float(r.abs().max()))
        assert_close(v.grad.cpu() / scale, (r / scale).float(), tol=1e-5, what=f"pool {wf} d{v.name}")


def test_was_graph_representation_parity(dev):
    from tf2_gnn_amd.layers import NodesToGraphRepresentationInput, WASGraphRepresentation

    g = torch.Generator().manual_seed(8)
    sizes = [4, 6, 2]
    ids = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(sizes)])
    X = torch.randn((int(ids.numel()), 12), generator=g)
    layer = WASGraphRepresentation(graph_representation_size=8, num_heads=2, pooling_mlp_layers=[16, 16])
    out = layer(NodesToGraphRepresentationInput(X.to(dev), ids.to(dev), 3))
    cfg = {"graph_representation_size": 8, "num_heads": 2, "scoring_mlp_activation_fun": "elu",
           "transformation_mlp_activation_fun": "elu"}
    w = {"avg": _pool_weights(layer._weighted_avg_graph_repr_layer), "sum": _pool_weights(layer._weighted_sum_graph_repr_layer),
         "out_projection": layer._out_projection.value.cpu().clone()}
    ref = orc.was_graph_representation(cfg, w, X, ids, 3)
    assert_close(out.cpu(), ref, tol=1e-5, what="WAS")


def test_unsorted_node_to_graph_map_raises(dev):
    from tf2_gnn_amd.layers import NodesToGraphRepresentationInput, WeightedSumGraphRepresentation

    layer = WeightedSumGraphRepresentation(4, 2)
    X = torch.randn((4, 6), device=dev)
    with pytest.raises(ValueError, match="sorted"):
        layer(NodesToGraphRepresentationInput(X, torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=dev), 2))


@pytest.mark.parametrize("K,act", [(4, "relu"), (8, "tanh"), (3, "gelu")])
def test_rgat_backward_parity(dev, K, act):
    """RGAT backward (csrc/rgat.hip + generic gathers) vs autograd through the fp64 oracle."""
    check_rgat_backward(dev, K, act, V=90, E=900, L=3, H=24)


def check_rgat_backward(dev, K, act, V, E, L, H, dout_scale=1.0):
    from tf2_gnn_amd.layers import MessagePassingInput

    adjs = random_graph(V, E, L, seed=6, hub=(1, min(120, V // 2)))
    layer, p = _build("RGAT", {"hidden_dim": H, "num_heads": K, "message_activation_function": act}, H, L)
    adj_t = [torch.from_numpy(a) for a in adjs]
    w32 = mp_weights_from_layer(layer)
    X, dOut = draw_inputs_clear_of_kinks(lambda x: orc.message_passing_call("rgat", p, _to64(w32), x.double(), adj_t), V, H, 12)
    out = layer(MessagePassingInput(X.to(dev), to_dev(adjs, dev)), training=True)
    dX = layer.backward((dOut * dout_scale).to(dev)) / dout_scale  # (see check_layer_backward)
    w64 = _to64(w32)
    for key in ("kernels", "attn"):
        w64[key] = [t.requires_grad_(True) for t in w64[key]]
    X64 = X.double().requires_grad_(True)
    ref = orc.message_passing_call("rgat", p, w64, X64, [torch.from_numpy(a) for a in adjs])
    assert_close(out.cpu(), ref.detach().float(), tol=1e-5, what="rgat fwd")
    grads = torch.autograd.grad((ref * dOut.double()).sum(), [X64] + w64["kernels"] + w64["attn"])
    assert_close(dX.cpu(), grads[0].float(), tol=1e-5, what="rgat dX")
    for l in range(L):
        gk = layer._edge_type_to_message_computation_layer[l].grad
        ga = layer._edge_type_to_attention_parameters[l].grad
        rk, ra = grads[1 + l], grads[1 + L + l]
        sk, sa = max(1.0, float(rk.abs().max())), max(1.0, float(ra.abs().max()))
        assert_close(gk.cpu() / (sk * dout_scale), (rk / sk).float(), tol=1e-5, what=f"rgat dW_{l}")
        assert_close(ga.cpu() / (sa * dout_scale), (ra / sa).float(), tol=1e-5, what=f"rgat dalpha_{l}")


def test_gnn_rgat_stack_backward_runs(dev):
    """RGAT inside the GNN stack (PPI_RGAT.json shape, small): forward parity + finite gradients."""
    from tf2_gnn_amd.layers import GNN, GNNInput

    V, L, Din, H = 70, 2, 9, 16
    params = GNN.get_default_hyperparameters("rgat")
    params.update({"hidden_dim": H, "num_heads": 4, "num_layers": 3, "global_exchange_every_num_layers": 10000,
                   "dense_every_num_layers": 10000, "residual_every_num_layers": 10000})
    adjs = random_graph(V, 500, L, seed=3)
    gnn = GNN(params)
    X = torch.randn((V, Din), generator=torch.Generator().manual_seed(2))
    inp = GNNInput(X.to(dev), to_dev(adjs, dev), torch.zeros(V, dtype=torch.int32, device=dev), 1)
    out = gnn(inp, training=False)
    ref, _ = orc.gnn_internal_call(params, _gnn_oracle_weights(gnn), X, [torch.from_numpy(a) for a in adjs])
    assert_close(out.cpu(), ref, tol=1e-5, what="gnn rgat")
    gnn.backward(torch.ones_like(out))
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in gnn.trainable_variables)


def test_rgcn_compact_bucket_path_on_sparse_graph(dev):
    """Opt-in path over the non-empty (node, type) buckets: forward + backward parity on a graph where
    most buckets are empty."""
    from tf2_gnn_amd.layers import MessagePassingInput

    V, L, H = 400, 4, 32
    adjs = random_graph(V, 360, L, seed=8, empty_types=(2,), hub=(9, 80))
    layer, p = _build("RGCN", {"hidden_dim": H, "use_compact_buckets": True}, H, L)
    g = torch.Generator().manual_seed(3)
    X = torch.randn((V, H), generator=g)
    dOut = torch.randn((V, H), generator=g)
    out = layer(MessagePassingInput(X.to(dev), to_dev(adjs, dev)), training=True)
    assert layer._ctx["path"] == "Ac"
    dX = layer.backward(dOut.to(dev))
    w64 = _to64(mp_weights_from_layer(layer))
    for l in range(L):
        w64["edge_mlps"][l] = [k.requires_grad_(True) for k in w64["edge_mlps"][l]]
    X64 = X.double().requires_grad_(True)
    ref = orc.message_passing_call("rgcn", p, w64, X64, [torch.from_numpy(a) for a in adjs])
    assert_close(out.cpu(), ref.detach().float(), tol=1e-5, what="compact fwd")
    grads = torch.autograd.grad((ref * dOut.double()).sum(), [X64] + [w64["edge_mlps"][l][0] for l in range(L)])
    assert_close(dX.cpu(), grads[0].float(), tol=1e-5, what="compact dX")
    for l in range(L):
        assert_close(layer._edge_type_mlps.vars[l][0].grad.cpu(), grads[1 + l].float(), tol=1e-5, what=f"compact dW{l}")


@pytest.mark.parametrize("cls_name,over", [("RGIN", {}), ("GNN_Edge_MLP", {"use_target_state_as_input": False, "num_edge_MLP_hidden_layers": 2,
                                                                        "normalize_by_num_incoming": True, "aggregation_function": "mean"}),
                                           ("RGIN", {"aggregation_function": "max"}),
                                           ("GNN_Edge_MLP", {"use_target_state_as_input": False, "aggregation_function": "mean",
                                                             "message_activation_before_aggregation": True,
                                                             "message_activation_function": "tanh"})])
def test_path_b_compact_sources_many_edge_types(dev, cls_name, over):
    """Many edge types, few edges per type: the per-type MLPs run over the non-empty (source, type) pairs
    only (grouped GEMMs); forward + backward parity."""
    from tf2_gnn_amd.layers import MessagePassingInput

    V, L, H = 120, 12, 16
    rng = np.random.default_rng(5)
    adjs = [rng.integers(0, V, size=(int(rng.integers(0, 40)), 2)).astype(np.int32) for _ in range(L)]
    adjs[3] = np.zeros((0, 2), np.int32)
    layer, p = _build(cls_name, dict(over, hidden_dim=H), H, L)
    g = torch.Generator().manual_seed(4)
    X = torch.randn((V, H), generator=g)
    dOut = torch.randn((V, H), generator=g)
    out = layer(MessagePassingInput(X.to(dev), to_dev(adjs, dev)), training=True)
    assert layer._ctx["path"] == "Bc"
    dX = layer.backward(dOut.to(dev))
    w64 = _to64(mp_weights_from_layer(layer))
    leaves = []
    for l in range(L):
        w64["edge_mlps"][l] = [k.requires_grad_(True) for k in w64["edge_mlps"][l]]
        leaves += w64["edge_mlps"][l]
    X64 = X.double().requires_grad_(True)
    ref = orc.message_passing_call(cls_name, p, w64, X64, [torch.from_numpy(a) for a in adjs])
    assert_close(out.cpu(), ref.detach().float(), tol=1e-5, what="Bc fwd")
    grads = torch.autograd.grad((ref * dOut.double()).sum(), [X64] + leaves, allow_unused=True)
    assert_close(dX.cpu(), grads[0].float(), tol=1e-5, what="Bc dX")
    i = 1
    for l in range(L):
        for v in layer._edge_type_mlps.vars[l]:
            r = grads[i]
            i += 1
            r = torch.zeros_like(v.grad.cpu().double()) if r is None else r
            assert_close(v.grad.cpu(), r.float(), tol=1e-5, what=f"Bc d{v.name}")


# ---- GNN_FiLM ("next" row f1) -------------------------------------------------------------------------
FILM_CASES = [
    ("film_default", {}),
    ("film_norm_mean_tanh", {"normalize_by_num_incoming": True, "aggregation_function": "mean", "message_activation_function": "tanh"}),
    ("film_hidden_edge_mlp_gelu", {"num_edge_MLP_hidden_layers": 1, "message_activation_function": "gelu"}),
    ("film_hidden_film_mlp_sqrt_n", {"film_parameter_MLP_hidden_layers": [20], "aggregation_function": "sqrt_n",
                                     "normalize_by_num_incoming": True}),
    # per-edge form (tfgnn_film_edge_*): max aggregation, activation before aggregation, target states as edge-MLP input
    ("film_max", {"aggregation_function": "max"}),
    ("film_max_norm_hidden_tanh", {"aggregation_function": "max", "normalize_by_num_incoming": True, "num_edge_MLP_hidden_layers": 1,
                                   "message_activation_function": "tanh"}),
    ("film_act_before_sum_elu", {"message_activation_before_aggregation": True, "message_activation_function": "elu",
                                 "normalize_by_num_incoming": True}),
    ("film_act_before_mean_gelu", {"message_activation_before_aggregation": True, "message_activation_function": "gelu",
                                   "aggregation_function": "mean", "film_parameter_MLP_hidden_layers": [12]}),
    ("film_target_input_sum", {"use_target_state_as_input": True}),
    ("film_target_input_hidden_sqrt_n_norm", {"use_target_state_as_input": True, "num_edge_MLP_hidden_layers": 1,
                                              "aggregation_function": "sqrt_n", "normalize_by_num_incoming": True}),
    ("film_target_input_max_act_before", {"use_target_state_as_input": True, "aggregation_function": "max",
                                          "message_activation_before_aggregation": True, "message_activation_function": "tanh"}),
]


@pytest.mark.parametrize("name,over", FILM_CASES, ids=[c[0] for c in FILM_CASES])
def test_gnn_film_forward_backward_parity(dev, name, over):
    """gnn_film.py:84-108 against the per-edge oracle (fp64 autograd for the gradients)."""
    check_film(dev, name, over, V=90, E=900, L=3, H=24)


def check_film(dev, name, over, V, E, L, H):
    from tf2_gnn_amd.layers import MessagePassingInput

    adjs = random_graph(V, E, L, seed=8, empty_types=(), hub=(3, min(70, V // 2)))
    layer, p = _build("GNN_FiLM", dict(over, hidden_dim=H), H, L)
    adj_t = [torch.from_numpy(a) for a in adjs]
    w32 = mp_weights_from_layer(layer)
    X, dOut = draw_inputs_clear_of_kinks(lambda x: orc.message_passing_call("gnn_film", p, _to64(w32), x.double(), adj_t), V, H, 13)
    out = layer(MessagePassingInput(X.to(dev), to_dev(adjs, dev)), training=True)
    dX = layer.backward(dOut.to(dev))
    w64 = _to64(w32)
    leaves = []
    for key in ("film_mlps", "edge_mlps"):
        for l in range(L):
            w64[key][l] = [k.requires_grad_(True) for k in w64[key][l]]
            leaves += w64[key][l]
    X64 = X.double().requires_grad_(True)
    ref = orc.message_passing_call("gnn_film", p, w64, X64, adj_t)
    # yardstick: the reference-order fp32 evaluation (forward + autograd) against the same fp64 result - un-normalised
    # sums over the hub's 70 edges times gamma: where ITS rounding error exceeds the bound the HIP path may be at most twice that
    X32 = X.clone().requires_grad_(True)
    ref32 = orc.message_passing_call("gnn_film", p, w32, X32, adj_t)
    (dX32,) = torch.autograd.grad((ref32 * dOut).sum(), [X32])
    slack = 4 if p.get("normalize_by_num_incoming", True) is False else 2  # as in check_layer_backward
    assert_close(out.cpu(), ref.detach().float(), tol=max(1e-5, slack * scaled_error(ref32.detach(), ref.detach())), what=name + " fwd")
    grads = torch.autograd.grad((ref * dOut.double()).sum(), [X64] + leaves)
    assert_close(dX.cpu(), grads[0].float(), tol=max(1e-5, slack * scaled_error(dX32, grads[0])), what=name + " dX")
    # variable order of the reference: all FiLM MLPs first, then the edge MLPs (gnn_film.py:72-82)
    hip_vars = [v for l in range(L) for v in layer._film_mlps.vars[l]] + [v for l in range(L) for v in layer._edge_type_mlps.vars[l]]
    assert [v.name for v in layer.trainable_variables] == [v.name for v in hip_vars]
    for v, r in zip(hip_vars, grads[1:]):
        scale = max(1.0, float(r.abs().max()))
        assert_close(v.grad.cpu() / scale, (r / scale).float(), tol=1e-5, what=f"{name} d{v.name}")


def test_gnn_film_in_a_gnn_stack_and_without_edges(dev):
    from tf2_gnn_amd.layers import GNN, GNNInput, MessagePassingInput

    V, L, Din, H = 60, 2, 7, 16
    params = GNN.get_default_hyperparameters("gnn_film")
    params.update({"hidden_dim": H, "num_layers": 2, "global_exchange_every_num_layers": 10000})
    adjs = random_graph(V, 300, L, seed=3)
    gnn = GNN(params)
    X = torch.randn((V, Din), generator=torch.Generator().manual_seed(2))
    inp = GNNInput(X.to(dev), to_dev(adjs, dev), torch.zeros(V, dtype=torch.int32, device=dev), 1)
    out = gnn(inp, training=False)
    assert out.shape == (V, H) and bool(torch.isfinite(out).all())
    gnn.backward(torch.ones_like(out))
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) for v in gnn.trainable_variables)
    # the per-edge form on a batch without edges: activation of the empty aggregate, zero gradients
    layer, _ = _build("GNN_FiLM", {"hidden_dim": H, "aggregation_function": "mean", "use_target_state_as_input": True}, H, L)
    empty = tuple(torch.zeros((0, 2), dtype=torch.int32, device=dev) for _ in range(L))
    out = layer(MessagePassingInput(torch.ones((V, H), device=dev), empty))
    assert float(out.abs().max()) == 0.0
    dX = layer.backward(torch.ones_like(out))
    assert float(dX.abs().max()) == 0.0 and all(float(v.grad.abs().max()) == 0.0 for v in layer.trainable_variables)


# ---- graph global exchange ("next" row f3) --------------------------------------------------------------
def _exchange_weights(ex):
    w = {"pool": _pool_weights(ex._node_to_graph_representation_layer)}
    if hasattr(ex, "_gru"):
        w["gru_kernel"] = ex._gru["kernel"].value.cpu().clone()
        w["gru_recurrent_kernel"] = ex._gru["recurrent_kernel"].value.cpu().clone()
        w["gru_bias"] = ex._gru["bias"].value.cpu().clone()
    if hasattr(ex, "_mlp"):
        w["mlp"] = [k.value.cpu().clone() for k in ex._mlp.kernels]
    return w


@pytest.mark.parametrize("mode,wf", [("gru", "softmax"), ("mean", "sigmoid"), ("mlp", "softmax")])
def test_gnn_with_graph_global_exchange_parity(dev, mode, wf):
    """gnn.py:307-315 + graph_global_exchange.py: a 3-layer RGCN stack with an exchange after layer 2 on a batch of
    5 graphs; forward and every weight gradient against fp64 autograd through the oracle."""
    from tf2_gnn_amd.layers import GNN, GNNInput

    sizes = [13, 1, 22, 9, 15]
    V, L, Din, H = sum(sizes), 2, 6, 16
    rng = np.random.default_rng(3)
    adjs = []
    for _ in range(L):
        parts, base = [], 0
        for n in sizes:
            parts.append(rng.integers(0, n, size=(3 * n, 2)) + base)
            base += n
        adjs.append(np.concatenate(parts).astype(np.int32))
    n2g = np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)
    params = GNN.get_default_hyperparameters("rgcn")
    params.update({"hidden_dim": H, "num_layers": 3, "global_exchange_every_num_layers": 2, "global_exchange_mode": mode,
                   "global_exchange_weighting_fun": wf, "global_exchange_num_heads": 4,
                   "dense_every_num_layers": 10000, "residual_every_num_layers": 10000})
    gnn = GNN(params)
    g = torch.Generator().manual_seed(9)
    X = torch.randn((V, Din), generator=g)
    dOut = torch.randn((V, H), generator=g)
    inp = GNNInput(X.to(dev), to_dev(adjs, dev), torch.from_numpy(n2g).to(dev), len(sizes))
    out = gnn(inp, training=False)
    assert sorted(gnn._global_exchange_layers) == ["2"]
    w = _gnn_oracle_weights(gnn)
    w["global_exchange"] = {2: _exchange_weights(gnn._global_exchange_layers["2"])}
    tadjs = [torch.from_numpy(a) for a in adjs]
    ref, _ = orc.gnn_internal_call(params, w, X, tadjs, node_to_graph_map=torch.from_numpy(n2g), num_graphs=len(sizes))
    assert_close(out.cpu(), ref, tol=1e-5, what=f"gnn + {mode} exchange")

    w64 = _to64(w)
    leaves = []

    def visit(obj):
        if isinstance(obj, torch.Tensor):
            obj.requires_grad_(True)
            leaves.append(obj)
        elif isinstance(obj, dict):
            for k in obj:
                visit(obj[k])
        elif isinstance(obj, (list, tuple)):
            for v in obj:
                if v is not None:
                    visit(v)

    visit(w64)
    ref64, _ = orc.gnn_internal_call(params, w64, X.double(), tadjs, node_to_graph_map=torch.from_numpy(n2g),
                                     num_graphs=len(sizes))
    grads = torch.autograd.grad((ref64 * dOut.double()).sum(), leaves, allow_unused=True)
    by_id = {id(t): gr for t, gr in zip(leaves, grads)}
    gnn.backward(dOut.to(dev))

    def check(var, ref_t, what):
        r = by_id[id(ref_t)]
        assert var.grad is not None, what
        scale = max(1.0, float(r.abs().max()))
        assert_close(var.grad.cpu() / scale, (r / scale).float(), tol=1e-5, what=what)

    check(gnn._initial_projection_layer, w64["initial_projection"], "d initial projection")
    for i, mp in enumerate(gnn._mp_layers):
        for l in range(L):
            for j, v in enumerate(mp._edge_type_mlps.vars[l]):
                check(v, w64["mp"][i]["edge_mlps"][l][j], f"layer {i} {v.name}")
    ex = gnn._global_exchange_layers["2"]
    ew = w64["global_exchange"][2]
    pool = ex._node_to_graph_representation_layer
    for k, t in zip(pool._scoring_mlp.kernels, ew["pool"]["scoring"][0]):
        check(k, t, "exchange scoring " + k.name)
    for k, t in zip(pool._transformation_mlp.kernels, ew["pool"]["transformation"][0]):
        check(k, t, "exchange transformation " + k.name)
    if mode == "gru":
        check(ex._gru["kernel"], ew["gru_kernel"], "exchange gru kernel")
        check(ex._gru["recurrent_kernel"], ew["gru_recurrent_kernel"], "exchange gru recurrent kernel")
        check(ex._gru["bias"], ew["gru_bias"], "exchange gru bias")
    if mode == "mlp":
        for k, t in zip(ex._mlp.kernels, ew["mlp"]):
            check(k, t, "exchange mlp " + k.name)
    # training mode: dropout on the broadcast graph representations is drawn and finite
    out_t = gnn(inp, training=True)
    gnn.backward(dOut.to(dev))
    assert bool(torch.isfinite(out_t).all())


@pytest.mark.parametrize("wf", ["softmax", "sigmoid"])
def test_pooling_training_mode_dropout_and_clipping_parity(dev, wf):
    """Training mode of WeightedSumGraphRepresentation: tf.nn.dropout on the inputs of the MLPs' hidden layers (default
    rate 0.2, nodes_to_graph_representation.py:130-148) and the result clipping (:194-197), forward and backward, with
    the masks the HIP path DREW handed to the oracle; and: the masks are real (rate, scaling), eval mode draws none."""
    from tf2_gnn_amd.layers import NodesToGraphRepresentationInput, WeightedSumGraphRepresentation

    g = torch.Generator().manual_seed(5)
    sizes = [4, 9, 1, 30, 7]
    ids = torch.cat([torch.full((n,), i, dtype=torch.int32) for i, n in enumerate(sizes)])
    V, VD, GD, heads = int(ids.numel()), 24, 16, 4
    X = torch.randn((V, VD), generator=g)
    layer = WeightedSumGraphRepresentation(GD, heads, weighting_fun=wf, scoring_mlp_layers=[32], transformation_mlp_layers=[32, 16],
                                           transformation_mlp_activation_fun="tanh", scoring_mlp_dropout_rate=0.25,
                                           transformation_mlp_dropout_rate=0.5, transformation_mlp_result_lower_bound=-0.3,
                                           transformation_mlp_result_upper_bound=0.4)
    inp = NodesToGraphRepresentationInput(X.to(dev), ids.to(dev), len(sizes))
    out = layer(inp, training=True)
    masks = {"scoring": [None if m is None else m.cpu() for m in layer._scoring_mlp.last_dropout_masks],
             "transformation": [None if m is None else m.cpu() for m in layer._transformation_mlp.last_dropout_masks]}
    assert masks["scoring"][0] is not None and masks["scoring"][-1] is None  # hidden-layer inputs only
    assert masks["transformation"][0] is not None and masks["transformation"][1] is not None and masks["transformation"][2] is None
    m0 = masks["transformation"][0]
    assert set(torch.unique(m0).tolist()) <= {0.0, 2.0} and 0.3 < float((m0 == 0).float().mean()) < 0.7
    cfg = {"graph_representation_size": GD, "num_heads": heads, "weighting_fun": wf, "scoring_mlp_activation_fun": "ReLU",
           "transformation_mlp_activation_fun": "tanh", "transformation_mlp_result_lower_bound": -0.3,
           "transformation_mlp_result_upper_bound": 0.4}
    w = _pool_weights(layer)
    X64 = X.double().requires_grad_(True)
    w64 = {k: ([t.double().requires_grad_(True) for t in ks], [None if b is None else b.double() for b in bs]) for k, (ks, bs) in w.items()}
    m64 = {k: [None if m is None else m.double() for m in v] for k, v in masks.items()}
    ref = orc.weighted_sum_graph_representation(cfg, w64, X64, ids, len(sizes), dropout_masks=m64)
    assert_close(out.cpu(), ref.detach().float(), tol=1e-5, what=f"pool training {wf}")
    dOut = torch.randn((len(sizes), GD), generator=g)
    dX = layer.backward(dOut.to(dev))
    leaves = [X64] + w64["transformation"][0] + w64["scoring"][0]
    grads = torch.autograd.grad((ref * dOut.double()).sum(), leaves)
    assert_close(dX.cpu(), grads[0].float(), tol=1e-5, what=f"pool training {wf} dX")
    got_k = [v.grad.cpu() for v in layer._transformation_mlp.kernels] + [v.grad.cpu() for v in layer._scoring_mlp.kernels]
    for a, b in zip(got_k, grads[1:]):
        assert_close(a, b.float(), tol=1e-5, what=f"pool training {wf} dKernel")
    # the same masks injected reproduce the forward bit for bit; eval mode draws none
    layer.dropout_masks = {k: [None if m is None else m.to(dev) for m in v] for k, v in masks.items()}
    assert torch.equal(layer(inp, training=True), out)
    layer.dropout_masks = None
    layer(inp, training=False)
    assert all(m is None for m in layer._transformation_mlp.last_dropout_masks)


def test_graph_cache_does_not_return_a_stale_graph_for_reallocated_adjacency_tensors(dev):
    """the Graph cache was keyed on tensor addresses only - a new batch whose adjacency tensors got the freed
    addresses of the previous one (same shapes, fresh version counters) was handed the old bucketing."""
    import gc

    from tf2_gnn_amd.layers import MessagePassingInput, RGCN
    from tf2_gnn_amd.layers.message_passing import clear_graph_cache

    V, L, H = 50, 2, 8
    layer = RGCN(dict(RGCN.get_default_hyperparameters(), hidden_dim=H))
    layer.build(MessagePassingInput((None, H), tuple((None, 2) for _ in range(L))))
    X = torch.randn((V, H), generator=torch.Generator().manual_seed(0)).to(dev)
    clear_graph_cache()
    outs, ptrs = [], []
    for seed in range(4):
        adjs = random_graph(V, 400, L, seed=seed)
        adj_dev = to_dev(adjs, dev)
        ptrs.append(tuple(a.data_ptr() for a in adj_dev))
        out = layer(MessagePassingInput(X, adj_dev), training=False)
        ref = orc.message_passing_call("rgcn", layer._params if hasattr(layer, "_params") else dict(RGCN.get_default_hyperparameters(), hidden_dim=H),
                                       mp_weights_from_layer(layer), X.cpu(), [torch.from_numpy(a) for a in adjs])
        assert_close(out.cpu(), ref, tol=1e-5, what=f"graph cache batch {seed}")
        del adj_dev, out
        gc.collect()
    # strides and devices are part of the key: a transposed view of the same storage is a different graph
    a = torch.randint(0, V, (2, 300), dtype=torch.int32, device=dev)
    view = a.t()  # [300, 2] with strides (1, 300)
    o1 = layer(MessagePassingInput(X, (view, view.contiguous())), training=False)
    o2 = layer(MessagePassingInput(X, (view.contiguous(), view.contiguous())), training=False)
    assert torch.allclose(o1, o2)


# ---- user-defined message functions: the generic path and its backward ------------------------------------------
@pytest.mark.parametrize("agg,act,before", [("sum", "relu", False), ("mean", "tanh", True), ("max", "elu", False),
                                            ("sqrt_n", "gelu", False), ("max", "tanh", True)])
def test_generic_message_passing_forward_backward_with_a_user_message_function(dev, agg, act, before):
    """A subclass that only implements _message_function (as the reference's extension point, message_passing.py:64-93):
    forward through the gather / aggregation kernels, backward = kernels + torch autograd of the user's function,
    against a plain fp64 torch restatement."""
    from tf2_gnn_amd.layers import MessagePassingInput
    from tf2_gnn_amd.layers.message_passing import MessagePassing
    from tf2_gnn_amd.layers.message_passing.message_passing import glorot_uniform

    class UserLayer(MessagePassing):
        def build(self, input_shapes):
            D = int(input_shapes.node_embeddings[-1])
            L = len(input_shapes.adjacency_lists)
            self.w_src = [self.add_weight(f"edge_type_{l}/w_src", glorot_uniform((D, self._hidden_dim))) for l in range(L)]
            self.w_tgt = [self.add_weight(f"edge_type_{l}/w_tgt", glorot_uniform((D, self._hidden_dim))) for l in range(L)]
            super().build(input_shapes)

        def _message_function(self, edge_source_states, edge_target_states, num_incoming_to_node_per_message, edge_type_idx,
                              training):
            m = edge_source_states @ self.w_src[edge_type_idx].value + torch.sin(edge_target_states @ self.w_tgt[edge_type_idx].value)
            return m / (num_incoming_to_node_per_message + 1.0).unsqueeze(-1)

    V, L, D, H = 70, 3, 12, 20
    adjs = random_graph(V, 600, L, seed=21, empty_types=(1,), hub=(5, 40))
    p = MessagePassing.get_default_hyperparameters()
    p.update({"hidden_dim": H, "aggregation_function": agg, "message_activation_function": act,
              "message_activation_before_aggregation": before})
    layer = UserLayer(p)
    gen = torch.Generator().manual_seed(5)
    X = torch.randn((V, D), generator=gen)
    dOut = torch.randn((V, H), generator=gen)
    out = layer(MessagePassingInput(X.to(dev), to_dev(adjs, dev)), training=True)
    dX = layer.backward(dOut.to(dev))
    assert all(not v.value.requires_grad for v in layer.trainable_variables)

    # fp64 restatement
    X64 = X.double().requires_grad_(True)
    ws = [v.value.detach().cpu().double().requires_grad_(True) for v in layer.w_src]
    wt = [v.value.detach().cpu().double().requires_grad_(True) for v in layer.w_tgt]
    cnt = orc.calculate_type_to_num_incoming_edges(X64, [torch.from_numpy(a) for a in adjs])
    msgs, tgts = [], []
    for l, a in enumerate(adjs):
        a = torch.from_numpy(a).long()
        m = X64[a[:, 0]] @ ws[l] + torch.sin(X64[a[:, 1]] @ wt[l])
        msgs.append(m / (cnt[l][a[:, 1]] + 1.0).unsqueeze(-1))
        tgts.append(a[:, 1])
    m_all, t_all = torch.cat(msgs), torch.cat(tgts)
    act_fn = orc.get_activation_function(act)
    if before:
        m_all = act_fn(m_all)
    ref = orc.get_aggregation_function(agg)(m_all, t_all, V)
    if not before:
        ref = act_fn(ref)
    assert_close(out.cpu(), ref.detach().float(), tol=1e-5, what=f"generic {agg}/{act}/{before} fwd")
    grads = torch.autograd.grad((ref * dOut.double()).sum(), [X64] + ws + wt)
    assert_close(dX.cpu(), grads[0].float(), tol=1e-5, what=f"generic {agg}/{act}/{before} dX")
    for v, r in zip(layer.w_src + layer.w_tgt, grads[1:]):
        scale = max(1.0, float(r.abs().max()))
        assert_close(v.grad.cpu() / scale, (r / scale).float(), tol=1e-5, what=f"generic {agg}/{act}/{before} d{v.name}")


def test_generic_backward_refuses_what_it_cannot_differentiate(dev):
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers import MessagePassingInput
    from tf2_gnn_amd.layers.message_passing import MessagePassing

    class KernelOnly(MessagePassing):
        def _message_function(self, edge_source_states, edge_target_states, num_incoming_to_node_per_message, edge_type_idx,
                              training):
            return ops.activation_forward("tanh", edge_source_states.detach())  # a HIP call: no autograd history

    p = MessagePassing.get_default_hyperparameters()
    p["hidden_dim"] = 8
    layer = KernelOnly(p)
    adjs = random_graph(20, 60, 2, seed=1)
    out = layer(MessagePassingInput(torch.randn((20, 8), device=dev), to_dev(adjs, dev)), training=True)
    with pytest.raises(NotImplementedError, match="autograd history"):
        layer.backward(torch.ones_like(out))
    # eval-mode forward passes record no tape (and leave the variables plain tensors): backward says so
    out = layer(MessagePassingInput(torch.randn((20, 8), device=dev), to_dev(adjs, dev)), training=False)
    with pytest.raises(RuntimeError, match="training"):
        layer.backward(torch.ones_like(out))


@pytest.mark.parametrize("cls_name,over", [("RGCN", {}), ("GNN_Edge_MLP", {"num_edge_MLP_hidden_layers": 1}),
                                           ("GNN_FiLM", {"normalize_by_num_incoming": True})])
def test_overriding_message_function_on_a_builtin_layer(dev, cls_name, over):
    """A user subclass of a built-in layer that post-processes ``super()._message_function`` (the reference's plug-in
    point, message_passing.py:64-93): runs on the generic path with the built-in's weights.  Doubling every message
    must double the relu output and every gradient of the built-in layer."""
    import tf2_gnn_amd.layers as layers
    from tf2_gnn_amd.layers import MessagePassingInput

    base = getattr(layers, cls_name)

    class Doubled(base):
        def _message_function(self, edge_source_states, edge_target_states, num_incoming_to_node_per_message, edge_type_idx,
                              training):
            return 2.0 * super()._message_function(edge_source_states, edge_target_states, num_incoming_to_node_per_message,
                                                   edge_type_idx, training)

    V, L, H = 80, 3, 16
    adjs = random_graph(V, 700, L, seed=4, hub=(2, 50))
    p = base.get_default_hyperparameters()
    p.update(dict(over, hidden_dim=H, message_activation_function="relu"))
    builtin, user = base(p), Doubled(p)
    shapes = MessagePassingInput((None, H), tuple((None, 2) for _ in range(L)))
    builtin.build(shapes)
    user.build(shapes)
    for a, b in zip(builtin.trainable_variables, user.trainable_variables):
        b.assign(a.value)
    g = torch.Generator().manual_seed(3)
    X = torch.randn((V, H), generator=g).to(dev)
    dOut = torch.randn((V, H), generator=g).to(dev)
    inp = MessagePassingInput(X, to_dev(adjs, dev))
    o1 = builtin(inp, training=True)
    dx1 = builtin.backward(dOut)
    o2 = user(inp, training=True)
    dx2 = user.backward(dOut)
    assert_close(o2.cpu(), 2.0 * o1.cpu(), tol=1e-5, what=f"{cls_name} user override fwd")
    assert_close(dx2.cpu(), 2.0 * dx1.cpu(), tol=1e-5, what=f"{cls_name} user override dX")
    for a, b in zip(builtin.trainable_variables, user.trainable_variables):
        scale = max(1.0, float(a.grad.abs().max()))
        assert_close(b.grad.cpu() / scale, 2.0 * a.grad.cpu() / scale, tol=1e-5, what=f"{cls_name} user override d{a.name}")


def test_overriding_message_function_where_the_aggregation_is_not_the_base_class_raises(dev):
    from tf2_gnn_amd.layers import GGNN, RGAT, MessagePassingInput

    for base, extra in ((GGNN, {}), (RGAT, {"num_heads": 2})):
        class Mine(base):
            def _message_function(self, *args, **kwargs):
                return args[0]

        p = base.get_default_hyperparameters()
        p.update(dict(extra, hidden_dim=8))
        layer = Mine(p)
        with pytest.raises(NotImplementedError, match="override call"):
            layer(MessagePassingInput(torch.zeros((10, 8), device=dev), to_dev(random_graph(10, 20, 2, seed=0), dev)))


PER_EDGE_CASES = [
    ("ggnn", "GGNN", {}),
    ("ggnn_nonorm", "GGNN", {"normalize_by_num_incoming": False}),
    ("rgcn_tanh_mean", "RGCN", {"message_activation_function": "tanh", "aggregation_function": "mean"}),
    ("rgcn_sqrt_n_nonorm_gelu", "RGCN", {"aggregation_function": "sqrt_n", "normalize_by_num_incoming": False,
                                         "message_activation_function": "gelu"}),
    # (tanh: with fewer edges than buckets some nodes have no in-edge, and relu(0) sits exactly on its kink)
    ("edge_mlp_default_tanh", "GNN_Edge_MLP", {"message_activation_function": "tanh"}),
    ("edge_mlp_2hidden_norm_mean", "GNN_Edge_MLP", {"num_edge_MLP_hidden_layers": 2, "normalize_by_num_incoming": True,
                                                    "aggregation_function": "mean", "message_activation_function": "tanh"}),
]


@pytest.mark.parametrize("name,cls_name,over", PER_EDGE_CASES, ids=[c[0] for c in PER_EDGE_CASES])
def test_one_message_per_edge_formulation(dev, monkeypatch, name, cls_name, over):
    """Graphs with fewer edges than (node, type) buckets take the per-edge formulation (rows of X read through the edge's source /
    target index, tfgnn_gemm_gathered) once every edge type is large enough for the streaming kernel; here the size threshold is
    lowered so that the layer logic - index arrays, normalisation, aggregation, the unchanged backward pass - is held against the
    fp64 oracle on a small graph (the products themselves then take the gather + gemm route of ops.gemm_gathered)."""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers.message_passing import gnn_edge_mlp

    monkeypatch.setattr(gnn_edge_mlp, "PER_EDGE_MIN_ROWS", 1)
    calls = []
    real = ops.gemm_gathered
    monkeypatch.setattr(ops, "gemm_gathered", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    check_layer_backward(dev, "per-edge " + name, cls_name, over, V=400, E=900, L=3, H=128)
    if ops.get_gemm_mode() != ops.GEMM_FP32:
        assert calls, "the per-edge formulation did not run"
    else:
        assert not calls
