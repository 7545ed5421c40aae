"""RGCN_Basis on the device against the layer-level reference of tests/rgcn_basis_reference.py: RGCN with composed kernels
W_l = sum_b a[l,b] V_b through the per-edge fp64 oracle, gradients mapped back by the chain rule.  Bounds: what
tests/test_gpu_layers.py holds RGCN to at these widths - 1e-5 scaled (helpers.assert_close), or, where the reference's own
operation order evaluated in fp32 is already further from fp64 than that, twice its error (four times for un-normalised sums
over the hub, as there); both figures go to the parity log.  Then the layer in its surroundings: the identity case next to
RGCN, a GNN stack, the torch.autograd route, a captured step, a LinkPredictionTask on 37 planted relations, a checkpoint."""
import math
import zlib

import numpy as np
import pytest
import torch

from oracle import tf2gnn_oracle as orc
from tests import rgcn_basis_reference as ref
from tests.helpers import KINK_MARGIN, assert_close, kink_clearance, random_graph, scaled_error, to_dev

# every test runs in the three GEMM modes unless it names its own (conftest.py: gemm_modes)
pytestmark = [pytest.mark.gpu, pytest.mark.gemm_modes, pytest.mark.usefixtures("gemm_mode")]

V_L, E_L = 300, 3000


def _graph(L, seed=4):
    """V = 300, E ~ 3000 + a 150-edge hub at node 2; with L >= 3 the type L - 2 has no edges"""
    return random_graph(V_L, E_L, L, seed=seed, empty_types=(L - 2,) if L >= 3 else (), hub=(2, 150))


def _build(L, B, D, H, **over):
    import tf2_gnn_amd.layers.message_passing as mp

    p = mp.RGCN_Basis.get_default_hyperparameters()
    p.update({"hidden_dim": H, "num_bases": B}, **over)
    mp.set_seed(zlib.crc32(repr((sorted(p.items()), D, L)).encode()) & 0x7FFFFFFF)
    layer = mp.RGCN_Basis(p)
    layer.build(mp.MessagePassingInput((None, D), tuple((None, 2) for _ in range(L))))
    return layer, p


def _weights(layer, D):
    B = layer._num_bases
    return layer._coeff.detach().cpu().clone(), layer._bases.detach().cpu().clone().view(B, D, layer._hidden_dim)


def _oracle_params(p):
    return ref.rgcn_params(p["hidden_dim"], p["aggregation_function"], p["message_activation_function"],
                           p["normalize_by_num_incoming"])


def _draw(forward64, V, D, H, seed, clear_of_kinks):
    """(X, dOut) ~ N(0, 1); with ``clear_of_kinks`` such that no relu unit of the fp64 reference forward lies within KINK_MARGIN
    of 0 (helpers.kink_clearance): chosen on the oracle, before the device runs"""
    for attempt in range(60):
        g = torch.Generator().manual_seed(seed + 1000 * attempt)
        X, dOut = torch.randn((V, D), generator=g), torch.randn((V, H), generator=g)
        if not clear_of_kinks or kink_clearance(lambda: forward64(X)) >= KINK_MARGIN:
            return X, dOut
    raise AssertionError("no kink-free input found in 60 draws")


def _check_layer(dev, name, L, B, D, H, agg, norm, act, backward=True):
    from tf2_gnn_amd.layers import MessagePassingInput

    adjs = _graph(L)
    layer, p = _build(L, B, D, H, aggregation_function=agg, normalize_by_num_incoming=norm, message_activation_function=act)
    coeff, bases = _weights(layer, D)
    po = _oracle_params(p)
    X, dOut = _draw(lambda x: ref.layer_reference(po, coeff, bases, x, adjs)[0], V_L, D, H, 11, act == "relu" and backward)
    out = layer(MessagePassingInput(X.to(dev), to_dev(adjs, dev)), training=True)
    r64 = ref.layer_reference(po, coeff, bases, X, adjs, dOut)
    r32 = ref.layer_reference(po, coeff, bases, X, adjs, dOut, dtype=torch.float32)  # the reference's order in fp32
    slack = 2 if norm else 4

    def close(got, want64, want32, what, per_row=False):
        scale = want64.abs().amax(dim=1, keepdim=True).clamp(min=1.0) if per_row else max(1.0, float(want64.abs().max()))
        err32 = scaled_error(want32.double() / scale, want64 / scale)
        assert_close(got.cpu().double() / scale, want64 / scale, tol=max(1e-5, slack * err32),
                     what=f"rgcn_basis {name} L{L} B{B} {D}x{H} {agg} {what}")  # (the parity log keeps error and bound)

    close(out, r64[0], r32[0], "fwd", per_row=not norm)
    if not backward:
        return
    dX = layer.backward(dOut.to(dev))
    close(dX, r64[1], r32[1], "dX")
    close(torch.stack([v.grad for v in layer._basis_kernels]).reshape(B * D, H), r64[2].reshape(B * D, H),
          r32[2].reshape(B * D, H), "dbases")
    close(layer._coefficients.grad, r64[3], r32[3], "dcoeff")
    assert not layer._coefficients.grad[L - 2].any() if L >= 3 else True  # the type without edges


# L, B, (D, H), aggregation, normalise: every sum-like aggregation, both L, both B, the three width pairs
LAYER_CASES = [
    (4, 2, 64, 64, "sum", True), (37, 8, 64, 64, "mean", True), (4, 8, 65, 33, "sqrt_n", False), (37, 2, 65, 33, "sum", True),
    (4, 8, 128, 320, "mean", True), (37, 2, 128, 320, "sum", False),
]
_IDS = [f"L{c[0]}-B{c[1]}-{c[2]}x{c[3]}-{c[4]}-{'norm' if c[5] else 'raw'}" for c in LAYER_CASES]


@pytest.mark.parametrize("L,B,D,H,agg,norm", LAYER_CASES, ids=_IDS)
def test_forward_relu(dev, L, B, D, H, agg, norm):
    _check_layer(dev, "relu fwd", L, B, D, H, agg, norm, "relu", backward=False)


@pytest.mark.parametrize("L,B,D,H,agg,norm", LAYER_CASES, ids=_IDS)
def test_gradients_tanh(dev, L, B, D, H, agg, norm):
    _check_layer(dev, "tanh", L, B, D, H, agg, norm, "tanh")


@pytest.mark.parametrize("L,B,D,H,agg,norm", LAYER_CASES, ids=_IDS)
def test_gradients_relu_clear_of_kinks(dev, L, B, D, H, agg, norm):
    _check_layer(dev, "relu", L, B, D, H, agg, norm, "relu")


def test_gelu_keeps_the_pre_activation(dev):
    _check_layer(dev, "gelu", 4, 2, 64, 64, "sum", True, "gelu")


def test_identity_coefficients_are_rgcn(dev):
    """B = L, coeff = I: the layer and RGCN with W_l = V_l both meet the oracle"""
    import tf2_gnn_amd.layers.message_passing as mp
    from tf2_gnn_amd.layers import MessagePassingInput

    L, D, H = 4, 64, 64
    adjs = _graph(L)
    layer, p = _build(L, L, D, H, message_activation_function="tanh")
    layer._coefficients.assign(torch.eye(L))
    coeff, bases = _weights(layer, D)
    rp = mp.RGCN.get_default_hyperparameters()
    rp.update({"hidden_dim": H, "message_activation_function": "tanh"})
    rgcn = mp.RGCN(rp)
    rgcn.build(mp.MessagePassingInput((None, D), tuple((None, 2) for _ in range(L))))
    for l in range(L):
        (kernel,) = rgcn._edge_type_mlps.vars[l]
        kernel.assign(bases[l])
    g = torch.Generator().manual_seed(3)
    X, dOut = torch.randn((V_L, D), generator=g), torch.randn((V_L, H), generator=g)
    want, want_dX, _, _ = ref.layer_reference(_oracle_params(p), coeff, bases, X, adjs, dOut)
    inp = MessagePassingInput(X.to(dev), to_dev(adjs, dev))
    for name, lay in (("basis", layer), ("rgcn", rgcn)):
        out = lay(inp, training=True)
        assert_close(out.cpu().double(), want, tol=1e-5, what=f"identity case {name} fwd")
        assert_close(lay.backward(dOut.to(dev)).cpu().double(), want_dX, tol=1e-5, what=f"identity case {name} dX")


# ---- the layer in a GNN stack ---------------------------------------------------------------------------------------------
def _stack(dev, H=64, L=4, B=3, rate=0.0, Din=16, seed=11):
    from tf2_gnn_amd.layers import GNN, GNNInput
    from tf2_gnn_amd.layers.message_passing import set_seed

    params = GNN.get_default_hyperparameters("rgcn_basis")
    params.update({"hidden_dim": H, "num_layers": 2, "num_bases": B, "global_exchange_every_num_layers": 10000,
                   "layer_input_dropout_rate": rate, "dense_every_num_layers": 1, "residual_every_num_layers": 1,
                   "message_activation_function": "tanh", "dense_intermediate_layer_activation": "tanh"})
    set_seed(seed)
    gnn = GNN(params)
    adjs = _graph(L, seed=5)
    X = torch.randn((V_L, Din), generator=torch.Generator().manual_seed(2))
    inp = GNNInput(X.to(dev), to_dev(adjs, dev), torch.zeros(V_L, dtype=torch.int32, device=dev), 1)
    return gnn, params, inp, X, adjs


def test_gnn_stack_forward_and_backward(dev):
    """2 layers, residual and dense after every layer, against gnn_internal_call("rgcn") on composed kernels; the basis and
    coefficient gradients through the composition under fp64 autograd"""
    gnn, params, inp, X, adjs = _stack(dev)
    H, Din = params["hidden_dim"], X.shape[1]
    out = gnn(inp, training=False)
    assert all(type(m).__name__ == "RGCN_Basis" for m in gnn._mp_layers)
    assert gnn.graph_parts(V_L, [a.shape[0] for a in adjs]) == 3  # PLAN_TYPED | PLAN_NODE and nothing else
    dOut = torch.randn((V_L, H), generator=torch.Generator().manual_seed(9))
    gnn.backward(dOut.to(dev))

    def reference(dtype):
        leaves = {"proj": gnn._initial_projection_layer.value.cpu().to(dtype).requires_grad_(True), "coeff": [], "bases": [],
                  "dense": {}}
        w = {"initial_projection": leaves["proj"], "mp": [], "dense": {}, "layernorm": []}
        for i, m in enumerate(gnn._mp_layers):
            D = H  # the stack projects the inputs to H first
            coeff, bases = (t.to(dtype).requires_grad_(True) for t in _weights(m, D))
            leaves["coeff"].append(coeff), leaves["bases"].append(bases)
            w["mp"].append({"edge_mlps": [[k] for k in ref.compose_kernels(coeff, bases)], "aggr_mlp": None})
            w["dense"][i] = leaves["dense"][i] = gnn._dense_layers[str(i)].value.cpu().to(dtype).requires_grad_(True)
        po = dict(params, message_calculation_class="rgcn", use_target_state_as_input=False, num_edge_MLP_hidden_layers=0)
        res, _ = orc.gnn_internal_call(po, w, X.to(dtype), [torch.from_numpy(a) for a in adjs])
        flat = [leaves["proj"]] + leaves["coeff"] + leaves["bases"] + [leaves["dense"][i] for i in sorted(leaves["dense"])]
        return res.detach(), torch.autograd.grad((res * dOut.to(dtype)).sum(), flat)

    (r64, g64), (r32, g32) = reference(torch.float64), reference(torch.float32)
    assert_close(out.cpu().double(), r64, tol=max(1e-5, 2 * scaled_error(r32.double(), r64)), what="rgcn_basis stack fwd")
    n = len(gnn._mp_layers)
    got = ([gnn._initial_projection_layer.grad] + [m._coefficients.grad for m in gnn._mp_layers]
           + [torch.stack([v.grad for v in m._basis_kernels]) for m in gnn._mp_layers]
           + [gnn._dense_layers[str(i)].grad for i in range(n)])
    names = ["d projection"] + [f"d coeff {i}" for i in range(n)] + [f"d bases {i}" for i in range(n)] + [f"d dense {i}" for i in range(n)]
    for what, a, b64, b32 in zip(names, got, g64, g32):
        scale = max(1.0, float(b64.abs().max()))
        assert_close(a.cpu().double().reshape(b64.shape) / scale, b64 / scale,
                     tol=max(1e-5, 2 * scaled_error(b32.double() / scale, b64 / scale)), what=f"rgcn_basis stack {what}")


@pytest.mark.gemm_modes("f16x2", "bf16x3")
def test_torch_autograd_route_equals_the_explicit_backward(dev):
    from tf2_gnn_amd import TorchGNN, TorchMessagePassing
    from tf2_gnn_amd.layers import MessagePassingInput

    gnn, params, inp, _, _ = _stack(dev)
    H = params["hidden_dim"]
    mod = TorchGNN(gnn).train()
    head = torch.nn.Linear(H, 3).to(dev)
    x = inp.node_features.clone().requires_grad_(True)
    out = mod(inp._replace(node_features=x))
    assert out.requires_grad and len(list(mod.parameters())) == len(gnn.trainable_variables)
    head(out).tanh().square().sum().backward()
    got, got_x = [p.grad.clone() for p in mod.parameters()], x.grad.clone()
    out2 = gnn(inp, training=True).detach().requires_grad_(True)
    assert torch.equal(out2, out.detach())
    head(out2).tanh().square().sum().backward()
    dx = gnn.backward(out2.grad.contiguous(), need_input_grad=True)
    for g, v in zip(got, gnn.trainable_variables):
        assert torch.equal(g, v.grad.reshape(g.shape)), v.name
    assert torch.equal(got_x, dx)
    # one layer through TorchMessagePassing
    layer, _ = _build(4, 2, 64, 64, message_activation_function="tanh")
    X = torch.randn((V_L, 64), generator=torch.Generator().manual_seed(4)).to(dev).requires_grad_(True)
    adjs = to_dev(_graph(4), dev)
    tm = TorchMessagePassing(layer).eval()
    tm(MessagePassingInput(X, adjs)).square().sum().backward()
    h = layer(MessagePassingInput(X.detach(), adjs), training=False)
    dX = layer.backward((2.0 * h).contiguous())
    assert torch.equal(X.grad, dX)
    for p_, v in zip(tm.parameters(), layer.trainable_variables):
        assert torch.equal(p_.grad, v.grad.reshape(p_.grad.shape)), v.name


@pytest.mark.gemm_modes("f16x2", "bf16x3")
def test_captured_step_equals_the_eager_step(dev):
    from tf2_gnn_amd import CapturedStep, ops

    gnn, _, inp, _, _ = _stack(dev, L=37, B=8)
    dOut = torch.randn((V_L, 64), generator=torch.Generator().manual_seed(8)).to(dev)

    def step():
        out = gnn(inp, training=True)
        dx = gnn.backward(dOut, need_input_grad=True)
        return out, dx, [v.grad for v in gnn.trainable_variables]

    def snapshot(res):
        torch.cuda.synchronize()
        return [res[0].clone(), res[1].clone()] + [g.clone() for g in res[2]]

    try:
        cap = CapturedStep(step)
        cap.capture()
        for _ in range(2):
            res = cap.replay()
        replayed = snapshot(res)
        eager = snapshot(step())
        assert not cap.guard_tripped()
    finally:
        ops.dropout_epoch_set(0)  # every other test draws the masks of epoch 0
        torch.cuda.synchronize()
    assert len(replayed) == len(eager) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(replayed, eager))


# ---- link prediction on 37 planted relations ------------------------------------------------------------------------------
CLASSES, PER_CLASS = 19, 10  # relation of u -> v = class(u) + class(v): 0 .. 36


def _planted_dataset():
    from tf2_gnn_amd.data import LinkPredictionDataset

    rng = np.random.default_rng(21)
    V = CLASSES * PER_CLASS
    cls = np.arange(V) % CLASSES
    feats = (0.1 * rng.standard_normal((V, CLASSES))).astype(np.float32)
    feats[np.arange(V), cls] += 1.0
    pairs = rng.permutation(V * V)
    u, v = pairs // V, pairs % V
    rel = cls[u] + cls[v]
    train, valid, test = [], [], []
    for t in range(2 * CLASSES - 1):
        e = np.stack([u[rel == t], v[rel == t]], axis=1)
        train.append(e[:40]), valid.append(e[40:46]), test.append(e[46:52])
    params = LinkPredictionDataset.get_default_hyperparameters()
    params.update({"num_negatives_per_positive": 2, "tie_fwd_bkwd_edges": True})
    ds = LinkPredictionDataset(params)
    ds.load_data_from_arrays(feats, train, valid_edges=valid, test_edges=test)
    assert ds.num_relations == 37 and ds.num_edge_types == 38  # tied backward edges + self loops
    return ds


def _link_task(ds, seed):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import LinkPredictionTask

    set_seed(seed)
    params = LinkPredictionTask.get_default_hyperparameters("rgcn_basis")
    assert params["gnn_message_calculation_class"] == "rgcn_basis" and params["gnn_num_bases"] == 8
    params.update({"gnn_hidden_dim": 64, "gnn_num_layers": 2, "gnn_global_exchange_every_num_layers": 10000,
                   "gnn_layer_input_dropout_rate": 0.0, "optimizer": "Adam", "learning_rate": 0.01})
    model = LinkPredictionTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    return model


@pytest.mark.gemm_modes("f16x2", "bf16x3")
def test_link_prediction_trains_evaluates_and_round_trips_a_checkpoint(dev, tmp_path):
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.utils import model_utils as mu

    ds = _planted_dataset()
    np.random.seed(3)
    (batch,) = list(ds.get_batches(DataFold.TRAIN, dev))
    feats, labels = batch
    model = _link_task(ds, 4)
    assert all(type(m).__name__ == "RGCN_Basis" for m in model._gnn._mp_layers)
    losses = [float(model._run_step(feats, labels, training=True)["loss"]) for _ in range(30)]
    print(f"LinkPredictionTask(rgcn_basis) 30 Adam steps: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert all(math.isfinite(l) for l in losses) and losses[-1] < losses[0]
    metrics = model.evaluate_model(ds.get_batches(DataFold.TEST, dev))
    assert list(metrics) == ["mrr", "hits@1", "hits@3", "hits@10"]
    assert all(0.0 <= v <= 1.0 for v in metrics.values()) and metrics["hits@1"] <= metrics["hits@3"] <= metrics["hits@10"]

    names = [v.name for v in model.variables]
    assert len(set(names)) == len(names)
    for i in range(2):
        assert sum(1 for n in names if f"Layer_{i}" in n and "/basis_" in n and n.endswith("/kernel")) == 8, names
        assert sum(1 for n in names if f"Layer_{i}" in n and n.endswith("relation_coefficients")) == 1, names
    want = {v.name: v.value.clone() for v in model.variables}
    path = str(tmp_path / "model_best.pkl")
    mu.save_model(path, model)
    ptrs = [v.value.data_ptr() for v in model.variables]
    for v in model.variables:
        v.assign(torch.zeros_like(v.value))
    restored = mu.load_weights_verbosely(path, model)
    assert set(restored) == set(names)
    for v, ptr in zip(model.variables, ptrs):
        assert v.value.data_ptr() == ptr and torch.equal(v.value, want[v.name]), v.name  # in place: the views stay views
