"""RGCN_BlockDiag on the device against the layer-level reference of tests/rgcn_blockdiag_reference.py: RGCN with dense kernels
composed from the blocks through the per-edge fp64 oracle, gradients mapped back onto the band.  Bound: 1e-5 scaled
(helpers.assert_close), what tests/test_gpu_layers.py holds RGCN to.  Then the layer in its surroundings: C = 1 next to RGCN,
a GNN stack, the torch.autograd route, a captured step, a LinkPredictionTask on 37 planted relations, a checkpoint."""
import math
import zlib

import numpy as np
import pytest
import torch

from oracle import tf2gnn_oracle as orc
from tests import rgcn_blockdiag_reference as ref
from tests.helpers import KINK_MARGIN, assert_close, random_graph, to_dev

# the layer itself runs no product; the tests of its surroundings (Dense layers, projections, scoring) name their GEMM modes
pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("gemm_mode")]

V_L, E_L = 300, 3000
KINKED = ("relu", "leaky_relu", "selu")  # derivative discontinuous at 0


def _graph(L, seed=4):
    """V = 300, E ~ 3000 + a 150-edge hub at node 2; with L >= 3 the type L - 2 has no edges"""
    return random_graph(V_L, E_L, L, seed=seed, empty_types=(L - 2,) if L >= 3 else (), hub=(2, 150))


def _build(L, C, D, H, **over):
    import tf2_gnn_amd.layers.message_passing as mp

    p = mp.RGCN_BlockDiag.get_default_hyperparameters()
    p.update({"hidden_dim": H, "num_blocks": C}, **over)
    mp.set_seed(zlib.crc32(repr((sorted(p.items()), D, L)).encode()) & 0x7FFFFFFF)
    layer = mp.RGCN_BlockDiag(p)
    layer.build(mp.MessagePassingInput((None, D), tuple((None, 2) for _ in range(L))))
    return layer, p


def _oracle_params(p):
    return ref.rgcn_params(p["hidden_dim"], p["aggregation_function"], p["message_activation_function"],
                           p["normalize_by_num_incoming"])


def _draw(pre64, V, D, H, seed, clear_of_kinks):
    """(X, dOut) ~ N(0, 1); with ``clear_of_kinks`` such that no pre-activation of the fp64 reference lies within KINK_MARGIN
    (relative to max(1, the row's largest)) of 0: chosen on the fp64 reference, before the device runs"""
    for attempt in range(60):
        g = torch.Generator().manual_seed(seed + 1000 * attempt)
        X, dOut = torch.randn((V, D), generator=g), torch.randn((V, H), generator=g)
        if not clear_of_kinks:
            return X, dOut
        pre = pre64(X)
        live = pre[pre.abs().amax(dim=1) > 0]  # rows without in-edges are exact zeros on both sides
        if float((live.abs() / live.abs().amax(dim=1, keepdim=True).clamp(min=1.0)).min()) >= KINK_MARGIN:
            return X, dOut
    raise AssertionError("no kink-free input found in 60 draws")


def _check_layer(dev, L, C, D, H, agg, norm, act):
    from tf2_gnn_amd.layers import MessagePassingInput

    adjs = _graph(L)
    layer, p = _build(L, C, D, H, aggregation_function=agg, normalize_by_num_incoming=norm, message_activation_function=act)
    Qb = layer._qb.detach().cpu().clone()
    assert Qb.shape == (L, D // C, H)
    s, m, _ = ref.scales_tables(adjs, V_L, norm, agg)  # the pre-activation: the op-level loops in fp64 (the oracle has no identity)
    X, dOut = _draw(lambda x: torch.from_numpy(ref.forward(adjs, V_L, Qb.numpy(), x.numpy(), C, s, m)[0]), V_L, D, H, 11, act in KINKED)
    out = layer(MessagePassingInput(X.to(dev), to_dev(adjs, dev)), training=True)
    want, want_dX, want_dQ = ref.layer_reference(_oracle_params(p), Qb, C, X, adjs, dOut)

    def close(got, want64, what, per_row=False):
        scale = want64.abs().amax(dim=1, keepdim=True).clamp(min=1.0) if per_row else max(1.0, float(want64.abs().max()))
        assert_close(got.cpu().double() / scale, want64 / scale, tol=1e-5,
                     what=f"rgcn_blockdiag {act} L{L} C{C} {D}x{H} {agg} {'norm' if norm else 'raw'} {what}")

    close(out, want, "fwd", per_row=not norm)
    dX = layer.backward(dOut.to(dev))
    close(dX, want_dX, "dX")
    dQ = layer._block_kernels.grad
    assert dQ.shape == (L, D // C, H)
    close(dQ.reshape(L * (D // C), H), want_dQ.reshape(L * (D // C), H), "dQb")
    assert not dQ[L - 2].any() if L >= 3 else True  # the type without edges


# every sum-like aggregation with and without the degree normalisation, both width pairs, both L
LAYER_CASES = [(agg, norm, L, C, D, H) for agg in ("sum", "mean", "sqrt_n") for norm in (True, False)
               for (L, C, D, H) in ((4, 8, 64, 64), (37, 5, 65, 35))]


@pytest.mark.parametrize("agg,norm,L,C,D,H", LAYER_CASES, ids=[f"{c[0]}-{'norm' if c[1] else 'raw'}-L{c[2]}-C{c[3]}-{c[4]}x{c[5]}" for c in LAYER_CASES])
def test_forward_and_gradients_tanh(dev, agg, norm, L, C, D, H):
    _check_layer(dev, L, C, D, H, agg, norm, "tanh")


@pytest.mark.parametrize("act", ["relu", "leaky_relu", "elu", "selu", "gelu"])  # tanh: above; the oracle has no identity
@pytest.mark.parametrize("L,C,D,H", [(4, 8, 64, 64), (37, 5, 65, 35)])
def test_every_activation(dev, act, L, C, D, H):
    _check_layer(dev, L, C, D, H, "mean" if L == 37 else "sum", True, act)


def test_one_block_is_rgcn(dev):
    """C = 1: the layer and RGCN with the same dense kernels both meet the oracle, forward and every gradient"""
    import tf2_gnn_amd.layers.message_passing as mp
    from tf2_gnn_amd.layers import MessagePassingInput

    L, D, H = 4, 64, 64
    adjs = _graph(L)
    layer, p = _build(L, 1, D, H, message_activation_function="tanh")
    W = layer.dense_kernels().cpu()
    assert torch.equal(W, layer._qb.cpu())  # one block: the band is the dense kernel
    rp = mp.RGCN.get_default_hyperparameters()
    rp.update({"hidden_dim": H, "message_activation_function": "tanh"})
    rgcn = mp.RGCN(rp)
    rgcn.build(mp.MessagePassingInput((None, D), tuple((None, 2) for _ in range(L))))
    for l in range(L):
        (kernel,) = rgcn._edge_type_mlps.vars[l]
        kernel.assign(W[l])
    g = torch.Generator().manual_seed(3)
    X, dOut = torch.randn((V_L, D), generator=g), torch.randn((V_L, H), generator=g)
    want, want_dX, want_dQ = ref.layer_reference(_oracle_params(p), W, 1, X, adjs, dOut)
    inp = MessagePassingInput(X.to(dev), to_dev(adjs, dev))
    for name, lay in (("blockdiag", layer), ("rgcn", rgcn)):
        out = lay(inp, training=True)
        assert_close(out.cpu().double(), want, tol=1e-5, what=f"one block {name} fwd")
        assert_close(lay.backward(dOut.to(dev)).cpu().double(), want_dX, tol=1e-5, what=f"one block {name} dX")
    scale = max(1.0, float(want_dQ.abs().max()))
    got_rgcn = torch.stack([rgcn._edge_type_mlps.vars[l][0].grad.reshape(D, H) for l in range(L)])
    for name, got in (("blockdiag", layer._block_kernels.grad), ("rgcn", got_rgcn)):
        assert_close(got.cpu().double() / scale, want_dQ / scale, tol=1e-5, what=f"one block {name} dW")


# ---- the layer in a GNN stack ---------------------------------------------------------------------------------------------
def _stack(dev, H=64, L=4, C=4, rate=0.0, Din=16, seed=11):
    from tf2_gnn_amd.layers import GNN, GNNInput
    from tf2_gnn_amd.layers.message_passing import set_seed

    params = GNN.get_default_hyperparameters("rgcn_blockdiag")
    params.update({"hidden_dim": H, "num_layers": 2, "num_blocks": C, "global_exchange_every_num_layers": 10000,
                   "layer_input_dropout_rate": rate, "dense_every_num_layers": 1, "residual_every_num_layers": 1,
                   "message_activation_function": "tanh", "dense_intermediate_layer_activation": "tanh"})
    set_seed(seed)
    gnn = GNN(params)
    adjs = _graph(L, seed=5)
    X = torch.randn((V_L, Din), generator=torch.Generator().manual_seed(2))
    inp = GNNInput(X.to(dev), to_dev(adjs, dev), torch.zeros(V_L, dtype=torch.int32, device=dev), 1)
    return gnn, params, inp, X, adjs


@pytest.mark.gemm_modes("f16x2", "bf16x3")
def test_gnn_stack_forward_and_backward(dev):
    """2 layers, residual and dense after every layer, against gnn_internal_call("rgcn") on composed dense kernels; the block
    gradients through the composition under fp64 autograd"""
    from tests.helpers import scaled_error

    gnn, params, inp, X, adjs = _stack(dev)
    H, C = params["hidden_dim"], params["num_blocks"]
    out = gnn(inp, training=False)
    assert all(type(m).__name__ == "RGCN_BlockDiag" for m in gnn._mp_layers)
    assert gnn.graph_parts(V_L, [a.shape[0] for a in adjs]) == 1 | 2 | 16  # PLAN_TYPED | PLAN_NODE | EDGE_IDS
    dOut = torch.randn((V_L, H), generator=torch.Generator().manual_seed(9))
    gnn.backward(dOut.to(dev))

    def reference(dtype):
        leaves = {"proj": gnn._initial_projection_layer.value.cpu().to(dtype).requires_grad_(True), "qb": [], "dense": {}}
        w = {"initial_projection": leaves["proj"], "mp": [], "dense": {}, "layernorm": []}
        for i, m in enumerate(gnn._mp_layers):
            qb = m._qb.detach().cpu().to(dtype).requires_grad_(True)
            leaves["qb"].append(qb)
            ho = H // C
            mask = torch.block_diag(*[torch.ones((qb.shape[1], ho), dtype=dtype)] * C)
            dense = qb.repeat(1, C, 1) * mask  # W_l[c*di + i, h] = Qb[l, i, h] on the blocks, 0 elsewhere
            w["mp"].append({"edge_mlps": [[k] for k in dense], "aggr_mlp": None})
            w["dense"][i] = leaves["dense"][i] = gnn._dense_layers[str(i)].value.cpu().to(dtype).requires_grad_(True)
        po = dict(params, message_calculation_class="rgcn", use_target_state_as_input=False, num_edge_MLP_hidden_layers=0)
        res, _ = orc.gnn_internal_call(po, w, X.to(dtype), [torch.from_numpy(a) for a in adjs])
        flat = [leaves["proj"]] + leaves["qb"] + [leaves["dense"][i] for i in sorted(leaves["dense"])]
        return res.detach(), torch.autograd.grad((res * dOut.to(dtype)).sum(), flat)

    (r64, g64), (r32, g32) = reference(torch.float64), reference(torch.float32)
    # the Dense layers and the projection run on the products of the GEMM mode: held to what the basis stack is held to
    assert_close(out.cpu().double(), r64, tol=max(1e-5, 2 * scaled_error(r32.double(), r64)), what="rgcn_blockdiag stack fwd")
    n = len(gnn._mp_layers)
    got = ([gnn._initial_projection_layer.grad] + [m._block_kernels.grad for m in gnn._mp_layers]
           + [gnn._dense_layers[str(i)].grad for i in range(n)])
    names = ["d projection"] + [f"d blocks {i}" for i in range(n)] + [f"d dense {i}" for i in range(n)]
    for what, a, b64, b32 in zip(names, got, g64, g32):
        scale = max(1.0, float(b64.abs().max()))
        assert_close(a.cpu().double().reshape(b64.shape) / scale, b64 / scale,
                     tol=max(1e-5, 2 * scaled_error(b32.double() / scale, b64 / scale)), what=f"rgcn_blockdiag stack {what}")


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
    layer, _ = _build(4, 8, 64, 64, message_activation_function="tanh")
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

    gnn, _, inp, _, _ = _stack(dev, L=37, C=8)
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
    params = LinkPredictionTask.get_default_hyperparameters("rgcn_blockdiag")
    assert params["gnn_message_calculation_class"] == "rgcn_blockdiag" and params["gnn_num_blocks"] == 4
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
    assert all(type(m).__name__ == "RGCN_BlockDiag" for m in model._gnn._mp_layers)
    losses = [float(model._run_step(feats, labels, training=True)["loss"]) for _ in range(30)]
    print(f"LinkPredictionTask(rgcn_blockdiag) 30 Adam steps: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert all(math.isfinite(l) for l in losses) and losses[-1] < 0.1 * losses[0]
    metrics = model.evaluate_model(ds.get_batches(DataFold.TEST, dev))
    assert list(metrics) == ["mrr", "hits@1", "hits@3", "hits@10"]
    assert all(0.0 <= v <= 1.0 for v in metrics.values()) and metrics["hits@1"] <= metrics["hits@3"] <= metrics["hits@10"]

    names = [v.name for v in model.variables]
    assert len(set(names)) == len(names)
    for i in range(2):
        assert sum(1 for n in names if f"Layer_{i}" in n and n.endswith("block_kernels")) == 1, names
    logits = model(feats, training=False)[0].clone()
    want = {v.name: v.value.clone() for v in model.variables}
    path = str(tmp_path / "model_best.pkl")
    mu.save_model(path, model)
    for v in model.variables:
        v.assign(torch.zeros_like(v.value))
    restored = mu.load_weights_verbosely(path, model)
    assert set(restored) == set(names)
    for v in model.variables:
        assert torch.equal(v.value, want[v.name]), v.name
    again = model(feats, training=False)[0]
    assert logits.numel() > 0 and logits.any() and torch.equal(logits.view(torch.int32), again.view(torch.int32))  # bit for bit
