"""The optimizer step on the device (tfgnn_optimizer_apply, tf2_gnn_amd/optim.py; graph_task_model.py:224-365): (a) the update
arithmetic of every kind and clip mode against the fp64 restatement in tests/optim_model64.py, on strided views, biases, odd
widths and more tensors than one launch takes; (b) the model-level step in every GEMM mode; (c) the step captured with its
update and replayed equals the eager steps bit for bit."""
import math

import numpy as np
import pytest
import torch

from tests.optim_model64 import Optimizer64, schedule64

pytestmark = pytest.mark.gpu

SCHED = dict(learning_rate=0.01, warmup_steps=2, decay_steps=3, initial_learning_rate=0.002, final_learning_rate=0.004)


class _Set:
    """the tensor set of part (a): values, gradient sources per step"""

    def __init__(self, dev, seed=0):
        from tf2_gnn_amd.layers.message_passing.message_passing import Variable

        gen = torch.Generator().manual_seed(seed)

        def rnd(*shape, s=1.0):
            return (torch.randn(shape, generator=gen) * s).to(dev)

        self.fused = rnd(64, 4 * 24 + 8, s=0.1)          # a fused buffer: four column-slice variables + one odd one
        self.gfused = torch.zeros(64, 4 * 24 + 20, device=dev)  # their gradients: views of another buffer (other row stride)
        vs = [Variable("big", rnd(4096, 1280, s=0.05))]
        vs += [Variable(f"slice{i}", self.fused[:, i * 24:(i + 1) * 24]) for i in range(4)]
        vs += [Variable("slice_odd", self.fused[:, 97:104])]
        vs += [Variable("bias", rnd(121, s=0.1)), Variable("odd", rnd(37, 33, s=0.1)), Variable("no_grad", rnd(16, 8))]
        vs += [Variable(f"small{i}", rnd(3 + i, 8 + 4 * (i % 3), s=0.1)) for i in range(30)]
        self.vars = vs
        self.gen = torch.Generator().manual_seed(seed + 100)

    def grads(self, step):
        """fresh fp32 gradients; the slices' gradients are strided views of gfused"""
        out = []
        g = torch.Generator().manual_seed(1000 + step)
        self.gfused.copy_(torch.randn(self.gfused.shape, generator=g))
        for v in self.vars:
            if v.name == "no_grad":
                out.append(None)
            elif v.name.startswith("slice"):
                i = v.name[5:]
                out.append(self.gfused[:, 99:106] if i == "_odd" else self.gfused[:, int(i) * 26:int(i) * 26 + 24])
            else:
                scale = 1e-3 if v.name == "big" else 1.0
                out.append((torch.randn(v.shape, generator=g) * scale).to(self.gfused.device))
        return out


def _run(dev, kind, clip, steps=5):
    from tf2_gnn_amd.optim import Optimizer, PolynomialWarmupAndDecaySchedule

    ts = _Set(dev)
    mu = 0.85 if kind in ("sgd_mom", "rmsprop_mom") else 0.0
    opt = Optimizer(kind.split("_")[0], learning_rate=PolynomialWarmupAndDecaySchedule(**SCHED), momentum=mu, rho=0.98)
    hist = []
    for s in range(steps):
        gs = ts.grads(s)
        opt.apply_gradients(list(zip(ts.vars, gs)), clip=clip)
        hist.append([g.double().cpu().numpy() if g is not None else None for g in gs])
    torch.cuda.synchronize()
    return ts, opt, hist


CLIPS = [None, ("value", 0.5), ("norm", 1.0), ("global_norm", 10.0)]


@pytest.mark.parametrize("clip", CLIPS, ids=lambda c: "none" if c is None else c[0])
@pytest.mark.parametrize("kind", ["sgd", "sgd_mom", "rmsprop", "rmsprop_mom", "adam"])
def test_update_matches_fp64(dev, kind, clip):
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    ts0 = _Set(dev)
    w0 = [v.value.double().cpu().numpy().copy() for v in ts0.vars]
    del ts0
    c0 = lib.tfgnn_optimizer_launch_count()
    ts, opt, hist = _run(dev, kind, clip)
    launches = lib.tfgnn_optimizer_launch_count() - c0
    live = sum(1 for g in hist[0] if g is not None)
    chunks = math.ceil(live / 32)
    assert chunks == 2
    assert launches == 5 * chunks * (2 if clip is not None and "norm" in clip[0] else 1)
    assert opt.iterations == 5

    mu = 0.85 if kind in ("sgd_mom", "rmsprop_mom") else 0.0
    idx = [i for i, g in enumerate(hist[0]) if g is not None]
    ref = Optimizer64(kind.split("_")[0], lambda t: schedule64(t, **SCHED), momentum=mu, rho=0.98, clip=clip)
    w64 = [w0[i].copy() for i in idx]
    biggest = [0.0] * len(idx)
    for s in range(5):
        before = [w.copy() for w in w64]
        ref.step(w64, [hist[s][i] for i in idx])
        biggest = [max(b, float(np.abs(w - p).max())) for b, w, p in zip(biggest, w64, before)]
    for j, i in enumerate(idx):
        got = ts.vars[i].value.double().cpu().numpy()
        err = float(np.abs(got - w64[j]).max())
        tol = 1e-5 * biggest[j] + 2.0 ** -22 * float(np.abs(w64[j]).max())
        assert err <= tol, (ts.vars[i].name, err, tol)
    # the variable without a gradient is untouched and has no slots; the fused buffer's columns between the views too
    nog = [v for v in ts.vars if v.name == "no_grad"][0]
    assert np.array_equal(nog.value.double().cpu().numpy(), w0[ts.vars.index(nog)]) and opt.slots(nog) == []
    assert torch.equal(ts.fused[:, 96:97], _Set(dev).fused[:, 96:97])

    # bit-reproducible: the same run again
    ts2, opt2, _ = _run(dev, kind, clip)
    for a, b in zip(ts.vars, ts2.vars):
        assert torch.equal(a.value, b.value), a.name
        for sa, sb in zip(opt.slots(a), opt2.slots(b)):
            assert torch.equal(sa, sb), a.name


def test_global_norm_with_an_inf_gradient_gives_nan(dev):
    from tf2_gnn_amd.layers.message_passing.message_passing import Variable
    from tf2_gnn_amd.optim import Optimizer

    vs = [Variable("a", torch.ones(100, 16, device=dev)), Variable("b", torch.ones(7, device=dev))]
    gs = [torch.ones(100, 16, device=dev), torch.ones(7, device=dev)]
    gs[0][3, 5] = float("inf")
    opt = Optimizer("adam")
    opt.apply_gradients(list(zip(vs, gs)), clip=("global_norm", 1.0))
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v.value).all()) for v in vs)
    # per-tensor norm: only the tensor with the inf is poisoned (its finite entries become 0 * c / inf = 0, the inf NaN)
    vs = [Variable("a", torch.ones(100, 16, device=dev)), Variable("b", torch.ones(7, device=dev))]
    opt = Optimizer("sgd", learning_rate=0.5)
    opt.apply_gradients(list(zip(vs, gs)), clip=("norm", 1.0))
    torch.cuda.synchronize()
    assert bool(torch.isnan(vs[0].value[3, 5])) and int(torch.isnan(vs[0].value).sum()) == 1
    assert torch.allclose(vs[1].value, torch.full((7,), 1.0 - 0.5 / math.sqrt(7.0), device=dev))


def _ppi_model(dev, seed=1, **params):
    from tf2_gnn_amd.data import make_ppi_shaped_batch, process_adjacency_lists
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import NodeMulticlassTask

    feats, fwd, n2g, labels = make_ppi_shaped_batch(2, 300, 6, 50, 121, seed=3)
    V = feats.shape[0]
    X = torch.from_numpy(feats).to(dev)
    adjs, _ = process_adjacency_lists([torch.from_numpy(fwd).to(dev)], V, add_self_loop_edges=True, tied_fwd_bkwd_edge_types=set())
    p = NodeMulticlassTask.get_default_hyperparameters("rgcn")
    p.update({"gnn_hidden_dim": 128, "gnn_num_layers": 2, "gnn_layer_input_dropout_rate": 0.0})
    p.update(params)
    set_seed(seed)
    model = NodeMulticlassTask(p, num_edge_types=3, num_node_target_labels=121)
    batch = {"node_features": X, "node_to_graph_map": torch.from_numpy(n2g).to(dev), "num_graphs_in_batch": 2,
             **{f"adjacency_list_{i}": a for i, a in enumerate(adjs)}}
    model.build({"node_features": tuple(X.shape)})  # the weights are drawn now, from this seed
    return model, batch, {"node_labels": torch.from_numpy(labels).to(dev)}


@pytest.mark.gemm_modes()
def test_run_step_updates_the_model(dev, gemm_mode):
    model, batch, lab = _ppi_model(dev)
    m = model._run_step(batch, lab, training=False)  # builds the model; no update
    torch.cuda.synchronize()
    w0 = [v.value.clone() for v in model.trainable_variables]
    assert model._optimizer is None and model._train_step_counter == 0
    out0 = model(batch, training=False)[0].clone()

    model._run_step(batch, lab, training=True)
    torch.cuda.synchronize()
    assert model._optimizer.iterations == 1 and model._train_step_counter == 1
    changed = [not torch.equal(v.value, w) for v, w in zip(model.trainable_variables, w0)]
    assert all(changed), [v.name for v, c in zip(model.trainable_variables, changed) if not c]

    w1 = [v.value.clone() for v in model.trainable_variables]
    m = model._run_step(batch, lab, training=False)
    torch.cuda.synchronize()
    assert model._optimizer.iterations == 1 and model._train_step_counter == 1 and math.isfinite(float(m["loss"]))
    assert all(torch.equal(v.value, w) for v, w in zip(model.trainable_variables, w1))

    # the forward after the update is that of a fresh model holding the updated weights: no stale derived weight form is used
    out1 = model(batch, training=False)[0].clone()
    fresh, _, _ = _ppi_model(dev, seed=7)
    for v, w in zip(fresh.trainable_variables, w1):
        v.assign(w)
    out_f = fresh(batch, training=False)[0]
    torch.cuda.synchronize()
    moved = float((out1 - out0).abs().max())
    assert moved > 0 and float((out1 - out_f).abs().max()) <= 1e-4 * moved


@pytest.mark.gemm_modes()
def test_qm9_rgcn_settings_decrease_the_loss(dev, gemm_mode):
    """QM9_RGCN.json's update (RMSProp, momentum 0.85, rho 0.98, gradient_clip_value 1.0) on a fixed batch"""
    model, batch, lab = _ppi_model(dev, optimizer="RMSProp", momentum=0.85, rmsprop_rho=0.98, learning_rate=0.0005720408870458782,
                                   gradient_clip_value=1.0)
    losses = [float(model._run_step(batch, lab, training=True)["loss"]) for _ in range(20)]
    assert model._optimizer.kind == "rmsprop" and model._optimizer.iterations == 20
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0], losses


def test_captured_step_with_update_equals_the_eager_steps(dev):
    from tf2_gnn_amd import CapturedStep

    params = dict(optimizer="Adam", learning_rate=0.002, learning_rate_warmup_steps=6, learning_rate_decay_steps=20,
                  gradient_clip_global_norm=1.0)
    eager, batch, lab = _ppi_model(dev, seed=4, **params)
    twin, _, _ = _ppi_model(dev, seed=4, **params)

    def step():
        out = twin(batch, training=True)
        metrics = twin.compute_task_metrics(batch, out, lab)
        twin._apply_gradients(twin.backward())
        return metrics["loss"]

    cap = CapturedStep(step)  # 4 eager warm-up steps, each with its update
    cap.capture()
    replays = 5
    for _ in range(replays):
        loss_c = cap.replay()
    torch.cuda.synchronize()
    loss_c = float(loss_c)

    for _ in range(4 + replays):
        loss_e = eager._run_step(batch, lab, training=True)["loss"]
    torch.cuda.synchronize()
    assert float(loss_e) == loss_c
    assert eager._optimizer.iterations == twin._optimizer.iterations == 4 + replays
    for a, b in zip(eager.trainable_variables, twin.trainable_variables):
        assert torch.equal(a.value, b.value), a.name
        sa, sb = eager._optimizer.slots(a), twin._optimizer.slots(b)
        assert len(sa) == 2 and all(torch.equal(x, y) for x, y in zip(sa, sb)), a.name
