"""Host side of the optimizer step (tf2_gnn_amd/optim.py, GraphTaskModel._make_optimizer / _apply_gradients): the learning-rate
schedule's host mirror against an fp64 restatement, the optimizer names and errors of _make_optimizer, the clip-conflict
errors of _apply_gradients, and the argument checks of the C entries (rejected before any HIP call: no device needed)."""
import ctypes

import numpy as np
import pytest

from tests.optim_model64 import schedule64


def _params(**kw):
    from tf2_gnn_amd.tasks import NodeMulticlassTask

    p = NodeMulticlassTask.get_default_hyperparameters("rgcn")
    p.update(kw)
    return p


@pytest.mark.parametrize("warmup,decay", [(50, None), (None, 80), (30, 60), (None, None)])
def test_schedule_mirror_against_fp64(warmup, decay):
    from tf2_gnn_amd.optim import PolynomialWarmupAndDecaySchedule, make_optimizer

    lr = 0.003
    opt = make_optimizer(_params(optimizer="Adam", learning_rate=lr, learning_rate_warmup_steps=warmup,
                                 learning_rate_decay_steps=decay))
    if warmup is None and decay is None:
        assert opt.learning_rate == lr  # no schedule without a warm-up or decay key
        return
    sched = opt.learning_rate
    assert isinstance(sched, PolynomialWarmupAndDecaySchedule)
    # graph_task_model.py:240-256: the missing phase gets -1 warm-up steps / 1 decay step and the peak rate as its end point
    w = -1 if warmup is None else warmup
    d = 1 if decay is None else decay
    lr0 = lr if warmup is None else 1e-5
    lr1 = lr if decay is None else 1e-5
    assert sched.get_config() == {"learning_rate": lr, "initial_learning_rate": lr0, "final_learning_rate": lr1,
                                  "warmup_steps": w, "decay_steps": d, "power": 1.0, "name": None}
    for step in range(201):
        want = schedule64(step, lr, w, d, lr0, lr1)
        assert abs(sched(step) - want) <= 1e-6 * want, (step, sched(step), want)
    if warmup is None:
        # the -1 quirk: step 0 is already one step into the decay, min(step - warmup, decay) then holds the final rate
        assert sched(0) < lr and abs(sched(0) - schedule64(1, lr, 0, d, lr, lr1)) <= 1e-6 * lr
        assert sched(d - 1) == pytest.approx(1e-5, rel=1e-6) and sched(200) == pytest.approx(1e-5, rel=1e-6)
    else:
        assert sched(0) == pytest.approx(1e-5, rel=1e-6) and sched(w) == pytest.approx(lr, rel=1e-6)


def test_make_optimizer_names_and_errors():
    from tf2_gnn_amd.optim import Optimizer, make_optimizer

    for name, kind in (("Adam", "adam"), ("ADAM", "adam"), ("RMSProp", "rmsprop"), ("rmsprop", "rmsprop"), ("SGD", "sgd"), ("sgd", "sgd")):
        opt = make_optimizer(_params(optimizer=name, momentum=0.5, rmsprop_rho=0.95))
        assert isinstance(opt, Optimizer) and opt.kind == kind
        if kind == "sgd":
            assert opt.momentum == 0.5
        if kind == "rmsprop":
            assert opt.momentum == 0.5 and opt.rho == 0.95
        if kind == "adam":  # Keras defaults; the momentum key does not reach Adam
            assert (opt.beta_1, opt.beta_2, opt.epsilon, opt.momentum) == (0.9, 0.999, 1e-7, 0.0)
    with pytest.raises(Exception, match='Unknown optimizer "Adagrad".'):
        make_optimizer(_params(optimizer="Adagrad"))
    # an explicit learning rate wins over the schedule keys
    opt = make_optimizer(_params(optimizer="sgd", learning_rate_warmup_steps=10), learning_rate=0.25)
    assert opt.learning_rate == 0.25
    with pytest.raises(ValueError, match="momentum"):
        make_optimizer(_params(optimizer="sgd", momentum=1.5))


@pytest.mark.parametrize("keys,msg", [
    ({"gradient_clip_value": 1.0, "gradient_clip_norm": 1.0}, "'gradient_clip_value' and 'gradient_clip_norm'"),
    ({"gradient_clip_value": 1.0, "gradient_clip_global_norm": 1.0}, "'gradient_clip_value' and 'gradient_clip_global_norm'"),
    ({"gradient_clip_norm": 1.0, "gradient_clip_global_norm": 1.0}, "'gradient_clip_norm' and 'gradient_clip_global_norm'"),
])
def test_clip_conflicts_raise_on_the_host(keys, msg):
    from tf2_gnn_amd.tasks import NodeMulticlassTask

    model = NodeMulticlassTask(_params(**keys), num_edge_types=3, num_node_target_labels=4)
    with pytest.raises(ValueError, match=msg):
        model._apply_gradients([])
    assert model._optimizer is not None and model._optimizer._state is None  # nothing reached the device


def _cfg(**kw):
    from tf2_gnn_amd import _lib

    c = _lib.OptConfig()
    c.struct_size = ctypes.sizeof(_lib.OptConfig)
    c.kind, c.clip, c.clip_value, c.momentum, c.rho, c.beta_1, c.beta_2, c.epsilon = 2, 0, 0.0, 0.0, 0.9, 0.9, 0.999, 1e-7
    c.learning_rate = 1e-3
    c.state = 0x10000
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _tensors(rows, fake=0x100000):
    """descriptor rows (value, ld_value, grad, ld_grad, rows, cols, slot0, slot1) with fake, aligned, never dereferenced pointers"""
    return np.array(rows, dtype=np.int64).reshape(-1, 8)


def test_optimizer_entries_reject_bad_arguments_without_a_device():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    before = lib.tfgnn_optimizer_launch_count()
    P = 0x100000
    good = _tensors([(P, 8, P, 8, 4, 8, P, P)])

    def apply(t, n, cfg):
        return lib.tfgnn_optimizer_apply(t.ctypes.data if t is not None else None, n, ctypes.byref(cfg) if cfg is not None else None, None)

    assert apply(good, 1, None) == -1
    assert apply(good, 1, _cfg(struct_size=8)) == -1 and b"size" in lib.tfgnn_last_error()
    assert apply(good, 1, _cfg(kind=7)) == -1 and b"kind" in lib.tfgnn_last_error()
    assert apply(good, 1, _cfg(clip=9)) == -1 and b"clip" in lib.tfgnn_last_error()
    assert apply(good, 1, _cfg(clip=1, clip_value=0.0)) == -1
    assert apply(good, 1, _cfg(clip=2, clip_value=float("inf"))) == -1
    assert apply(good, 1, _cfg(kind=0, momentum=1.5)) == -1 and b"momentum" in lib.tfgnn_last_error()
    assert apply(good, 1, _cfg(schedule=3)) == -1
    assert apply(good, 1, _cfg(state=None)) == -1 and b"state" in lib.tfgnn_last_error()
    assert apply(good, 1, _cfg(state=0x10004)) == -1
    assert apply(None, 1, _cfg()) == -1
    assert apply(good, -1, _cfg()) == -1
    assert apply(_tensors([(P, 8, P, 8, -1, 8, P, P)]), 1, _cfg()) == -1 and b"negative" in lib.tfgnn_last_error()
    assert apply(_tensors([(0, 8, P, 8, 4, 8, P, P)]), 1, _cfg()) == -1
    assert apply(_tensors([(P, 8, P, 8, 4, 8, P, 0)]), 1, _cfg()) == -1 and b"slot" in lib.tfgnn_last_error()  # Adam needs v
    assert apply(_tensors([(P, 8, P, 8, 4, 8, P, 0)]), 1, _cfg(kind=1, momentum=0.5)) == -1  # RMSprop + momentum needs mom
    assert apply(_tensors([(P, 4, P, 8, 4, 8, P, P)]), 1, _cfg()) == -1 and b"stride" in lib.tfgnn_last_error()
    assert apply(_tensors([(P, 8, P, 8, 1 << 16, 1 << 16, P, P)]), 1, _cfg()) == -1  # more than 2^31 - 1 elements
    assert apply(_tensors([(P, 8, P, 8, 0, 8, P, P)]), 1, _cfg()) == -1 and b"no elements" in lib.tfgnn_last_error()
    assert apply(good, 1, _cfg(clip=3, clip_value=1.0)) == -1 and b"workspace" in lib.tfgnn_last_error()
    assert apply(good, 1, _cfg(clip=2, clip_value=1.0, workspace=0x20000, workspace_bytes=4)) == -1
    assert lib.tfgnn_optimizer_iterations_get(None, None, None) == -1
    assert lib.tfgnn_optimizer_iterations_set(None, 0, None) == -1
    assert lib.tfgnn_optimizer_iterations_set(ctypes.c_void_p(0x10000), -1, None) == -1
    assert lib.tfgnn_optimizer_launch_count() == before  # nothing was launched

    # workspace: one fp64 partial per 8192 elements of each tensor, only for the norm modes
    two = _tensors([(P, 0, P, 0, 1, 16385, P, P), (P, 64, P, 96, 100, 64, P, P)])
    assert lib.tfgnn_optimizer_workspace_bytes(two.ctypes.data, 2, 0) == 0
    assert lib.tfgnn_optimizer_workspace_bytes(two.ctypes.data, 2, 1) == 0
    assert lib.tfgnn_optimizer_workspace_bytes(two.ctypes.data, 2, 2) == 4 * 8
    assert lib.tfgnn_optimizer_workspace_bytes(two.ctypes.data, 2, 3) == 4 * 8


def test_training_loop_surface_exists():
    """the names the package exports for the update and the training loop"""
    import tf2_gnn_amd
    from tf2_gnn_amd.tasks import GraphTaskModel

    for name in ("Optimizer", "PolynomialWarmupAndDecaySchedule", "make_optimizer"):
        assert hasattr(tf2_gnn_amd, name)
    for name in ("_make_optimizer", "_apply_gradients", "_run_step", "run_one_epoch"):
        assert callable(getattr(GraphTaskModel, name))
