"""What the spread-guard policy of the f16x2 mode does to a layer stack, pass by pass, over a grid of scripted scenarios: the
record that pins every transition of the policy across a change of where its state is kept.

    python tools/record_guard_policy.py > tests/golden/guard_policy_parent.json

Only host code runs.  The three library entry points the policy talks to are a fake that behaves as the library does
(``tfgnn_gemm_set_mode``: f16x2 clears the flag; ``tfgnn_gemm_get_mode``: a raised flag takes the f16x2 mode off, sticky;
``tfgnn_sp_spread_flag``), the stream wait and the capturing query are stubs (``torch.cuda.current_stream``,
``torch.cuda.is_current_stream_capturing``), ``GNN._backward_walk`` is a stub that asks for the mode as the real walk does and
raises the fake's flag as the scenario says, and the stack is an unbuilt ``GNN`` over stub layers that carry the two flags of the
policy (``_grouped_tn_split_ok``, ``_grouped_tn_used``).  The forward pass is the real ``_internal_call`` over those stubs.  Only
names that exist before and after such a change are used: the public guard functions of ``ops``, ``GNN.backward``,
``guard_state()``, ``_dense_f16x2``, ``guard_check_every`` and the layer flags; to let the forward pass run without a device
the stack's weights and layers are set by hand and ``GNN._dense``, ``get_graph`` and ``ops.presplit_weight_operands`` are stubbed.
No attribute of the policy itself is touched.  tests/test_guard_policy_host.py replays
``record()`` and demands equality with the committed record.

Scenarios (``grid()``): the flag goes up in every walk that runs while the stack's stage is below k, k in none (no trip) / 1a /
1b / 2 / 3 / never (trips at every stage) x Dense products possible (hidden 128), impossible (hidden 24) or switched off
(TFGNN_DENSE_F16X2=0) x layers that use the grouped TN product or not x TFGNN_GUARD_SYNC_PASSES 0 / 1 / 3 x
``guard_check_every`` 0 / 2 x no re-arm, ``set_gemm_mode("f16x2")`` after pass 3 followed by a forward pass, by a
``_dense_f16x2`` query and a backward pass without a forward, or by such a backward pass alone x the walk itself asks for the mode twice after raising the flag
(a late trip seen inside the pass) or nobody does before the pass returns; six forward + backward passes each.  ``specials()``:
two stacks at once, a stack destroyed between trip and query, capturing, and mode bf16x3 throughout.

After every call the record holds: the walks that ran (stage and mode at their start), ``guard_state()``, ``get_gemm_mode()``,
the fake's flag, every layer's ``_grouped_tn_split_ok``, the first 60 characters of each warning and the type of an exception.
The warning about the demoted mode is issued once per process: ``record()`` wants a fresh process, or a caller that has reset
that flag.

Format: ``steps`` lists the distinct per-call records; ``scenarios[name]`` is the list of indices into it, call by call."""
from __future__ import annotations

import gc
import itertools
import json
import os
import sys
import warnings
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

STAGES = ("none", "1a", "1b", "2", "3", "never")
F16X2, BF16X3 = 3, 6
ENV_NAMES = ("TFGNN_GUARD_SYNC_PASSES", "TFGNN_GUARD_CHECK_EVERY", "TFGNN_DENSE_F16X2")


class FakeLib:
    """The mode and the spread flag as the library keeps them (gemm.hip tfgnn_gemm_set_mode / _get_mode, gemm_sp.hip
    tfgnn_sp_spread_flag)."""

    def __init__(self):
        self.f16x2, self.x3, self.flag = 1, BF16X3, 0

    def tfgnn_gemm_set_mode(self, mode):
        if mode == F16X2:
            self.flag, self.x3, self.f16x2 = 0, BF16X3, 1
        else:
            self.x3, self.f16x2 = mode, 0
        return 0

    def tfgnn_gemm_get_mode(self):
        if self.f16x2:
            if not self.flag:
                return F16X2
            self.f16x2 = 0
        return self.x3

    def tfgnn_sp_spread_flag(self, reset):
        v = self.flag
        if reset:
            self.flag = 0
        return v


class StubLayer:
    """What the stack reads of a message-passing layer, and the two flags of the guard policy."""

    built = True
    trainable_variables = ()

    def __init__(self, uses_grouped_tn: bool):
        self._grouped_tn_split_ok = True
        self._grouped_tn_used = False
        self.uses_grouped_tn = uses_grouped_tn

    def graph_parts(self, num_nodes, edges_per_type, hidden):
        return 0

    def weight_operand_requests(self, graph, V, H, backward):
        return []

    def call_with_epilogue(self, inputs, training=False, want_split_output=False, output_dropout=None):
        return inputs.node_embeddings, False


class World:
    """The fakes and stubs, installed for the lifetime of one ``record()``."""

    def __init__(self):
        import torch

        from tf2_gnn_amd import _lib, ops
        from tf2_gnn_amd.layers import gnn as gnn_module

        self.torch, self.ops, self.gnn_module, self._lib = torch, ops, gnn_module, _lib
        self.lib = FakeLib()
        self.capturing = False
        self.walks = []
        self.plans = {}  # id(stack) -> (trip while the stage is below, ask for the mode inside the pass?)
        GNN = gnn_module.GNN
        self._saved = [(_lib, "load", _lib.load), (torch.cuda, "current_stream", torch.cuda.current_stream),
                       (torch.cuda, "is_current_stream_capturing", torch.cuda.is_current_stream_capturing),
                       (gnn_module, "get_graph", gnn_module.get_graph), (ops, "presplit_weight_operands", ops.presplit_weight_operands),
                       (GNN, "_backward_walk", GNN._backward_walk), (GNN, "_dense", GNN._dense)]
        self._env = {k: os.environ.get(k) for k in ENV_NAMES}
        world = self
        _lib.load = lambda: world.lib
        torch.cuda.current_stream = lambda *a, **k: SimpleNamespace(synchronize=lambda: None, cuda_stream=0)
        torch.cuda.is_current_stream_capturing = lambda: world.capturing
        gnn_module.get_graph = lambda adj, V, parts=0: SimpleNamespace(num_edge_types=1)
        ops.presplit_weight_operands = lambda reqs: None
        GNN._dense = lambda self, x, w, act_name, drop=None: (x, None, False)
        GNN._backward_walk = lambda self, ctx, g, g_is_pre, g_last, extras, need_input_grad: world.walk(self)

    def close(self):
        for owner, name, value in self._saved:
            setattr(owner, name, value)
        for k, v in self._env.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v

    def walk(self, gnn):
        """Stands in for a backward walk: asks for the mode first (as ``_presplit_weights`` does), then its products report."""
        ops = self.ops
        mode = ops.get_gemm_mode()
        stage = gnn.guard_state()["stage"]
        self.walks.append([stage, mode])
        below, ask = self.plans[id(gnn)]
        if mode == F16X2:
            for layer in gnn._mp_layers:
                if layer.uses_grouped_tn and layer._grouped_tn_split_ok:
                    layer._grouped_tn_used = True
            if STAGES.index(stage) < STAGES.index(below):
                self.lib.flag = 1
        if ask:
            ops.get_gemm_mode()
            ops.get_gemm_mode()
        return None

    def stack(self, hidden: int, grouped: bool, sync_passes: int, check_every: int, below: str, ask: bool):
        torch = self.torch
        os.environ["TFGNN_GUARD_SYNC_PASSES"] = str(sync_passes)
        GNN = self.gnn_module.GNN
        params = GNN.get_default_hyperparameters("rgcn")
        params.update({"hidden_dim": hidden, "num_layers": 2, "dense_every_num_layers": 2, "residual_every_num_layers": 10000,
                       "global_exchange_every_num_layers": 10000, "layer_input_dropout_rate": 0.0})
        gnn = GNN(params)
        gnn.guard_check_every = check_every
        weight = SimpleNamespace(value=torch.empty((hidden, hidden)), grad=None)
        gnn._initial_projection_layer = weight
        gnn._dense_layers = {"0": weight}
        gnn._mp_layers = [StubLayer(grouped), StubLayer(grouped)]
        gnn.built = True
        self.plans[id(gnn)] = (below, ask)
        return gnn

    def inputs(self, hidden: int):
        from tf2_gnn_amd.layers import GNNInput

        return GNNInput(self.torch.zeros((4, hidden)), (), None, 1)


class Scenario:
    """Runs calls and keeps what the issue of each is."""

    def __init__(self, world: World, stacks):
        self.world, self.stacks, self.steps = world, list(stacks), []

    def call(self, name: str, fn):
        world, ops = self.world, self.world.ops
        world.walks = []
        exc = None
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                fn()
            except Exception as e:  # noqa: BLE001 - the type is the record
                exc = type(e).__name__
            states = [g.guard_state() for g in self.stacks]
            mode = ops.get_gemm_mode()
        walks, world.walks = world.walks, []
        self.steps.append({"call": name, "walks": walks, "state": states, "mode": mode, "flag": world.lib.flag,
                           "tn_ok": [[bool(layer._grouped_tn_split_ok) for layer in g._mp_layers] for g in self.stacks],
                           "warnings": [str(w.message)[:60] for w in caught], "exc": exc})

    def passes(self, gnn, inp, g, n: int, tag: str = ""):
        for _ in range(n):
            self.call(tag + "forward", lambda: gnn(inp, training=True))
            self.call(tag + "backward", lambda: gnn.backward(g))


def grid():
    """-> [(name, below, dense, grouped, sync passes, check every, re-arm, ask inside the pass)]"""
    out = []
    for below, dense, grouped, sync, every, rearm, ask in itertools.product(
            STAGES, ("h128", "h24", "off"), (False, True), (0, 1, 3), (0, 2), ("no", "forward", "no_forward", "no_query"), (False, True)):
        out.append((f"below={below} dense={dense} grouped={int(grouped)} sync={sync} every={every} rearm={rearm} ask={int(ask)}",
                    below, dense, grouped, sync, every, rearm, ask))
    return out


def run_grid_point(world: World, below, dense, grouped, sync, every, rearm, ask, mode="f16x2"):
    ops = world.ops
    hidden = 24 if dense == "h24" else 128
    os.environ["TFGNN_DENSE_F16X2"] = "0" if dense == "off" else "1"
    ops.set_gemm_mode(mode)
    gnn = world.stack(hidden, grouped, sync, every, below, ask)
    inp, g = world.inputs(hidden), world.torch.zeros((4, hidden))
    sc = Scenario(world, [gnn])
    sc.passes(gnn, inp, g, 3)
    if rearm != "no":
        sc.call("rearm", lambda: ops.set_gemm_mode("f16x2"))
        if rearm == "no_forward":
            sc.call("dense_query", lambda: gnn._dense_f16x2(hidden, hidden))
        if rearm != "forward":
            sc.call("backward", lambda: gnn.backward(g))
    sc.passes(gnn, inp, g, 3)
    return sc.steps


def specials(world: World):
    """-> {name: steps}: what the grid does not reach"""
    ops, torch = world.ops, world.torch
    out = {}
    os.environ["TFGNN_DENSE_F16X2"] = "1"
    inp, g = world.inputs(128), torch.zeros((4, 128))

    # two stacks: only the one with unchecked passes may move, one step per pass however many queries see the flag
    for both in (False, True):
        for ask in (False, True):
            ops.set_gemm_mode("f16x2")
            a = world.stack(128, True, 0, 0, "never", ask)
            b = world.stack(128, True, 0 if both else 3, 0, "none", False)
            sc = Scenario(world, [a, b])
            if both:
                sc.passes(b, inp, g, 1, "b.")
            for _ in range(4):
                sc.passes(a, inp, g, 1, "a.")
                sc.call("query", ops.get_gemm_mode)
                sc.call("query", ops.get_gemm_mode)
            sc.passes(b, inp, g, 2, "b.")
            out[f"two stacks both_unchecked={int(both)} ask={int(ask)}"] = sc.steps
            del sc, a, b
            gc.collect()

    # a stack destroyed between the trip and the query, with and without an idle stack alive
    for idle in (False, True):
        ops.set_gemm_mode("f16x2")
        a = world.stack(128, False, 0, 0, "never", False)
        others = [world.stack(128, False, 3, 0, "none", False)] if idle else []
        sc = Scenario(world, others)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            a(inp, training=True)
            a.backward(g)  # (unchecked: the flag is up and nobody has asked for the mode yet)
        del a
        gc.collect()
        sc.call("query", ops.get_gemm_mode)
        sc.call("rearm", lambda: ops.set_gemm_mode("f16x2"))
        sc.call("query", ops.get_gemm_mode)
        out[f"stack destroyed idle_stack={int(idle)}"] = sc.steps
        del sc, others
        gc.collect()

    # capturing: with checked passes left the pass raises; with none left no pass is ever checked, the periodic one included
    for sync, every, below in ((3, 0, "none"), (1, 2, "never"), (0, 2, "none"), (0, 2, "never"), (0, 0, "never")):
        ops.set_gemm_mode("f16x2")
        gnn = world.stack(128, True, sync, every, below, False)
        sc = Scenario(world, [gnn])
        sc.passes(gnn, inp, g, 1)  # (eagerly)
        world.capturing = True
        try:
            sc.passes(gnn, inp, g, 4, "captured.")
        finally:
            world.capturing = False
        sc.passes(gnn, inp, g, 2)
        out[f"capturing sync={sync} every={every} below={below}"] = sc.steps
        del sc, gnn
        gc.collect()

    # another mode throughout: the policy is inert
    for below, sync, every, rearm in itertools.product(("none", "never"), (0, 3), (0, 2), ("no", "forward")):
        # (with the re-arm: inert until the mode is switched on after pass 3)
        out[f"bf16x3 below={below} sync={sync} every={every} rearm={rearm}"] = run_grid_point(
            world, below, "h128", True, sync, every, rearm, True, mode="bf16x3")
    return out


def record():
    world = World()
    try:
        scenarios = {}
        for name, *point in grid():
            scenarios[name] = run_grid_point(world, *point)  # (the stack dies with its last reference: no cycles)
        scenarios.update(specials(world))
    finally:
        world.close()
    index, steps = {}, []
    packed = {}
    for name, sc in scenarios.items():
        row = []
        for step in sc:
            key = json.dumps(step, sort_keys=True)
            if key not in index:
                index[key] = len(steps)
                steps.append(step)
            row.append(index[key])
        packed[name] = row
    return {"steps": steps, "scenarios": packed}


if __name__ == "__main__":
    print(json.dumps(record(), sort_keys=True, separators=(",", ":")))
