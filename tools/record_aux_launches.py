"""The small-pass launches (tfgnn_aux_launch) of one training step per layer family, with a cleared weight-operand cache: the
record that pins WHICH weight splits a step launches, in which order, how they are grouped into launches and on which stream,
across a change of how the Python side hands them to the library.

    python tools/record_aux_launches.py > tests/golden/aux_launch_sequence_parent.json

Per case: ``launches`` = [[kinds of the launch's non-empty jobs, the launch's stream is the current one], ...] in issue order
(a spy on ``lib.tfgnn_aux_launch``: what the layer-level C entry points launch themselves never passes through it) and
``products`` = the step's launches per kernel family (``ops.launch_counts``).  Only API that does not depend on how the splits
are issued is used: the layer classes, ``ops.Graph``, ``ops.clear_weight_operand_cache``.  tests/test_gpu_split_jobs.py runs
the same cases through ``cases()`` / ``run_case()`` and compares with the committed record.

Shapes: V = 500, E = 5000, L = 3, D = H = 128 - every layer family takes its split-operand route there.  Two cases differ:
  * "edge_mlp_A_long_stack": D = 512, so the stacked kernels have L * D = 1536 > 1280 rows and their W^T split runs in two
    passes (column maxima, then the conversion): two consecutive launches inside the layer;
  * "edge_mlp_B_compact": the compact-row formulation is taken when fewer than 60 % of the (source, type) buckets hold an edge,
    so this case draws its sources from the first 200 nodes, and lowers the layer's row threshold for the split-operand
    grouped products (GROUPED_SPLIT_MIN_ROWS, 4096: more buckets than this graph has) as the layer tests do."""
from __future__ import annotations

import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

V, E, L, H = 500, 5000, 3, 128
SPLIT_FAMILIES = ("sp_nt", "sp_tn")  # the split-operand products: a case that ran neither did not take the route it pins


def cases():
    """-> [(name, kind, layer class | mp style, hyper-parameter overrides, input width, environment, sources drawn from [0, n))]"""
    src_only = {"use_target_state_as_input": False}
    linear = dict(src_only, num_edge_MLP_hidden_layers=0)
    stack = {"num_layers": 2, "dense_every_num_layers": 1, "residual_every_num_layers": 2, "global_exchange_every_num_layers": 10000}
    return [
        ("rgat", "layer", "RGAT", {"num_heads": 4}, H, {}, V),  # (the default, 3 heads, does not divide H)
        ("ggnn", "layer", "GGNN", {}, H, {}, V),
        ("edge_mlp_A_op_level", "layer", "GNN_Edge_MLP", linear, H, {"TFGNN_MP_ENTRY": "0"}, V),
        ("edge_mlp_A_one_call", "layer", "GNN_Edge_MLP", linear, H, {"TFGNN_MP_ENTRY": "1"}, V),
        ("edge_mlp_A_long_stack", "layer", "GNN_Edge_MLP", linear, 512, {"TFGNN_MP_ENTRY": "0"}, V),
        ("edge_mlp_B_compact", "layer", "GNN_Edge_MLP", src_only, H, {}, 200),
        ("edge_mlp_C_target_states", "layer", "GNN_Edge_MLP", {}, H, {}, V),
        ("gnn_stack_presplit", "stack", "rgcn", stack, H, {"TFGNN_PRESPLIT": "1"}, V),
        ("gnn_stack_no_presplit", "stack", "rgcn", stack, H, {"TFGNN_PRESPLIT": "0"}, V),
    ]


def adjacency_lists(num_sources: int):
    rng = np.random.default_rng(77 + num_sources)
    per = E // L
    return [np.stack([rng.integers(0, num_sources, size=per), rng.integers(0, V, size=per)], axis=1).astype(np.int32)
            for _ in range(L)]


class _Env:
    def __init__(self, values):
        self.values, self.old = values, {}

    def __enter__(self):
        for k, v in self.values.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def _build(case, dev):
    """-> step(): one forward and one backward pass -> [output, input gradient, weight gradients...]"""
    import torch

    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers import GNN, GNNInput, MessagePassingInput
    import tf2_gnn_amd.layers.message_passing as mp

    name, kind, what, over, D, _, num_sources = case
    gen = torch.Generator().manual_seed(len(name) + D)
    X = torch.randn((V, D), generator=gen).to(dev)
    dOut = torch.randn((V, H), generator=gen).to(dev)
    graph = ops.Graph([torch.from_numpy(a).to(dev) for a in adjacency_lists(num_sources)], V, parts=ops.G_PARTS_ALL)
    mp.set_seed(11)
    if kind == "stack":
        params = GNN.get_default_hyperparameters(what)
        params.update(over, hidden_dim=H)
        gnn = GNN(params)
        gnn.dropout_seed = 7
        inp = GNNInput(X, graph, torch.zeros(V, dtype=torch.int32, device=dev), 1)

        def step():
            gnn._dropout_calls = 0
            out = gnn(inp, training=True)
            dx = gnn.backward(dOut, need_input_grad=True)
            return [out, dx] + [v.grad for v in gnn.trainable_variables]

        return step
    cls = getattr(mp, what)
    p = cls.get_default_hyperparameters()
    p.update(over, hidden_dim=H)
    layer = cls(p)
    layer.build(MessagePassingInput((None, D), tuple((None, 2) for _ in range(L))))
    inp = MessagePassingInput(X, graph)

    def step():
        out = layer(inp, training=True)
        dx = layer.backward(dOut)
        return [out, dx] + [v.grad for v in layer.trainable_variables]

    return step


def run_case(case, dev):
    """One step of the case in f16x2 mode, from a cleared weight-operand cache -> ({"launches", "products"}, the step's tensors)"""
    import torch

    from tf2_gnn_amd import _lib, ops
    from tf2_gnn_amd.layers.message_passing import GNN_Edge_MLP

    lib = _lib.load()
    real = lib.tfgnn_aux_launch
    launches = []

    def spy(jobs, n, stream):
        kinds = [int(jobs[i].kind) for i in range(n) if jobs[i].kind != 0 and jobs[i].num_blocks != 0]
        st = getattr(stream, "value", stream) or 0
        launches.append([kinds, int(st) == int(torch.cuda.current_stream().cuda_stream)])
        return real(jobs, n, stream)

    prev_mode = ops.set_gemm_mode("f16x2")
    min_rows = GNN_Edge_MLP.GROUPED_SPLIT_MIN_ROWS
    GNN_Edge_MLP.GROUPED_SPLIT_MIN_ROWS = 64
    try:
        with _Env(case[5]):
            step = _build(case, dev)
            ops.clear_weight_operand_cache()
            before = ops.launch_counts()
            lib.tfgnn_aux_launch = spy
            try:
                tensors = step()
            finally:
                lib.tfgnn_aux_launch = real
            after = ops.launch_counts()
            torch.cuda.synchronize()
    finally:
        GNN_Edge_MLP.GROUPED_SPLIT_MIN_ROWS = min_rows
        ops.set_gemm_mode(prev_mode)
    products = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    return {"launches": launches, "products": products}, [t.clone() for t in tensors if t is not None]


def record(dev):
    out = {}
    for case in cases():
        rec, _ = run_case(case, dev)
        assert any(rec["products"].get(f, 0) > 0 for f in SPLIT_FAMILIES), (case[0], rec["products"])
        out[case[0]] = rec
    return out


if __name__ == "__main__":
    import torch

    print(json.dumps(record(torch.device("cuda", 0)), indent=1, sort_keys=True))
