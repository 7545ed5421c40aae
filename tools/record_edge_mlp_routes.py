"""SHA-256 of what one forward pass and one ``backward_with_epilogue`` of the GNN_Edge_MLP family compute, route by route: the
record that pins every formulation of the layer bit for bit across a change of how the layer picks and drives them.

    python tools/record_edge_mlp_routes.py > tests/golden/edge_mlp_routes_parent_bits.json

Per case of ``cases()``: ``ctx["path"]``, ``ctx["f16x2"]`` and ``_grouped_tn_used`` after the passes, the launches per kernel
family (``ops.launch_counts``) of the two passes, and the hashes of the output, of d(node states) and of every weight gradient.
The epilogue handed to the backward pass is a dropout-style mask and ``("tanh", saved)``.  All inputs come from seeded host
generators and the weights from the seeded initialiser, so the hashes depend on the kernels alone.  The recorder runs every case
twice in one process: an array whose two hashes differ is listed under ``not_reproducible`` with both and is not compared.
tests/test_gpu_edge_mlp_routes.py runs the same cases through ``cases()`` / ``run_case()`` and compares with the committed
record.

Only API that does not depend on how the layer is organised inside is used: the layer classes, ``ops.Graph``, the module
attribute ``PER_EDGE_MIN_ROWS`` and the class attribute ``GROUPED_SPLIT_MIN_ROWS`` that the layer tests lower as well."""
from __future__ import annotations

import hashlib
import json
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

H = 128
_LINEAR = {"num_edge_MLP_hidden_layers": 0, "use_target_state_as_input": False}
_SRC_ONLY = {"use_target_state_as_input": False}
_SPARSE = dict(V=400, E=360, L=4, empty_types=(2,), hub=(9, 80))  # most (node, type) buckets empty: the compact path A


def case(name, cls, over, mode, L=4, V=384, E=4200, width=H, env=None, per_edge_rows=None, grouped_rows=None, empty_types=(),
         hub=None, demote_to=None):
    return dict(name=name, cls=cls, over=over, mode=mode, L=L, V=V, E=E, width=width, env=env or {}, per_edge_rows=per_edge_rows,
                grouped_rows=grouped_rows, empty_types=tuple(empty_types), hub=hub, demote_to=demote_to)


def cases():
    """name, layer class, hyper-parameter overrides, GEMM mode, graph, and what the case lowers: ``per_edge_rows`` =
    PER_EDGE_MIN_ROWS, ``grouped_rows`` = GROUPED_SPLIT_MIN_ROWS; ``demote_to``: the mode set between the two passes"""
    e = "GNN_Edge_MLP"
    return [
        # the routes of test_edge_mlp_gradient_epilogue_is_applied_exactly_once_on_every_route, as they stand
        case("A_f16x2_one_call", e, _LINEAR, "f16x2", env={"TFGNN_MP_ENTRY": "1"}),
        case("A_f16x2_op_level", e, _LINEAR, "f16x2", env={"TFGNN_MP_ENTRY": "0"}),
        case("A_bf16x3", e, _LINEAR, "bf16x3"),
        case("C_exact_kernels", e, {}, "bf16x3", L=5),
        case("C_first_layer_split", e, {}, "f16x2", L=5),
        case("Bc", e, _SRC_ONLY, "bf16x3", L=8, V=400, E=900),
        case("Bc_grouped_split", e, _SRC_ONLY, "f16x2", L=8, V=3000, E=7000, grouped_rows=64),
        case("A_target_states", e, {"num_edge_MLP_hidden_layers": 0}, "bf16x3"),
        case("A_per_edge_f16x2", e, _LINEAR, "f16x2", L=3, V=400, E=900, per_edge_rows=1),
        case("A_per_edge_bf16x3", e, _LINEAR, "bf16x3", L=3, V=400, E=900, per_edge_rows=1),
        case("Ac", "RGCN", {"use_compact_buckets": True}, "f16x2", width=32, **_SPARSE),
        case("B_dense", e, _SRC_ONLY, "f16x2", L=3),
        case("B_max", e, dict(_SRC_ONLY, aggregation_function="max"), "f16x2", L=3),
        case("B_activation_before_aggregation", e, dict(_SRC_ONLY, message_activation_before_aggregation=True), "f16x2", L=3),
        case("C_max", e, {"aggregation_function": "max"}, "f16x2", L=5),
        case("C_per_edge_first_layer", e, {}, "f16x2", L=3, V=400, E=900, per_edge_rows=1),
        case("C_no_edges", e, {}, "f16x2", L=3, E=0),
        case("GGNN_f16x2", "GGNN", {}, "f16x2"),
        case("GGNN_compact_buckets", "GGNN", {"use_compact_buckets": True}, "f16x2", **_SPARSE),
        case("RGIN_aggregation_mlp", "RGIN", {"num_aggr_MLP_hidden_layers": 1}, "f16x2"),
        case("FiLM_target_states", "GNN_FiLM", {"use_target_state_as_input": True}, "f16x2"),
        case("A_mode_demoted_before_backward", "RGCN", {}, "f16x2", demote_to="bf16x3"),
    ]


def adjacency_lists(c):
    """seeded multigraph, int32 [E_l, 2] rows (source, target): E // (types with edges) edges per type, ``hub`` = (node, extra
    in-edges of type 0)"""
    rng = np.random.default_rng(4 + c["V"] + c["L"])
    V, L = c["V"], c["L"]
    per = c["E"] // max(1, L - len(c["empty_types"]))
    adjs = []
    for l in range(L):
        if l in c["empty_types"] or per == 0:
            adjs.append(np.zeros((0, 2), dtype=np.int32))
            continue
        a = rng.integers(0, V, size=(per, 2)).astype(np.int32)
        if c["hub"] is not None and l == 0:
            node, extra = c["hub"]
            a = np.concatenate([a, np.stack([rng.integers(0, V, size=extra), np.full(extra, node)], axis=1).astype(np.int32)])
            rng.shuffle(a, axis=0)
        adjs.append(a)
    return adjs


def host_inputs(c):
    """(X, d(output), mask, saved) [V, width] fp32 host tensors: the layer's input, the gradient of its output, a dropout mask of
    its input (rate 0.1, scaled) and the tanh output of the op below"""
    import torch

    gen = torch.Generator().manual_seed(29 + len(c["name"]))
    shape = (c["V"], c["width"])
    X = torch.randn(shape, generator=gen)
    dOut = torch.randn(shape, generator=gen)
    mask = (torch.rand(shape, generator=gen) >= 0.1).float() / 0.9
    saved = torch.tanh(torch.randn(shape, generator=gen))
    return X, dOut, mask, saved


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


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(c, dev):
    """-> {"path", "f16x2", "grouped_tn_used", "products": {family: launches}, "sha": {array: hash}}"""
    import torch

    import tf2_gnn_amd.layers.message_passing as mp
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers.message_passing import gnn_edge_mlp

    X, dOut, mask, saved = (t.to(dev) for t in host_inputs(c))
    graph = ops.Graph([torch.from_numpy(a).to(dev) for a in adjacency_lists(c)], c["V"], parts=ops.G_PARTS_ALL)
    cls, base = getattr(mp, c["cls"]), gnn_edge_mlp.GNN_Edge_MLP
    prev_mode = ops.set_gemm_mode(c["mode"])
    per_edge_rows, grouped_rows = gnn_edge_mlp.PER_EDGE_MIN_ROWS, base.GROUPED_SPLIT_MIN_ROWS
    if c["per_edge_rows"] is not None:
        gnn_edge_mlp.PER_EDGE_MIN_ROWS = c["per_edge_rows"]
    if c["grouped_rows"] is not None:
        base.GROUPED_SPLIT_MIN_ROWS = c["grouped_rows"]
    try:
        with _Env(c["env"]):
            p = cls.get_default_hyperparameters()
            p.update(c["over"], hidden_dim=c["width"], message_activation_function="tanh")
            mp.set_seed(1000 + len(c["name"]))
            layer = cls(p)
            layer.build(mp.MessagePassingInput((None, c["width"]), tuple((None, 2) for _ in range(c["L"]))))
            ops.clear_weight_operand_cache()
            before = ops.launch_counts()
            out = layer(mp.MessagePassingInput(X, graph), training=True)
            if c["demote_to"] is not None:
                ops.set_gemm_mode(c["demote_to"])
            dX = layer.backward_with_epilogue(dOut, out_mul=mask, out_act_grad=("tanh", saved))
            after = ops.launch_counts()
            torch.cuda.synchronize()
    finally:
        gnn_edge_mlp.PER_EDGE_MIN_ROWS, base.GROUPED_SPLIT_MIN_ROWS = per_edge_rows, grouped_rows
        ops.set_gemm_mode(prev_mode)
    ctx = layer._ctx
    hashes = {"output": sha(out), "dX": sha(dX)}
    for v in layer.trainable_variables:
        hashes["d " + v.name] = "no gradient" if v.grad is None else sha(v.grad)
    return {"path": ctx.get("path"), "f16x2": ctx.get("f16x2"), "grouped_tn_used": bool(layer._grouped_tn_used),
            "products": {k: after[k] - before[k] for k in after if after[k] != before[k]}, "sha": hashes}


def record(dev):
    out = {}
    for c in cases():
        first, second = run_case(c, dev), run_case(c, dev)
        differing = {k: [h, second["sha"][k]] for k, h in first["sha"].items() if second["sha"][k] != h}
        assert {k: v for k, v in first.items() if k != "sha"} == {k: v for k, v in second.items() if k != "sha"}, c["name"]
        if differing:
            first["not_reproducible"] = differing
        out[c["name"]] = first
    return out


if __name__ == "__main__":
    import torch

    print(json.dumps(record(torch.device("cuda", 0)), indent=1, sort_keys=True))
