"""What the GNN_Edge_MLP family tells a layer stack before a pass runs, over a grid of layers, GEMM modes and batch shapes: the
record that pins every predicate of the layer's choice of formulation across a change of where that choice is written down.

    python tools/record_edge_mlp_plan.py > tests/golden/edge_mlp_plan_parent.json

Per grid point: ``graph_parts``, ``recomputes_input_dropout``, the kinds of ``weight_operand_requests`` for the forward and
for the backward pass, and ``_path()``.  Only host code runs (no device): the layers are built on the meta device - the
answers depend on the shapes of the weights alone.  tests/test_edge_mlp_plan_host.py walks the same grid through ``record()``
and demands equality with the committed record.

The grid: every class x hyper-parameter set of ``layers()`` (target states on / off x 0, 1, 2 hidden layers, and on three of
those sum / mean / max aggregation, the activation before the aggregation, ``use_compact_buckets``) at L in {1, 4, 8, 9} edge
types and widths H = D in {16, 24, 128, 320, 1040}; per layer the points of ``points()``: the three GEMM modes, fewer / more
edges than (node, type) buckets and a batch without nodes, one edge type empty or none, ``PER_EDGE_MIN_ROWS`` at its default
and at 1, ``_grouped_tn_split_ok`` set and cleared.  V = 200 000, so that with fewer edges than buckets every edge type still
has the 65 536 rows the fused per-edge product asks for.

Format: ``answers`` lists the distinct answers; ``layers[name]`` is one character per point of ``points()``, in order, the
character's position in ``ALPHABET`` being the index of the point's answer."""
from __future__ import annotations

import itertools
import json
import sys
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

CLASSES = ("RGCN", "GGNN", "RGIN", "GNN_FiLM", "GNN_Edge_MLP")
EDGE_TYPES = (1, 4, 8, 9)
WIDTHS = (16, 24, 128, 320, 1040)
MODES = ("f16x2", "bf16x3", "fp32")
NUM_NODES = 200000
ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"


def hyper_parameter_sets():
    """-> [(tag, overrides)]: target states x hidden layers with sum aggregation; on three of them the other switches"""
    out = []
    for target, hidden in itertools.product((False, True), (0, 1, 2)):
        base = {"use_target_state_as_input": target, "num_edge_MLP_hidden_layers": hidden}
        out.append((f"t{int(target)}h{hidden}", base))
        if (target, hidden) in ((False, 0), (False, 1), (True, 1)):
            out.append((f"t{int(target)}h{hidden}mean", dict(base, aggregation_function="mean")))
            out.append((f"t{int(target)}h{hidden}max", dict(base, aggregation_function="max")))
            out.append((f"t{int(target)}h{hidden}pre", dict(base, message_activation_before_aggregation=True)))
            out.append((f"t{int(target)}h{hidden}compact", dict(base, use_compact_buckets=True)))
    out.append(("t1h0compact", {"use_target_state_as_input": True, "num_edge_MLP_hidden_layers": 0, "use_compact_buckets": True}))
    return out


def layers():
    """-> [(name, class name, overrides, L, H)]"""
    return [(f"{cls} {tag} L{L} H{H}", cls, dict(over, hidden_dim=H), L, H)
            for cls in CLASSES for tag, over in hyper_parameter_sets() for L in EDGE_TYPES for H in WIDTHS]


def points():
    """-> [(mode, shape, one edge type empty?, PER_EDGE_MIN_ROWS | None, _grouped_tn_split_ok)], shape = "few" (E = V L / 2),
    "many" (E = 2 V L) or "nothing" (V = 0)"""
    return list(itertools.product(MODES, ("few", "many", "nothing"), (False, True), (None, 1), (True, False)))


def batch_shape(shape: str, L: int, one_empty: bool):
    """-> (num_nodes, edges per type)"""
    if shape == "nothing":
        return 0, (0,) * L
    per_type = NUM_NODES // 2 if shape == "few" else 2 * NUM_NODES
    counts = [per_type] * L
    if one_empty:
        counts[L // 2] = 0
    return NUM_NODES, tuple(counts)


def build_layer(cls_name: str, over: dict, L: int, H: int):
    """the layer with its weights on the meta device (shapes only; the initialiser draws nothing)"""
    import torch

    import tf2_gnn_amd.layers.message_passing as mp
    from tf2_gnn_amd.layers.message_passing import ggnn, gnn_edge_mlp, message_passing, rgin

    meta = torch.device("meta")
    modules = (message_passing, gnn_edge_mlp, ggnn, rgin)
    real = [m.glorot_uniform for m in modules]
    for m in modules:
        m.glorot_uniform = lambda shape, fan_in=None, fan_out=None, device=None: torch.empty(tuple(shape), device=meta)
    message_passing.set_default_device(meta)
    try:
        cls = getattr(mp, cls_name)
        p = cls.get_default_hyperparameters()
        p.update(over)
        layer = cls(p)
        layer.build(mp.MessagePassingInput((None, H), tuple((None, 2) for _ in range(L))))
    finally:
        message_passing.set_default_device(None)
        for m, f in zip(modules, real):
            m.glorot_uniform = f
    return layer


def answer(layer, V: int, counts, H: int) -> str:
    graph = SimpleNamespace(num_edge_types=len(counts), num_edges=int(sum(counts)), num_nodes=V, edges_per_type=tuple(counts))
    kinds = ["+".join(kind for _, kind, _ in layer.weight_operand_requests(graph, V, H, backward)) for backward in (False, True)]
    return (f"parts={layer.graph_parts(V, counts, H)} recompute={int(bool(layer.recomputes_input_dropout(V, H, len(counts))))} "
            f"forward=[{kinds[0]}] backward=[{kinds[1]}] path={layer._path()}")


def record():
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers.message_passing import gnn_edge_mlp

    built = [(name, build_layer(cls, over, L, H), L, H) for name, cls, over, L, H in layers()]
    rows = {name: [] for name, _, _, _ in built}
    prev_mode = ops.get_gemm_mode()
    min_rows = gnn_edge_mlp.PER_EDGE_MIN_ROWS
    try:
        for mode, shape, one_empty, per_edge_rows, tn_ok in points():
            ops.set_gemm_mode(mode)
            gnn_edge_mlp.PER_EDGE_MIN_ROWS = min_rows if per_edge_rows is None else per_edge_rows
            for name, layer, L, H in built:
                layer._grouped_tn_split_ok = tn_ok
                V, counts = batch_shape(shape, L, one_empty)
                rows[name].append(answer(layer, V, counts, H))
    finally:
        gnn_edge_mlp.PER_EDGE_MIN_ROWS = min_rows
        ops.set_gemm_mode(prev_mode)
    answers = sorted({a for r in rows.values() for a in r})
    assert len(answers) <= len(ALPHABET), len(answers)
    index = {a: ALPHABET[i] for i, a in enumerate(answers)}
    return {"answers": answers, "points": [list(p) for p in points()],
            "layers": {name: "".join(index[a] for a in r) for name, r in rows.items()}}


if __name__ == "__main__":
    print(json.dumps(record(), indent=1, sort_keys=True))
