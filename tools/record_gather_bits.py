"""SHA-256 of every output array of the planned graph gather over a small hub graph: the record that pins the gather's
results bit for bit across a change of how its multi-item rows are combined.

    python tools/record_gather_bits.py > tests/golden/gather_combine_parent_bits.json

The graph (V = 300, L = 3, type 2 without edges) puts in- and out-degrees of type 0 at both sides of the plan's limits
(graph.hpp: typed threshold 48, 512-edge items): 48 (short row), 49 (one item, no slot), 513 (two items, the last holds
one edge), 1025 (three items) and 2600 (six items: the combine's four-at-a-time loop plus a tail of two).  All inputs come
from seeded host generators, so the hashes depend on the kernels alone.  tests/test_gpu_gather_fused_combine.py builds the
same cases through ``cases()`` / ``run_case()`` and compares with the committed record."""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

NUM_NODES = 300
HUB_DEGREES = (48, 49, 513, 1025, 2600)
HUB_TARGETS = tuple(range(0, 5))    # in-degree HUB_DEGREES[i] in type 0
HUB_SOURCES = tuple(range(10, 15))  # out-degree HUB_DEGREES[i] in type 0
FIRST_PLAIN_NODE = 20               # the other end of every hub edge is drawn from [20, V)
VIEW_BY_DST_TYPED, VIEW_BY_DST_NODE, VIEW_BY_SRC_TYPED, VIEW_BY_DST_TYPED_PATTERN = 0, 1, 2, 6
VIEWS = (VIEW_BY_DST_TYPED, VIEW_BY_SRC_TYPED, VIEW_BY_DST_TYPED_PATTERN, VIEW_BY_DST_NODE)
SP_WIDTHS = (64, 320)
FP32_WIDTHS = (64, 320, 1280)  # 1280: four feature windows


def adjacency_lists():
    """[type 0: the hubs, type 1: 300 random edges among the plain nodes, type 2: empty], int32 [E_l, 2] rows (source, target)"""
    rng = np.random.default_rng(20240)
    plain = lambda n: rng.integers(FIRST_PLAIN_NODE, NUM_NODES, size=n)
    src, tgt = [], []
    for node, deg in zip(HUB_TARGETS, HUB_DEGREES):
        src.append(plain(deg))
        tgt.append(np.full(deg, node))
    for node, deg in zip(HUB_SOURCES, HUB_DEGREES):
        src.append(np.full(deg, node))
        tgt.append(plain(deg))
    a0 = np.stack([np.concatenate(src), np.concatenate(tgt)], axis=1)
    rng.shuffle(a0, axis=0)
    a1 = np.stack([plain(300), plain(300)], axis=1)
    return [a0.astype(np.int32), a1.astype(np.int32), np.zeros((0, 2), dtype=np.int32)]


def cases():
    """-> [(name, view, width, weighted, kind)], kind = "sp" (SP16 output), "fp32" (sums) or "max" """
    out = []
    for view in VIEWS:
        for weighted in (False, True):
            for w in SP_WIDTHS:
                out.append((f"sp view{view} w{w} {'weighted' if weighted else 'plain'}", view, w, weighted, "sp"))
            for w in FP32_WIDTHS:
                out.append((f"fp32 view{view} w{w} {'weighted' if weighted else 'plain'}", view, w, weighted, "fp32"))
    for view in (VIEW_BY_DST_TYPED, VIEW_BY_DST_NODE):
        out.append((f"max view{view} w64 weighted", view, 64, True, "max"))
    return out


def host_inputs(view: int, width: int):
    """(X [input rows, width], edge weights [E], row scales [CSR rows]) as fp32 numpy arrays"""
    lists = adjacency_lists()
    L = len(lists)
    E = sum(a.shape[0] for a in lists)
    node = view == VIEW_BY_DST_NODE
    rng = np.random.default_rng(1000 * view + width)
    X = rng.standard_normal((NUM_NODES * (L if node else 1), width)).astype(np.float32)
    ew = (rng.random(E) + 0.5).astype(np.float32)
    rs = (rng.random(NUM_NODES * (1 if node else L)) * 0.7 + 0.3).astype(np.float32)
    return X, ew, rs


def make_graph(dev):
    import torch

    from tf2_gnn_amd import ops

    return ops.Graph([torch.from_numpy(a).to(dev) for a in adjacency_lists()], NUM_NODES, parts=ops.G_PARTS_ALL)


def run_case(graph, case, dev, inputs=None):
    """one gather -> {array name: device tensor}: "data" and "inv_scale" of an SP16 result, "rows" of an fp32 one"""
    import torch

    from tf2_gnn_amd import ops

    _, view, width, weighted, kind = case
    if inputs is None:
        inputs = tuple(torch.from_numpy(a).to(dev) for a in host_inputs(view, width))
    X, ew, rs = inputs
    kw = dict(edge_weight=ew, row_scale=rs) if weighted else {}
    if kind == "sp":
        op = ops.graph_gather_sp(graph, view, X, **kw)
        return {"data": op.data, "inv_scale": op.inv_scale}
    return {"rows": ops.graph_gather(graph, view, X, reduce=ops.REDUCE_MAX if kind == "max" else ops.REDUCE_SUM, **kw)}


def bucket_order(graph, view: int, t):
    """rows of a result in bucket order (v * L + l): the pattern view writes bucket (v, l) at row pos[v] * L + l, and the
    order of the nodes inside one pattern is free (it differs from build to build), so its rows are put back first"""
    if view != VIEW_BY_DST_TYPED_PATTERN:
        return t
    from tf2_gnn_amd import ops

    L = graph.num_edge_types
    pos = graph.array(ops.G_PATTERN_POS_BY_DST).long()
    return t.reshape(graph.num_nodes, L, -1)[pos].reshape(t.shape)


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def record(dev):
    import torch

    graph = make_graph(dev)
    out = {}
    for case in cases():
        res = run_case(graph, case, dev)
        torch.cuda.synchronize()
        for name, t in res.items():
            out[f"{case[0]} {name}"] = sha(bucket_order(graph, case[1], t))
    return out


if __name__ == "__main__":
    import torch

    print(json.dumps(record(torch.device("cuda", 0)), indent=1, sort_keys=True))
