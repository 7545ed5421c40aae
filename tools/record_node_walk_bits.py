"""SHA-256 of what the two node-view walks compute - the R-GCN basis gather (csrc/basis.hip) and the block-diagonal walk
(csrc/blockdiag.hip), forward and both reverse passes - and the launches each call counts: the record that pins both bit for
bit across a change of the skeleton they share (csrc/node_walk.hpp: item slicing, short-row selection, the group sum in LDS,
the combine launch).

    python tools/record_node_walk_bits.py > tests/golden/node_walk_parent_bits.json

Cases: every entry of ``CASES`` in tests/test_gpu_basis_gather.py and tests/test_gpu_blockdiag_ops.py, FLOAT family only (the
EXACT family gives the same bits in any order and would pin nothing), each at the placement its own test uses (the misaligned
ones shifted by one float).  The inputs come from those files' seeded generators (``_graph_case``, ``_case``, ``_wide``) and
the scales from ``graph_scales``, so the hashes depend on the kernels alone.  Per case: the hash of each output (basis: Z, dX,
dcoeff; block-diagonal: pre, dX, dQb) and the launch-count deltas of one forward and one backward call.  The recorder runs
every case twice in one process and refuses to write a record if two runs of a case differ: the kernels use no atomics and
fixed sum orders, so no case is exempt.  tests/test_gpu_node_walk_bits.py runs the same cases through ``cases()`` /
``run_case()`` and compares with the committed record."""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def cases():
    from tests import test_gpu_basis_gather as tb
    from tests import test_gpu_blockdiag_ops as td

    out = []
    for V, D, L, B, hub in tb.CASES:
        mis = (V, D, L, B) in tb._MISALIGNED
        out.append(dict(name=f"basis_V{V}_D{D}_L{L}_B{B}" + ("_hub" if hub else "") + ("_misaligned" if mis else ""),
                        kind="basis", V=V, D=D, L=L, B=B, hub=hub, misaligned=mis))
    for kind, V, L, D, H, C, mis in td.CASES:
        out.append(dict(name=f"blockdiag_{kind}_V{V}_L{L}_D{D}_H{H}_C{C}" + ("_misaligned" if mis else ""),
                        kind="blockdiag", graph=kind, V=V, L=L, D=D, H=H, C=C, misaligned=mis))
    return out


def sha(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def _graph(adjs, V, dev):
    import torch

    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers.graph_scales import graph_scales

    g = ops.Graph([torch.from_numpy(a).to(dev) for a in adjs], V)
    return g, graph_scales(g, True, "mean")


def _basis(c, dev):
    import numpy as np
    import torch

    from tests import test_gpu_basis_gather as tb
    from tf2_gnn_amd import ops

    V, D, L, B = c["V"], c["D"], c["L"], c["B"]
    data = tb._case("float", V, D, L, B, c["hub"])
    g, sc = _graph(data["adjs"], V, dev)
    coeff = torch.from_numpy(data["coeff"]).to(dev)
    left = tb.PAD_LEFT - 1 if c["misaligned"] else tb.PAD_LEFT
    _, X = tb._wide(data["X"], dev, left)
    _, dZ = tb._wide(data["dZ"], dev, left)
    _, Z = tb._wide(np.zeros((V, B * D), np.float32), dev, left)
    _, dX = tb._wide(np.zeros((V, D), np.float32), dev, left)
    n0 = ops.basis_launch_counts()
    ops.basis_gather_forward(g, coeff, X, edge_weight=sc.edge_weight_by_dst, node_scale=sc.node_scale, out=Z)
    n1 = ops.basis_launch_counts()
    _, dcoeff = ops.basis_gather_backward(g, coeff, dZ, X, out_dx=dX, edge_weight_by_dst=sc.edge_weight_by_dst,
                                          edge_weight_by_src=sc.edge_weight_by_src, node_scale=sc.node_scale)
    n2 = ops.basis_launch_counts()
    return {"sha": {"Z": sha(Z), "dX": sha(dX), "dcoeff": sha(dcoeff)},
            "launches": {"forward": _delta(n0, n1), "backward": _delta(n1, n2)}}


def _blockdiag(c, dev):
    import numpy as np
    import torch

    from tests import test_gpu_blockdiag_ops as td
    from tf2_gnn_amd import ops

    V, L, D, H, C, mis = c["V"], c["L"], c["D"], c["H"], c["C"], c["misaligned"]
    data = td._case("float", c["graph"], V, L, D, H, C)
    g, sc = _graph(data["adjs"], V, dev)
    left = td.PAD_LEFT - 1 if mis else td.PAD_LEFT
    qflat = torch.zeros(data["Qb"].size + 4, device=dev)
    Qb = qflat[1 if mis else 0:][:data["Qb"].size].view(data["Qb"].shape)
    Qb.copy_(torch.from_numpy(data["Qb"]))
    assert (Qb.data_ptr() % 16 != 0) == mis
    _, X = td._wide(data["X"], dev, left)
    _, dPre = td._wide(data["dPre"], dev, left)
    _, P = td._wide(np.zeros((V, H), np.float32), dev, left)
    _, dX = td._wide(np.zeros((V, D), np.float32), dev, left)
    n0 = ops.blockdiag_launch_counts()
    ops.blockdiag_forward(g, Qb, X, C, edge_weight=sc.edge_weight_by_dst, node_scale=sc.node_scale, out=P)
    n1 = ops.blockdiag_launch_counts()
    _, dQb = ops.blockdiag_backward(g, Qb, dPre, X, C, out_dx=dX, edge_weight_by_dst=sc.edge_weight_by_dst,
                                    edge_weight_by_src=sc.edge_weight_by_src, node_scale=sc.node_scale)
    n2 = ops.blockdiag_launch_counts()
    return {"sha": {"pre": sha(P), "dX": sha(dX), "dQb": sha(dQb)},
            "launches": {"forward": _delta(n0, n1), "backward": _delta(n1, n2)}}


def run_case(c, dev):
    """-> {"sha": {output: hash}, "launches": {"forward": deltas, "backward": deltas}}"""
    return (_basis if c["kind"] == "basis" else _blockdiag)(c, dev)


def run_twice(cs, dev):
    out = {}
    for c in cs:
        first, second = run_case(c, dev), run_case(c, dev)
        if first != second:
            raise SystemExit(f"{c['name']}: two runs in one process differ - a finding, not a case to exempt:\n{first}\n{second}")
        out[c["name"]] = first
    return out


if __name__ == "__main__":
    import torch

    print(json.dumps(run_twice(cases(), torch.device("cuda", 0)), indent=1, sort_keys=True))
