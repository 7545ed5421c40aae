"""Times one RGAT layer, forward + backward in training mode, on the graph of bench.py's rgat workload (BASELINE configs[2]:
30 000 nodes, 900 000 edges, 4 edge types, R-MAT) at a head count that is not a power of two, two ways in one process:

  row kernels  tfgnn_rgat_attention_forward / _backward (wave per short row, workgroup per item, in-order combine)
  piecewise    the branch of RGAT._edge_attention / RGAT._backward behind return code -4: edge scores, segment max, exp, segment
               sum, divide; backward mul + segment sum + edge kernel, and the re-ordering gather for the by-source weights.
               It is forced by answering -4 for the two entries without calling them, which is what the library did for
               these head counts before the row kernels took them.
               (The layer no longer has that branch: NOTEBOOK.md §17 keeps the measurement, and this leg runs only in a checkout
               of the commit that recorded it.)

    python tools/rgat_heads_probe.py --heads 3 [--hidden 192] [--repeats 30]

One head count per process, so that a caller can give every timed step a time limit of its own:

    timeout -k 10 300 python tools/rgat_heads_probe.py --heads 3 && timeout -k 10 300 python tools/rgat_heads_probe.py --heads 6

Method: 5 warm-up rounds of both routes, then `repeats` rounds that alternate the two routes, each forward + backward pair
bracketed by its own pair of events; reported are the median, the 10th and 90th percentile and the spread (p90 - p10) / median
per route, the ratio of the medians, and the largest difference between the two routes' outputs and gradients."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tf2_gnn_amd import _lib  # noqa: E402
from tf2_gnn_amd.data import make_synthetic_batch  # noqa: E402
from tf2_gnn_amd.layers import MessagePassingInput  # noqa: E402
from tf2_gnn_amd.layers.message_passing import RGAT  # noqa: E402

V, E, L = 30000, 900000, 4
ENTRIES = ("tfgnn_rgat_attention_forward", "tfgnn_rgat_attention_backward")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, required=True)
    ap.add_argument("--hidden", type=int, default=192)
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    H, K = args.hidden, args.heads
    feats, adjs = make_synthetic_batch(V, E, L, H, seed=1)
    p = RGAT.get_default_hyperparameters()
    p.update({"hidden_dim": H, "num_heads": K})
    layer = RGAT(p)
    layer.build(MessagePassingInput((None, H), tuple((None, 2) for _ in range(L))))
    inp = MessagePassingInput(torch.from_numpy(feats).to(dev), tuple(torch.from_numpy(a).to(dev) for a in adjs))
    d_out = torch.randn((V, H), generator=torch.Generator().manual_seed(1)).to(dev)
    lib = _lib.load()
    native = {name: getattr(lib, name) for name in ENTRIES}

    def step(route):
        for name in ENTRIES:
            setattr(lib, name, native[name] if route == "row kernels" else (lambda *a: -4))
        try:
            out = layer(inp, training=True)
            took_rows = layer._ctx["att_by_src"] is not None
            dx = layer.backward(d_out)
        finally:
            for name in ENTRIES:
                setattr(lib, name, native[name])
        return took_rows, out, dx, [v.grad for v in layer.trainable_variables]

    routes = ("row kernels", "piecewise")
    results = {}
    for name in routes:
        for _ in range(5):
            results[name] = step(name)
    torch.cuda.synchronize()
    took = {name: results[name][0] for name in routes}
    a, b = results["row kernels"], results["piecewise"]
    worst = max(float((x - y).abs().max()) for x, y in zip([a[1], a[2]] + a[3], [b[1], b[2]] + b[3]))
    times = {name: [] for name in routes}
    for _ in range(args.repeats):
        for name in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    print(f"RGAT layer forward + backward, training mode: V = {V}, E = {E}, L = {L}, H = {H}, heads = {K}, repeats = {args.repeats}, "
          f"device = {torch.cuda.get_device_name(0)}; the 'row kernels' route ran the row kernels: {took['row kernels']} "
          f"(piecewise route: {took['piecewise']}); largest |row kernels - piecewise| over out, dX, weight gradients = {worst:.3e}")
    med = {}
    for name, ts in times.items():
        ts = np.array(ts)
        med[name] = float(np.median(ts))
        p10, p90 = np.percentile(ts, 10), np.percentile(ts, 90)
        print(f"  {name:11s} median {med[name]:9.1f} us   p10 {p10:9.1f}   p90 {p90:9.1f}   spread {(p90 - p10) / med[name]:.3f}")
    print(f"  piecewise / row kernels = {med['piecewise'] / med['row kernels']:.3f}", flush=True)


if __name__ == "__main__":
    main()
