"""Times the graph readout tail, forward + backward, two ways on the same tensors: the op-level sequence
(tfgnn_segment_softmax, tfgnn_clip, tfgnn_segment_weighted_sum, tfgnn_segment_weighted_sum_backward, tfgnn_clip_backward,
tfgnn_segment_softmax_backward - called through _lib exactly as the layer did before the fused entry points) against
tfgnn_pool_forward + tfgnn_pool_backward.

    python tools/pool_probe.py --shape qm9|ppi|one [--kind softmax] [--no-bounds] [--repeats 30]

One shape per process, so that a caller can give every timed step a time limit of its own:

    timeout -k 10 300 python tools/pool_probe.py --shape qm9 && timeout -k 10 300 python tools/pool_probe.py --shape ppi && ...

Method: 5 warm-up rounds of both routes, then `repeats` rounds that alternate the two routes, each forward + backward pair
bracketed by its own pair of events; reported are the median, the 10th and 90th percentile and the spread (p90 - p10) / median
per route, and the ratio of the medians."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tf2_gnn_amd import _lib, ops  # noqa: E402
from tf2_gnn_amd.layers.nodes_to_graph_representation import segment_offsets  # noqa: E402

SHAPES = {
    "qm9": dict(what="128 000 graphs of 1-29 nodes", GD=128, heads=8),
    "ppi": dict(what="20 graphs of about 2 400 nodes", GD=128, heads=8),
    "one": dict(what="one graph of 170 000 nodes", GD=128, heads=4),
}


def sizes_of(shape):
    rng = np.random.default_rng(0)
    if shape == "qm9":
        return rng.integers(1, 30, size=128000)
    if shape == "ppi":
        return rng.integers(2200, 2600, size=20)
    return np.array([170000])


def op_level(kind, ptr, ids, T, S, g, heads, lo, hi):
    lib = _lib.load()
    G, (V, GD) = ptr.numel() - 1, T.shape
    mean = int(kind == "average")
    w = None
    if kind == "sigmoid":
        w = S
    elif kind == "softmax":
        w = torch.empty_like(S)
        _lib.check(lib.tfgnn_segment_softmax(ops._ptr(S), heads, heads, ops._ptr(ptr), G, ops._ptr(w), heads, ops._stream()))
    bounded = lo is not None or hi is not None
    R = ops.clip(T, lo, hi) if bounded else T
    out = torch.empty((G, GD), dtype=torch.float32, device=T.device)
    _lib.check(lib.tfgnn_segment_weighted_sum(ops._ptr(R), ops._ptr(w), ops._ptr(ptr), G, GD, heads, mean, ops._ptr(out), ops._stream()))
    dR = torch.empty_like(T)
    dW = torch.empty_like(S) if w is not None else None
    _lib.check(lib.tfgnn_segment_weighted_sum_backward(ops._ptr(g), ops._ptr(R) if w is not None else None, ops._ptr(w), ops._ptr(ids),
                                                       ops._ptr(ptr), V, GD, heads, mean, ops._ptr(dR), ops._ptr(dW), ops._stream()))
    if bounded:
        dR = ops.clip_backward(dR, T, lo, hi)
    dS = dW
    if kind == "softmax":
        dS = torch.empty_like(dW)
        _lib.check(lib.tfgnn_segment_softmax_backward(ops._ptr(w), ops._ptr(dW), heads, ops._ptr(ptr), G, ops._ptr(dS), ops._stream()))
    return out, dR, dS


def fused(kind, ptr, ids, T, S, g, heads, lo, hi):
    out, w = ops.pool_forward(kind, ptr, T, S, heads, lo, hi)
    dT, dS = ops.pool_backward(kind, ptr, ids, g, T, w if kind == "softmax" else S, heads, lo, hi)
    return out, dT, dS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), required=True)
    ap.add_argument("--kind", default="softmax", choices=["softmax", "sigmoid", "none", "average"])
    ap.add_argument("--no-bounds", action="store_true")
    ap.add_argument("--repeats", type=int, default=30)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = SHAPES[args.shape]
    GD, heads = cfg["GD"], cfg["heads"]
    sizes = sizes_of(args.shape)
    ids = torch.from_numpy(np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)).to(dev)
    V, G = int(ids.numel()), len(sizes)
    ptr = segment_offsets(ids, G)
    gen = torch.Generator().manual_seed(1)
    T = torch.tanh(torch.randn((V, GD), generator=gen)).to(dev)
    S = torch.randn((V, heads), generator=gen).to(dev) if args.kind in ("softmax", "sigmoid") else None
    if args.kind == "sigmoid":
        S = torch.sigmoid(S)
    g = torch.randn((G, GD), generator=gen).to(dev)
    lo, hi = (None, None) if args.no_bounds else (-0.5, 0.5)
    routes = {"op-level": op_level, "fused": fused}
    results = {}
    for name, fn in routes.items():
        for _ in range(5):
            results[name] = fn(args.kind, ptr, ids, T, S, g, heads, lo, hi)
    torch.cuda.synchronize()
    worst = max(float((a - b).abs().max()) for a, b in zip(results["fused"], results["op-level"]) if a is not None)
    times = {name: [] for name in routes}
    for _ in range(args.repeats):
        for name, fn in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(args.kind, ptr, ids, T, S, g, heads, lo, hi)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3)
    print(f"shape {args.shape}: {cfg['what']}; V = {V}, G = {G}, GD = {GD}, heads = {heads}, kind = {args.kind}, "
          f"bounds = {(lo, hi)}, repeats = {args.repeats}; largest |fused - op-level| = {worst:.3e}")
    med = {}
    for name, ts in times.items():
        ts = np.array(ts)
        med[name] = float(np.median(ts))
        p10, p90 = np.percentile(ts, 10), np.percentile(ts, 90)
        print(f"  {name:9s} forward + backward: median {med[name]:10.1f} us   p10 {p10:10.1f}   p90 {p90:10.1f}   "
              f"spread {(p90 - p10) / med[name]:.3f}")
    print(f"  op-level / fused = {med['op-level'] / med['fused']:.2f}", flush=True)


if __name__ == "__main__":
    main()
