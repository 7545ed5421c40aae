"""Times what edge dropout costs one message-passing layer, forward + backward, on the synthetic graph of FB15k-237's shape that
tools/basis_probe.py and tools/blockdiag_probe.py use: RGCN_BlockDiag and RGCN_Basis at rate 0 and at the paper's rates (0.2 for
the self loops - edge type 0 -, 0.4 for every other type), then the launch that draws the step's scales on its own.

    python tools/edge_dropout_probe.py --hidden 64|320 [--repeats 20] [--mode f16x2|bf16x3|fp32] [--rate0-only]

D = H = --hidden; RGCN_BlockDiag at C = 64 (320) or 16 (64), RGCN_Basis at B = 8.  One width per process, so that a caller can
give every timed step a time limit of its own.  --rate0-only times the two rate-0 lines alone and touches nothing the feature
added, so the same script runs against a build of the commit before it: the figure "rate 0 costs what it cost" is held against.

Method, as blockdiag_probe: 3 warm-up rounds per variant, then `repeats` rounds that alternate the variants, each forward +
backward pair between its own pair of events, a variant's saved tensors dropped after its pair.  Per variant: median, 10th and
90th percentile in milliseconds and the spread (p90 - p10) / median.  The new launch alone: bursts of 50 calls per event pair,
per (normalize, mode).
The bytes-per-edge model printed next to it is COMPUTED from the kernel's accesses, not measured.  No GPU: the script fails."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.basis_probe import V_FB, fb15k_shaped_graph  # noqa: E402


def build_layer(kind, n, D, H, L, rates):
    import tf2_gnn_amd.layers.message_passing as mp

    cls = {"basis": mp.RGCN_Basis, "blockdiag": mp.RGCN_BlockDiag}[kind]
    p = cls.get_default_hyperparameters()
    p["hidden_dim"] = H
    p["num_bases" if kind == "basis" else "num_blocks"] = n
    if rates is not None:
        p["edge_dropout_rate"] = rates
    mp.set_seed(1)
    layer = cls(p)
    layer.build(mp.MessagePassingInput((None, D), tuple((None, 2) for _ in range(L))))
    return layer


def timed(fn, repeats):
    """-> milliseconds of `repeats` calls of fn, each between its own pair of events, after 3 warm-up calls"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1))
    return np.array(out)


def line(name, t):
    med, p10, p90 = np.median(t), np.percentile(t, 10), np.percentile(t, 90)
    return f"{name:>34}: median {med:8.3f} ms  p10 {p10:8.3f}  p90 {p90:8.3f}  spread {(p90 - p10) / med:5.1%}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, required=True)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--mode", default="f16x2")
    ap.add_argument("--rate0-only", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("edge_dropout_probe: no ROCm device - nothing is measured on a CPU")
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers import MessagePassingInput
    from tf2_gnn_amd.layers.message_passing import get_graph

    ops.set_gemm_mode(args.mode)
    dev = torch.device("cuda", 0)
    D = H = args.hidden
    adjs_np = fb15k_shaped_graph()
    L, E = len(adjs_np), sum(a.shape[0] for a in adjs_np)
    indeg = np.zeros(V_FB, dtype=np.int64)
    for a in adjs_np:
        np.add.at(indeg, a[:, 1], 1)
    adjs = tuple(torch.from_numpy(a).to(dev) for a in adjs_np)
    gen = torch.Generator().manual_seed(0)
    X = torch.randn((V_FB, D), generator=gen).to(dev)
    dOut = (torch.randn((V_FB, H), generator=gen) * 1e-3).to(dev)
    inp = MessagePassingInput(X, adjs)
    paper = [0.2] + [0.4] * (L - 1)
    print(f"edge_dropout_probe: library with tfgnn_graph_scales_edge_dropout: {'yes' if hasattr(ops, 'graph_scales_edge_dropout') else 'no (the commit before the feature)'}")
    print(f"edge_dropout_probe: V={V_FB} E={E} L={L} D=H={H} mode={args.mode} repeats={args.repeats} largest in-degree {indeg.max()}"
          f"{' rate-0 lines only' if args.rate0_only else ''}")

    def pair(layer):
        out = layer(inp, training=True)
        return out, layer.backward(dOut)

    C = 64 if H == 320 else 16
    wanted = []
    for name, kind, n in ((f"rgcn_blockdiag C={C}", "blockdiag", C), ("rgcn_basis B=8", "basis", 8)):
        wanted.append((name + " rate 0", kind, n, None))
        if not args.rate0_only:
            wanted.append((name + " rates 0.2/0.4", kind, n, paper))
    variants = {}
    for name, kind, n, rates in wanted:
        layer = build_layer(kind, n, D, H, L, rates)
        for _ in range(3):
            pair(layer)
        torch.cuda.synchronize()
        layer._ctx = None
        variants[name] = layer
    times = {n: [] for n in variants}
    for _ in range(args.repeats):
        for name, layer in variants.items():
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            res = pair(layer)
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1))
            del res
            layer._ctx = None
    for name in variants:
        print(line(name + " fwd+bwd", np.array(times[name])))
    if args.rate0_only:
        return
    for kind in (f"rgcn_blockdiag C={C}", "rgcn_basis B=8"):
        a, b = np.median(times[kind + " rate 0"]), np.median(times[kind + " rates 0.2/0.4"])
        print(f"{kind:>34}: dropped step - rate-0 step = {b - a:+.3f} ms")

    # the launch that draws a step's scales, alone: bursts of 50 calls between one pair of events, so that the figure is the
    # kernel back to back and not one launch's latency (its three output tensors come from the caching allocator)
    BURST = 50

    def burst_of(fn):
        def run():
            for _ in range(BURST):
                fn()
        return run

    g = get_graph(adjs, V_FB)
    rates = torch.tensor(paper, dtype=torch.float32, device=dev)
    zeros = torch.zeros(L, dtype=torch.float32, device=dev)
    for normalize, mode, label in ((True, 0, "normalize, sum (the layers' default)"), (True, 1, "normalize, mean"), (False, 0, "raw sum")):
        t = timed(burst_of(lambda: ops.graph_scales_edge_dropout(g, normalize, mode, rates, 7)), args.repeats) / BURST
        print(line(f"scales launch: {label}", t))
    print(line("scales launch: all rates 0", timed(burst_of(lambda: ops.graph_scales_edge_dropout(g, True, 0, zeros, 7)), args.repeats) / BURST))
    print(line("scales launch: one call per event pair", timed(lambda: ops.graph_scales_edge_dropout(g, True, 0, rates, 7), args.repeats)))
    # COMPUTED, not measured: per edge the walk reads the type word (4 B), the edge id (4 B) and the by-source position (4 B) and
    # writes both weights (4 B + 4 B, the second scattered); with the degree normalisation two row pointers per edge (8 B, shared by
    # a bucket's edges, served from cache); mean / sqrt_n read type word and edge id once more for N'; per node 8 B of pointers
    # and 4 B of m_v.  Edges of border-crossing buckets are hashed (type word + edge id) once more.
    model = E * 20 + V_FB * 12
    t = float(np.median(timed(burst_of(lambda: ops.graph_scales_edge_dropout(g, True, 0, rates, 7)), args.repeats))) / BURST
    print(f"bytes model (computed): 20 B/edge + 12 B/node = {model / 1e6:.2f} MB; at the measured {t * 1e3:.1f} us that is "
          f"{model / (t * 1e-3) / 1e9:.0f} GB/s (row pointers: up to {E * 8 / 1e6:.2f} MB more, from cache)")
    print(f"edge dropout launches so far: {ops.edge_dropout_launch_counts()['edge_dropout_scales']}")


if __name__ == "__main__":
    main()
