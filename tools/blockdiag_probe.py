"""Times one message-passing layer, forward + backward, on a synthetic graph of FB15k-237's shape: RGCN_BlockDiag at two block
counts against RGCN_Basis at 8 bases and, at D = 64, RGCN - same graph, same inputs, same process.

    python tools/blockdiag_probe.py --hidden 64|320 [--repeats 20] [--mode f16x2|bf16x3|fp32]

The graph is tools/basis_probe.py's: V = 14 541, L = 238 edge types, E = 558 771.  D = H = --hidden; block counts 16 and 4 at 64,
64 (the paper's 5 x 5 blocks) and 8 at 320.  One width per process, so that a caller can give every timed step a time limit of
its own:

    timeout -k 10 300 python tools/blockdiag_probe.py --hidden 64 && timeout -k 10 420 python tools/blockdiag_probe.py --hidden 320

Method, as basis_probe: 3 warm-up rounds per variant, then `repeats` rounds that alternate the variants, each forward + backward
pair bracketed by its own pair of events, the allocation peak reset before and read after each pair, a variant's saved tensors
dropped after its pair.  Reported per variant: median, 10th and 90th percentile in milliseconds, the peak allocation, the
parameter count.  Then, for every block-diagonal variant, its three calls and the two activation passes on their own (same
method, `repeats` rounds each): where the pair's time goes, and the activation passes' share of it.  No GPU: the script fails."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.basis_probe import V_FB, fb15k_shaped_graph  # noqa: E402


def build_layer(kind, n, D, H, L):
    import tf2_gnn_amd.layers.message_passing as mp

    cls = {"rgcn": mp.RGCN, "basis": mp.RGCN_Basis, "blockdiag": mp.RGCN_BlockDiag}[kind]
    p = cls.get_default_hyperparameters()
    p["hidden_dim"] = H
    if kind == "basis":
        p["num_bases"] = n
    if kind == "blockdiag":
        p["num_blocks"] = n
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, required=True)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--mode", default="f16x2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("blockdiag_probe: no ROCm device - nothing is measured on a CPU")
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers import MessagePassingInput
    from tf2_gnn_amd.layers.graph_scales import graph_scales
    from tf2_gnn_amd.layers.message_passing import get_graph

    ops.set_gemm_mode(args.mode)
    dev = torch.device("cuda", 0)
    D = H = args.hidden
    adjs_np = fb15k_shaped_graph()
    L, E = len(adjs_np), sum(a.shape[0] for a in adjs_np)
    adjs = tuple(torch.from_numpy(a).to(dev) for a in adjs_np)
    gen = torch.Generator().manual_seed(0)
    X = torch.randn((V_FB, D), generator=gen).to(dev)
    dOut = (torch.randn((V_FB, H), generator=gen) * 1e-3).to(dev)
    inp = MessagePassingInput(X, adjs)
    print(f"blockdiag_probe: V={V_FB} E={E} L={L} D=H={H} mode={args.mode} repeats={args.repeats}")

    def pair(layer):
        out = layer(inp, training=True)
        return out, layer.backward(dOut)

    blocks = (64, 8) if H == 320 else (16, 4)
    wanted = [(f"rgcn_blockdiag C={c}", "blockdiag", c) for c in blocks] + [("rgcn_basis B=8", "basis", 8)]
    if H <= 64:
        wanted.append(("rgcn", "rgcn", 0))
    variants = {}
    for name, kind, n in wanted:
        try:
            layer = build_layer(kind, n, D, H, L)
            for _ in range(3):
                pair(layer)
            torch.cuda.synchronize()
            layer._ctx = None
            variants[name] = layer
        except (torch.OutOfMemoryError, RuntimeError, ValueError) as e:  # reported, not timed
            print(f"{name:>20}: did not run: {type(e).__name__}: {str(e).splitlines()[0][:200]}")
            layer = None
            torch.cuda.empty_cache()
    times = {n: [] for n in variants}
    peak = {n: 0 for n in variants}
    for _ in range(args.repeats):
        for name, layer in variants.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            res = pair(layer)
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1))
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated())
            del res
            layer._ctx = None  # the saved tensors of this pass do not count against the next variant
    base = float(np.median(times["rgcn_basis B=8"])) if "rgcn_basis B=8" in times else None
    for name, layer in variants.items():
        t = np.array(times[name])
        med, p10, p90 = np.median(t), np.percentile(t, 10), np.percentile(t, 90)
        params = sum(v.value.numel() for v in layer.trainable_variables)
        ratio = f"  basis B=8 / this = {base / med:.2f}" if base is not None and name != "rgcn_basis B=8" else ""
        print(f"{name:>20}: fwd+bwd median {med:8.3f} ms  p10 {p10:8.3f}  p90 {p90:8.3f}  spread {(p90 - p10) / med:5.1%}  "
              f"max_memory_allocated {peak[name] / 2 ** 20:9.1f} MiB  parameters {params:>10d}{ratio}")

    # where a block-diagonal pair's time goes: its three calls and the two activation passes, each on its own
    g = get_graph(adjs, V_FB)
    sc = graph_scales(g, True, "sum")
    kw = dict(edge_weight_by_dst=sc.edge_weight_by_dst, edge_weight_by_src=sc.edge_weight_by_src, node_scale=sc.node_scale)
    for name, layer in variants.items():
        if not name.startswith("rgcn_blockdiag"):
            continue
        qb, C = layer._qb, layer._num_blocks
        pre = ops.blockdiag_forward(g, qb, X, C, edge_weight=sc.edge_weight_by_dst, node_scale=sc.node_scale)
        act = layer._activation_name
        out = ops.activation_forward(act, pre)
        parts = {
            "forward": lambda: ops.blockdiag_forward(g, qb, X, C, edge_weight=sc.edge_weight_by_dst, node_scale=sc.node_scale, out=pre),
            "dX": lambda: ops.blockdiag_backward(g, qb, dOut, None, C, want_dq=False, **kw),
            "dQb": lambda: ops.blockdiag_backward(g, qb, dOut, X, C, want_dx=False, **kw),
            f"activation ({act}) fwd+bwd": lambda: (ops.activation_forward(act, pre), ops.activation_backward(act, dOut, out)),
        }
        med = {k: float(np.median(timed(fn, args.repeats))) for k, fn in parts.items()}
        whole = float(np.median(times[name]))
        print(f"{name:>20}: " + "  ".join(f"{k} {v:.3f} ms" for k, v in med.items())
              + f"  (activation share of the pair: {med[f'activation ({act}) fwd+bwd'] / whole:.1%})")
    c, b = ops.blockdiag_launch_counts(), ops.basis_launch_counts()
    print(f"blockdiag launches so far (fwd, dx, dq): {c['fwd']}, {c['dx']}, {c['dq']}; "
          f"basis launches (forward, dX, dcoeff): {b['basis_fwd']}, {b['basis_dx']}, {b['basis_dcoeff']}")


if __name__ == "__main__":
    main()
