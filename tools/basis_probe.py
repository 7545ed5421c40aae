"""Times one message-passing layer, forward + backward, on a synthetic graph of FB15k-237's shape: RGCN_Basis at
num_bases 4, 8 and 30 against RGCN (one [D, H] kernel per edge type), same graph, same inputs, same process.

    python tools/basis_probe.py --hidden 64|320 [--repeats 20] [--mode f16x2|bf16x3|fp32]

The graph: V = 14 541 nodes, 272 115 forward edges over 237 relation types (relation sizes and node popularity both
Zipf-distributed, seeded), backward edges tied to their forward type, self loops as type 0 - L = 238 edge types and
558 771 edges, what LinkPredictionDataset builds with tie_fwd_bkwd_edges=True.  D = H = --hidden.

One width per process, so that a caller can give every timed step a time limit of its own:

    timeout -k 10 300 python tools/basis_probe.py --hidden 64 && timeout -k 10 420 python tools/basis_probe.py --hidden 320

Method: every variant that runs is warmed up 3 rounds; then `repeats` rounds that alternate the variants, each forward +
backward pair bracketed by its own pair of events on the stream, the peak of torch.cuda.max_memory_allocated reset before
and read after each pair (a variant's saved tensors are dropped after its pair: the peak is the variant's own, on top of the
inputs, the weights of all variants and the library's workspaces).  Reported per variant: median, 10th and 90th percentile
in milliseconds, the peak allocation, the parameter count, and the ratio of RGCN's median to the variant's.  A variant that
cannot run (RGCN's [V, L*D] operand may not fit, or its products may refuse the shape) is reported with its error and left
out of the rounds.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V_FB, E_FB, T_FB = 14541, 272115, 237


def fb15k_shaped_graph(seed=0):
    """-> list of L = 238 int32 [E_l, 2] arrays: self loops, then the 237 relations with their backward edges tied"""
    rng = np.random.default_rng(seed)
    rel_p = 1.0 / np.arange(1, T_FB + 1) ** 0.9
    node_p = 1.0 / np.arange(1, V_FB + 1) ** 0.8
    rel = rng.choice(T_FB, size=E_FB, p=rel_p / rel_p.sum())
    perm = rng.permutation(V_FB)
    src = perm[rng.choice(V_FB, size=E_FB, p=node_p / node_p.sum())]
    dst = rng.integers(0, V_FB, size=E_FB)
    loops = np.arange(V_FB)
    adjs = [np.stack([loops, loops], axis=1).astype(np.int32)]
    for t in range(T_FB):
        e = np.stack([src[rel == t], dst[rel == t]], axis=1)
        adjs.append(np.concatenate([e, e[:, ::-1]]).astype(np.int32))
    return adjs


def build_layer(kind, num_bases, D, H, L):
    import tf2_gnn_amd.layers.message_passing as mp

    cls = mp.RGCN if kind == "rgcn" else mp.RGCN_Basis
    p = cls.get_default_hyperparameters()
    p["hidden_dim"] = H
    if kind != "rgcn":
        p["num_bases"] = num_bases
    mp.set_seed(1)
    layer = cls(p)
    layer.build(mp.MessagePassingInput((None, D), tuple((None, 2) for _ in range(L))))
    return layer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, required=True)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--mode", default="f16x2")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("basis_probe: no ROCm device - nothing is measured on a CPU")
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers import MessagePassingInput

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
    indeg = np.bincount(np.concatenate([a[:, 1] for a in adjs_np]), minlength=V_FB)
    print(f"basis_probe: V={V_FB} E={E} L={L} D=H={H} mode={args.mode} repeats={args.repeats}; in-degree max {indeg.max()}, "
          f"{int((indeg > 32).sum())} targets with more than 32 in-edges, {int((indeg > 512).sum())} with more than 512")

    def pair(layer):
        out = layer(inp, training=True)
        return out, layer.backward(dOut)

    variants = {}
    for name, kind, B in (("rgcn_basis B=4", "basis", 4), ("rgcn_basis B=8", "basis", 8), ("rgcn_basis B=30", "basis", 30),
                          ("rgcn", "rgcn", 0)):
        try:
            layer = build_layer(kind, B, D, H, L)
            for _ in range(3):
                pair(layer)
            torch.cuda.synchronize()
            layer._ctx = None
            variants[name] = layer
        except (torch.OutOfMemoryError, RuntimeError, ValueError) as e:  # reported, not timed
            print(f"{name:>16}: did not run: {type(e).__name__}: {str(e).splitlines()[0][:200]}")
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
            layer._ctx = None  # the saved tensors of this pass (RGCN: the [V, L*D] operand) do not count against the next variant
    base = float(np.median(times["rgcn"])) if "rgcn" in times else None
    for name, layer in variants.items():
        t = np.array(times[name])
        med, p10, p90 = np.median(t), np.percentile(t, 10), np.percentile(t, 90)
        params = sum(v.value.numel() for v in layer.trainable_variables)
        ratio = f"  rgcn / this = {base / med:.2f}" if base is not None and name != "rgcn" else ""
        print(f"{name:>16}: fwd+bwd median {med:8.3f} ms  p10 {p10:8.3f}  p90 {p90:8.3f}  spread {(p90 - p10) / med:5.1%}  "
              f"max_memory_allocated {peak[name] / 2 ** 20:9.1f} MiB  parameters {params:>10d}{ratio}")
    c = ops.basis_launch_counts()
    print(f"basis launches so far (forward, dX, dcoeff): {c['basis_fwd']}, {c['basis_dx']}, {c['basis_dcoeff']}")


if __name__ == "__main__":
    main()
