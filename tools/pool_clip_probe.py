"""Times the graph readout (tfgnn_pool_forward + tfgnn_pool_backward, softmax weights, both clip bounds set) between device
events and prints one JSON line.  ``--lib FILE`` binds another build of libtfgnn.so (the parent commit's, say) so that two
builds can take turns in alternating processes of one session: profiles/pool_nan_probe.txt.

    python tools/pool_clip_probe.py [--lib path/to/libtfgnn.so]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    from tf2_gnn_amd import _lib

    if args.lib:
        assert _lib._lib is None, "the library is bound on first use: too late to choose another file"
        _lib.LIB_PATH = Path(args.lib).resolve()
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers.nodes_to_graph_representation import segment_offsets

    if not torch.cuda.is_available():
        sys.exit("pool_clip_probe.py needs a ROCm device")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    res = {"lib": str(_lib.LIB_PATH)}
    shapes = (("molecules", rng.integers(9, 30, size=16384), 128, 8), ("large_graphs", rng.integers(2000, 6000, size=64), 128, 8))
    for tag, sizes, GD, heads in shapes:
        ids = torch.from_numpy(np.repeat(np.arange(len(sizes)), sizes).astype(np.int32)).to(dev)
        V, G = int(ids.numel()), len(sizes)
        ptr = segment_offsets(ids, G)
        g = torch.Generator().manual_seed(1)
        T = torch.randn((V, GD), generator=g).to(dev)
        S = torch.randn((V, heads), generator=g).to(dev)
        dOut = torch.randn((G, GD), generator=g).to(dev)

        def step():
            out, w = ops.pool_forward("softmax", ptr, T, S, heads, -0.5, 0.75)
            return ops.pool_backward("softmax", ptr, ids, dOut, T, w, heads, -0.5, 0.75)

        for _ in range(50):
            step()
        torch.cuda.synchronize()
        rounds = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                step()
            e1.record()
            torch.cuda.synchronize()
            rounds.append(e0.elapsed_time(e1) * 1000.0 / args.calls)
        res[tag] = {"V": V, "G": G, "GD": GD, "heads": heads, "us_per_fwd_bwd_median": round(float(np.median(rounds)), 2),
                    "us_min": round(float(min(rounds)), 2), "us_max": round(float(max(rounds)), 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
