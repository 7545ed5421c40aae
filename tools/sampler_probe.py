"""Neighbour-sampled batches of an ogbn-arxiv-shaped R-MAT graph (169 343 nodes, 1 166 243 forward edges -> self loops,
forward and backward: 3 processed types; F = 128, 40 classes, 54 % of the nodes in the training fold).

Part 1 - batch production, batches per second, for several seed counts S at ``--fanouts``:
  device   data.sampled_batch: tfgnn_neighbor_sample (3 + 6 K launches), one read-back of the counts, tfgnn_gather_node_rows
  host     the only other route there is: a numpy sampler on the host (per hop and type: the frontier's in-edge ranges, a
           random key per candidate edge and the f smallest per row by one sort, np.unique for the new nodes), the rows
           gathered on the host, and one upload per tensor of the batch
Both end in a device synchronise per batch (a batch is consumed before the next one is made).  The host sampler draws with
numpy's generator, not with the library's keyed positions: the same distribution, other draws.

Part 2 - training: one epoch of sampled steps (seeds_per_batch = 1024) of an RGCN NodeClassificationTask next to the
full-batch step on the same graph: time per epoch and per step.

``--warmup`` repeats are discarded, ``--repeats`` measured; median, minimum and maximum are printed.

    python tools/sampler_probe.py [--fanouts 10 10] [--hidden 320] [--layers 2] [--out profiles/sampler_probe.txt]
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tf2_gnn_amd import tasks  # noqa: E402
from tf2_gnn_amd.data import DataFold, NodeClassificationDataset, batch_key, rmat_edges, sampled_batch  # noqa: E402

V_ARXIV, E_ARXIV, F_ARXIV, C_ARXIV = 169343, 1166243, 128, 40


def arxiv_shaped(seed=0, num_nodes=V_ARXIV, num_edges=E_ARXIV):
    rng = np.random.default_rng(seed)
    edges = rmat_edges(num_nodes, num_edges, rng)
    feats = rng.standard_normal((num_nodes, F_ARXIV), dtype=np.float32)
    labels = rng.integers(0, C_ARXIV, size=num_nodes)
    perm = rng.permutation(num_nodes)
    a, b = int(0.54 * num_nodes), int(0.72 * num_nodes)
    return feats, labels, [edges], {"train_idx": perm[:a], "valid_idx": perm[a:b], "test_idx": perm[b:]}


def host_sampled_batch(store, seeds: np.ndarray, fanouts, rng, weights: np.ndarray, device):
    """The numpy route: sample on the host from the store's host in-CSR, gather the rows, upload the batch."""
    V = store.num_nodes
    local = np.full(V, -1, dtype=np.int64)
    nodes = [seeds.astype(np.int64)]
    local[seeds] = np.arange(len(seeds))
    n = len(seeds)
    frontier = nodes[0]
    per_type = [[] for _ in range(store.num_edge_types)]
    for f in fanouts:
        found = []
        for t in range(store.num_edge_types):
            ptr, src = store.in_ptr_host[t], store.in_src_host[t]
            first = ptr[frontier].astype(np.int64)
            deg = ptr[frontier + 1].astype(np.int64) - first
            row = np.repeat(np.arange(len(frontier)), deg)
            within = np.arange(int(deg.sum())) - np.repeat(np.cumsum(deg) - deg, deg)
            if f >= 0:
                keys = rng.random(len(row))
                keys[np.repeat(deg <= f, deg)] = 0.0  # short rows are taken whole
                order = np.lexsort((keys, row))
                rank = np.arange(len(row)) - np.repeat(np.cumsum(deg) - deg, deg)
                keep = order[rank < f]
                keep.sort()
                row, within = row[keep], within[keep]
            s = src[first[row] + within].astype(np.int64)
            per_type[t].append((s, frontier[row]))
            found.append(s)
        new = np.unique(np.concatenate(found)) if found else np.zeros(0, dtype=np.int64)
        new = new[local[new] < 0]
        local[new] = n + np.arange(len(new))
        n += len(new)
        nodes.append(new)
        frontier = new
    ids = np.concatenate(nodes)
    feats = {"node_features": torch.from_numpy(store.fold.features[ids]).to(device),
             "node_to_graph_map": torch.zeros(n, dtype=torch.int32, device=device), "num_graphs_in_batch": 1, "num_seed_nodes": len(seeds)}
    for t, parts in enumerate(per_type):
        s = np.concatenate([p[0] for p in parts])
        d = np.concatenate([p[1] for p in parts])
        feats[f"adjacency_list_{t}"] = torch.from_numpy(np.stack([local[s], local[d]], axis=1).astype(np.int32)).to(device)
    w = np.zeros((n, 1), dtype=np.float32)
    w[:len(seeds), 0] = weights[seeds]
    labels = {"node_labels": torch.from_numpy(store.fold.node_columns["node_labels"][ids]).to(device),
              "node_label_weights": torch.from_numpy(w).to(device)}
    return feats, labels


def spread(xs):
    return f"median {statistics.median(xs):10.3f}  min {min(xs):10.3f}  max {max(xs):10.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fanouts", type=int, nargs="+", default=[10, 10])
    ap.add_argument("--seeds", type=int, nargs="+", default=[64, 256, 1024, 4096])
    ap.add_argument("--batches", type=int, default=20, help="batches per timed repeat of part 1")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hidden", type=int, default=320)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--nodes", type=int, default=V_ARXIV)
    ap.add_argument("--edges", type=int, default=E_ARXIV)
    ap.add_argument("--skip-training", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampler_probe needs a ROCm device: a timing taken anywhere else says nothing")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    feats, labels, edges, idx = arxiv_shaped(num_nodes=args.nodes, num_edges=args.edges)
    params = NodeClassificationDataset.get_default_hyperparameters()
    params.update(neighbor_fanouts=args.fanouts, seeds_per_batch=1024)
    ds = NodeClassificationDataset(params)
    t0 = time.perf_counter()
    ds.load_data_from_arrays(feats, labels, edges, **idx)
    store = ds.neighbor_store(DataFold.TRAIN, dev)
    torch.cuda.synchronize()
    say(f"sampler_probe on {torch.cuda.get_device_name(0)}")
    say(f"R-MAT graph: {args.nodes} nodes, {args.edges} forward edges, {store.num_edge_types} processed types, "
        f"largest in-degrees {store.max_in_degree}, F = {F_ARXIV}; fanouts {args.fanouts}; "
        f"{args.warmup} warm-up + {args.repeats} measured repeats of {args.batches} batches")
    say(f"  pack, in-CSR and upload, once: {1e3 * (time.perf_counter() - t0):.1f} ms")

    # ---- part 1: batches per second ------------------------------------------------------------------------------------------
    rng = np.random.default_rng(1)
    weights = ds.packed_fold(DataFold.TRAIN).node_columns["node_label_weights"][:, 0]
    train = idx["train_idx"]
    for S in args.seeds:
        chunks = [train[rng.permutation(len(train))[:S]] for _ in range(args.batches)]
        dev_chunks = [torch.from_numpy(c.astype(np.int32)).to(dev) for c in chunks]
        rates = {"device": [], "host": []}
        sizes = None
        for rep in range(args.warmup + args.repeats):
            for route in ("device", "host"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for b in range(args.batches):
                    if route == "device":
                        f, _ = sampled_batch(store, dev_chunks[b], args.fanouts, batch_key(0, rep, b))
                    else:
                        f, _ = host_sampled_batch(store, chunks[b], args.fanouts, rng, weights, dev)
                    torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep >= args.warmup:
                    rates[route].append(args.batches / dt)
                if route == "device":
                    sizes = (int(f["node_features"].shape[0]), sum(int(f[f"adjacency_list_{t}"].shape[0]) for t in range(store.num_edge_types)))
        say(f"S = {S:5d} (last batch: {sizes[0]} nodes, {sizes[1]} edges)")
        say(f"  device sampler  batches/s: {spread(rates['device'])}")
        say(f"  host sampler    batches/s: {spread(rates['host'])}")
        md, mh = statistics.median(rates["device"]), statistics.median(rates["host"])
        verdict = "beats" if min(rates["device"]) > max(rates["host"]) else ("does NOT beat" if md <= mh else "is ahead in the median only of")
        say(f"  the device sampler {verdict} the host route ({md / mh:.2f}x in the median)")

    # ---- part 2: training ----------------------------------------------------------------------------------------------------
    if not args.skip_training:
        p = tasks.NodeClassificationTask.get_default_hyperparameters("rgcn")
        p.update(gnn_hidden_dim=args.hidden, gnn_num_layers=args.layers, gnn_global_exchange_every_num_layers=10000,
                 optimizer="Adam", learning_rate=0.001)
        full_params = NodeClassificationDataset.get_default_hyperparameters()
        full = NodeClassificationDataset(full_params)
        full.load_data_from_arrays(feats, labels, edges, **idx)
        for name, dataset in (("sampled", ds), ("full-batch", full)):
            model = tasks.NodeClassificationTask(p, dataset=dataset)
            model.build({"node_features": (None, F_ARXIV)})
            batches = dataset.get_batches(DataFold.TRAIN, dev)
            epochs, steps = [], 0
            reps = args.warmup + (args.repeats if name == "full-batch" else max(2, args.repeats // 3))
            for rep in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _, _, results = model.run_one_epoch(batches, quiet=True, training=True)
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    epochs.append(1e3 * (time.perf_counter() - t0))
                steps = len(results)
            say(f"training, {name}: RGCN H = {args.hidden}, {args.layers} layers, Adam; {steps} step(s) per epoch over {len(train)} training nodes")
            say(f"  epoch ms: {spread(epochs)};  step ms (median epoch / steps): {statistics.median(epochs) / steps:.3f}")
    if args.out:
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
