"""Times ``exclude_batch_positives`` of the mini-batch link-prediction route on the synthetic WN18RR shape of
tools/link_minibatch_probe.py (40 943 entities, 11 relations, 86 835 train triples, tied, self loops: 12 processed types;
``triples_per_batch`` 4096, K = 1), for fanouts [10, 10] and for [-1, -1], where every positive of a batch is drawn.

    python tools/exclude_probe.py [--epochs 7] [--calls 60] [--out FILE]
    python tools/exclude_probe.py --flag-off-only [--root OTHER_CHECKOUT] [--out FILE]

Per fanout row:
  production, flag off / flag on   wall clock per batch of iterating ``get_batches(TRAIN)`` - triple batch, sampler, (the
                                   exclusion,) triple tables; no model - over whole epochs that end in a synchronise,
                                   flag off and flag on alternating.
  sampled_batch, events            the sampler's part of a batch (its read-back included) between device events, plain and
                                   with ``exclude=``, alternating on the same seeds.
  sample_exclude_edges, events     the new call alone - its four launches, nothing read back - on fresh copies of a
                                   sampled batch's lists, with the edges it removed per batch.
``--flag-off-only`` uses nothing but the API of the commit before this feature, so the same file runs on a checkout of that
commit (``--root``: import tf2_gnn_amd from there): flag-off production on both builds in one session says whether the
feature costs anything when it is off.  Per line: median, 10th and 90th percentile in milliseconds and the spread
(p90 - p10) / median.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

V_WN, T_WN, P_WN = 40943, 11, 86835
PER_BATCH, K_NEG = 4096, 1
ROWS = ([10, 10], [-1, -1])


def wn18rr_shaped_edges(seed=0):
    """tools/link_minibatch_probe.py's graph: R-MAT pairs, each given a relation with probability ~ 1 / rank"""
    from tf2_gnn_amd.data import rmat_edges

    rng = np.random.default_rng(seed)
    pairs = rmat_edges(V_WN, P_WN, rng).astype(np.int64)
    p = 1.0 / np.arange(1, T_WN + 1)
    rel = rng.choice(T_WN, size=P_WN, p=p / p.sum())
    rel[:T_WN] = np.arange(T_WN)
    return [pairs[rel == t] for t in range(T_WN)]


def line(name, t):
    t = np.asarray(t, dtype=np.float64)
    med, p10, p90 = np.median(t), np.percentile(t, 10), np.percentile(t, 90)
    return f"{name:>58}: median {med:9.3f} ms  p10 {p10:9.3f}  p90 {p90:9.3f}  spread {(p90 - p10) / med:5.1%}"


def dataset(edges, fanouts, exclude):
    from tf2_gnn_amd.data import LinkPredictionDataset

    params = dict(LinkPredictionDataset.get_default_hyperparameters(), tie_fwd_bkwd_edges=True, num_negatives_per_positive=K_NEG,
                  negative_sampling="device", neighbor_fanouts=list(fanouts), triples_per_batch=PER_BATCH)
    if exclude:
        params["exclude_batch_positives"] = True
    ds = LinkPredictionDataset(params)
    ds.load_data_from_arrays(None, edges, num_nodes=V_WN)
    return ds


def production_epoch(batches):
    """wall clock per batch (ms) of one epoch of batch production, and the edges removed per batch where the flag is on"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, removed = 0, []
    for feats, _ in batches:
        n += 1
        if "excluded_edge_counts" in feats:
            removed.append(feats["excluded_edge_counts"])  # a device tensor: nothing is read here
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / n
    return ms, [int(r.sum()) for r in removed]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=7)
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--flag-off-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=os.path.join("profiles", "exclude_probe.txt"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    if not torch.cuda.is_available():
        sys.exit("exclude_probe: no ROCm device - nothing is measured on a CPU")
    from tf2_gnn_amd.data import DataFold

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    dev = torch.device("cuda", 0)
    edges = wn18rr_shaped_edges()
    own = os.path.abspath(args.root) == os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    say(f"exclude_probe: V={V_WN} T={T_WN} P={P_WN} tied, self loops; triples_per_batch={PER_BATCH} K={K_NEG}; "
        f"{'flag off only, ' if args.flag_off_only else ''}tf2_gnn_amd from {'this tree' if own else os.path.abspath(args.root)}")
    for fanouts in ROWS:
        say(f"--- fanouts {fanouts}")
        off = dataset(edges, fanouts, False).get_batches(DataFold.TRAIN, dev)
        np.random.seed(0)
        production_epoch(off)  # warm-up: the store, buffers, workspaces, every kernel once
        if args.flag_off_only:
            say(line("production per batch, flag off, wall", [production_epoch(off)[0] for _ in range(args.epochs)]))
            continue
        on_ds = dataset(edges, fanouts, True)
        on = on_ds.get_batches(DataFold.TRAIN, dev)
        production_epoch(on)
        t_off, t_on, removed = [], [], []
        for _ in range(args.epochs):
            t_off.append(production_epoch(off)[0])
            ms, r = production_epoch(on)
            t_on.append(ms)
            removed += r[:-1]  # full chunks: one shape of work
        say(line("production per batch, flag off, wall", t_off))
        say(line("production per batch, flag on, wall", t_on))
        say(f"    flag on / flag off = {np.median(t_on) / np.median(t_off):.3f}; edges removed per batch of {PER_BATCH} positives: "
            f"median {int(np.median(removed))}, min {min(removed)}, max {max(removed)}")
        parts(say, on_ds, fanouts, dev, args.calls)
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


def parts(say, ds, fanouts, dev, calls):
    """the sampler's part of a batch with and without the exclusion, and the new call alone, between device events"""
    from tf2_gnn_amd import _lib, ops
    from tf2_gnn_amd.data import DataFold, batch_key, plan_seed_chunks, sampled_batch

    store = ds.neighbor_store(dev)
    positives = torch.from_numpy(ds.positive_triples(DataFold.TRAIN)).to(dev)
    workspace = ops.triple_batch_workspace(V_WN, dev)
    fwd, inv = (t.tolist() for t in ds.exclusion_type_tables())
    chunks = plan_seed_chunks(P_WN, PER_BATCH)[:-1]
    L = ds.num_edge_types
    times = {"plain": [], "exclude": [], "call": []}
    sizes = []
    ids = torch.from_numpy(np.random.permutation(P_WN).astype(np.int32)).to(dev)
    for c in range(calls + 2):
        s, e = chunks[c % len(chunks)]
        _, local, seeds, S, status = ops.triple_batch(positives, ids[s:e], K_NEG, V_WN, c, workspace)
        assert status == 0
        key = batch_key(0, 0, c)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        torch.cuda.synchronize()
        ev[0].record()
        plain, _ = sampled_batch(store, seeds, fanouts, key, seed_only_columns=())
        ev[1].record()
        torch.cuda.synchronize()
        ev[2].record()
        feats, _ = sampled_batch(store, seeds, fanouts, key, seed_only_columns=(), exclude=(local[:e - s], fwd, inv))
        ev[3].record()
        # the call alone, on copies of the plain batch's lists at their own length as capacity
        lists = [plain[f"adjacency_list_{t}"].clone() for t in range(L)]
        meta = torch.zeros(_lib.sample_meta_words(L, len(fanouts)), dtype=torch.int32)
        meta[_lib.SAMPLE_META_EDGES:_lib.SAMPLE_META_EDGES + L] = torch.tensor([a.shape[0] for a in lists], dtype=torch.int32)
        meta = meta.to(dev)
        ws = torch.empty(ops.sample_exclude_workspace_words([a.shape[0] for a in lists]), dtype=torch.int32, device=dev)
        record = torch.empty(L + 1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ev[4].record()
        ops.sample_exclude_edges(lists, meta, S, local[:e - s], fwd, inv, workspace=ws, record=record)
        ev[5].record()
        torch.cuda.synchronize()
        assert torch.equal(record[:L], feats["excluded_edge_counts"]) and int(record[L]) == 0
        if c >= 2:
            times["plain"].append(ev[0].elapsed_time(ev[1]))
            times["exclude"].append(ev[2].elapsed_time(ev[3]))
            times["call"].append(ev[4].elapsed_time(ev[5]))
            sizes.append((S, int(plain["sampled_node_ids"].shape[0]), sum(a.shape[0] for a in lists), int(record[:L].sum())))
    sz = np.asarray(sizes)
    say(f"    {calls} batches; medians: S = {int(np.median(sz[:, 0]))} seeds, n = {int(np.median(sz[:, 1]))} nodes, "
        f"{int(np.median(sz[:, 2]))} sampled edges, {int(np.median(sz[:, 3]))} removed")
    say(line("sampled_batch, events", times["plain"]))
    say(line("sampled_batch with exclude=, events", times["exclude"]))
    say(line("sample_exclude_edges alone (4 launches), events", times["call"]))
    say(f"    launches so far: sampler {ops.sample_launch_counts()}, exclusion {ops.sample_exclude_launch_counts()}")


if __name__ == "__main__":
    main()
