"""Times the row-sparse optimizer step (``optim.RowGradient``, the hyper-parameter ``node_embedding_update="rows"``) against the
dense route on one MI355X, both routes alternating in one process:

    python tools/sparse_update_probe.py [--repeats 20] [--nodes 2400000] [--edges 8000000] [--out profiles/sparse_update_probe.txt]

  (a) the update alone: a table of N = 2 400 000 rows of D = 128 floats, a row gradient of n = 20 000 distinct rows, Adam.
      dense: ``ops.embedding_scatter_rows`` into a dense [N, D] buffer, then ``apply_gradients`` with it (3 launches);
      rows:  ``apply_gradients`` with the ``RowGradient`` (1 launch).  Bursts of ``--burst`` calls between one pair of events.
  (b) the sampled training step of tools/sampler_probe.py's model (RGCN, H = 320, 2 layers, Adam, fanouts [10, 10], 1024 seeds
      per batch) on a featureless R-MAT graph of N nodes with learned embeddings of width D, ``node_embedding_update`` "dense"
      against "rows": ``_run_step(training=True)`` over the same ``--batches`` pre-sampled batches, wall clock ending in a
      synchronise, per step.
Per line: median, 10th and 90th percentile in milliseconds.  The bytes next to the times are COMPUTED from the kernels' accesses,
not measured.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, N_ROWS = 128, 20_000


def line(name, t):
    t = np.asarray(t, dtype=np.float64)
    return f"{name:>58}: median {np.median(t):9.4f} ms  p10 {np.percentile(t, 10):9.4f}  p90 {np.percentile(t, 90):9.4f}"


def alternate(routes, repeats, per, clock):
    """``routes``: name -> callable.  Three warm-up bursts each, then ``repeats`` rounds in which every route runs one burst of
    ``per`` calls; -> name -> [ms per call]"""
    for fn in routes.values():
        for _ in range(3 * per):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in routes}
    for _ in range(repeats):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            if clock == "events":
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(per):
                    fn()
                t1.record()
                torch.cuda.synchronize()
                out[name].append(t0.elapsed_time(t1) / per)
            else:
                w0 = time.perf_counter()
                for _ in range(per):
                    fn()
                torch.cuda.synchronize()
                out[name].append((time.perf_counter() - w0) * 1e3 / per)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--burst", type=int, default=10)
    ap.add_argument("--nodes", type=int, default=2_400_000)
    ap.add_argument("--edges", type=int, default=8_000_000)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=320)
    ap.add_argument("--skip-training", action="store_true", help="part (a) only")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sparse_update_probe: no ROCm device - nothing is measured on a CPU")
    from tf2_gnn_amd import _lib, ops, tasks
    from tf2_gnn_amd.data import DataFold, NodeClassificationDataset, rmat_edges
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.layers.message_passing.message_passing import Variable
    from tf2_gnn_amd.optim import Optimizer, RowGradient

    dev = torch.device("cuda", 0)
    lib = _lib.load()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N = args.nodes
    say(f"sparse_update_probe on {torch.cuda.get_device_name(0)}: N = {N}, D = {D}, repeats = {args.repeats}")

    # ---- (a) ------------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(2)
    rows = torch.from_numpy(rng.standard_normal((N_ROWS, D)).astype(np.float32)).to(dev)
    ids = torch.from_numpy(rng.permutation(N)[:N_ROWS].astype(np.int32)).to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    tables = {name: Variable(name, torch.zeros((N, D), device=dev).normal_(0.0, 0.1)) for name in ("dense", "rows")}
    opts = {name: Optimizer("adam", learning_rate=0.001) for name in tables}
    grad = torch.empty((N, D), device=dev)

    def dense_update():
        ops.embedding_scatter_rows(rows, ids, N, out=grad, bad_flag=flag)
        opts["dense"].apply_gradients([(tables["dense"], grad)])

    def rows_update():
        opts["rows"].apply_gradients([(tables["rows"], RowGradient(rows, ids, N, bad_flag=flag))])

    counts = {}
    for name, fn in (("dense", dense_update), ("rows", rows_update)):
        before = (lib.tfgnn_optimizer_launch_count(), ops.embedding_launch_count())
        fn()
        counts[name] = (lib.tfgnn_optimizer_launch_count() - before[0]) + (ops.embedding_launch_count() - before[1])
    t = alternate({"dense": dense_update, "rows": rows_update}, args.repeats, args.burst, "events")
    table_bytes, rows_bytes = 4 * N * D, 4 * N_ROWS * D
    dense_bytes = (table_bytes + 2 * rows_bytes + 4 * N_ROWS) + 7 * table_bytes  # fill, scatter; Adam: 4 arrays read, 3 written
    sparse_bytes = 7 * rows_bytes + 4 * N_ROWS
    say(f"--- (a) the update alone, Adam, n = {N_ROWS} rows; bursts of {args.burst} calls between events, the routes alternating")
    say(line(f"(a) dense: scatter + dense step, {counts['dense']} launches", t["dense"]))
    say(line(f"(a) rows: RowGradient, {counts['rows']} launch", t["rows"]))
    for name, nbytes in (("dense", dense_bytes), ("rows", sparse_bytes)):
        med = np.median(t[name])
        say(f"    bytes model (computed) {name}: {nbytes / 1e6:.1f} MB; at the measured {med * 1e3:.1f} us that is "
            f"{nbytes / (med * 1e-3) / 1e9:.0f} GB/s")
    say(f"    dense / rows = {np.median(t['dense']) / np.median(t['rows']):.1f}x")
    assert int(flag) == 0 and opts["dense"].iterations == opts["rows"].iterations
    del tables, opts, grad, rows, ids
    torch.cuda.empty_cache()
    if args.skip_training:
        if args.out:
            open(args.out, "w").write("\n".join(lines) + "\n")
        return

    # ---- (b) ------------------------------------------------------------------------------------------------------------------
    rng = np.random.default_rng(0)
    edges = rmat_edges(N, args.edges, rng)
    labels = rng.integers(0, 40, size=N)
    perm = rng.permutation(N)
    params = NodeClassificationDataset.get_default_hyperparameters()
    params.update(neighbor_fanouts=[10, 10], seeds_per_batch=1024)
    ds = NodeClassificationDataset(params)
    ds.load_data_from_arrays(None, labels, [edges], train_idx=perm[:int(0.54 * N)], valid_idx=perm[int(0.54 * N):int(0.72 * N)],
                             test_idx=perm[int(0.72 * N):])
    np.random.seed(1)
    it = iter(ds.get_batches(DataFold.TRAIN, dev))
    batches = [next(it) for _ in range(args.batches)]
    sizes = [int(f["sampled_node_ids"].shape[0]) for f, _ in batches]
    models = {}
    for update in ("dense", "rows"):
        set_seed(1)
        p = tasks.NodeClassificationTask.get_default_hyperparameters("rgcn")
        p.update(gnn_hidden_dim=args.hidden, gnn_num_layers=2, gnn_global_exchange_every_num_layers=10000, optimizer="Adam",
                 learning_rate=0.001, node_embedding_dim=D, node_embedding_update=update)
        model = tasks.NodeClassificationTask(p, dataset=ds)
        model.build({"node_features": (None, 0)})
        models[update] = model

    def epoch(model):
        def run():
            for feats, labs in batches:
                model._run_step(feats, labs, training=True)
        return run

    t = alternate({name: epoch(m) for name, m in models.items()}, args.repeats, 1, "wall")
    say(f"--- (b) sampled training step: R-MAT graph of {N} nodes, {args.edges} forward edges, featureless, embeddings of width {D}; "
        f"RGCN H = {args.hidden}, 2 layers, Adam, fanouts [10, 10], 1024 seeds; {args.batches} pre-sampled batches of "
        f"{min(sizes)} - {max(sizes)} nodes; wall clock over the {args.batches} steps ending in a synchronise, per step")
    for name in ("dense", "rows"):
        say(line(f'(b) node_embedding_update = "{name}"', np.asarray(t[name]) / args.batches))
    d, r = np.median(t["dense"]) / args.batches, np.median(t["rows"]) / args.batches
    say(f"    dense - rows = {d - r:+.3f} ms per step ({d / r:.2f}x)")
    say(f"    bad ids: {[int(m.embedding_bad_index) for m in models.values()]}; the dense model holds a [{N}, {D}] gradient buffer "
        f"({table_bytes / 1e9:.2f} GB), the rows model none: {models['rows']._node_embeddings_grad is None}")
    if args.out:
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
