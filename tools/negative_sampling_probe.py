"""Times the per-epoch negative sampling of LinkPredictionDataset on the synthetic graph of FB15k-237's shape that
tools/basis_probe.py uses (V = 14 541, 272 115 positives over 237 relations), host route against device route, at
num_negatives_per_positive K = 1 and K = 4:

    python tools/negative_sampling_probe.py [--repeats 10] [--mode f16x2|bf16x3|fp32] [--skip-epoch]

  (a) the host route's triple_batch(TRAIN) alone - np.random draw, two argsorts, the copies into the device buffers - wall
      clock around a call that ends in a device synchronise;
  (b) the device draw alone and the node-table build alone, bursts of 20 calls between one pair of events;
  (c) one epoch as the user runs it, RGCN_BlockDiag C = 64 at D = H = 320 with 2 layers, Adam, a CapturedStep of
      _run_step(training=True): the host route is `replay(); next(iter(train))`, the device route is `replay()` alone.  Wall
      clock over bursts of 5 epochs that end in a synchronise, the two routes alternating burst by burst in one process.
      (The graph part of the batch is built by hand, once, and `next(iter(train))` is triple_batch(TRAIN) - what an iter()
      does on top of the graph part.  When this probe was written batch assembly took at most 48 edge types and this graph
      has 238; get_batches takes it now - tools/embedding_probe.py goes that way - and the probe stays as measured.)
Per line: median, 10th and 90th percentile in milliseconds and the spread (p90 - p10) / median.  The bytes next to (b) are
COMPUTED from the kernels' accesses, not measured.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.basis_probe import E_FB, T_FB, V_FB, fb15k_shaped_graph  # noqa: E402

WIDTH, BLOCKS, BURST_CALLS, BURST_EPOCHS = 320, 64, 20, 5


def fb15k_shaped_edges(seed=0):
    """the forward edges of tools/basis_probe.py's fb15k_shaped_graph (same generator, same order of draws), one [E_t, 2]
    array per relation"""
    rng = np.random.default_rng(seed)
    rel_p = 1.0 / np.arange(1, T_FB + 1) ** 0.9
    node_p = 1.0 / np.arange(1, V_FB + 1) ** 0.8
    rel = rng.choice(T_FB, size=E_FB, p=rel_p / rel_p.sum())
    perm = rng.permutation(V_FB)
    src = perm[rng.choice(V_FB, size=E_FB, p=node_p / node_p.sum())]
    dst = rng.integers(0, V_FB, size=E_FB)
    return [np.stack([src[rel == t], dst[rel == t]], axis=1).astype(np.int64) for t in range(T_FB)]


def line(name, t):
    t = np.asarray(t, dtype=np.float64)
    med, p10, p90 = np.median(t), np.percentile(t, 10), np.percentile(t, 90)
    return f"{name:>52}: median {med:9.3f} ms  p10 {p10:9.3f}  p90 {p90:9.3f}  spread {(p90 - p10) / med:5.1%}"


def wall_ms(fn, repeats, per=1):
    """milliseconds per unit of `repeats` calls of fn (each `per` units, ending in a synchronise), after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / per)
    return out


def event_ms(fn, repeats, per):
    for _ in range(3):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(per):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) / per)
    return out


def dataset(K, route, feats, edges):
    from tf2_gnn_amd.data import LinkPredictionDataset

    params = dict(LinkPredictionDataset.get_default_hyperparameters(), tie_fwd_bkwd_edges=True, num_negatives_per_positive=K,
                  negative_sampling=route)
    ds = LinkPredictionDataset(params)
    ds.load_data_from_arrays(feats, edges)
    return ds


class _TripleEpochs:
    """Stands in for ds.get_batches(TRAIN) (see the module docstring): the graph
    part of the batch is built once by hand, and every iter() does what the dataset's does on top of it - triple_batch(TRAIN):
    the draw, the tables and, on the host route, the copies."""

    def __init__(self, ds, graph_part, dev):
        self._ds, self._graph_part, self._dev = ds, graph_part, dev

    def __iter__(self):
        from tf2_gnn_amd.data import DataFold

        part = self._ds.triple_batch(DataFold.TRAIN, self._dev)
        labels = {k: v for k, v in part.items() if k != "triple_sampler"}
        features = dict(self._graph_part)
        features.update({k: part[k] for k in ("triples", "triple_labels", "triple_weights", "triple_tables", "triple_sampler") if k in part})
        yield features, labels


def task(ds):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import LinkPredictionTask

    set_seed(1)
    params = LinkPredictionTask.get_default_hyperparameters("rgcn_blockdiag")
    params.update({"gnn_hidden_dim": WIDTH, "gnn_num_layers": 2, "gnn_num_blocks": BLOCKS, "gnn_global_exchange_every_num_layers": 10000,
                   "gnn_layer_input_dropout_rate": 0.0, "optimizer": "Adam", "learning_rate": 0.001})
    model = LinkPredictionTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--mode", default="f16x2")
    ap.add_argument("--skip-epoch", action="store_true", help="parts (a) and (b) only")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("negative_sampling_probe: no ROCm device - nothing is measured on a CPU")
    from tf2_gnn_amd import CapturedStep, ops
    from tf2_gnn_amd.data import DataFold

    ops.set_gemm_mode(args.mode)
    dev = torch.device("cuda", 0)
    edges = fb15k_shaped_edges()
    feats = (0.1 * np.random.default_rng(1).standard_normal((V_FB, WIDTH))).astype(np.float32)
    graph_part = {"node_features": torch.from_numpy(feats).to(dev), "node_to_graph_map": torch.zeros(V_FB, dtype=torch.int32, device=dev),
                  "num_graphs_in_batch": 1}
    for i, a in enumerate(fb15k_shaped_graph()):  # self loops, then the 237 relations with their backward edges tied
        graph_part[f"adjacency_list_{i}"] = torch.from_numpy(a).to(dev)
    print(f"negative_sampling_probe: V={V_FB} P={E_FB} T={T_FB} D=H={WIDTH} rgcn_blockdiag C={BLOCKS} mode={args.mode} repeats={args.repeats}")
    for K in (1, 4):
        N = E_FB * (1 + K)
        print(f"--- K = {K}: N = {N} triples, {2 * N} node entries")
        host, device = dataset(K, "host", feats, edges), dataset(K, "device", feats, edges)
        np.random.seed(0)
        host.triple_batch(DataFold.TRAIN, dev)
        buffers = device.triple_batch(DataFold.TRAIN, dev)
        sampler = buffers["triple_sampler"]
        # (a)
        a = wall_ms(lambda: host.triple_batch(DataFold.TRAIN, dev), args.repeats)
        print(line("(a) host triple_batch(TRAIN), wall", a))
        # (b)
        triples, tables, ws = buffers["triples"], buffers["triple_tables"], sampler.workspace
        draw = event_ms(lambda: ops.draw_negative_triples(triples, E_FB, V_FB, 7), args.repeats, BURST_CALLS)
        build = event_ms(lambda: ops.build_triple_tables_device(triples, V_FB, T_FB, out=tables, rel=False, workspace=ws),
                         args.repeats, BURST_CALLS)
        both = event_ms(sampler.redraw, args.repeats, BURST_CALLS)
        print(line("(b) device draw, events", draw))
        print(line("(b) device node tables, events", build))
        print(line("(b) sampler.redraw() = draw + node tables, events", both))
        # COMPUTED, not measured.  Draw: per negative 12 B of its positive read (K negatives share a row: from cache after the
        # first) and 12 B written.  Node tables, n = 2 N keys, p passes: the first histogram and scatter read the node word of an
        # entry out of the triples (4 B of a 12 B row, both passes: the rows stream through once per pass = 12 N B each), later
        # passes read keys (4 n) for the histogram and keys + payloads (8 n) for the scatter; every scatter writes 8 n; the row
        # pointers read ~log2(n) words per node, from cache.  The [512][tiles] table is left out (tiles^2 * 2 KiB of L2 reads).
        p, n = ops.triple_table_passes(V_FB), 2 * N
        draw_bytes = E_FB * 12 + E_FB * K * 12
        build_bytes = 2 * 12 * N + (p - 1) * (4 * n + 8 * n) + p * 8 * n + 4 * (V_FB + 1)
        for name, nbytes, t in (("draw", draw_bytes, np.median(draw)), ("node tables", build_bytes, np.median(build))):
            print(f"    bytes model (computed) {name}: {nbytes / 1e6:.2f} MB; at the measured {t * 1e3:.1f} us that is {nbytes / (t * 1e-3) / 1e9:.0f} GB/s")
        uploaded = 12 * N + 4 * (V_FB + 1 + 2 * N + T_FB + 1 + N)
        print(f"    the host route uploads (computed) {uploaded / 1e6:.2f} MB per epoch: triples and the four tables")
        if args.skip_epoch:
            continue
        # (c)
        steps = {}
        for route, ds in (("host", host), ("device", device)):
            batches = _TripleEpochs(ds, graph_part, dev)
            features, labels = next(iter(batches))
            model = task(ds)
            cap = CapturedStep(lambda model=model, features=features, labels=labels: model._run_step(features, labels, training=True)["loss"])
            cap.capture()
            steps[route] = (cap, batches)

        def host_epochs():
            cap, batches = steps["host"]
            for _ in range(BURST_EPOCHS):
                cap.replay()
                next(iter(batches))

        def device_epochs():
            cap, _ = steps["device"]
            for _ in range(BURST_EPOCHS):
                cap.replay()

        def replay_only():  # the host route's step without its host part: what the device route adds to the replay
            cap, _ = steps["host"]
            for _ in range(BURST_EPOCHS):
                cap.replay()

        times = {"host": [], "device": [], "replay": []}
        for fn in (host_epochs, device_epochs, replay_only):
            fn()
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for name, fn in (("host", host_epochs), ("device", device_epochs), ("replay", replay_only)):
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3 / BURST_EPOCHS)
        print(line("(c) host route: replay(); next(iter(train)), wall", times["host"]))
        print(line("(c) device route: replay(), wall", times["device"]))
        print(line("    host route's replay() alone (stale negatives), wall", times["replay"]))
        h, d = np.median(times["host"]), np.median(times["device"])
        print(f"    per epoch: host / device = {h / d:.2f}x ({h - d:+.3f} ms); guard tripped: {steps['device'][0].guard_tripped()}")
        del steps
    print(f"launches so far: {ops.negatives_launch_counts()}")


if __name__ == "__main__":
    main()
