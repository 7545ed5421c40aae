"""Times learned node embeddings (the hyper-parameter ``node_embedding_dim``) on the synthetic graph of FB15k-237's shape that
tools/basis_probe.py uses (V = 14 541, 272 115 positives over 237 relations, backward edges tied, self loops: 238 processed
edge types), every batch built through ``LinkPredictionDataset.get_batches`` - five tfgnn_batch_assemble calls at 238 types:

    python tools/embedding_probe.py [--repeats 10] [--mode f16x2|bf16x3|fp32] [--skip-epoch] [--skip-large]

  (a) the five tfgnn_batch_assemble calls of one batch, bursts of 20 ``assemble_batch`` calls between one pair of events: the
      feature-fed dataset with its outputs handed in (no allocation; the 14 541 x 320 feature rows are copied), and the
      featureless dataset as ``get_batches`` calls it (two allocations, a placeholder column instead of the features);
  (b) ``ops.embedding_scatter_rows`` alone, D = 128, bursts of 20 between events: N = 14 541 with n = 14 541 (n cannot exceed N:
      the ids are distinct) and N = 2 400 000 with n = 20 000;
  (c) one epoch as a ``replay()`` of a CapturedStep of ``_run_step(training=True)``: RGCN_BlockDiag C = 64 at width 320, 2
      layers, Adam, device negatives with K = 1 - the setting of tools/negative_sampling_probe.py (c) - for a model with learned
      embeddings of width 320 on the featureless dataset and for a twin fed fixed features of width 320.  Wall clock over
      bursts of 5 replays that end in a synchronise, the two models alternating burst by burst in one process.
Per line: median, 10th and 90th percentile in milliseconds and the spread (p90 - p10) / median.  The bytes next to (b) and (c)
are COMPUTED from the kernels' accesses, not measured.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.basis_probe import E_FB, T_FB, V_FB  # noqa: E402
from tools.negative_sampling_probe import event_ms, fb15k_shaped_edges, line  # noqa: E402

WIDTH, BLOCKS, BURST_CALLS, BURST_EPOCHS, SCATTER_D = 320, 64, 20, 5, 128


def dataset(feats, edges):
    from tf2_gnn_amd.data import LinkPredictionDataset

    params = dict(LinkPredictionDataset.get_default_hyperparameters(), tie_fwd_bkwd_edges=True, num_negatives_per_positive=1,
                  negative_sampling="device")
    ds = LinkPredictionDataset(params)
    ds.load_data_from_arrays(feats, edges, num_nodes=V_FB)
    return ds


def task(ds, embeddings):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import LinkPredictionTask

    set_seed(1)
    params = LinkPredictionTask.get_default_hyperparameters("rgcn_blockdiag")
    params.update({"gnn_hidden_dim": WIDTH, "gnn_num_layers": 2, "gnn_num_blocks": BLOCKS, "gnn_global_exchange_every_num_layers": 10000,
                   "gnn_layer_input_dropout_rate": 0.0, "optimizer": "Adam", "learning_rate": 0.001})
    if embeddings:
        params["node_embedding_dim"] = WIDTH
    model = LinkPredictionTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--mode", default="f16x2")
    ap.add_argument("--skip-epoch", action="store_true", help="parts (a) and (b) only")
    ap.add_argument("--skip-large", action="store_true", help="leave out the 2 400 000-row table of part (b) (1.2 GB)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("embedding_probe: no ROCm device - nothing is measured on a CPU")
    from tf2_gnn_amd import CapturedStep, ops
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.data.graph_dataset import assemble_batch, batch_assemble_launch_counts

    ops.set_gemm_mode(args.mode)
    dev = torch.device("cuda", 0)
    edges = fb15k_shaped_edges()
    feats = (0.1 * np.random.default_rng(1).standard_normal((V_FB, WIDTH))).astype(np.float32)
    fed, featureless = dataset(feats, edges), dataset(None, edges)
    L = fed.num_edge_types
    print(f"embedding_probe: V={V_FB} P={E_FB} T={T_FB} L={L} width={WIDTH} rgcn_blockdiag C={BLOCKS} K=1 mode={args.mode} "
          f"repeats={args.repeats}")
    assert featureless.num_edge_types == L and featureless.node_feature_shape == (0,) and featureless.num_nodes == V_FB

    # (a)
    plan = fed.plan_epoch(DataFold.TRAIN, dev)
    before = batch_assemble_launch_counts()
    features, labels = assemble_batch(plan, 0, 1)
    calls = batch_assemble_launch_counts() - before
    out = {k: v for k, v in features.items() if isinstance(v, torch.Tensor) and k != "_bad_local_index"}
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    a_fed = event_ms(lambda: assemble_batch(plan, 0, 1, out=out, bad_flag=flag), args.repeats, BURST_CALLS)
    plan0 = featureless.plan_epoch(DataFold.TRAIN, dev)
    a_less = event_ms(lambda: assemble_batch(plan0, 0, 1, bad_flag=flag), args.repeats, BURST_CALLS)
    E = sum(int(features[f"adjacency_list_{t}"].shape[0]) for t in range(L))
    print(f"--- (a) batch assembly: {L} edge types = {calls} tfgnn_batch_assemble launches per batch, {E} edges")
    print(line("(a) fed, outputs handed in, events", a_fed))
    print(line("(a) featureless, as get_batches calls it, events", a_less))
    # COMPUTED, not measured: an edge is 8 B read and 8 B written, a feature row 4 F B read and written, a map entry 4 B
    edge_bytes, row_bytes = 16 * E, V_FB * (8 * WIDTH + 4)
    for name, nbytes, t in (("fed", edge_bytes + row_bytes, np.median(a_fed)), ("featureless", edge_bytes + 12 * V_FB, np.median(a_less))):
        print(f"    bytes model (computed) {name}: {nbytes / 1e6:.2f} MB; at the measured {t * 1e3:.1f} us that is {nbytes / (t * 1e-3) / 1e9:.0f} GB/s")
    assert int(flag) == 0

    # (b)
    print(f"--- (b) ops.embedding_scatter_rows, D = {SCATTER_D}")
    rng = np.random.default_rng(2)
    for N, n in ((V_FB, V_FB),) + (() if args.skip_large else ((2_400_000, 20_000),)):
        rows = torch.from_numpy(rng.standard_normal((n, SCATTER_D)).astype(np.float32)).to(dev)
        ids = torch.from_numpy(rng.permutation(N)[:n].astype(np.int32)).to(dev)
        grad = torch.empty((N, SCATTER_D), dtype=torch.float32, device=dev)
        t = event_ms(lambda: ops.embedding_scatter_rows(rows, ids, N, out=grad, bad_flag=flag), args.repeats, BURST_CALLS)
        print(line(f"(b) N = {N}, n = {n}, events", t))
        nbytes = 4 * SCATTER_D * (N + 2 * n) + 4 * n  # the fill writes N rows; the scatter reads and writes n rows and reads n ids
        print(f"    bytes model (computed): {nbytes / 1e6:.2f} MB; at the measured {np.median(t) * 1e3:.1f} us that is "
              f"{nbytes / (np.median(t) * 1e-3) / 1e9:.0f} GB/s")
        del rows, ids, grad
    assert int(flag) == 0
    if args.skip_epoch:
        return

    # (c)
    steps = {}
    for name, ds, embeddings in (("embeddings", featureless, True), ("fed", fed, False)):
        features, labels = next(iter(ds.get_batches(DataFold.TRAIN, dev)))
        model = task(ds, embeddings)
        cap = CapturedStep(lambda model=model, features=features, labels=labels: model._run_step(features, labels, training=True)["loss"])
        cap.capture()
        steps[name] = (cap, model)

    def epochs(name):
        cap, _ = steps[name]
        for _ in range(BURST_EPOCHS):
            cap.replay()

    times = {"embeddings": [], "fed": []}
    for name in times:
        epochs(name)
    torch.cuda.synchronize()
    for _ in range(args.repeats):
        for name in times:
            t0 = time.perf_counter()
            epochs(name)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / BURST_EPOCHS)
    print(f"--- (c) one epoch = one replay(), bursts of {BURST_EPOCHS}, wall clock ending in a synchronise")
    print(line("(c) learned embeddings [14541, 320], featureless", times["embeddings"]))
    print(line("(c) twin fed fixed features of width 320", times["fed"]))
    e, f = np.median(times["embeddings"]), np.median(times["fed"])
    table = 4 * V_FB * WIDTH
    # COMPUTED, not measured: Adam reads value, gradient and two moments and writes value and two moments (7 arrays); the
    # projection's input-gradient product reads d_pre [V, 320] and writes dX [V, 320] (the 320 x 320 weight is cache-resident)
    print(f"    embeddings - fed = {e - f:+.3f} ms per epoch ({e / f:.3f}x).  Bytes model (computed): the dense Adam step over the table "
          f"moves 7 x {table / 1e6:.2f} = {7 * table / 1e6:.1f} MB, the input-gradient product of the projection 2 x {table / 1e6:.2f} "
          f"MB and 2 x 14541 x 320 x 320 = {2 * V_FB * WIDTH * WIDTH / 1e9:.2f} GFLOP")
    print(f"    guard tripped: {steps['embeddings'][0].guard_tripped()}; losses after the bursts: "
          f"embeddings {float(steps['embeddings'][0].replay()):.4f}, fed {float(steps['fed'][0].replay()):.4f}")
    print(f"launches so far: batch assembly {batch_assemble_launch_counts()}, embedding scatter {ops.embedding_launch_count()}")


if __name__ == "__main__":
    main()
