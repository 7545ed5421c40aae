"""Times mini-batch link prediction (LinkPredictionDataset with ``neighbor_fanouts``) on a synthetic graph of WN18RR's shape:
40 943 entities, 11 relations, 86 835 train triples drawn by data/synthetic.rmat_edges, relations Zipf-distributed;
``tie_fwd_bkwd_edges=True`` and self loops give 12 processed edge types.  Featureless, ``node_embedding_dim`` = 128 updated by
rows, a 2-layer rgcn of width 128, Adam; ``triples_per_batch`` 4096 (22 batches an epoch), fanouts [10, 10], K = 1.

    python tools/link_minibatch_probe.py [--batches 110] [--repeats 5] [--mode f16x2|bf16x3|fp32] [--out FILE]

  (a) per batch, the four parts of a training step as the dataset runs them - ops.triple_batch, sampled_batch,
      ops.build_triple_tables_device, _run_step(training=True) - between device events, over ``--batches`` batches after one
      warm-up epoch.  The first two read sizes back, so their event times include what the device waits for the host.
  (b) the batch preparation - ops.triple_batch, its read-back included - against the numpy restatement
      (tests/triple_batch_reference.py) plus the upload of its three arrays: wall clock around a synchronise, alternating.
  (c) an epoch - run_one_epoch over get_batches(TRAIN) - of 22 mini-batches against the one full-graph batch of the device
      route (``negative_sampling="device"`` without ``neighbor_fanouts``): wall clock around a synchronise, alternating, with
      torch's peak allocated bytes of each epoch (every workspace of the library is a torch allocation).
The last lines name the GEMM mode the run ended in and the library's warnings (a tripped f16x2 spread guard moves products to
the bf16x3 kernels for the rest of the process).
Per line: median, 10th and 90th percentile in milliseconds and the spread (p90 - p10) / median.  No GPU: the script fails, it
measures nothing on a CPU."""
import argparse
import os
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

V_WN, T_WN, P_WN = 40943, 11, 86835
WIDTH, PER_BATCH, FANOUTS, K_NEG = 128, 4096, [10, 10], 1


def wn18rr_shaped_edges(seed=0):
    """one [E_t, 2] array per relation: R-MAT pairs, each given a relation with probability ~ 1 / rank"""
    from tf2_gnn_amd.data import rmat_edges

    rng = np.random.default_rng(seed)
    pairs = rmat_edges(V_WN, P_WN, rng).astype(np.int64)
    p = 1.0 / np.arange(1, T_WN + 1)
    rel = rng.choice(T_WN, size=P_WN, p=p / p.sum())
    rel[:T_WN] = np.arange(T_WN)  # no relation without an edge
    return [pairs[rel == t] for t in range(T_WN)]


def line(name, t):
    t = np.asarray(t, dtype=np.float64)
    med, p10, p90 = np.median(t), np.percentile(t, 10), np.percentile(t, 90)
    return f"{name:>58}: median {med:9.3f} ms  p10 {p10:9.3f}  p90 {p90:9.3f}  spread {(p90 - p10) / med:5.1%}"


def dataset(edges, minibatched):
    from tf2_gnn_amd.data import LinkPredictionDataset

    params = dict(LinkPredictionDataset.get_default_hyperparameters(), tie_fwd_bkwd_edges=True, num_negatives_per_positive=K_NEG,
                  negative_sampling="device")
    if minibatched:
        params.update({"neighbor_fanouts": FANOUTS, "triples_per_batch": PER_BATCH})
    ds = LinkPredictionDataset(params)
    ds.load_data_from_arrays(None, edges, num_nodes=V_WN)
    return ds


def task(ds):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import LinkPredictionTask

    set_seed(1)
    params = LinkPredictionTask.get_default_hyperparameters("rgcn")
    params.update({"gnn_hidden_dim": WIDTH, "gnn_num_layers": 2, "gnn_global_exchange_every_num_layers": 10000,
                   "gnn_layer_input_dropout_rate": 0.0, "optimizer": "Adam", "learning_rate": 0.001,
                   "node_embedding_dim": WIDTH, "node_embedding_update": "rows"})
    model = LinkPredictionTask(params, dataset=ds)
    model.build({"node_features": (None,) + ds.node_feature_shape})
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=110)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mode", default="f16x2")
    ap.add_argument("--out", default=os.path.join("profiles", "link_minibatch_probe.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("link_minibatch_probe: no ROCm device - nothing is measured on a CPU")
    from tests import triple_batch_reference as ref
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import DataFold, batch_key, plan_seed_chunks, sampled_batch

    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    ops.set_gemm_mode(args.mode)
    caught = warnings.catch_warnings(record=True)
    issued = caught.__enter__()  # the spread guard's warnings: reported at the end, they say which products the steps ran on
    warnings.simplefilter("always")
    dev = torch.device("cuda", 0)
    edges = wn18rr_shaped_edges()
    mini, full = dataset(edges, True), dataset(edges, False)
    chunks = plan_seed_chunks(P_WN, PER_BATCH)
    say(f"link_minibatch_probe: V={V_WN} T={T_WN} P={P_WN} types={mini.num_edge_types} rgcn 2 layers H={WIDTH} node_embedding_dim={WIDTH} "
        f"rows; triples_per_batch={PER_BATCH} ({len(chunks)} batches) fanouts={FANOUTS} K={K_NEG} mode={args.mode}")
    model = task(mini)
    train = mini.get_batches(DataFold.TRAIN, dev)
    np.random.seed(0)
    model.run_one_epoch(train, quiet=True, training=True)  # warm-up: stores, buffers, workspaces, every kernel once
    torch.cuda.synchronize()

    # (a) the parts of a step, as LinkPredictionDataset.minibatch runs them
    store = mini.neighbor_store(dev)
    positives = torch.from_numpy(mini.positive_triples(DataFold.TRAIN)).to(dev)
    workspace = ops.triple_batch_workspace(V_WN, dev)
    parts = {"triple_batch": [], "sampled_batch": [], "triple_tables": [], "training step": [], "whole batch": []}
    sizes = []
    done, epoch = 0, 0
    while done < args.batches:
        ids = torch.from_numpy(np.random.permutation(P_WN).astype(np.int32)).to(dev)
        for b, (s, e) in enumerate(chunks[:-1]):  # full chunks: one shape of work
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            torch.cuda.synchronize()
            ev[0].record()
            _, local, seeds, S, status = ops.triple_batch(positives, ids[s:e], K_NEG, V_WN, done, workspace)
            ev[1].record()
            feats, labels = sampled_batch(store, seeds, FANOUTS, batch_key(0, epoch, b), seed_only_columns=())
            ev[2].record()
            n = int(feats["sampled_node_ids"].shape[0])
            tables = ops.build_triple_tables_device(local, n, T_WN)
            ev[3].record()
            N = local.shape[0]
            y = torch.zeros(N, device=dev)
            y[:e - s] = 1.0
            part = {"triples": local, "triple_labels": y, "triple_weights": torch.ones(N, device=dev), "triple_tables": tables}
            feats.update(part)
            labels.update(part)
            model._run_step(feats, labels, training=True)
            ev[4].record()
            torch.cuda.synchronize()
            assert status == 0
            for name, i in zip(parts, range(4)):
                parts[name].append(ev[i].elapsed_time(ev[i + 1]))
            parts["whole batch"].append(ev[0].elapsed_time(ev[4]))
            sizes.append((S, n, sum(int(feats[f"adjacency_list_{t}"].shape[0]) for t in range(mini.num_edge_types))))
            done += 1
            if done >= args.batches:
                break
        epoch += 1
    sz = np.asarray(sizes)
    say(f"--- (a) {done} batches of {PER_BATCH} positives + {PER_BATCH * K_NEG} negatives; medians: S = {int(np.median(sz[:, 0]))} seeds, "
        f"n = {int(np.median(sz[:, 1]))} nodes of {V_WN}, {int(np.median(sz[:, 2]))} sampled edges")
    for name, t in parts.items():
        say(line(f"(a) {name}, events", t))

    # (b) preparation: device call against numpy + upload
    host_pos = mini.positive_triples(DataFold.TRAIN)
    prep = {"device": [], "numpy": []}
    for r in range(max(args.repeats * 4, 20) + 2):
        host_ids = np.random.permutation(P_WN)[:PER_BATCH].astype(np.int32)
        dev_ids = torch.from_numpy(host_ids).to(dev)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ops.triple_batch(positives, dev_ids, K_NEG, V_WN, r, workspace)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        triples, local, seeds, _, _ = ref.build(host_pos, host_ids, K_NEG, V_WN, r, min(4 * PER_BATCH, V_WN))
        uploaded = [torch.from_numpy(a).to(dev) for a in (triples, local, seeds)]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        del uploaded
        if r >= 2:
            prep["device"].append((t1 - t0) * 1e3)
            prep["numpy"].append((t2 - t1) * 1e3)
    say(f"--- (b) preparing one batch of {PER_BATCH} positives, K = {K_NEG}")
    say(line("(b) ops.triple_batch with its read-back, wall", prep["device"]))
    say(line("(b) numpy restatement + upload of 3 arrays, wall", prep["numpy"]))
    say(f"    numpy / device = {np.median(prep['numpy']) / np.median(prep['device']):.2f}x")

    # (c) an epoch of mini-batches against the full-graph batch
    full_model = task(full)
    full_train = full.get_batches(DataFold.TRAIN, dev)
    full_model.run_one_epoch(full_train, quiet=True, training=True)
    torch.cuda.synchronize()
    epochs = {"mini": [], "full": []}
    peak = {"mini": 0, "full": 0}
    for _ in range(args.repeats):
        for name, m, batches in (("mini", model, train), ("full", full_model, full_train)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            m.run_one_epoch(batches, quiet=True, training=True)
            torch.cuda.synchronize()
            epochs[name].append((time.perf_counter() - t0) * 1e3)
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated() - base)
    say(f"--- (c) one epoch over the {P_WN} train triples")
    say(line(f"(c) {len(chunks)} mini-batches ({len(chunks)} optimizer steps), wall", epochs["mini"]))
    say(line("(c) the full-graph batch (1 optimizer step), wall", epochs["full"]))
    mm, fm = np.median(epochs["mini"]), np.median(epochs["full"])
    say(f"    per epoch: mini / full = {mm / fm:.2f}x; per optimizer step: {mm / len(chunks):.3f} ms against {fm:.3f} ms")
    say(f"    torch peak allocated above the epoch's start: mini-batches {peak['mini'] / 2 ** 20:.1f} MiB, full batch {peak['full'] / 2 ** 20:.1f} MiB")
    say(f"launches so far: triple_batch {ops.triple_batch_launch_counts()}, sampler {ops.sample_launch_counts()}, {ops.negatives_launch_counts()}")
    caught.__exit__(None, None, None)
    texts = sorted({str(w.message).split(";")[0][:150] for w in issued if "tf2_gnn_amd" in str(w.message)})
    from tf2_gnn_amd import guard

    mode = {v: k for k, v in guard._GEMM_MODE_NAMES.items()}.get(ops.get_gemm_mode(), "?")
    say(f"GEMM mode at the end: {mode}; library warnings during the run: {len(texts)}")
    for t in texts:
        say(f"    {t}")
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
