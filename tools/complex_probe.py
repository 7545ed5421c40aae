"""Times the three link-prediction decoder calls - ce_metrics, backward (both gradients), rank (both sides, filtered) - for the
DistMult and the ComplEx decoder on the synthetic graph of FB15k-237's shape the other link probes use (V = 14 541, T = 237,
272 115 positives; tools/negative_sampling_probe.py's generator), at K = 1 and K = 4 negatives per positive and at D = 320 and
D = 128:

    python tools/complex_probe.py [--repeats 12] [--decoders distmult,complex] [--tree CHECKOUT] [--label TEXT]

Op level: H and R are random fp32 arrays, the negatives corrupt one end of a positive, the tables come from
ops.build_triple_tables.  The "test fold" is 20 466 further triples (FB15k-237's test-fold size) from the same generator with
another seed; a query's filter is every entity that completes its (u, t, .) or (., t, v) among the positives and the fold.
Both decoders run in the same process and ALTERNATE repetition by repetition; every figure is a device-event time around one
call after three warm-up calls, reported as median, 10th and 90th percentile and the spread (p90 - p10) / median.
--tree: import tf2_gnn_amd from another checkout (with its own built library), e.g. the parent commit, to time the DistMult
calls of that build with the same script: run the two checkouts as alternating processes and compare medians against the
spread.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_TEST = 20466
WARMUP = 3


def line(name, t):
    t = np.asarray(t, dtype=np.float64)
    med, p10, p90 = np.median(t), np.percentile(t, 10), np.percentile(t, 90)
    return f"{name:>44}: median {med:9.3f} ms  p10 {p10:9.3f}  p90 {p90:9.3f}  spread {(p90 - p10) / med:5.1%}"


def alternating_event_ms(fns, repeats):
    """{name: [ms]}: after WARMUP calls of each, `repeats` rounds in which every fn runs once between its own pair of events"""
    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            out[name].append(t0.elapsed_time(t1))
    return out


def filters(known, queries, slot):
    """CSR (offsets, ids) per query: the entities in `slot` (2: targets, 0: sources) of the known triples that share the
    query's other two entries, sorted and unique"""
    other = 0 if slot == 2 else 2
    V = int(known[:, [0, 2]].max()) + 1
    key = lambda a: a[:, 1].astype(np.int64) * V + a[:, other]
    order = np.argsort(key(known), kind="stable")
    keys, vals = key(known)[order], known[order, slot]
    lo, hi = np.searchsorted(keys, key(queries), "left"), np.searchsorted(keys, key(queries), "right")
    lists = [np.unique(vals[a:b]) for a, b in zip(lo, hi)]
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    return offsets.astype(np.int32), np.concatenate(lists).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--decoders", default="distmult,complex")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--label", default="")
    ap.add_argument("--widths", default="320,128")
    ap.add_argument("--negatives", default="1,4")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    sys.path.insert(1, HERE)
    from tf2_gnn_amd import ops
    from tools.negative_sampling_probe import fb15k_shaped_edges

    decoders = args.decoders.split(",")
    dev = torch.device("cuda", 0)
    as_triples = lambda edges: np.concatenate([np.stack([e[:, 0], np.full(len(e), t), e[:, 1]], axis=1) for t, e in enumerate(edges)])
    pos = as_triples(fb15k_shaped_edges(0)).astype(np.int64)
    test = as_triples(fb15k_shaped_edges(1)).astype(np.int64)
    test = test[np.random.default_rng(2).permutation(len(test))[:Q_TEST]]
    V, T, P = 14541, 237, len(pos)
    known = np.concatenate([pos, test])
    flt = {"dst": filters(known, test, 2), "src": filters(known, test, 0)}
    queries = torch.from_numpy(test.astype(np.int32)).to(dev)
    flt_dev = {s: tuple(torch.from_numpy(a).to(dev) for a in f) for s, f in flt.items()}
    print(f"complex_probe{' [' + args.label + ']' if args.label else ''}: tree={os.path.relpath(args.tree, HERE)} V={V} T={T} P={P} "
          f"Q={len(test)} filter ids dst/src={len(flt['dst'][1])}/{len(flt['src'][1])} decoders={decoders} repeats={args.repeats}")
    rng = np.random.default_rng(3)
    for D in (int(x) for x in args.widths.split(",")):
        H = torch.from_numpy(rng.standard_normal((V, D)).astype(np.float32) * 0.3).to(dev)
        R = torch.from_numpy(rng.standard_normal((T, D)).astype(np.float32)).to(dev)
        for K in (int(x) for x in args.negatives.split(",")):
            neg = np.repeat(pos, K, axis=0)
            side = rng.integers(0, 2, len(neg)) * 2
            neg[np.arange(len(neg)), side] = rng.integers(0, V, len(neg))
            triples = np.concatenate([pos, neg]).astype(np.int32)
            N = len(triples)
            labels = torch.cat([torch.ones(P), torch.zeros(N - P)]).to(dev)
            tables = {k: torch.from_numpy(v).to(dev) for k, v in ops.build_triple_tables(triples, V, T).items()}
            tr = torch.from_numpy(triples).to(dev)
            g = {d: getattr(ops, f"{d}_ce_metrics")(H, R, tr, labels)[3] for d in decoders}
            print(f"--- D = {D}, K = {K}: N = {N} triples, {2 * N} node entries")
            fwd = alternating_event_ms({d: (lambda d=d: getattr(ops, f"{d}_ce_metrics")(H, R, tr, labels)) for d in decoders}, args.repeats)
            bwd = alternating_event_ms({d: (lambda d=d: getattr(ops, f"{d}_backward")(H, R, tr, g[d], tables)) for d in decoders}, args.repeats)
            for name, times in (("ce_metrics", fwd), ("backward (dH and dR)", bwd)):
                for d in decoders:
                    print(line(f"{d} {name}", times[d]))
                if len(decoders) == 2:
                    print(f"{'':>44}  complex / distmult (medians) = {np.median(times['complex']) / np.median(times['distmult']):.3f}")
        rank = alternating_event_ms({d: (lambda d=d: [getattr(ops, f"{d}_rank")(H, R, queries, s, *flt_dev[s]) for s in ("dst", "src")])
                                     for d in decoders}, max(4, args.repeats // 2))
        print(f"--- D = {D}: rank, Q = {len(test)} queries x V = {V} candidates, both sides, filtered")
        for d in decoders:
            print(line(f"{d} rank (dst + src)", rank[d]))
        if len(decoders) == 2:
            print(f"{'':>44}  complex / distmult (medians) = {np.median(rank['complex']) / np.median(rank['distmult']):.3f}")
    counts = dict(ops.link_launch_counts())
    if hasattr(ops, "complex_launch_counts"):
        counts.update(ops.complex_launch_counts())
    print(f"launches so far: {counts}")


if __name__ == "__main__":
    main()
