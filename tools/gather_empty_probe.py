"""What the empty (node, type) buckets cost a planned gather launch of the headline step: the launches of
tools/gather_chain_probe.py (benchmark batch make_synthetic_batch(30000, 900000, 4, 320, seed=1), width 320, SP16 output,
plain sums) next to the same buckets gathered through the compact views, which give an empty bucket neither a lane group nor
an output row:

    python tools/gather_empty_probe.py [--out FILE]
    python tools/gather_empty_probe.py --root OTHER_CHECKOUT [--root ANOTHER ...] [--processes 5] [--out FILE]

  fwd          typed by-target buckets in pattern order, all V * L rows written (the forward pass)
  bwd          typed by-source buckets, all V * L rows written (the backward pass)
  fwd-l2       fwd with its columns folded onto 2048 distinct source rows (every source row an L2 hit)
  fwd-compact  the by-target buckets through TFGNN_VIEW_BY_DST_TYPED_COMPACT: non-empty buckets only
  bwd-compact  the by-source buckets through TFGNN_VIEW_BY_SRC_TYPED_COMPACT
  fwd-keep     fwd into the operand the graph owns (ops.graph_gather_sp_owned), every launch after the first: the rows of the
               empty buckets are in the operand already and the launch ends in front of them
  bwd-keep     bwd likewise (a tree without ops.graph_gather_sp_owned has neither of the two)

fwd - fwd-compact and bwd - bwd-compact are what the empty buckets cost a launch: their lane groups plus their zero rows.
That difference is the ceiling for anything that moves the zero-fill elsewhere inside the launch (the rows still have to be
written).  Protocol of gather_chain_probe.py: ROUNDS rounds of REPS back-to-back launches between two device events, variants
alternating within a round; with ``--root`` every tree runs in ``--processes`` alternating processes, the figure is the median
of the process medians and the spread their max - min.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, E, L, H = 30000, 900000, 4, 320
ROUNDS, REPS, WARM = 9, 20, 5
VARIANTS = ("fwd", "bwd", "fwd-l2", "fwd-compact", "bwd-compact")
KEEP_VARIANTS = ("fwd-keep", "bwd-keep")
CHILD_SECONDS = 240  # a process that takes longer than this is stuck: the probe stops, it starts nothing after it


def measure(root):
    """({variant: [us per launch, one per round]}, facts about the batch) with tf2_gnn_amd imported from ``root``"""
    sys.path.insert(0, os.path.abspath(root))
    import torch

    if not torch.cuda.is_available():
        sys.exit("gather_empty_probe: no ROCm device - nothing is measured on a CPU")
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import make_synthetic_batch

    dev = torch.device("cuda", 0)
    _, adjs = make_synthetic_batch(V, E, L, H, seed=1)
    g = ops.Graph(tuple(torch.from_numpy(a).to(dev) for a in adjs), V, parts=ops.G_PARTS_ALL)
    gen = torch.Generator().manual_seed(1)
    X = torch.randn((V, H), generator=gen).to(dev)
    folded = (g.array(ops.G_COL_BY_DST) % 2048).contiguous()
    facts = {"rows": V * L, "nonempty_by_dst": int(g.nonempty_offsets(False)[-1]), "nonempty_by_src": int(g.nonempty_offsets(True)[-1])}
    run = {
        "fwd": lambda: ops.graph_gather_sp(g, ops.VIEW_BY_DST_TYPED_PATTERN, X, rows_per_operand_row=L),
        "bwd": lambda: ops.graph_gather_sp(g, ops.VIEW_BY_SRC_TYPED, X, rows_per_operand_row=L),
        "fwd-l2": lambda: ops.graph_gather_sp(g, ops.VIEW_BY_DST_TYPED_PATTERN, X, col=folded, rows_per_operand_row=L),
        "fwd-compact": lambda: ops.graph_gather_sp(g, ops.VIEW_BY_DST_TYPED_COMPACT, X),
        "bwd-compact": lambda: ops.graph_gather_sp(g, ops.VIEW_BY_SRC_TYPED_COMPACT, X),
    }
    if hasattr(ops, "graph_gather_sp_owned"):
        run["fwd-keep"] = lambda: ops.graph_gather_sp_owned(g, ops.VIEW_BY_DST_TYPED_PATTERN, X)
        run["bwd-keep"] = lambda: ops.graph_gather_sp_owned(g, ops.VIEW_BY_SRC_TYPED, X)
    variants = tuple(v for v in VARIANTS + KEEP_VARIANTS if v in run)
    for v in variants:
        for _ in range(WARM):
            run[v]()
    torch.cuda.synchronize()
    times = {v: [] for v in variants}
    for _ in range(ROUNDS):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                run[v]()
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1000.0 / REPS)
    return times, facts


def table(title, per_variant, unit):
    lines = [title]
    for v in VARIANTS + KEEP_VARIANTS:
        t = per_variant[v]
        if not t:
            continue
        lines.append(f"  {v:12s} {statistics.median(t):8.1f} us   spread {max(t) - min(t):5.1f}   ({unit})")
    for full, compact in (("fwd", "fwd-compact"), ("bwd", "bwd-compact")):
        a, b = per_variant[full], per_variant[compact]
        diff = statistics.median(a) - statistics.median(b)
        spread = max(max(a) - min(a), max(b) - min(b))
        lines.append(f"  {full} - {compact}: {diff:6.1f} us, the empty buckets of a launch; three times the larger spread: {3 * spread:5.1f} us")
        k = per_variant[full + "-keep"]
        if k:
            gain = statistics.median(a) - statistics.median(k)
            spread = max(max(a) - min(a), max(k) - min(k))
            lines.append(f"  {full} - {full}-keep:    {gain:6.1f} us recovered by keeping the empty rows ({100 * gain / diff if diff else 0:.0f} % of the line above); "
                         f"three times the larger spread: {3 * spread:5.1f} us")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", action="append", default=[], help="another checkout with its own built library; may be repeated")
    ap.add_argument("--processes", type=int, default=5)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join("profiles", "gather_empty_probe.txt"))
    args = ap.parse_args()
    if args.child:  # one process of the alternating mode: the rounds as one JSON line
        times, facts = measure(args.child)
        print("PROBE " + json.dumps({"times": times, "facts": facts}), flush=True)
        return
    head = (f"planned gather of the headline step and its empty buckets, V = {V}, E = {E}, L = {L}, width {H}, SP16 output: "
            f"us per launch, {ROUNDS} rounds of {REPS} launches, variants alternating")
    lines = [head]
    trees = [HERE] + [os.path.abspath(r) for r in args.root]
    medians = {t: {v: [] for v in VARIANTS + KEEP_VARIANTS} for t in trees}
    facts = None
    for _ in range(args.processes):
        for t in trees:  # one process at a time has the device open
            try:
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", t], capture_output=True, text=True,
                                     timeout=CHILD_SECONDS)
            except subprocess.TimeoutExpired:
                sys.exit(f"gather_empty_probe: the process for {t} did not finish in {CHILD_SECONDS} s")
            if res.returncode != 0:
                sys.exit(f"gather_empty_probe: the process for {t} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
            got = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("PROBE ")][-1][6:])
            facts = got["facts"]
            for v in got["times"]:
                medians[t][v].append(statistics.median(got["times"][v]))
    lines.append(f"{facts['rows']} buckets per typed view; non-empty: {facts['nonempty_by_dst']} by target, {facts['nonempty_by_src']} by source")
    lines.append("")
    for t in trees:
        name = "this tree" if t == HERE else f"checkout '{os.path.basename(t)}'"
        lines += table(f"{name} ({args.processes} processes" + (", alternating with the other trees)" if args.root else ")"), medians[t],
                       f"median and spread of {args.processes} process medians")
        lines.append("")
    text = "\n".join(lines).rstrip() + "\n"
    print(text)
    out_dir = os.path.dirname(args.out)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
