"""Times the planned gather launches of the headline step on the benchmark's batch (make_synthetic_batch(30000, 900000, 4, 320,
seed=1), width 320, SP16 output folded into the [V, L * 320] operand, plain sums):

    python tools/gather_chain_probe.py [--out FILE]
    python tools/gather_chain_probe.py --root OTHER_CHECKOUT [--root ANOTHER ...] [--processes 4] [--out FILE]

  fwd      typed by-target buckets in pattern order (the forward pass: source rows = node states)
  bwd      typed by-source buckets (the backward pass: source rows = gradient rows)
  fwd-l2   the forward launch with its columns folded onto 2048 distinct source rows (2.6 MB: every source row is an L2 hit) -
           what is left of the launch when the row loads cost least; the walk's own chain of loads is in it
  fwd-fp32 the by-target launch with fp32 output (the same walk, 4 bytes per element written instead of the split pair)
  fp32-256 the same at width 256 (four chunks per lane: the plain-sum kernel whose register count the index blocks take
           from 7 to 6 waves per SIMD)

Each variant runs ROUNDS rounds of REPS back-to-back launches between two device events, variants alternating within a round;
the figure is the median over the rounds of (time of a round) / REPS with the spread (max - min) next to it.
``--root``: this tree and every other checkout (each with its own built library, e.g. an unpacked archive of the parent
commit) are timed in alternating processes of one session, ``--processes`` of each; per tree the median over its processes'
medians and the spread of those.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, E, L, H = 30000, 900000, 4, 320
ROUNDS, REPS, WARM = 9, 20, 5
VARIANTS = ("fwd", "bwd", "fwd-l2", "fwd-fp32", "fp32-256")


def measure(root):
    """{variant: [us per launch, one per round]} with tf2_gnn_amd imported from ``root``"""
    sys.path.insert(0, os.path.abspath(root))
    import torch

    if not torch.cuda.is_available():
        sys.exit("gather_chain_probe: no ROCm device - nothing is measured on a CPU")
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import make_synthetic_batch

    dev = torch.device("cuda", 0)
    _, adjs = make_synthetic_batch(V, E, L, H, seed=1)
    g = ops.Graph(tuple(torch.from_numpy(a).to(dev) for a in adjs), V, parts=ops.G_PARTS_ALL)
    gen = torch.Generator().manual_seed(1)
    X = torch.randn((V, H), generator=gen).to(dev)
    folded = (g.array(ops.G_COL_BY_DST) % 2048).contiguous()
    out32 = torch.empty((V * L, H), device=dev)
    X256, out256 = X[:, :256].contiguous(), torch.empty((V * L, 256), device=dev)
    run = {
        "fwd": lambda: ops.graph_gather_sp(g, ops.VIEW_BY_DST_TYPED_PATTERN, X, rows_per_operand_row=L),
        "bwd": lambda: ops.graph_gather_sp(g, ops.VIEW_BY_SRC_TYPED, X, rows_per_operand_row=L),
        "fwd-l2": lambda: ops.graph_gather_sp(g, ops.VIEW_BY_DST_TYPED_PATTERN, X, col=folded, rows_per_operand_row=L),
        "fwd-fp32": lambda: ops.graph_gather(g, ops.VIEW_BY_DST_TYPED, X, out=out32),
        "fp32-256": lambda: ops.graph_gather(g, ops.VIEW_BY_DST_TYPED, X256, out=out256),
    }
    for v in VARIANTS:
        for _ in range(WARM):
            run[v]()
    torch.cuda.synchronize()
    times = {v: [] for v in VARIANTS}
    for _ in range(ROUNDS):
        for v in VARIANTS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                run[v]()
            e1.record()
            e1.synchronize()
            times[v].append(e0.elapsed_time(e1) * 1000.0 / REPS)
    return times


def table(title, per_variant, unit):
    lines = [title]
    for v in VARIANTS:
        t = per_variant[v]
        lines.append(f"  {v:10s} {statistics.median(t):8.1f} us   spread {max(t) - min(t):5.1f}   ({unit})")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", action="append", default=[], help="another checkout with its own built library; may be repeated")
    ap.add_argument("--processes", type=int, default=4)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join("profiles", "gather_chain_probe.txt"))
    args = ap.parse_args()
    if args.child:  # one process of the --root mode: the rounds as one JSON line
        print("PROBE " + json.dumps(measure(args.child)), flush=True)
        return
    head = (f"planned gather of the headline step, V = {V}, E = {E}, L = {L}, width {H}: us per launch, "
            f"{ROUNDS} rounds of {REPS} launches, variants alternating")
    lines = [head, ""]
    if not args.root:
        lines += table("this tree", measure(HERE), f"median of {ROUNDS} rounds")
    else:
        trees = [HERE] + [os.path.abspath(r) for r in args.root]
        medians = {t: {v: [] for v in VARIANTS} for t in trees}
        for _ in range(args.processes):
            for t in trees:  # one process at a time has the device open
                res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", t], capture_output=True, text=True)
                if res.returncode != 0:
                    sys.exit(f"gather_chain_probe: the process for {t} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
                got = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("PROBE ")][-1][6:])
                for v in VARIANTS:
                    medians[t][v].append(statistics.median(got[v]))
        for t in trees:
            name = "this tree" if t == HERE else f"checkout '{os.path.basename(t)}'"
            lines += table(f"{name} ({args.processes} processes, alternating with the other trees)", medians[t],
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
