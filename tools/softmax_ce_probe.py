"""tfgnn_softmax_ce_metrics (ops.softmax_ce_metrics) next to torch's F.cross_entropy on the same tensors, at the two node
classification shapes of BASELINE: ogbn-arxiv scale (V = 169 343, C = 40) and PPI scale (V = 7 110, C = 121).
   python tools/softmax_ce_probe.py [--out profiles/softmax_ce_probe.txt]

Protocol: device events around a window of ITERS calls on the launch stream, after a warm-up of every variant; WINDOWS
windows per variant, the variants alternating window by window; median and range of the windows are printed.  "rotating":
every call of a window reads another copy of the logits (and writes another gradient), enough copies to exceed 512 MiB, so
that the part's 256 MiB last-level cache cannot hold the stream; "hot": the same buffers every call.  Bytes per call are
what the algorithm needs: 4 V C read (+ 4 V C written with the gradient) + 8 V for labels and weights, each read by the
weight pass and by the main pass.  tools/stream_pass_probe.py measured 5.0 - 5.3 TB/s for mixed read + write streams of
hundreds of MB; at these sizes (27 MB and 3.4 MB of logits) a call is a few launches of a few microseconds each, so launch
and tail effects weigh in, and a window measures the host's enqueue rate wherever that is the slower of the two.  torch: F.cross_entropy(ignore_index=-1, reduction="mean") forward (+ backward to the logits) -
unweighted labels only, so the library is timed with weights=None as well as with a 0/1 mask."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ITERS, WINDOWS, WARMUP = 1000, 7, 20


def _window(fn, n):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(n):
        fn(i)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / n * 1000.0  # us per call


def probe(V, C, lines):
    import torch
    import torch.nn.functional as F

    from tf2_gnn_amd import ops

    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(V + C)
    copies = max(2, -(-(512 << 20) // (V * C * 4)))
    base = (torch.randn((V, C), generator=g) * 3).to(dev)
    logits = [base.clone() for _ in range(copies)]
    grads = [torch.empty_like(base) for _ in range(copies)]
    labels_long = torch.randint(0, C, (V,), generator=g)
    labels_long[::13] = -1
    labels_long = labels_long.to(dev)
    labels = labels_long.float()
    mask = (torch.rand(V, generator=g) < 0.5).float().to(dev)
    leaves = [x.clone().requires_grad_(True) for x in logits]

    def torch_fwd_bwd(x):
        x.grad = None
        F.cross_entropy(x, labels_long, ignore_index=-1).backward()

    def torch_fwd(x):
        with torch.no_grad():
            F.cross_entropy(x, labels_long, ignore_index=-1)

    nb_f, nb_g = 4 * V * C + 16 * V, 8 * V * C + 16 * V
    variants = [
        ("tfgnn loss only, no weights", lambda i, k: ops.softmax_ce_metrics(logits[k % copies], labels, None, need_grad=False), nb_f - 8 * V),
        ("tfgnn loss only, 0/1 mask", lambda i, k: ops.softmax_ce_metrics(logits[k % copies], labels, mask, need_grad=False), nb_f),
        ("tfgnn loss + grad, no weights", lambda i, k: ops.softmax_ce_metrics(logits[k % copies], labels, None, out=grads[k % len(grads)]), nb_g - 8 * V),
        ("tfgnn loss + grad, 0/1 mask", lambda i, k: ops.softmax_ce_metrics(logits[k % copies], labels, mask, out=grads[k % len(grads)]), nb_g),
        ("torch cross_entropy forward", lambda i, k: torch_fwd(leaves[k % len(leaves)]), nb_f - 12 * V),
        ("torch cross_entropy fwd + bwd", lambda i, k: torch_fwd_bwd(leaves[k % len(leaves)]), nb_g - 12 * V),
    ]
    for _, fn, _ in variants:
        for i in range(WARMUP):
            fn(i, i)
    torch.cuda.synchronize()
    times = {(name, mode): [] for name, _, _ in variants for mode in ("hot", "rotating")}
    for _ in range(WINDOWS):
        for name, fn, _ in variants:
            times[(name, "hot")].append(_window(lambda i: fn(i, 0), ITERS))
            times[(name, "rotating")].append(_window(lambda i: fn(i, i), ITERS))
    lines.append(f"V = {V}, C = {C}: logits {V * C * 4 / 1e6:.1f} MB, {copies} rotating copies; {WINDOWS} windows of {ITERS} calls")
    lines.append(f"  {'variant':32s} {'mode':9s} {'us / call (median)':>18s} {'min':>8s} {'max':>8s} {'MB / call':>10s} {'TB/s':>6s}")
    for name, _, nbytes in variants:
        for mode in ("hot", "rotating"):
            t = times[(name, mode)]
            med = statistics.median(t)
            lines.append(f"  {name:32s} {mode:9s} {med:18.1f} {min(t):8.1f} {max(t):8.1f} {nbytes / 1e6:10.2f} {nbytes / med / 1e6:6.2f}")


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_ce_probe needs a ROCm device: nothing is measured without one")
    lines = [f"softmax_ce_probe on {torch.cuda.get_device_name(0)}; mixed read + write streams on this part: 5.0 - 5.3 TB/s "
             "(tools/stream_pass_probe.py)"]
    for V, C in ((169343, 40), (7110, 121)):
        probe(V, C, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
