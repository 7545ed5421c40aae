"""Times the vocabulary embedding kernels (ops.vocab_embedding_forward / vocab_embedding_backward, csrc/vocab_embedding.hip)
alone, at the sizes a user would run:

    python tools/vocab_embedding_probe.py [--repeats 10] [--out profiles/vocab_embedding_probe.txt]

  molecule shape  n = the nodes of bench.py's QM9-shaped batch (128 000 molecules), ids uniform over N = 5 and over N = 100
                  (atom types), D = 128;
  token shape     the same n, N = 10 000, ids Zipf-distributed (p ~ 1 / rank: the first id covers about a tenth of the rows),
                  D = 128.
Per shape: the forward call (lookup + plan: sort and row pointers), the backward call, and next to them what a user would
otherwise write - ``table.index_select(0, ids)`` and ``zeros.index_add_(0, ids, d_rows)``.  ``index_add_`` adds with float
atomics in no fixed order: it is a yardstick for speed, NOT a reference for correctness.  Bursts of 20 calls between one pair
of device events, after a warm-up of every shape; median, 10th and 90th percentile and the spread (p90 - p10) / median.
The floor next to the backward call is its compulsory traffic, n * D * 4 bytes read plus N * D * 4 written, at the copy
bandwidth this run measures itself: a device-to-device ``copy_`` of n * D * 4 bytes (read + write counted).  Before timing,
each shape's gradient is checked on the device against a float64 ``index_add_`` with the bound of include/tfgnn.h, and two
calls for equal bits.  No GPU: the script fails, it measures nothing on a CPU."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.negative_sampling_probe import event_ms, line  # noqa: E402

D, BURST, QM9_GRAPHS = 128, 20, 128000


def shapes(n):
    rng = np.random.default_rng(7)
    zipf = 1.0 / np.arange(1, 10001)
    return [("molecule N = 5", 5, rng.integers(0, 5, size=n)), ("molecule N = 100", 100, rng.integers(0, 100, size=n)),
            ("token N = 10000, Zipf", 10000, rng.choice(10000, size=n, p=zipf / zipf.sum()))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vocab_embedding_probe: no ROCm device - nothing is measured on a CPU")
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import make_qm9_shaped_batch

    dev = torch.device("cuda", 0)
    n = int(make_qm9_shaped_batch(QM9_GRAPHS, seed=1, feature_dim=1)[2].shape[0])
    report = [f"vocab_embedding_probe: n = {n} rows (the QM9-shaped batch of {QM9_GRAPHS} molecules), D = {D}, bursts of {BURST}, "
              f"repeats = {args.repeats}"]
    g = torch.Generator().manual_seed(3)
    d_rows = torch.randn(n, D, generator=g).to(dev)
    scratch = torch.empty_like(d_rows)
    copy = np.median(event_ms(lambda: scratch.copy_(d_rows), args.repeats, BURST))
    copy_rate = 2 * n * D * 4 / (copy * 1e-3)  # bytes per second, read + write
    report.append(f"copy_ of n * D * 4 = {n * D * 4 / 1e6:.1f} MB: median {copy:.3f} ms = {copy_rate / 1e9:.0f} GB/s (read + write), measured")
    for name, N, ids_np in shapes(n):
        ids = torch.from_numpy(ids_np.astype(np.int32)).to(dev)
        ids64 = ids.long()
        table = torch.randn(N, D, generator=g).to(dev)
        rows, plan = ops.vocab_embedding_forward(table, ids)
        grad = ops.vocab_embedding_backward(d_rows, plan, N)
        # results at the timed size: the lookup bit for bit, the gradient inside the derived bound, the same bits again
        assert torch.equal(rows, table.index_select(0, ids64))
        ref = torch.zeros(N, D, dtype=torch.float64, device=dev).index_add_(0, ids64, d_rows.double())
        S = torch.zeros(N, D, dtype=torch.float64, device=dev).index_add_(0, ids64, d_rows.double().abs())
        m = torch.bincount(ids64, minlength=N).double()
        ratio = float(((grad.double() - ref).abs() / ((256 + torch.ceil(m / 256)).unsqueeze(1) * 2.0 ** -24 * S).clamp_min(1e-300)).max())
        assert ratio <= 1.0 and torch.equal(grad, ops.vocab_embedding_backward(d_rows, plan, N).clone())
        out, buf, zeros = torch.empty_like(rows), torch.empty_like(grad), torch.empty_like(grad)
        floor = (n * D * 4 + N * D * 4) / copy_rate * 1e3
        report.append(f"--- {name}: largest id {int(m.max())} rows = {int(np.ceil(float(m.max()) / 256))} chunks; "
                      f"max error / bound {ratio:.3g}; two calls equal bits")
        fwd = event_ms(lambda: ops.vocab_embedding_forward(table, ids, plan=plan, out=out), args.repeats, BURST)
        bwd = event_ms(lambda: ops.vocab_embedding_backward(d_rows, plan, N, out=buf), args.repeats, BURST)
        sel = event_ms(lambda: torch.index_select(table, 0, ids64, out=out), args.repeats, BURST)
        add = event_ms(lambda: zeros.zero_().index_add_(0, ids64, d_rows), args.repeats, BURST)
        report += [line("vocab_embedding_forward (lookup + plan)", fwd), line("torch index_select (no plan)", sel),
                   line("vocab_embedding_backward", bwd), line("torch zero_ + index_add_ (float atomics)", add),
                   f"    backward floor (computed): {(n * D * 4 + N * D * 4) / 1e6:.1f} MB at the measured copy rate = {floor:.3f} ms; "
                   f"measured / floor = {np.median(bwd) / floor:.2f}; index_add_ / backward = {np.median(add) / np.median(bwd):.2f}"]
    report.append("launches so far (forward, backward): %d, %d" % ops.vocab_embedding_launch_counts())
    text = "\n".join(report)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
