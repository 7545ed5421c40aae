"""What does the in-stream repair of the weight-gradient product cost (ops.set_guard_repair, csrc/tn_repair.hip)?
     python tools/tn_repair_probe.py [out.txt]      (needs an MI355X; default profiles/tn_repair_probe.txt)
At the headline's Dense shape (M = N = 320, K = 30 000) and its message shape (M = 1 280, N = 320, K = 30 000):
  (a) quiet operands, product with repair armed against the same product with repair off.  With the switch off the library
      launches exactly the kernels it launched before the switch existed, so this is the price of the memset node plus the
      repair kernel's early-exit launch;
  (b) operands that trip the guard (every third row 2^-30 below the others on both sides), the repaired product against
      ops.gemm(a^T b) of the same shape in mode bf16x3 - the kernel a demoted stack would run instead.
And for the grouped product (ops.sp_gemm_tn_grouped, repaired K range by K range) at the shape class of bench.py's arxiv-rgin
workload (40 relations, widths 512):
  (c) quiet operands, armed against off; armed, every range tripping against a single range tripping.
Device events around windows of REPS calls after a warm-up of every variant; the two variants of a comparison alternate,
ROUNDS windows each; printed: median and min .. max of the per-call time over the windows."""
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from tf2_gnn_amd import ops  # noqa: E402

REPS, ROUNDS, WARMUP = 200, 7, 20
SHAPES = [("dense  M=320  N=320 K=30000", 320, 320, 320, 30000), ("message M=1280 N=320 K=30000", 1280, 320, 320, 30000)]


def window(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps  # microseconds per call


def alternate(variants, reps=REPS):
    """variants: [(name, setup, fn)] -> {name: [us per call, one per round]}; setup() runs before each window of its variant."""
    times = {name: [] for name, _, _ in variants}
    for name, setup, fn in variants:
        setup()
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for name, setup, fn in variants:
            setup()
            times[name].append(window(fn, reps))
    return times


def line(name, ts, reps=REPS):
    return f"    {name:<34s} median {statistics.median(ts):9.1f} us   ({min(ts):.1f} .. {max(ts):.1f}, {len(ts)} windows of {reps} calls)"


GROUPED_L, GROUPED_H, GROUPED_ROWS = 40, 512, 8000  # relations and widths of bench.py --workload arxiv-rgin; rows per relation


def grouped_case(dev):
    """(c) the grouped product (ops.sp_gemm_tn_grouped) at arxiv-rgin's shape class: GROUPED_L relations, M = N = GROUPED_H,
    GROUPED_ROWS compact rows per relation (4 K ranges of 2000 rows each: 160 ranges per launch).  Quiet operands, armed against
    off; then armed, "every range trips" (every third row of all of them 2^-30 below the others on both sides) against "one
    range trips" (such rows in the last range of the last relation only)."""
    off = [i * GROUPED_ROWS for i in range(GROUPED_L + 1)]
    R, H = off[-1], GROUPED_H
    groups = ops.RowGroups(off, dev)
    ranges = groups.tn_tables()[2]
    g = torch.Generator().manual_seed(R + H)
    a = torch.randn((R, H), generator=g).to(dev)
    b = torch.randn((R, H), generator=g).to(dev)
    k = torch.arange(R)
    out = torch.empty((GROUPED_L, H, H), device=dev)
    lines = [f"grouped L={GROUPED_L} M=N={H}, {GROUPED_ROWS} rows per relation ({R} rows, {ranges} K ranges)"]
    ops.set_gemm_mode("f16x2")
    a_sp, b_sp = ops.sp_split_rows(a), ops.sp_split_rows(b)
    quiet = lambda: ops.sp_gemm_tn_grouped(a_sp, b_sp, groups, out)  # noqa: E731
    ops.repair_stats(reset=True)
    t = alternate([("repair off", lambda: ops.set_guard_repair(False), quiet),
                   ("repair armed, quiet", lambda: ops.set_guard_repair(True), quiet)], reps=50)
    st = ops.repair_stats(reset=True)
    assert st["repaired_products"] == 0 and st["armed_products"] > 0 and not ops.f16x2_guard_tripped_sync(), st
    lines.append("  (c) grouped two-factor product, quiet operands")
    lines += [line(n, ts, 50) for n, ts in t.items()]
    d = statistics.median(t["repair armed, quiet"]) - statistics.median(t["repair off"])
    lines.append(f"    armed - off (medians): {d:+.1f} us per product")
    ops.set_guard_repair(True)
    variants = []
    for name, where in (("armed, every range trips", k >= 0), ("armed, one range trips", k >= R - 2000)):
        low = ((k % 3 == 1) & where).to(dev).unsqueeze(1)
        sp = ops.sp_split_rows(torch.where(low, a * 2.0 ** -30, a)), ops.sp_split_rows(torch.where(low, b * 2.0 ** -30, b))
        variants.append((name, lambda: None, lambda sp=sp: ops.sp_gemm_tn_grouped(sp[0], sp[1], groups, out)))
    ops.repair_stats(reset=True)
    t = alternate(variants, reps=5)
    st = ops.repair_stats(reset=True)
    assert st["repaired_products"] == st["armed_products"] > 0 and not ops.f16x2_guard_tripped_sync(), st
    ops.set_guard_repair(False)
    lines.append("  (c) grouped two-factor product, tripping operands")
    lines += [line(n, ts, 5) for n, ts in t.items()]
    return lines


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "tn_repair_probe.txt")
    dev = torch.device("cuda", 0)
    lines = [f"tn_repair_probe: {torch.cuda.get_device_name(0)}; REPS={REPS} ROUNDS={ROUNDS} WARMUP={WARMUP}"]
    was = ops.set_guard_repair(False)
    try:
        for label, M, N, sb, K in SHAPES:
            g = torch.Generator().manual_seed(K + M)
            a = torch.randn((K, M), generator=g).to(dev)
            b = torch.randn((K, N), generator=g).to(dev)
            low = (torch.arange(K) % 3 == 1).to(dev).unsqueeze(1)
            a_trip = torch.where(low, a * 2.0 ** -30, a)
            b_trip = torch.where(low, b * 2.0 ** -30, b)
            out = torch.empty((M, N), device=dev)
            lines.append(label)
            for wide in (False, True):
                ops.set_gemm_mode("f16x2")
                a_sp, b_sp = ops.sp_split_rows(a, scale_block=sb), ops.sp_split_rows(b)
                quiet = lambda: ops.sp_gemm_tn(a_sp, b_sp, out=out, wide=wide)  # noqa: E731
                ops.repair_stats(reset=True)
                t = alternate([("repair off", lambda: ops.set_guard_repair(False), quiet),
                               ("repair armed, quiet", lambda: ops.set_guard_repair(True), quiet)])
                st = ops.repair_stats(reset=True)
                assert st["repaired_products"] == 0 and st["armed_products"] > 0 and not ops.f16x2_guard_tripped_sync(), st
                form = "two-factor" if wide else "one-factor"
                lines.append(f"  (a) {form} product, quiet operands")
                lines += [line(n, ts) for n, ts in t.items()]
                d = statistics.median(t["repair armed, quiet"]) - statistics.median(t["repair off"])
                lines.append(f"    armed - off (medians): {d:+.1f} us per product")
            # (b)
            ops.set_gemm_mode("f16x2")
            ops.set_guard_repair(True)
            a_sp, b_sp = ops.sp_split_rows(a_trip, scale_block=sb), ops.sp_split_rows(b_trip)
            ops.repair_stats(reset=True)
            t_rep = alternate([("repaired one-factor product", lambda: None, lambda: ops.sp_gemm_tn(a_sp, b_sp, out=out))], reps=20)
            st = ops.repair_stats(reset=True)
            assert st["repaired_products"] == st["armed_products"] > 0, st
            ops.set_guard_repair(False)
            ops.set_gemm_mode("bf16x3")
            t_x3 = alternate([("ops.gemm(a^T b), bf16x3", lambda: None, lambda: ops.gemm(a_trip, b_trip, trans_a=True, out=out))], reps=20)
            lines.append("  (b) tripping operands")
            lines += [line(n, ts, 20) for n, ts in list(t_rep.items()) + list(t_x3.items())]
        lines += grouped_case(dev)
    finally:
        ops.set_guard_repair(was)
        ops.set_gemm_mode("f16x2")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
