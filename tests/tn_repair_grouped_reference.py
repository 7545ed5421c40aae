"""Operands and a CPU model for the range-level repair of the grouped split-operand weight-gradient product
(tfgnn_sp_gemm_tn_grouped with ``ops.set_guard_repair(True)``), shared by tests/test_tn_repair_grouped_host.py (no GPU) and
tests/test_gpu_tn_repair_grouped.py.

The operands: seven row groups of 0, 1, 5, 2016, 2017, 300 and 4100 rows.  Deficient rows (k % 3 == 1, 2^-30 below the others
on A and on B: pairs at 2^-60, beyond the two-factor product's 2^44) fill group 3 and the local rows >= 2752 of group 6 - group
6 is cut into K ranges of 1376, 1376 and 1348 rows, so exactly its last range trips.  Columns m % 8 == 5 of A are zero on every
other row (tests/test_gpu_tn_repair.py ``orphan_case``): those outputs of groups 3 and 6 receive terms from the deficient rows
only, and nothing at all in the quiet groups."""
import torch

from tests.test_gpu_tn_repair import orphan_case

SIZES = [0, 1, 5, 2016, 2017, 300, 4100]
SHAPES = [(128, 128, 64), (256, 128, 128)]  # M, N, scale block of A
TRIPPING_RANGES = {3: [0], 6: [2]}  # group -> its K ranges that hold deficient rows
MAX_CHUNK = 2016  # rows of a K range (ops.TN_GROUPED_MAX_CHUNK; gemm_sp.hip SP_TN_BSC_MAX_CHUNK)
MARKER = 1.1754943508222875e-38  # the inverse scale of an all-zero (row, block): 2^-126


def offsets(sizes=SIZES):
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    return off


def ranges_of(off):
    """The K ranges of every group, by the arithmetic of ``ops.RowGroups.tn_tables``: equal shares of at most MAX_CHUNK rows,
    rounded up to whole k16 steps.  -> [[(first row, rows), ..] per group]"""
    out = []
    for gi in range(len(off) - 1):
        r0, r1 = off[gi], off[gi + 1]
        n = -(-(r1 - r0) // MAX_CHUNK)
        rs = []
        if n:
            chunk = -(-(-(-(r1 - r0) // n)) // 16) * 16
            for r in range(r0, r1, chunk):
                rs.append((r, min(chunk, r1 - r)))
        out.append(rs)
    return out


def tripping_case(M, N, sb, seed):
    """-> a [R, M], b [R, N] (CPU fp32), offsets"""
    off = offsets()
    R = off[-1]
    k = torch.arange(R)
    inside = ((k >= off[3]) & (k < off[4])) | (k >= off[6] + 2752)
    a, b = orphan_case(R, M, N, sb, 30, 30, seed, low=(k % 3 == 1) & inside)
    return a, b, off


def sp16_decode(x, sb):
    """What an SP16 operand holds of ``x`` [K, C] with one power-of-two scale per (row, block of ``sb`` columns)
    (csrc/sp16.hpp): scale s with max * s in [2^14, 2^15), h = fp16(x s), l = fp16(x s - h).  -> (h + l in fp32 [K, C], inverse
    scales fp32 [K, C // sb]; all-zero blocks carry the marker 2^-126)."""
    K, C = x.shape
    xb = x.view(K, C // sb, sb)
    mx = xb.abs().amax(-1)
    _, ex = torch.frexp(mx)  # mx = m 2^ex, m in [0.5, 1)
    e = (15 - ex).clamp(max=126).to(torch.float32)
    zero = mx == 0
    scale = torch.where(zero, torch.ones_like(mx), torch.exp2(e))
    inv = torch.where(zero, torch.full_like(mx, MARKER), torch.exp2(-e))
    xs = xb * scale.unsqueeze(-1)
    h = xs.half()
    lo = (xs - h.float()).half()
    return (h.float() + lo.float()).reshape(K, C), inv


def repaired_model(a, b, sb, off):
    """The repaired grouped product on the CPU, every K range taken as repaired: element = (h + l) * inv_scale in fp32, (k,
    block) pairs with a marker scale on either side skipped, one fp32 multiply-add chain in ascending k per K range (the product
    of two fp32 numbers is exact in fp64; the sum is rounded to fp32 once per step), the ranges' slabs added in range order.
    -> fp32 [G, M, N]"""
    da, ia = sp16_decode(a, sb)
    db, ib = sp16_decode(b, b.shape[1])
    holds = (ia > 1.2e-38) & (ib > 1.2e-38)
    va = torch.where(holds.repeat_interleave(sb, dim=1), da * ia.repeat_interleave(sb, dim=1), torch.zeros_like(da))
    vb = db * ib
    out = torch.zeros((len(off) - 1, a.shape[1], b.shape[1]), dtype=torch.float32)
    for gi, rs in enumerate(ranges_of(off)):
        for r0, n in rs:
            acc = torch.zeros_like(out[gi])
            for k in range(r0, r0 + n):
                acc = (acc.double() + va[k].double().unsqueeze(1) * vb[k].double().unsqueeze(0)).float()
            out[gi] += acc
    return out
