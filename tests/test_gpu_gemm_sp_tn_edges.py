"""Split-operand weight-gradient (TN) products where their format is weakest: column blocks of A that are all zero over a K
range (the typed aggregate of an edge type with no edges), rows far below their block's largest, K tails, the documented
guard thresholds and the 2^-112 floor - through every entry point that reaches the kernel (plain, scattered / accumulating /
column range, deferred reduction, row-range loop, grouped), each against the fp64 product.

The operands are built so that the scale exponents are exactly the deficits meant: the largest magnitude of every (row, block)
of A and of every row of B is pinned to 2^PIN, and a deficit d multiplies the whole (row, block) by 2^-d."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

PIN = 3  # the largest magnitude of every (row, block): 2^3 (the other entries are clamped below it)


def ref(a, b):
    return a.double().t() @ b.double()


def mag(a, b):
    return a.double().abs().t() @ b.double().abs()


def check(got, r, m, bound, what, exact=None):
    """(a) every output finite; (b) entries whose terms are all zero (m == 0, or ``exact``) equal the fp64 reference exactly;
    (c) max |got - r| / m <= bound over the others.  -> the measured error."""
    got = got.detach().cpu().double()
    assert bool(torch.isfinite(got).all()), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite outputs"
    zero = m == 0 if exact is None else exact
    assert torch.equal(got[zero], r[zero]), f"{what}: entries without a non-zero term are not exact"
    nz = ~zero
    e = float(((got[nz] - r[nz]).abs() / m[nz]).max()) if bool(nz.any()) else 0.0
    assert e <= bound, f"{what}: max err / sum |a||b| = {e:.3e} > {bound:.0e}"
    return e


def structured(K, cols, sb, seed, deficit=None, zero=(), zero_rows=None):
    """Seeded randn [K, cols] whose largest magnitude in every (row, block of ``sb`` columns) is exactly 2^PIN, times
    2^-deficit[k, block] (integer tensor [K, cols // sb]); ``zero`` = (block, r0, r1) triples: that block zeroed over rows
    [r0, r1); ``zero_rows``: whole rows zeroed."""
    g = torch.Generator().manual_seed(seed)
    nb = cols // sb
    x = torch.randn((K, nb, sb), generator=g).clamp(-0.9 * 2.0 ** PIN, 0.9 * 2.0 ** PIN)
    at = torch.randint(0, sb, (K, nb, 1), generator=g)
    sign = torch.randint(0, 2, (K, nb, 1), generator=g).float() * 2 - 1
    x.scatter_(2, at, sign * 2.0 ** PIN)
    if deficit is not None:
        x = x * torch.exp2(-deficit.to(torch.int64).double()).float().unsqueeze(-1)
    x = x.reshape(K, cols)
    for blk, r0, r1 in zero:
        x[r0:r1, blk * sb:(blk + 1) * sb] = 0.0
    if zero_rows is not None:
        x[zero_rows] = 0.0
    return x


def lib_flag():
    from tf2_gnn_amd import _lib

    torch.cuda.synchronize()
    return _lib.load().tfgnn_sp_spread_flag(0)


def assert_quiet():
    from tf2_gnn_amd import ops

    assert lib_flag() == 0 and ops.get_gemm_mode() == ops.GEMM_F16X2


def assert_tripped():
    from tf2_gnn_amd import ops

    assert lib_flag() == 1
    ops.set_gemm_mode("f16x2")  # re-arm for what follows
    assert lib_flag() == 0


def zero_block_case(K, M, N, sb, seed, deficits, zero_until=None, b_spread=3):
    """A [K, M]: block 1 zero over rows [0, zero_until) (all of K by default); in blocks 0 and 1 every other row sits 2^-d below
    the block's largest, d cycling through ``deficits``, on rows where B's row is at B's maximum (e_b = 0).  The other rows of B
    and the other blocks of A spread over 2^b_spread.  A few whole rows of A and of B are zero.  (Both blocks share a tile for
    sb = 64 and 320; where block 1 holds data its row carries the same deficit as block 0's: the two-factor form splits the
    deficit of a row's LEAST deficient block of the tile, and a block 2^44 below another one at the same k is a real trip.)"""
    g = torch.Generator().manual_seed(seed + 1)
    nb = M // sb
    da = torch.randint(0, b_spread + 1, (K, nb), generator=g)
    db = torch.randint(0, b_spread + 1, (K, 1), generator=g)
    low = torch.arange(K) % 2 == 1
    d = torch.tensor(deficits)[(torch.arange(K) // 2) % len(deficits)]
    da[:, :2] = torch.where(low, d, torch.zeros_like(d)).unsqueeze(-1)
    db[low] = 0
    a = structured(K, M, sb, seed, deficit=da, zero=((1, 0, K if zero_until is None else zero_until),),
                   zero_rows=torch.arange(K)[5::97])
    b = structured(K, N, N, seed + 2, deficit=db, zero_rows=torch.arange(K)[11::89])
    return a, b


# sb = 64: two blocks per 128-column tile of A; 320: a tile straddles blocks 0 and 1 (the first-layer Edge-MLP gradient at
# H0 = 320); 128 / 256: whole tiles inside a block
SHAPES = [(64, 256, 128), (128, 256, 128), (256, 512, 256), (320, 640, 128)]
WIDE_DEFICITS = (32, 36, 40, 44)


@pytest.mark.parametrize("sb,M,N", SHAPES, ids=[f"sb{s[0]}" for s in SHAPES])
@pytest.mark.parametrize("K", [1, 17, 2016, 2017, 6053])
def test_two_factor_product_with_a_zero_block_and_large_deficits(dev, K, sb, M, N):
    """tfgnn_sp_gemm_tn_wide: a column block of A that is all zero over the K range carries the marker scale in every row; its
    factor must not become 2^16 (fp16 inf, times the zero fragments: NaN) when the other block's rows at k are 2^32 .. 2^44
    below their maximum.  Pair deficits up to 2^44: the guard stays quiet and nothing is lost."""
    from tf2_gnn_amd import ops

    ops.set_gemm_mode("f16x2")
    a, b = zero_block_case(K, M, N, sb, K + sb, WIDE_DEFICITS)
    got = ops.sp_gemm_tn(ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev)), wide=True)
    m = mag(a, b)
    assert not bool(m[sb:2 * sb].any())  # the zero block's output rows
    check(got, ref(a, b), m, 2e-6, f"wide K={K} sb={sb}")
    assert_quiet()


@pytest.mark.parametrize("sb,M,N", SHAPES, ids=[f"sb{s[0]}" for s in SHAPES])
def test_two_factor_product_with_a_block_zero_over_some_k_ranges(dev, sb, M, N):
    """The same block zero only over rows [0, 4100) of 6053: every K range (<= 2016 rows) that lies wholly inside the interval
    sees an all-zero block, the ranges after it do not.  Immediate call; the row-range loop of operands longer than one launch
    covers (TN_WIDE_MAX_ROWS patched to 2016, as for 10^6-row operands)."""
    from tf2_gnn_amd import ops

    ops.set_gemm_mode("f16x2")
    K = 6053
    a, b = zero_block_case(K, M, N, sb, 77 + sb, WIDE_DEFICITS, zero_until=4100)
    a_sp, b_sp = ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev))
    r, m = ref(a, b), mag(a, b)
    now = ops.sp_gemm_tn(a_sp, b_sp, wide=True)
    check(now, r, m, 2e-6, f"wide, block zero over [0, 4100), sb={sb}")
    assert_quiet()
    a2, b2 = zero_block_case(K, M, N, sb, 91 + sb, WIDE_DEFICITS)  # ... and zero over all of K
    a2_sp, b2_sp = ops.sp_split_rows(a2.to(dev), scale_block=sb), ops.sp_split_rows(b2.to(dev))
    check(ops.sp_gemm_tn(a2_sp, b2_sp, wide=True), ref(a2, b2), mag(a2, b2), 2e-6, f"wide, block zero over all of K, sb={sb}")
    keep = ops.TN_WIDE_MAX_ROWS
    try:
        ops.TN_WIDE_MAX_ROWS = 2016
        for a_, b_, a_sp_, b_sp_ in ((a, b, a_sp, b_sp), (a2, b2, a2_sp, b2_sp)):
            out = ops.sp_gemm_tn(a_sp_, b_sp_, wide=True, out=torch.empty((M, N), device=dev))
            check(out, ref(a_, b_), mag(a_, b_), 2e-6, f"wide row-range loop sb={sb}")
    finally:
        ops.TN_WIDE_MAX_ROWS = keep
    assert_quiet()


@pytest.mark.parametrize("sb", [64, 128, 320])
def test_two_factor_product_scattered_accumulated_over_a_column_range(dev, sb):
    """The zero block on the other side of the output: scatter writes the product transposed, accumulates into a random ``out``,
    and ``a_cols`` starts the first tile 64 columns before the end of the zero block (block 1): the tile holds the zero block's
    last 64 columns and the first 64 of block 2, whose rows sit 2^-32 .. 2^-44 below (as do block 3's, which shares a tile
    with block 2 for sb = 128)."""
    from tf2_gnn_amd import ops

    ops.set_gemm_mode("f16x2")
    K, N = 2017, 128
    Mt = (4 if sb < 320 else 3) * sb
    a0 = 2 * sb - 64
    Mc = Mt - a0
    g = torch.Generator().manual_seed(sb)
    da = torch.randint(0, 4, (K, Mt // sb), generator=g)
    db = torch.randint(0, 4, (K, 1), generator=g)
    low = torch.arange(K) % 3 != 0
    d = torch.tensor(WIDE_DEFICITS)[torch.arange(K) % 4]
    da[:, 2:] = torch.where(low, d, torch.zeros_like(d)).unsqueeze(-1)
    db[low] = 0
    a = structured(K, Mt, sb, 5 + sb, deficit=da, zero=((1, 0, K),), zero_rows=torch.arange(K)[3::101])
    b = structured(K, N, N, 6 + sb, deficit=db)
    base = torch.randn((N, Mc), generator=g)
    out = base.clone().to(dev)
    got = ops.sp_gemm_tn(ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev)), a_cols=(a0, Mc), wide=True,
                         out=out, scatter=(Mc, 0, 1, Mc), accumulate=True)
    ac = a[:, a0:a0 + Mc]
    pm = mag(ac, b).t()
    assert bool((pm[:, :64] == 0).all()) and not bool((pm[:, 64:] == 0).any())
    check(got, ref(ac, b).t() + base.double(), pm + base.double().abs(), 2e-6, f"wide scatter sb={sb}", exact=pm == 0)
    assert_quiet()


@pytest.mark.parametrize("transposed", [False, True])
def test_grouped_two_factor_product_with_zero_blocks_and_empty_groups(dev, transposed):
    """tfgnn_sp_gemm_tn_grouped: in group 3 block 1 of A is zero over all of the group's rows while block 0's rows sit 2^-36
    below (B at its maximum there), in group 4 the other way round at 2^-44; the empty group gives exact zeros."""
    from tf2_gnn_amd import ops

    ops.set_gemm_mode("f16x2")
    sizes = [0, 1, 5, 2016, 2017, 300]
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    R, M, N, sb = off[-1], 128, 128, 64
    g = torch.Generator().manual_seed(3 + transposed)
    da = torch.randint(0, 4, (R, 2), generator=g)
    db = torch.randint(0, 4, (R, 1), generator=g)
    low = torch.arange(R) % 2 == 1
    zero = []
    for grp, zb, dd in ((3, 1, 36), (4, 0, 44)):
        rows = torch.zeros(R, dtype=torch.bool)
        rows[off[grp]:off[grp + 1]] = True
        da[rows & low, 1 - zb] = dd
        da[rows & ~low, 1 - zb] = 0
        db[rows & low] = 0
        zero.append((zb, off[grp], off[grp + 1]))
    a = structured(R, M, sb, 21, deficit=da, zero=zero, zero_rows=torch.arange(R)[7::83])
    b = structured(R, N, N, 22, deficit=db)
    groups = ops.RowGroups(off, dev)
    out = torch.full((len(sizes), M, N), float("nan"), device=dev)
    got = ops.sp_gemm_tn_grouped(ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev)), groups, out,
                                 transposed=transposed).cpu()
    for gi in range(len(sizes)):
        sl = slice(off[gi], off[gi + 1])
        r, m = ref(a[sl], b[sl]), mag(a[sl], b[sl])
        gg = got[gi].t() if transposed else got[gi]
        if sizes[gi] == 0:
            assert torch.equal(gg, torch.zeros_like(gg)), gi
            continue
        if gi in (3, 4):
            assert not bool(m[zero[gi - 3][0] * sb:(zero[gi - 3][0] + 1) * sb].any())
        check(gg, r, m, 2e-6, f"grouped group {gi} transposed={transposed}")
    assert_quiet()


ONE_FACTOR_SHAPES = [(64, 256, 128, 2016), (128, 256, 128, 17), (320, 640, 128, 6053), (64, 256, 256, 6053)]


@pytest.mark.parametrize("sb,M,N,K", ONE_FACTOR_SHAPES)
def test_one_factor_product_with_a_zero_block(dev, sb, M, N, K):
    """tfgnn_sp_gemm_tn (one combined factor on A's fragments): the same zero-block operands at spreads of the scale products up
    to 2^13 (A's rows over 2^9, B's over 2^4) - finite, exact zeros, the fp32 error class of the existing bound.  Also over
    K ranges that hold the zero block only in part."""
    from tf2_gnn_amd import ops

    ops.set_gemm_mode("f16x2")
    for zero_until in (None, min(K, 4100)):
        a, b = zero_block_case(K, M, N, sb, K + sb + 5, (5, 7, 9), zero_until=zero_until, b_spread=4)
        a_sp, b_sp = ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev))
        got = ops.sp_gemm_tn(a_sp, b_sp)
        check(got, ref(a, b), mag(a, b), 6e-7, f"one-factor K={K} sb={sb} zero until {zero_until}")
    assert_quiet()


def test_one_factor_product_with_a_zero_block_through_the_separate_factor_pass(dev):
    """The same with the factors computed by their own pass (sp_tn_factors_kernel; TFGNN_TN_FIK=0, read once per process: a
    child process)."""
    code = (
        "import torch\n"
        "from tf2_gnn_amd import ops\n"
        "from tests.test_gpu_gemm_sp_tn_edges import check, mag, ref, zero_block_case\n"
        "dev = torch.device('cuda', 0)\n"
        "ops.set_gemm_mode('f16x2')\n"
        "for sb, M, N, K in ((64, 256, 128, 2016), (320, 640, 128, 3000)):\n"
        "    a, b = zero_block_case(K, M, N, sb, K, (5, 7, 9), b_spread=4)\n"
        "    a_sp, b_sp = ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev))\n"
        "    r, m = ref(a, b), mag(a, b)\n"
        "    check(ops.sp_gemm_tn(a_sp, b_sp), r, m, 6e-7, 'factor pass')\n"
        "torch.cuda.synchronize()\n"
        "from tf2_gnn_amd import _lib\n"
        "assert _lib.load().tfgnn_sp_spread_flag(0) == 0\n"
        "print('CHILD OK')\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TFGNN_TN_FIK="0",
               PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert res.returncode == 0 and "CHILD OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


def _threshold_operands(ea, eb, K=256, M=128, N=128, seed=0):
    """One scale block; rows 7, 100 and 201 sit 2^-ea (A) and 2^-eb (B) below every other row, which are at the maximum."""
    da = torch.zeros((K, 1), dtype=torch.int64)
    db = torch.zeros((K, 1), dtype=torch.int64)
    rows = torch.tensor([7, 100, 201])
    da[rows] = ea
    db[rows] = eb
    return structured(K, M, M, seed + 1, deficit=da), structured(K, N, N, seed + 2, deficit=db)


@pytest.mark.parametrize("ea,eb,tripped", [(20, 0, False), (10, 10, False), (0, 20, False), (21, 0, True), (11, 10, True),
                                           (0, 21, True)])
def test_one_factor_guard_threshold(dev, ea, eb, tripped):
    """sp_row_too_small (csrc/sp16.hpp): a non-zero row whose scale product is more than 2^20 below the K range's largest is
    reported - 2^-20 exactly is not.  K = 256: one K range, the reference rows and the deficient ones share it."""
    from tf2_gnn_amd import ops

    ops.set_gemm_mode("f16x2")
    a, b = _threshold_operands(ea, eb, seed=ea * 64 + eb)
    got = ops.sp_gemm_tn(ops.sp_split_rows(a.to(dev), scale_block=128), ops.sp_split_rows(b.to(dev)))
    check(got, ref(a, b), mag(a, b), 2e-6, f"one-factor e_a={ea} e_b={eb}")
    if tripped:
        assert_tripped()
    else:
        assert_quiet()


@pytest.mark.parametrize("ea,eb,tripped", [(44, 0, False), (22, 22, False), (0, 44, False), (45, 0, True), (23, 22, True),
                                           (22, 23, True), (0, 45, True)])
def test_two_factor_guard_threshold(dev, ea, eb, tripped):
    """Two-factor form (csrc/gemm_sp.hip, the factor table of the BSC kernel): a pair deficit e = e_a + e_b is split into
    F_b = 2^-floor(e / 2) and F_a = 2^-ceil(e / 2) for the row's largest non-zero block; the guard trips when either is below
    2^-22, i.e. at e = 45 and not at e = 44, however the deficit is split between the operands."""
    from tf2_gnn_amd import ops

    ops.set_gemm_mode("f16x2")
    a, b = _threshold_operands(ea, eb, seed=ea * 64 + eb + 7)
    got = ops.sp_gemm_tn(ops.sp_split_rows(a.to(dev), scale_block=128), ops.sp_split_rows(b.to(dev)), wide=True)
    check(got, ref(a, b), mag(a, b), 2e-6, f"two-factor e_a={ea} e_b={eb}")
    if tripped:
        assert_tripped()
    else:
        assert_quiet()


@pytest.mark.parametrize("wide", [False, True])
def test_rows_below_the_floor_contribute_nothing(dev, wide):
    """Block 1 of A holds rows whose largest entry lies in [2^-126, 2^-112): sp_scale_for_max gives them the marker scale, so by
    design they contribute nothing (beside deficient rows of block 0 in the two-factor form).  Finite, within 2^-111 sum_k
    |b[k, n]| of the fp64 product in that block, the usual relative bound everywhere else, no guard trip."""
    from tf2_gnn_amd import ops

    ops.set_gemm_mode("f16x2")
    K, M, N, sb = 2017, 256, 128, 64
    g = torch.Generator().manual_seed(17 + wide)
    da = torch.zeros((K, M // sb), dtype=torch.int64)
    da[:, 1] = torch.randint(PIN + 113, PIN + 127, (K,), generator=g)  # row maxima 2^-113 .. 2^-126 (normal fp32)
    if wide:
        da[1::2, 0] = 36
    a = structured(K, M, sb, 31 + wide, deficit=da)
    b = structured(K, N, N, 32 + wide)
    assert float(a[:, sb:2 * sb].abs().max()) < 2.0 ** -112 and float(a[:, sb:2 * sb].abs().max()) >= 2.0 ** -126
    got = ops.sp_gemm_tn(ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev)), wide=wide).cpu().double()
    assert bool(torch.isfinite(got).all())
    r, m = ref(a, b), mag(a, b)
    tiny = slice(sb, 2 * sb)
    floor = 2.0 ** -111 * b.double().abs().sum(0)
    assert bool(((got[tiny] - r[tiny]).abs() <= floor).all())
    rest = torch.ones(M, dtype=torch.bool)
    rest[tiny] = False
    check(got[rest], r[rest], m[rest], 2e-6 if wide else 6e-7, f"floor wide={wide}")
    assert_quiet()
