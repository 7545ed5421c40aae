"""The 320-column NT product runs eight waves of 32 x 160 per 128 x 320 tile, two per SIMD, with the ring's DMAs issued every
other k16 step for two steps (csrc/gemm_sp.hip gemm_sp_nt_kernel, SpGeo<5, 1>).  MFMA instruction, k order, order of the piece
products, K-split boundaries and the split-order addition did not change, so every output bit stays where it was: the checks are
bit-identity with the parent commit (hashes recorded there), the fp64 product behind every case, flags of the in-launch K split
back at zero after a launch, and a captured forward / backward pair replayed to the eager bits.

Cases: tools/record_nt_epilogue_bits.py ``eight_waves_lists()`` - N = 320; M in {31, 32, 33, 96, 97, 127, 128, 129} (the 32-row
boundaries of the new wave shape and the tile edge); K in {16, 48, 80, 112, 320} (one k16 step; fewer steps than the ring has
stages; odd and even step counts - the DMAs are issued on even steps); the five routes and ten epilogue forms of the epilogue
record; grouped calls at K = 48 and 320 (groups of 1, 70, 0, 130, 63 rows); K splits in two (K = 480) and in four (K = 960) at
M = 257, each launched twice back to back.

Bounds (those tests/test_gpu_gemm_sp.py applies to the same product forms, |got - ref| <= tol * max(1, |ref|)):
  the bare product      1e-5 of max(1, 0.05 sqrt(K)) (test_gemm_nt_matches_fp64, test_gemm_nt_k_split_inside_the_launch)
  epilogue forms        2e-5 (test_gemm_nt_epilogues)
  grouped products      1e-5 (test_grouped_products_on_split_operands)
  split output          the fp32 result is the plain product's bit for bit and the SP16 form is the split of exactly those
                        values: same scales, same fp16 values"""
import json

import pytest
import torch

from tests import test_gpu_nt_epilogue_flight as flight
from tests.helpers import assert_close

pytestmark = pytest.mark.gpu

rec = flight.rec
SHAPES, GROUPED, KSPLIT = rec.eight_waves_lists()


@pytest.fixture(scope="module")
def golden():
    return json.loads((flight.ROOT / "tests" / "golden" / "nt_eight_waves_parent_bits.json").read_text())


@pytest.fixture(autouse=True)
def epoch_zero():
    from tf2_gnn_amd import ops

    ops.dropout_epoch_set(0)  # the recorded masks are those of epoch 0
    yield
    ops.dropout_epoch_set(0)


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_shape_reproduces_the_parent_bits_and_the_fp64_product(dev, golden, shape):
    flight.test_shape_reproduces_the_parent_bits_and_the_fp64_product(dev, golden, shape)


@pytest.mark.parametrize("shape", GROUPED, ids=[s[0] for s in GROUPED])
def test_grouped_call_reproduces_the_parent_bits_and_the_fp64_product(dev, golden, shape):
    flight.test_grouped_call_reproduces_the_parent_bits_and_the_fp64_product(dev, golden, shape)


@pytest.mark.parametrize("shape", KSPLIT, ids=[s[0] for s in KSPLIT])
def test_k_split_reproduces_the_parent_bits_twice_and_the_fp64_product(dev, golden, shape):
    """both launches split K (the count of split launches says so) and give the recorded bits, no reducer timed out, and behind
    EVERY launch all flag words of the workspace (its first 64 KB) read zero.  Equal results of the two launches would not show
    the reset: the operands are the same, so a reducer that found a stale flag would add the slabs the first launch left, which
    hold the very values its producers are about to write."""
    from tf2_gnn_amd import ops

    name, M, N, K, _, S = shape
    assert min(4, (K // 16) // 15) == S and -(-M // 128) * S <= 232, "the shape no longer splits K this many ways"
    ops.sp_gemm_nt_splitk(True)
    d = rec.device_inputs(shape[:5], dev)
    _, _, before = ops.sp_gemm_nt_splitk()
    flags_left = {}

    def read_flags(key):
        torch.cuda.synchronize()
        flags_left[key] = int(ops._SPLITK_WS["ws"][:65536].view(torch.int32).count_nonzero())

    res = rec.run_ksplit(shape, dev, d, after_launch=read_flags)
    torch.cuda.synchronize()
    assert len(flags_left) == 2 * len(rec.KSPLIT_FORMS) and not any(flags_left.values()), f"{name}: flags left set {flags_left}"
    on, timed_out, after = ops.sp_gemm_nt_splitk()
    assert on and not timed_out and after == before + 2 * len(rec.KSPLIT_FORMS), "the products under test did not split"
    got = rec.hashes(name, res)
    wrong = [k for k in got if golden.get(k) != got[k]]
    assert not wrong, wrong
    h = rec.host_inputs(shape[:5])
    scale = max(1.0, 0.05 * K ** 0.5)
    for form in rec.KSPLIT_FORMS:
        assert torch.equal(res[f"{form} first"], res[f"{form} second"]), f"{name} {form}: second launch"
        ref = flight._reference(form, h, {})
        tol = flight.TOL_PRODUCT if form == "fwd" else flight.TOL_EPILOGUE
        assert_close(res[f"{form} first"].cpu() / scale, (ref / scale).float(), tol=tol, what=f"{name} {form}")


def test_the_record_holds_exactly_these_cases(golden):
    want = ({f"{s[0]} | {form}" for s in SHAPES for form in rec.FORMS} | {f"{s[0]} | {form}" for s in GROUPED for form in rec.GROUPED_FORMS}
            | {f"{s[0]} | {form}" for s in KSPLIT for form in rec.KSPLIT_FORMS})
    assert set(golden) == want


def test_captured_forward_backward_pair_replays_to_the_eager_bits(dev):
    """a 2-layer RGCN stack at V = 2500, H = 320 in f16x2 mode: one forward / backward pair captured into a hipGraph and replayed
    twice, both replays equal to the eager run bit for bit.  (The same capture as tests/test_gpu_nt_epilogue_flight.py's test of
    that name, called from here because the issue of this geometry lists it: the suite runs it twice, 0.1 s each.)"""
    flight.test_captured_forward_backward_pair_replays_to_the_eager_bits(dev)
