"""In-stream repair of tripped split-operand weight-gradient (TN) products (``ops.set_guard_repair``; include/tfgnn.h
tfgnn_sp_guard_repair): with repair armed, a product whose spread guard trips is recomputed in fp32 from its SP16 operands on the
stream, before its reduce pass - the gradient of that very pass is right, the host flag stays down, the mode stays f16x2, and a
replayed hipGraph step gets the same.

Operands that separate a repaired product from an unrepaired one ("orphan columns"): rows k % 3 == 1 sit 2^-ea (A) and 2^-eb (B)
below all the others - beyond the product's guard - and the columns m % 8 == 5 of A are zero on every OTHER row, so their outputs
receive terms from the deficient rows only.  A product that drops those rows is off by 0.15 .. 1.0 of sum |a||b| there; the
repair's arithmetic (SP16 decode, fp32 FMA) gives 3e-7 or less (CPU model of it at K = 17 / 2017 / 6053: 2.6e-7, 9.7e-8,
4.8e-8).  The bound is the project's own for in-range TN products: 2e-6 of sum |a||b| per entry."""
import contextlib
import os
import subprocess
import sys
import warnings

import pytest
import torch

from tests.helpers import record_parity
from tests.test_gpu_gemm_sp_tn_edges import PIN, check, mag, ref, structured, zero_block_case  # noqa: F401

pytestmark = pytest.mark.gpu

BOUND = 2e-6


@contextlib.contextmanager
def armed():
    """Mode f16x2, repair armed, counters at zero; the previous switch state, the mode and the counters are put back."""
    from tf2_gnn_amd import ops

    ops.set_gemm_mode("f16x2")
    prev = ops.set_guard_repair(True)
    ops.repair_stats(reset=True)
    try:
        yield ops
    finally:
        torch.cuda.synchronize()
        ops.set_guard_repair(prev)
        ops.set_gemm_mode("f16x2")
        ops.repair_stats(reset=True)


def host_flag():
    from tf2_gnn_amd import _lib

    torch.cuda.synchronize()
    return _lib.load().tfgnn_sp_spread_flag(0)


def orphan_case(K, M, N, sb, ea, eb, seed, low=None):
    """-> a [K, M], b [K, N] (CPU fp32).  ``low``: the deficient rows (default k % 3 == 1)."""
    k = torch.arange(K)
    if low is None:
        low = k % 3 == 1
    da = torch.zeros((K, M // sb), dtype=torch.int64)
    db = torch.zeros((K, 1), dtype=torch.int64)
    da[low] = ea
    db[low] = eb
    a = structured(K, M, sb, seed, deficit=da)
    b = structured(K, N, N, seed + 1, deficit=db)
    orphan = torch.arange(M) % 8 == 5
    a[(~low).unsqueeze(1) & orphan.unsqueeze(0)] = 0.0
    return a, b


def split(ops, a, b, sb, dev):
    return ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev))


# one-factor form: a deficit of 2^30 on either operand or on both is beyond its 2^20; two-factor form: 2^30 + 2^30 is beyond the
# 2^22 per factor (a pair deficit of 2^30 alone is within that form's range and trips nothing)
FORMS = [(False, 30, 0), (False, 0, 30), (False, 30, 30), (True, 30, 30)]
SHAPES = [(64, 256, 128), (320, 640, 128)]


@pytest.mark.parametrize("sb,M,N", SHAPES, ids=[f"sb{s[0]}" for s in SHAPES])
@pytest.mark.parametrize("K", [17, 2017, 6053])
@pytest.mark.parametrize("wide,ea,eb", FORMS, ids=[f"{'wide' if f[0] else 'one'}-{f[1]}-{f[2]}" for f in FORMS])
def test_repaired_product(dev, wide, ea, eb, K, sb, M, N):
    """Plain call: the orphan outputs are right (a repair that does nothing leaves them off by 0.15 .. 1.0), the host flag stays
    down, the mode stays f16x2, one product repaired per launch."""
    with armed() as ops:
        a, b = orphan_case(K, M, N, sb, ea, eb, K + sb + ea)
        a_sp, b_sp = split(ops, a, b, sb, dev)
        got = ops.sp_gemm_tn(a_sp, b_sp, wide=wide)
        r, m = ref(a, b), mag(a, b)
        what = f"repaired {'two' if wide else 'one'}-factor product K={K} sb={sb} e_a={ea} e_b={eb}"
        orphan = torch.arange(M) % 8 == 5
        e_orphan = float(((got.cpu().double() - r).abs() / m)[orphan].max())
        print(f"{what}: orphan rows err / sum |a||b| = {e_orphan:.3e}")
        e = check(got, r, m, BOUND, what)
        record_parity(f"repaired sp_gemm_tn{'_wide' if wide else ''} error / sum |a||b| (orphan columns)",
                      max_err_over_sum_abs_products=e, bound=BOUND)
        assert host_flag() == 0 and ops.get_gemm_mode() == ops.GEMM_F16X2
        stats = ops.repair_stats()
        assert stats == {"armed_products": 1, "repaired_products": 1}, stats


@pytest.mark.parametrize("wide", [False, True])
def test_trip_confined_to_one_k_range_repairs_the_whole_product(dev, wide):
    """K = 6053: deficient rows only in [4100, 6053) - the K ranges before them see nothing wrong; one trip word per product, the
    whole product is recomputed and meets the bound."""
    with armed() as ops:
        K, sb, M, N = 6053, 64, 256, 128
        k = torch.arange(K)
        a, b = orphan_case(K, M, N, sb, 30, 30, 71 + wide, low=(k % 3 == 1) & (k >= 4100))
        a_sp, b_sp = split(ops, a, b, sb, dev)
        got = ops.sp_gemm_tn(a_sp, b_sp, wide=wide)
        e = check(got, ref(a, b), mag(a, b), BOUND, f"trip in the last K ranges only, wide={wide}")
        record_parity("repaired sp_gemm_tn error / sum |a||b| (trip confined to rows 4100..)", max_err_over_sum_abs_products=e,
                      bound=BOUND)
        assert host_flag() == 0 and ops.get_gemm_mode() == ops.GEMM_F16X2
        assert ops.repair_stats()["repaired_products"] == 1


@pytest.mark.parametrize("wide", [False, True])
def test_repaired_product_scattered_accumulated_over_a_column_range(dev, wide):
    """The repaired slabs land through the product's own reduce pass: ``out`` pre-filled, accumulate, groups of ``sb`` result
    rows written transposed ([G, N, sb]) and ``a_cols`` starting one block in.  The pre-fill is added exactly once."""
    with armed() as ops:
        K, sb, M, N = 2017, 64, 256, 128
        a, b = orphan_case(K, M, N, sb, 30, 30, 5 + wide)
        a_sp, b_sp = split(ops, a, b, sb, dev)
        Mc = M - sb
        G = Mc // sb
        base = torch.randn((G, N, sb), generator=torch.Generator().manual_seed(3))
        out = base.clone().to(dev)
        ops.sp_gemm_tn(a_sp, b_sp, a_cols=(sb, Mc), out=out, scatter=(sb, N * sb, 1, sb), accumulate=True, wide=wide)
        ac = a[:, sb:]
        want = ref(ac, b).reshape(G, sb, N).permute(0, 2, 1) + base.double()
        pm = mag(ac, b).reshape(G, sb, N).permute(0, 2, 1)
        e = check(out, want, pm + base.double().abs(), BOUND, f"repaired scatter wide={wide}", exact=pm == 0)
        record_parity("repaired sp_gemm_tn error / sum |a||b| (scatter, accumulate, column range)",
                      max_err_over_sum_abs_products=e, bound=BOUND)
        assert host_flag() == 0 and ops.repair_stats()["repaired_products"] == 1


@pytest.mark.parametrize("wide", [False, True])
def test_quiet_operands_are_bit_equal_armed_and_disarmed(dev, wide):
    """Nothing beyond the guard: the repair kernel returns at its first load and the product is the unarmed one, bit for bit."""
    from tf2_gnn_amd import ops

    K, sb, M, N = 2017, 64, 256, 128
    a, b = zero_block_case(K, M, N, sb, 13, (5, 7, 9), b_spread=4)
    ops.set_gemm_mode("f16x2")
    was = ops.set_guard_repair(False)
    try:
        a_sp, b_sp = split(ops, a, b, sb, dev)
        plain = ops.sp_gemm_tn(a_sp, b_sp, wide=wide).clone()
    finally:
        ops.set_guard_repair(was)
    with armed():
        got = ops.sp_gemm_tn(a_sp, b_sp, wide=wide)
        assert torch.equal(got, plain)
        assert ops.repair_stats() == {"armed_products": 1, "repaired_products": 0}
        assert host_flag() == 0


def test_the_trip_word_is_zeroed_per_product(dev):
    """A tripping product and then a quiet one of the same shape on the same stream share a workspace, hence the trip word:
    the second one's memset node clears it - one repair, and the quiet product is its unarmed twin bit for bit."""
    from tf2_gnn_amd import ops

    K, sb, M, N = 2017, 64, 256, 128
    a, b = orphan_case(K, M, N, sb, 30, 30, 23)
    qa, qb = zero_block_case(K, M, N, sb, 29, (5, 7, 9), b_spread=4)
    ops.set_gemm_mode("f16x2")
    was = ops.set_guard_repair(False)
    try:
        qa_sp, qb_sp = split(ops, qa, qb, sb, dev)
        plain = ops.sp_gemm_tn(qa_sp, qb_sp).clone()
    finally:
        ops.set_guard_repair(was)
    with armed():
        a_sp, b_sp = split(ops, a, b, sb, dev)
        first = ops.sp_gemm_tn(a_sp, b_sp)
        second = ops.sp_gemm_tn(qa_sp, qb_sp)
        check(first, ref(a, b), mag(a, b), BOUND, "tripping product in front of a quiet one")
        assert torch.equal(second, plain)
        assert ops.repair_stats() == {"armed_products": 2, "repaired_products": 1}
        assert host_flag() == 0


def test_repair_through_the_separate_factor_pass(dev):
    """The same with the factors computed by their own pass (TFGNN_TN_FIK=0, read once per process: one child process): the
    factor pass reports into the trip word, the repair sets the one reference scale per block to 1."""
    code = (
        "import torch\n"
        "from tf2_gnn_amd import _lib, ops\n"
        "from tests.test_gpu_tn_repair import BOUND, orphan_case\n"
        "from tests.test_gpu_gemm_sp_tn_edges import check, mag, ref\n"
        "dev = torch.device('cuda', 0)\n"
        "ops.set_gemm_mode('f16x2')\n"
        "ops.set_guard_repair(True)\n"
        "n = 0\n"
        "for sb, M, N, K in ((64, 256, 128, 2016), (320, 640, 128, 3000)):\n"
        "    for ea, eb in ((30, 0), (0, 30), (30, 30)):\n"
        "        a, b = orphan_case(K, M, N, sb, ea, eb, K + ea)\n"
        "        a_sp, b_sp = ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev))\n"
        "        e = check(ops.sp_gemm_tn(a_sp, b_sp), ref(a, b), mag(a, b), BOUND, 'factor pass, repaired')\n"
        "        n += 1\n"
        "        print('ERR', sb, K, ea, eb, e)\n"
        "torch.cuda.synchronize()\n"
        "assert _lib.load().tfgnn_sp_spread_flag(0) == 0 and ops.get_gemm_mode() == ops.GEMM_F16X2\n"
        "assert ops.repair_stats() == {'armed_products': n, 'repaired_products': n}, ops.repair_stats()\n"
        "print('CHILD OK')\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TFGNN_TN_FIK="0", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert res.returncode == 0 and "CHILD OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    worst = max(float(line.split()[-1]) for line in res.stdout.splitlines() if line.startswith("ERR"))
    record_parity("repaired sp_gemm_tn error / sum |a||b| (separate factor pass)", max_err_over_sum_abs_products=worst, bound=BOUND)


# ---- through the layers --------------------------------------------------------------------------------------------------
def _two_component_graph(V, L, edges_per_type_and_component, seed):
    import numpy as np

    rng = np.random.default_rng(seed)
    half = V // 2
    adjs = []
    for _ in range(L):
        parts = [rng.integers(0, half, size=(edges_per_type_and_component, 2)) + c * half for c in range(2)]
        a = np.concatenate(parts, axis=0).astype(np.int32)
        rng.shuffle(a, axis=0)
        adjs.append(a)
    return adjs


def test_layer_weight_gradient_through_mp_backward_is_repaired(dev):
    """RGCN layer, the product inside tfgnn_mp_backward.  Two disconnected components of 192 nodes: the rows of dOut of component
    1 are 2^-40 of component 0's, and the input columns 64..127 are zero on component 0 - rows 64..127 of every relation's dW
    receive terms from component 1 only, which an unrepaired one-factor product drops.  Their error, relative to the largest
    fp64 entry of that slice, is held to max(1e-5, 2 x the same quantity in mode bf16x3) (the exact kernels, not the code under
    test); the other rows to the existing 1e-5 of the relation's largest entry."""
    from oracle import tf2gnn_oracle as orc
    from tests.helpers import ForcedKinks, mp_weights_from_layer, to_dev
    from tests.test_gpu_layers import _build, _to64
    from tf2_gnn_amd.layers import MessagePassingInput

    V, L, H = 384, 2, 128
    adjs = _two_component_graph(V, L, 1050, seed=5)
    adj_t = [torch.from_numpy(a) for a in adjs]
    gen = torch.Generator().manual_seed(2)
    X = torch.randn((V, H), generator=gen)
    X[: V // 2, 64:] = 0.0
    dOut = torch.randn((V, H), generator=gen)
    dOut[V // 2:] *= 2.0 ** -40

    def slice_errors(ops, mode):
        ops.set_gemm_mode(mode)
        layer, p = _build("RGCN", {"hidden_dim": H}, H, L)
        inp = MessagePassingInput(X.to(dev), to_dev(adjs, dev))
        out = layer(inp, training=True)
        assert bool(layer._ctx.get("f16x2")) == (mode == "f16x2")
        layer.backward(dOut.to(dev))
        torch.cuda.synchronize()
        w64 = _to64(mp_weights_from_layer(layer))
        leaves = []
        for l in range(L):
            w64["edge_mlps"][l] = [k.requires_grad_(True) for k in w64["edge_mlps"][l]]
            leaves += w64["edge_mlps"][l]
        mask = (out > 0).cpu()
        with ForcedKinks(lambda i, x: mask):
            want = orc.message_passing_call("rgcn", p, w64, X.double(), adj_t)
        grads = torch.autograd.grad((want * dOut.double()).sum(), leaves)
        orphan, rest = [], []
        for l in range(L):
            r = grads[l]
            d = (layer._edge_type_mlps.vars[l][0].grad.cpu().double() - r).abs()
            assert float(r[64:].abs().max()) > 0 and float(r[64:].abs().max()) < 2.0 ** -30 * float(r.abs().max())
            orphan.append(float(d[64:].max()) / float(r[64:].abs().max()))
            rest.append(float(d[:64].max()) / float(r.abs().max()))
        return orphan, rest

    with armed() as ops:
        exact_orphan, _ = slice_errors(ops, "bf16x3")
        ops.set_gemm_mode("f16x2")
        ops.repair_stats(reset=True)
        got_orphan, got_rest = slice_errors(ops, "f16x2")
        for l in range(L):
            bound = max(1e-5, 2 * exact_orphan[l])
            print(f"relation {l}: dW[64:128] err / largest of the slice = {got_orphan[l]:.3e} (bf16x3: {exact_orphan[l]:.3e}), "
                  f"dW[:64] err / largest = {got_rest[l]:.3e}")
            record_parity(f"RGCN dW rows fed by the 2^-40 component only, relation {l} (repair armed)",
                          max_err_over_largest_of_slice=got_orphan[l], bound=bound)
            record_parity(f"RGCN dW rows fed by the 2^-40 component only, relation {l} (bf16x3)",
                          max_err_over_largest_of_slice=exact_orphan[l], bound=bound)
            assert got_orphan[l] <= bound, (l, got_orphan[l], exact_orphan[l])
            assert got_rest[l] <= 1e-5, (l, got_rest[l])
        assert host_flag() == 0 and ops.get_gemm_mode() == ops.GEMM_F16X2
        assert ops.repair_stats()["repaired_products"] >= 1


def _stack(dev):
    from tf2_gnn_amd.data import make_synthetic_batch
    from tf2_gnn_amd.layers import GNN, GNNInput

    V, E, L, H = 384, 4200, 3, 128
    feats, adjs = make_synthetic_batch(V, E, L, H, seed=4)
    params = GNN.get_default_hyperparameters("rgcn")
    params.update({"hidden_dim": H, "num_layers": 2, "dense_every_num_layers": 10000, "residual_every_num_layers": 10000,
                   "global_exchange_every_num_layers": 10000, "layer_input_dropout_rate": 0.0})
    inp = GNNInput(torch.from_numpy(feats).to(dev), tuple(torch.from_numpy(a).to(dev) for a in adjs),
                   torch.zeros(V, dtype=torch.int32, device=dev), 1)
    gen = torch.Generator().manual_seed(9)
    # per-node gradient magnitudes over 2^60: the rows of the transposed gather are spread far beyond 2^20
    dOut = (torch.randn((V, H), generator=gen) * torch.exp2(torch.randint(-40, 20, (V, 1), generator=gen).float())).to(dev)
    return params, inp, dOut


def _new_gnn(params):
    from tf2_gnn_amd.layers import GNN
    from tf2_gnn_amd.layers.message_passing import set_seed

    set_seed(3)
    return GNN(params)


def test_an_unchecked_pass_of_a_stack_hands_out_repaired_gradients(dev):
    """2-layer RGCN stack, dOut rows spread over 2^60, no synchronous guard passes: the pass that would have tripped the guard
    repairs its own products - no warning, host flag down, no policy stage taken, gradients those of the exact kernels."""
    from tf2_gnn_amd import guard

    params, inp, dOut = _stack(dev)
    with armed() as ops:
        ops.set_gemm_mode("bf16x3")
        twin = _new_gnn(params)
        twin(inp, training=True)
        twin.backward(dOut)
        torch.cuda.synchronize()
        exact = [v.grad.clone() for v in twin.trainable_variables]
        ops.set_gemm_mode("f16x2")
        ops.repair_stats(reset=True)
        guard.reset_warned()  # (the warning is issued once per process)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            gnn = _new_gnn(params)
            gnn.guard.sync_passes_left = 0
            gnn(inp, training=True)
            gnn.guard.sync_passes_left = 0
            gnn.backward(dOut)
            torch.cuda.synchronize()
            assert ops.get_gemm_mode() == ops.GEMM_F16X2
        assert not any("spread" in str(x.message) for x in w), [str(x.message) for x in w]
        assert host_flag() == 0
        assert gnn.guard_state()["stage"] == "none"
        assert ops.repair_stats()["repaired_products"] > 0
        for v, b in zip(gnn.trainable_variables, exact):
            scale = max(float(b.abs().max()), 1e-30)
            err = float((v.grad - b).abs().max()) / scale
            print(f"{v.name}: |repaired - bf16x3| / largest = {err:.3e}")
            assert err <= 1e-5, (v.name, err)


@contextlib.contextmanager
def _epoch_zero_afterwards():
    """Every replay advances the dropout epoch word; every other test draws the masks of epoch 0."""
    from tf2_gnn_amd import ops

    try:
        yield
    finally:
        ops.dropout_epoch_set(0)
        torch.cuda.synchronize()


def test_a_replayed_step_repairs_itself(dev):
    """The same stack and dOut as one hipGraph: every replay repairs its products on the device - gradients bit-equal to an eager
    armed step of a twin model, no trip reported, as many repairs per replay as per eager step."""
    from tf2_gnn_amd import CapturedStep

    params, inp, dOut = _stack(dev)
    with armed() as ops, _epoch_zero_afterwards():
        twin = _new_gnn(params)
        twin(inp, training=True)
        twin.backward(dOut)
        per_step = ops.repair_stats(reset=True)["repaired_products"]
        assert per_step > 0
        eager = [v.grad.clone() for v in twin.trainable_variables]

        gnn = _new_gnn(params)
        step = CapturedStep(lambda: (gnn(inp, training=True), gnn.backward(dOut), [v.grad for v in gnn.trainable_variables]))
        step.capture()  # four eager steps first
        before = ops.repair_stats()["repaired_products"]
        assert before == 4 * per_step
        for i in range(2):
            res = step.replay()
            torch.cuda.synchronize()
            assert ops.repair_stats()["repaired_products"] == before + (i + 1) * per_step
            for v, g, e in zip(gnn.trainable_variables, res[2], eager):
                assert torch.equal(g, e), v.name
        assert not step.guard_tripped()
        assert ops.get_gemm_mode() == ops.GEMM_F16X2
