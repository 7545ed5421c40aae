"""In-stream repair of the GROUPED split-operand weight-gradient product (``ops.sp_gemm_tn_grouped`` with
``ops.set_guard_repair(True)``; include/tfgnn.h tfgnn_sp_gemm_tn_grouped): the product's guard reports into one trip word per K
range of its split table, and the repair kernel rewrites the slabs of the ranges that tripped - and only those - in fp32 from
the SP16 operands, before the grouped reduce pass.  The per-relation MLP weight gradients of RGIN (the compact-row route of
GNN_Edge_MLP) are that product: with repair armed an RGIN backward pass that trips the guard hands out right gradients, keeps
the host flag down and its stack's policy at stage "none", and a replayed hipGraph step gets the same.

Operands: tests/tn_repair_grouped_reference.py (its CPU model of the repair's arithmetic gives 4.2e-7 / 3.8e-7 of sum |a||b| on
them: tests/test_tn_repair_grouped_host.py).  The bound is the project's own for in-range TN products, ``BOUND`` = 2e-6 of
sum |a||b| per entry; the arithmetic is that of the plain products' repair, over ranges of at most 2016 rows."""
import warnings

import numpy as np
import pytest
import torch

from tests import tn_repair_grouped_reference as grp
from tests.helpers import record_parity
from tests.test_gpu_gemm_sp_tn_edges import check, mag, ref, structured, zero_block_case
from tests.test_gpu_tn_repair import BOUND, _epoch_zero_afterwards, _new_gnn, armed, host_flag

pytestmark = pytest.mark.gpu


def _split(ops, a, b, sb, dev):
    return ops.sp_split_rows(a.to(dev), scale_block=sb), ops.sp_split_rows(b.to(dev))


def _grouped(ops, a_sp, b_sp, groups, M, N, transposed, dev):
    out = torch.full((groups.num_groups, N, M) if transposed else (groups.num_groups, M, N), float("nan"), device=dev)
    return ops.sp_gemm_tn_grouped(a_sp, b_sp, groups, out, transposed=transposed)


def _disarmed(ops, fn):
    """fn() with repair off and mode f16x2 -> (its result, the host flag after it); the mode is re-armed afterwards."""
    ops.set_gemm_mode("f16x2")
    was = ops.set_guard_repair(False)
    try:
        got = fn().clone()
        flag = host_flag()
    finally:
        ops.set_guard_repair(was)
        ops.set_gemm_mode("f16x2")  # re-arm for what follows (a trip demoted the mode)
    assert host_flag() == 0
    return got, flag


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("M,N,sb", grp.SHAPES, ids=[f"m{s[0]}_sb{s[2]}" for s in grp.SHAPES])
def test_tripped_ranges_are_repaired_and_quiet_groups_untouched(dev, M, N, sb, transposed):
    """Groups of 0, 1, 5, 2016, 2017, 300 and 4100 rows; group 3 and the last of group 6's three K ranges hold pairs at 2^-60.
    Armed: every group meets BOUND (an unrepaired orphan column is off by 0.15 .. 1.0), the empty group is exact zeros, host
    flag down, mode f16x2, ONE product repaired; the groups without a tripping range equal the disarmed run bit for bit."""
    from tf2_gnn_amd import ops

    a, b, off = grp.tripping_case(M, N, sb, 40 + M)
    groups = ops.RowGroups(off, dev)
    assert groups.tn_tables()[2] == 9
    ops.set_gemm_mode("f16x2")
    a_sp, b_sp = _split(ops, a, b, sb, dev)
    plain, flag = _disarmed(ops, lambda: _grouped(ops, a_sp, b_sp, groups, M, N, transposed, dev))
    assert flag == 1  # (the operands do trip)
    with armed():
        got = _grouped(ops, a_sp, b_sp, groups, M, N, transposed, dev)
        assert host_flag() == 0 and ops.get_gemm_mode() == ops.GEMM_F16X2
        stats = ops.repair_stats()
        assert stats == {"armed_products": 1, "repaired_products": 1}, stats
        orphan = torch.arange(M) % 8 == 5
        worst = 0.0
        for gi, n in enumerate(grp.SIZES):
            gg, pp = (got[gi].t(), plain[gi].t()) if transposed else (got[gi], plain[gi])
            if n == 0:
                assert torch.equal(gg, torch.zeros_like(gg)), gi
                continue
            sl = slice(off[gi], off[gi + 1])
            r, m = ref(a[sl], b[sl]), mag(a[sl], b[sl])
            what = f"grouped, armed: group {gi} M={M} sb={sb} transposed={transposed}"
            if gi in grp.TRIPPING_RANGES:
                assert bool((m[orphan] > 0).all())
                e_plain = float(((pp.cpu().double() - r).abs() / m)[orphan].max())
                e_orphan = float(((gg.cpu().double() - r).abs() / m)[orphan].max())
                print(f"{what}: orphan rows err / sum |a||b| = {e_orphan:.3e} (disarmed: {e_plain:.3e})")
            else:
                assert torch.equal(gg, pp), what
            worst = max(worst, check(gg, r, m, BOUND, what))
        record_parity("repaired sp_gemm_tn_grouped error / sum |a||b| (orphan columns, one of three ranges tripping)",
                      max_err_over_sum_abs_products=worst, bound=BOUND)


def _quiet_case(transposed):
    """The operands of test_grouped_two_factor_product_with_zero_blocks_and_empty_groups (tests/test_gpu_gemm_sp_tn_edges.py)."""
    sizes = [0, 1, 5, 2016, 2017, 300]
    off = grp.offsets(sizes)
    R, M, N, sb = off[-1], 128, 128, 64
    g = torch.Generator().manual_seed(3 + transposed)
    da = torch.randint(0, 4, (R, 2), generator=g)
    db = torch.randint(0, 4, (R, 1), generator=g)
    low = torch.arange(R) % 2 == 1
    zero = []
    for group, zb, dd in ((3, 1, 36), (4, 0, 44)):
        rows = torch.zeros(R, dtype=torch.bool)
        rows[off[group]:off[group + 1]] = True
        da[rows & low, 1 - zb] = dd
        da[rows & ~low, 1 - zb] = 0
        db[rows & low] = 0
        zero.append((zb, off[group], off[group + 1]))
    a = structured(R, M, sb, 21, deficit=da, zero=zero, zero_rows=torch.arange(R)[7::83])
    b = structured(R, N, N, 22, deficit=db)
    return a, b, off, M, N, sb


@pytest.mark.parametrize("transposed", [False, True])
def test_quiet_operands_are_bit_equal_armed_and_disarmed(dev, transposed):
    """Nothing beyond the guard (pair deficits up to 2^44): every repair workgroup returns at its first load."""
    from tf2_gnn_amd import ops

    a, b, off, M, N, sb = _quiet_case(transposed)
    groups = ops.RowGroups(off, dev)
    ops.set_gemm_mode("f16x2")
    a_sp, b_sp = _split(ops, a, b, sb, dev)
    plain, flag = _disarmed(ops, lambda: _grouped(ops, a_sp, b_sp, groups, M, N, transposed, dev))
    assert flag == 0
    with armed():
        got = _grouped(ops, a_sp, b_sp, groups, M, N, transposed, dev)
        assert torch.equal(got, plain)
        assert ops.repair_stats() == {"armed_products": 1, "repaired_products": 0}
        assert host_flag() == 0


def test_the_tail_is_zeroed_per_product(dev):
    """A tripping grouped product and then a quiet one over the same groups on the same stream share a workspace, hence the trip
    words and the counted word: the second one's memset node clears them - one repair, and the quiet product is its disarmed
    twin bit for bit."""
    from tf2_gnn_amd import ops

    M, N, sb = 128, 128, 64
    a, b, off = grp.tripping_case(M, N, sb, 7)
    qa, qb = zero_block_case(off[-1], M, N, sb, 29, (5, 7, 9), b_spread=4)
    groups = ops.RowGroups(off, dev)
    ops.set_gemm_mode("f16x2")
    qa_sp, qb_sp = _split(ops, qa, qb, sb, dev)
    plain, flag = _disarmed(ops, lambda: _grouped(ops, qa_sp, qb_sp, groups, M, N, False, dev))
    assert flag == 0
    with armed():
        a_sp, b_sp = _split(ops, a, b, sb, dev)
        first = _grouped(ops, a_sp, b_sp, groups, M, N, False, dev).clone()
        second = _grouped(ops, qa_sp, qb_sp, groups, M, N, False, dev)
        for gi in (3, 6):
            sl = slice(off[gi], off[gi + 1])
            check(first[gi], ref(a[sl], b[sl]), mag(a[sl], b[sl]), BOUND, f"tripping grouped product in front of a quiet one, group {gi}")
        assert torch.equal(second, plain)
        assert ops.repair_stats() == {"armed_products": 2, "repaired_products": 1}
        assert host_flag() == 0


def test_disarmed_the_grouped_product_reports_through_the_host_flag(dev):
    """No behaviour change with the switch off: the tripping operands raise the library-wide flag, nothing is counted."""
    from tf2_gnn_amd import ops

    M, N, sb = 128, 128, 64
    a, b, off = grp.tripping_case(M, N, sb, 40 + M)
    groups = ops.RowGroups(off, dev)
    ops.set_gemm_mode("f16x2")
    ops.repair_stats(reset=True)
    a_sp, b_sp = _split(ops, a, b, sb, dev)
    got, flag = _disarmed(ops, lambda: _grouped(ops, a_sp, b_sp, groups, M, N, False, dev))
    assert flag == 1
    assert ops.repair_stats() == {"armed_products": 0, "repaired_products": 0}
    sl = slice(off[4], off[5])  # a quiet group is right as ever
    check(got[4], ref(a[sl], b[sl]), mag(a[sl], b[sl]), BOUND, "disarmed, quiet group 4")


# ---- through the layers --------------------------------------------------------------------------------------------------
def _hub_graph(V, L, components, hubs, extra, seed):
    """In the manner of tests/test_gpu_tn_repair.py ``_two_component_graph``: ``components`` disconnected parts of V //
    components nodes, but every edge type's sources are ``hubs`` nodes per component only - most (source, type) pairs have no
    edge, which is what takes the compact-row route - and every node is the target of at least one edge of every type (no
    output unit sits exactly on its activation's kink)."""
    rng = np.random.default_rng(seed)
    part = V // components
    adjs = []
    for _ in range(L):
        parts = []
        for c in range(components):
            own = rng.choice(part, size=hubs, replace=False)
            dst = np.concatenate([np.arange(part), rng.integers(0, part, size=extra)])
            parts.append(np.stack([rng.choice(own, size=dst.size), dst], axis=1) + c * part)
        a = np.concatenate(parts, axis=0).astype(np.int32)
        rng.shuffle(a, axis=0)
        adjs.append(a)
    return adjs


def test_rgin_layer_weight_gradients_through_the_grouped_product_are_repaired(dev, monkeypatch):
    """RGIN layer, H = 128, two relations, the compact-row route: the kernel gradients are grouped two-factor products.  Two
    disconnected components of 192 nodes: the rows of dOut of component 1 are 2^-50 of component 0's, and the input columns
    64..127 are zero on component 0 - rows 64..127 of every relation's first-layer kernel gradient receive terms from
    component 1 only, pairs 2^-50 below their K range's largest, which an unrepaired product drops.  Their error, relative to
    the largest fp64 entry of that slice, is held to max(1e-5, 2 x the same quantity in mode bf16x3) (the exact kernels, not the
    code under test); every other gradient to 1e-5 of its largest entry.  The inputs are drawn clear of the activations' kinks
    on the fp64 oracle (tests/test_gpu_layers.py ``draw_inputs_clear_of_kinks``)."""
    from oracle import tf2gnn_oracle as orc
    from tests.helpers import KINK_MARGIN, KernelsUsed, kink_clearance, mp_weights_from_layer, to_dev
    from tests.test_gpu_layers import _build, _to64
    from tf2_gnn_amd.layers import MessagePassingInput
    from tf2_gnn_amd.layers.message_passing import RGIN

    monkeypatch.setattr(RGIN, "GROUPED_SPLIT_MIN_ROWS", 64)
    V, L, H = 384, 2, 128
    adjs = _hub_graph(V, L, 2, 40, 300, seed=5)
    adj_t = [torch.from_numpy(a) for a in adjs]

    def draw(layer, p):
        w64 = _to64(mp_weights_from_layer(layer))
        for attempt in range(60):
            gen = torch.Generator().manual_seed(2 + 1000 * attempt)
            X = torch.randn((V, H), generator=gen)
            X[: V // 2, 64:] = 0.0
            dOut = torch.randn((V, H), generator=gen)
            dOut[V // 2:] *= 2.0 ** -50
            if kink_clearance(lambda: orc.message_passing_call("rgin", p, w64, X.double(), adj_t)) >= KINK_MARGIN:
                return X, dOut
        raise AssertionError("no kink-free input found in 60 draws")

    def slice_errors(ops, mode):
        ops.set_gemm_mode(mode)
        layer, p = _build("RGIN", {"hidden_dim": H}, H, L)
        X, dOut = draw(layer, p)
        inp = MessagePassingInput(X.to(dev), to_dev(adjs, dev))
        with KernelsUsed() as k:
            layer(inp, training=True)
            layer.backward(dOut.to(dev))
            torch.cuda.synchronize()
        if mode == "f16x2":
            assert layer._grouped_tn_used and k.delta["sp_tn"] >= 2, k.delta
        else:
            assert k.delta["sp_tn"] == 0, k.delta
        w64 = _to64(mp_weights_from_layer(layer))
        leaves = []
        for l in range(L):
            w64["edge_mlps"][l] = [kk.requires_grad_(True) for kk in w64["edge_mlps"][l]]
            leaves += w64["edge_mlps"][l]
        want = orc.message_passing_call("rgin", p, w64, X.double(), adj_t)
        grads = torch.autograd.grad((want * dOut.double()).sum(), leaves)
        orphan, rest = [], []
        i = 0
        for l in range(L):
            for j, v in enumerate(layer._edge_type_mlps.vars[l]):
                r = grads[i]
                i += 1
                d = (v.grad.cpu().double() - r).abs()
                if j == 0:
                    assert float(r[64:].abs().max()) > 0 and float(r[64:].abs().max()) < 2.0 ** -30 * float(r.abs().max())
                    orphan.append(float(d[64:].max()) / float(r[64:].abs().max()))
                    rest.append((v.name + "[:64]", float(d[:64].max()) / float(r.abs().max())))
                else:
                    rest.append((v.name, float(d.max()) / float(r.abs().max())))
        assert i == len(grads) == len(layer.trainable_variables)
        return orphan, rest

    with armed() as ops:
        exact_orphan, _ = slice_errors(ops, "bf16x3")
        ops.set_gemm_mode("f16x2")
        ops.repair_stats(reset=True)
        got_orphan, got_rest = slice_errors(ops, "f16x2")
        for l in range(L):
            bound = max(1e-5, 2 * exact_orphan[l])
            print(f"relation {l}: dW1[64:128] err / largest of the slice = {got_orphan[l]:.3e} (bf16x3: {exact_orphan[l]:.3e})")
            record_parity(f"RGIN dW1 rows fed by the 2^-50 component only, relation {l} (repair armed)",
                          max_err_over_largest_of_slice=got_orphan[l], bound=bound)
            record_parity(f"RGIN dW1 rows fed by the 2^-50 component only, relation {l} (bf16x3)",
                          max_err_over_largest_of_slice=exact_orphan[l], bound=bound)
            assert got_orphan[l] <= bound, (l, got_orphan[l], exact_orphan[l])
        for name, e in got_rest:
            print(f"{name}: err / largest = {e:.3e}")
            assert e <= 1e-5, (name, e)
        assert host_flag() == 0 and ops.get_gemm_mode() == ops.GEMM_F16X2
        assert ops.repair_stats()["repaired_products"] >= 1


def _rgin_stack(dev):
    """2-layer RGIN stack over 384 nodes and 3 relations whose (source, type) rows have one or two edges each (100 sources per
    relation): the compact rows of the gradient keep the spread of dOut's rows - over 2^60, as in tests/test_gpu_tn_repair.py
    ``_stack`` - instead of averaging it away over many targets."""
    from tf2_gnn_amd.layers import GNN, GNNInput

    V, L, H = 384, 3, 128
    rng = np.random.default_rng(8)
    adjs = []
    for _ in range(L):
        src = rng.choice(V, size=100, replace=False)
        src = np.concatenate([src, src[:50]])  # half of the sources send two edges
        adjs.append(np.stack([src, rng.integers(0, V, size=src.size)], axis=1).astype(np.int32))
    gen = torch.Generator().manual_seed(4)
    feats = torch.randn((V, H), generator=gen)
    params = GNN.get_default_hyperparameters("rgin")
    params.update({"hidden_dim": H, "num_layers": 2, "dense_every_num_layers": 10000, "residual_every_num_layers": 10000,
                   "global_exchange_every_num_layers": 10000, "layer_input_dropout_rate": 0.0})
    inp = GNNInput(feats.to(dev), tuple(torch.from_numpy(a).to(dev) for a in adjs), torch.zeros(V, dtype=torch.int32, device=dev), 1)
    gen = torch.Generator().manual_seed(9)
    dOut = (torch.randn((V, H), generator=gen) * torch.exp2(torch.randint(-40, 20, (V, 1), generator=gen).float())).to(dev)
    return params, inp, dOut


def test_an_unchecked_pass_of_an_rgin_stack_hands_out_repaired_gradients(dev, monkeypatch):
    """No synchronous guard passes: the pass that would have tripped the guard of the grouped product repairs its own ranges -
    no warning, host flag down, no policy stage taken (the later steps stay on the split-operand kernels), gradients those of
    the exact kernels."""
    from tf2_gnn_amd import guard
    from tf2_gnn_amd.layers.message_passing import RGIN

    monkeypatch.setattr(RGIN, "GROUPED_SPLIT_MIN_ROWS", 64)
    params, inp, dOut = _rgin_stack(dev)
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
        assert any(mp._grouped_tn_used for mp in gnn._mp_layers)
        assert not any("spread" in str(x.message) for x in w), [str(x.message) for x in w]
        assert host_flag() == 0
        assert gnn.guard_state()["stage"] == "none"
        assert ops.repair_stats()["repaired_products"] > 0
        for v, b in zip(gnn.trainable_variables, exact):
            scale = max(float(b.abs().max()), 1e-30)
            err = float((v.grad - b).abs().max()) / scale
            print(f"{v.name}: |repaired - bf16x3| / largest = {err:.3e}")
            assert err <= 1e-5, (v.name, err)


def test_a_replayed_rgin_step_repairs_itself(dev, monkeypatch):
    """The same stack and dOut as one hipGraph, armed before building: every replay repairs its grouped products on the device -
    gradients bit-equal to an eager armed step of a twin model, no trip reported, as many repairs per replay as per eager
    step."""
    from tf2_gnn_amd import CapturedStep
    from tf2_gnn_amd.layers.message_passing import RGIN

    monkeypatch.setattr(RGIN, "GROUPED_SPLIT_MIN_ROWS", 64)
    params, inp, dOut = _rgin_stack(dev)
    with armed() as ops, _epoch_zero_afterwards():
        twin = _new_gnn(params)
        twin(inp, training=True)
        twin.backward(dOut)
        per_step = ops.repair_stats(reset=True)["repaired_products"]
        assert per_step > 0 and any(mp._grouped_tn_used for mp in twin._mp_layers)
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
        assert host_flag() == 0 and ops.get_gemm_mode() == ops.GEMM_F16X2
