"""The row-sparse optimizer step on the device (tfgnn_optimizer_apply_rows, optim.RowGradient; include/tfgnn.h "The row-sparse
step"): (1) bit for bit against a twin - the unchanged dense tfgnn_optimizer_apply on a compact variable holding the listed
rows -, every kind and clip mode, next to ordinary dense variables; (2) against the fp64 restatement applied to the gathered
rows; (3) ids outside the table; (4) table offsets beyond 2^31; (5) launch counts; (6) a captured call."""
import numpy as np
import pytest
import torch

from tests.optim_model64 import schedule64
from tests.optim_rows_reference import LazyRows64
from tests.test_gpu_optim import CLIPS, SCHED

pytestmark = pytest.mark.gpu

KINDS = ["sgd", "sgd_mom", "rmsprop", "rmsprop_mom", "adam"]
CASES = [(1, 1, 1, 1), (5, 0, 3, 3), (300, 37, 64, 64), (300, 300, 65, 65), (1000, 513, 320, 336), (70000, 1000, 4, 4)]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _optimizer(kind, learning_rate=None):
    from tf2_gnn_amd.optim import Optimizer, PolynomialWarmupAndDecaySchedule

    mu = 0.85 if kind in ("sgd_mom", "rmsprop_mom") else 0.0
    lr = PolynomialWarmupAndDecaySchedule(**SCHED) if learning_rate is None else learning_rate
    return Optimizer(kind.split("_")[0], learning_rate=lr, momentum=mu, rho=0.98)


def _prefill_slots(opt, var, slots):
    """slots the optimizer would otherwise create as zeros at the variable's first update"""
    opt._slots[id(var)] = (var, slots)


class _Dense:
    """three ordinary variables next to the table: a matrix of odd shape, a bias, a strided column slice of a fused buffer"""

    def __init__(self, dev, gen):
        from tf2_gnn_amd.layers.message_passing.message_passing import Variable

        rnd = lambda *shape: (torch.randn(shape, generator=gen) * 0.1).to(dev)
        self.fused = rnd(16, 40)
        self.vars = [Variable("odd", rnd(33, 7)), Variable("bias", rnd(121)), Variable("slice", self.fused[:, 8:32])]

    def twin(self):
        from tf2_gnn_amd.layers.message_passing.message_passing import Variable

        other = object.__new__(_Dense)
        other.fused = self.fused.clone()
        other.vars = [Variable("odd", self.vars[0].value.clone()), Variable("bias", self.vars[1].value.clone()),
                      Variable("slice", other.fused[:, 8:32])]
        return other

    @staticmethod
    def grads(dev, gen):
        gfused = torch.randn((16, 44), generator=gen).to(dev)  # another row pitch than the values'
        return [torch.randn((33, 7), generator=gen).to(dev), torch.randn((121,), generator=gen).to(dev), gfused[:, 3:27]]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "N%d_n%d_D%d_ld%d" % c)
def test_rows_equal_the_dense_step_on_a_compact_twin(dev, case, kind):
    """three steps per clip mode, new ids and rows each step, on the polynomial schedule; slots from a random prefill"""
    from tf2_gnn_amd.layers.message_passing.message_passing import Variable
    from tf2_gnn_amd.optim import RowGradient

    N, n, D, pitch = case
    for clip in CLIPS:
        gen = torch.Generator().manual_seed(1234 + N + n)
        what = f"{case} {kind} {clip}"
        buf = torch.full((N, pitch), float("nan"), device=dev)
        table = Variable("table", buf[:, :D])
        table.value.copy_((torch.randn((N, D), generator=gen) * 0.1).to(dev))
        dense = _Dense(dev, gen)
        twin = dense.twin()
        compact = Variable("compact", torch.empty((n, D), device=dev))
        opt, opt2 = _optimizer(kind), _optimizer(kind)
        slots = [(torch.randn(N * D, generator=gen).abs() * 0.1).to(dev) for _ in range(opt._nslots)]
        slots2 = [torch.empty(n * D, device=dev) for _ in range(opt._nslots)]
        _prefill_slots(opt, table, slots)
        _prefill_slots(opt2, compact, slots2)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        for step in range(3):
            ids_host = torch.randperm(N, generator=gen)[:n]
            ids = ids_host.to(torch.int32).to(dev)
            rows = torch.randn((n, D), generator=gen).to(dev)
            grads = _Dense.grads(dev, gen)
            buf_before, slots_before = buf.clone(), [s.clone() for s in slots]
            index = ids_host.to(dev)
            compact.value.copy_(table.value[index])
            for s2, s in zip(slots2, slots):
                s2.view(n, D).copy_(s.view(N, D)[index])
            # the row gradient in the middle of the list: its place in the squared-sum pass is after the dense tensors anyway
            pairs = [(dense.vars[0], grads[0]), (table, RowGradient(rows, ids, N, bad_flag=flag)), (dense.vars[1], grads[1]),
                     (dense.vars[2], grads[2])]
            opt.apply_gradients(pairs, clip=clip)
            opt2.apply_gradients(list(zip(twin.vars, grads)) + [(compact, rows)], clip=clip)
            torch.cuda.synchronize()
            assert _same(table.value[index], compact.value), what
            untouched = torch.ones(N, dtype=torch.bool, device=dev)
            untouched[index] = False
            assert _same(buf[untouched], buf_before[untouched]), what  # the other rows, guard columns included
            assert _same(buf[:, D:], buf_before[:, D:]), what  # the guard columns of every row: still NaN
            assert bool(torch.isnan(buf[:, D:]).all()) and not bool(torch.isnan(table.value).any()), what
            assert [s.data_ptr() for s in opt.slots(table)] == [s.data_ptr() for s in slots]  # the prefilled ones, as today
            for s, s2, s_before in zip(opt.slots(table), opt2.slots(compact), slots_before):
                assert _same(s.view(N, D)[index], s2.view(n, D)), what
                assert _same(s.view(N, D)[untouched], s_before.view(N, D)[untouched]), what
            for a, b in zip(dense.vars, twin.vars):
                assert _same(a.value, b.value), (what, a.name)
                for sa, sb in zip(opt.slots(a), opt2.slots(b)):
                    assert _same(sa, sb), (what, a.name)
            assert _same(dense.fused, twin.fused), what
            if n:
                assert not _same(table.value[index], buf_before[:, :D][index]), what  # the step moved the listed rows
            assert opt.iterations == step + 1 and opt2.iterations == step + 1, what
            assert int(flag) == 0, what


@pytest.mark.parametrize("kind", ["adam", "rmsprop_mom"])
def test_rows_match_fp64(dev, kind):
    """five steps whose ids overlap: some rows carry moments from earlier steps, others do not.  The bound is that of
    test_gpu_optim.test_update_matches_fp64: 1e-5 * biggest_step + 2^-22 * max|w|."""
    from tf2_gnn_amd.layers.message_passing.message_passing import Variable
    from tf2_gnn_amd.optim import RowGradient

    N, n, D = 300, 37, 64
    gen = torch.Generator().manual_seed(77)
    w0 = torch.randn((N, D), generator=gen) * 0.1
    table = Variable("table", w0.to(dev))
    opt = _optimizer(kind)
    mu = 0.85 if kind == "rmsprop_mom" else 0.0
    ref = LazyRows64(w0.double().numpy().copy(), kind.split("_")[0], lambda t: schedule64(t, **SCHED), momentum=mu, rho=0.98)
    biggest, seen, repeated = 0.0, set(), 0
    for step in range(5):
        ids = torch.randperm(60 + 40 * step, generator=gen)[:n]  # drawn from a growing prefix of the table: they overlap
        rows = torch.randn((n, D), generator=gen)
        repeated += len(seen & set(ids.tolist()))
        seen |= set(ids.tolist())
        opt.apply_gradients([(table, RowGradient(rows.to(dev), ids.to(torch.int32).to(dev), N))])
        before = ref.table.copy()
        ref.step(ids.numpy(), rows.double().numpy())
        biggest = max(biggest, float(np.abs(ref.table - before).max()))
    torch.cuda.synchronize()
    assert repeated > 20 and len(seen) < N  # rows updated more than once, rows updated once, rows never updated
    got = table.value.double().cpu().numpy()
    err = float(np.abs(got - ref.table).max())
    tol = 1e-5 * biggest + 2.0 ** -22 * float(np.abs(ref.table).max())
    print(f"{kind}: max error {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (kind, err, tol)
    never = np.array(sorted(set(range(N)) - seen))
    assert np.array_equal(got[never], w0.double().numpy()[never])
    # the slots (not part of the issue's bound): five updates of a few fp32 roundings each, 2^-24 relative per rounding, stay
    # far below 1e-5 of the largest entry
    for s, s64 in zip(opt.slots(table), ref.slots):
        assert float(np.abs(s.view(N, D).double().cpu().numpy() - s64).max()) <= 1e-5 * float(np.abs(s64).max())
    assert opt.iterations == 5


@pytest.mark.parametrize("with_flag", [True, False])
def test_bad_ids_are_skipped(dev, with_flag):
    from tf2_gnn_amd.layers.message_passing.message_passing import Variable
    from tf2_gnn_amd.optim import RowGradient

    N, D = 50, 8
    gen = torch.Generator().manual_seed(5)
    table = Variable("table", torch.randn((N, D), generator=gen).to(dev))
    before = table.value.clone()
    ids = torch.tensor([3, -1, 20, N, 49 - 10], dtype=torch.int32, device=dev)
    rows = torch.randn((5, D), generator=gen).to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if with_flag else None
    opt = _optimizer("adam", learning_rate=0.01)
    opt.apply_gradients([(table, RowGradient(rows, ids, N, bad_flag=flag))])
    torch.cuda.synchronize()
    moved = (_bits(table.value) != _bits(before)).any(dim=1).cpu().numpy()
    assert sorted(np.nonzero(moved)[0].tolist()) == [3, 20, 39]  # rows 0 and N - 1, which a bad id might alias, keep their bits
    m, v = (s.view(N, D) for s in opt.slots(table))
    assert sorted(np.nonzero((m != 0).any(dim=1).cpu().numpy())[0].tolist()) == [3, 20, 39]
    assert sorted(np.nonzero((v != 0).any(dim=1).cpu().numpy())[0].tolist()) == [3, 20, 39]
    # the good rows got the update of a call without the bad ones
    twin = Variable("table", before.clone())
    keep = torch.tensor([0, 2, 4], device=dev)
    _optimizer("adam", learning_rate=0.01).apply_gradients([(twin, RowGradient(rows[keep], ids[keep], N))])
    torch.cuda.synchronize()
    assert _same(table.value, twin.value)
    if with_flag:
        assert int(flag) == 1
    assert opt.iterations == 1


def test_offsets_beyond_2_to_31(dev):
    """plain SGD (no slots) on a table of 2^25 + 8 rows of 64 floats: 8 GiB, uninitialised, a handful of rows written"""
    from tf2_gnn_amd.layers.message_passing.message_passing import Variable
    from tf2_gnn_amd.optim import RowGradient

    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip("less than 16 GiB of device memory free")
    N, D, lr = 2 ** 25 + 8, 64, 0.25
    value = torch.empty((N, D), device=dev)
    table = Variable("table", value)
    listed, aliases = [2 ** 25, 2 ** 25 + 7, 5], [0, 7]  # (2^25 + r) * 64 floats is r * 64 in 32 bits
    gen = torch.Generator().manual_seed(11)
    known = {r: torch.randn(D, generator=gen).to(dev) for r in listed + aliases}
    for r, x in known.items():
        value[r].copy_(x)
    rows = torch.randn((3, D), generator=gen).to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    opt = _optimizer("sgd", learning_rate=lr)
    opt.apply_gradients([(table, RowGradient(rows, torch.tensor(listed, dtype=torch.int32, device=dev), N, bad_flag=flag))])
    torch.cuda.synchronize()
    assert opt.slots(table) == [] and int(flag) == 0 and opt.iterations == 1
    for i, r in enumerate(listed):
        want = (known[r].double() - float(np.float32(lr)) * rows[i].double()).float()  # w - lr * g, exact in fp64, rounded once
        assert _same(value[r], want), r
    for r in aliases:
        assert _same(value[r], known[r]), r
    del table, value
    torch.cuda.empty_cache()


@pytest.mark.parametrize("d", [1, 3, 32])
def test_launch_counts(dev, d):
    from tf2_gnn_amd import _lib, ops
    from tf2_gnn_amd.layers.message_passing.message_passing import Variable
    from tf2_gnn_amd.optim import RowGradient

    lib = _lib.load()
    N, n, D = 40, 9, 16
    dense = [Variable(f"v{i}", torch.ones(3 + i, 5, device=dev)) for i in range(d)]
    grads = [torch.ones(3 + i, 5, device=dev) for i in range(d)]
    table = Variable("table", torch.ones(N, D, device=dev))
    ids = torch.arange(n, dtype=torch.int32, device=dev) * 3
    rows = torch.ones(n, D, device=dev)
    embedding = ops.embedding_launch_count()
    for clip, want in ((None, 2), (("value", 0.5), 2), (("norm", 1.0), 3), (("global_norm", 1.0), 3)):
        opt = _optimizer("adam", learning_rate=0.01)
        before = lib.tfgnn_optimizer_launch_count()
        opt.apply_gradients(list(zip(dense, grads)) + [(table, RowGradient(rows, ids, N))], clip=clip)
        assert lib.tfgnn_optimizer_launch_count() - before == want, (d, clip)
        # no row to update: the dense launches alone, and the counter still advances
        before = lib.tfgnn_optimizer_launch_count()
        opt.apply_gradients(list(zip(dense, grads)) + [(table, RowGradient(rows[:0], ids[:0], N))], clip=clip)
        assert lib.tfgnn_optimizer_launch_count() - before == want - 1, (d, clip)
        # the row gradient alone
        before = lib.tfgnn_optimizer_launch_count()
        opt.apply_gradients([(table, RowGradient(rows, ids, N))], clip=clip)
        assert lib.tfgnn_optimizer_launch_count() - before == want - 1, (d, clip)
        # nothing at all to update: one workgroup that advances the counter
        before = lib.tfgnn_optimizer_launch_count()
        opt.apply_gradients([(table, RowGradient(rows[:0], ids[:0], N))], clip=clip)
        assert lib.tfgnn_optimizer_launch_count() - before == 1, (d, clip)
        torch.cuda.synchronize()
        assert opt.iterations == 4, (d, clip)
    assert ops.embedding_launch_count() == embedding


def test_captured_call_equals_two_eager_calls(dev):
    from tf2_gnn_amd.layers.message_passing.message_passing import Variable
    from tf2_gnn_amd.optim import RowGradient

    N, n, D = 300, 37, 64
    gen = torch.Generator().manual_seed(9)
    w0, b0 = (torch.randn((N, D), generator=gen) * 0.1).to(dev), torch.randn((121,), generator=gen).to(dev)
    ids = torch.randperm(N, generator=gen)[:n].to(torch.int32).to(dev)
    rows0 = torch.randn((n, D), generator=gen).to(dev)
    gb = torch.randn((121,), generator=gen).to(dev)
    clip = ("global_norm", 1.0)

    def fresh():
        return Variable("table", w0.clone()), Variable("bias", b0.clone()), _optimizer("adam"), rows0.clone()

    # eager: two calls, the rows changed in place in between
    table_e, bias_e, opt_e, rows_e = fresh()
    for _ in range(2):
        opt_e.apply_gradients([(table_e, RowGradient(rows_e, ids, N)), (bias_e, gb)], clip=clip)
        rows_e.mul_(-3.0).add_(1.0)
    torch.cuda.synchronize()

    table, bias, opt, rows = fresh()
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    call = lambda: opt.apply_gradients([(table, RowGradient(rows, ids, N, bad_flag=flag)), (bias, gb)], clip=clip)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # once eagerly: kernels loaded, slots, state and workspace allocated before the capture
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    table.value.copy_(w0)  # back to the start
    bias.value.copy_(b0)
    for v in (table, bias):
        for s in opt.slots(v):
            s.zero_()
    opt.iterations = 0
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # no allocation, copy or synchronisation inside: the call is capturable
        call()
    torch.cuda.synchronize()
    assert opt.iterations == 0 and _same(table.value, w0)  # captured, not run
    graph.replay()
    rows.mul_(-3.0).add_(1.0)
    graph.replay()
    torch.cuda.synchronize()
    assert opt.iterations == 2 and opt_e.iterations == 2 and int(flag) == 0
    assert _same(table.value, table_e.value) and _same(bias.value, bias_e.value) and not _same(table.value, w0)
    for v, v_e in ((table, table_e), (bias, bias_e)):
        for s, s_e in zip(opt.slots(v), opt_e.slots(v_e)):
            assert _same(s, s_e), v.name
