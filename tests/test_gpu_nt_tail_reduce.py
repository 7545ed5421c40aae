"""The reduce pass of a weight-gradient (TN) product carried by the NT launch that follows it (include/tfgnn.h
tfgnn_tn_reduce_job; csrc/gemm_sp.hip SpArgs::tail): extra workgroups behind the product's own run sp_tn_reduce_body, the same
device function the stand-alone sp_tn_reduce_kernel runs.  Expected values never come from the carried path: dW is compared
bit for bit with what the stand-alone ``ops.sp_gemm_tn`` writes from the same operands (itself held to the fp64 bound of
tests/test_gpu_gemm_sp.py test_gemm_tn_matches_fp64), the NT result with the NT product alone (held to the fp64 bound of
test_gemm_nt_matches_fp64)."""
import itertools
import os
import subprocess
import sys

import pytest
import torch

from tests.helpers import assert_close, random_graph, to_dev

pytestmark = pytest.mark.gpu

# NT products: every tile width, row counts around the 128-row tile, K without and with the in-launch K split
# (K = 960: 60 k16 steps split four ways - both workspaces live in one launch), the three row routes
NT_CASES = list(itertools.product((128, 256, 320), (1, 127, 129, 257), (48, 960), ("plain", "masked", "by_source")))
# TN products whose reduction rides: (columns of A, N, K rows, accumulate, scatter): K rows 16 / 257 / 2500 = one, a few and
# many K ranges (sp_tn_splits: a range per 256 rows while the output tiles leave workgroups of one round free)
TN_CASES = list(itertools.product((320, 1280), (128, 320), (16, 257, 2500), (0, 1), (False, True)))
TN_BOUND = 6e-7  # test_gemm_tn_matches_fp64: max error / sum |a||b| while every row keeps its 22 bits


def _nt_inputs(dev, case):
    """operands and keyword arguments of one NT case + its fp64 reference"""
    from tf2_gnn_amd import ops

    N, M, K, route = case
    g = torch.Generator().manual_seed(N + 7 * M + K + len(route))
    sb = 16 if K == 48 else 320  # three scale blocks that tile K: what the tile mask needs
    A = torch.randn((M, K), generator=g)
    Bt = torch.randn((N, K), generator=g) * 0.05
    kw = {}
    if route == "masked":  # bit b of a tile's byte: block b holds non-zeros there; rows land through row_map
        tiles = (M + 127) // 128
        mask = torch.tensor([(1, 5, 7)[t % 3] for t in range(tiles)], dtype=torch.uint8)
        for t in range(tiles):
            for b in range(3):
                if not (int(mask[t]) >> b) & 1:
                    A[t * 128:(t + 1) * 128, b * sb:(b + 1) * sb] = 0.0
        perm = torch.randperm(M, generator=g).to(torch.int32)
        ref = torch.zeros((M, N), dtype=torch.float64)
        ref[perm.long()] = A.double() @ Bt.double().t()
        kw = dict(tile_kmask=mask.to(dev), row_map=perm.to(dev))
    elif route == "by_source":  # product row r reads row a_rows[r] of the operand
        perm = torch.randperm(M, generator=g).to(torch.int32)
        ref = A[perm.long()].double() @ Bt.double().t()
        kw = dict(a_rows=perm.to(dev))
    else:
        ref = A.double() @ Bt.double().t()
    return ops.sp_split_rows(A.to(dev), scale_block=sb), ops.sp_split_rows(Bt.to(dev)), kw, ref


_TN_OPERANDS = {}


def _tn_operands(dev, cols, n, k):
    """(split X [k, cols] with scale blocks of cols / 4 or 160 columns, split G [k, n], fp64 product, sum |a||b|), built once"""
    from tf2_gnn_amd import ops

    key = (cols, n, k)
    if key not in _TN_OPERANDS:
        g = torch.Generator().manual_seed(cols + n + k)
        # rows (= k) on different scales, exp(N(0, 1)): the per-k factors at work, every row well inside the 2^20 the format
        # gives a K range (exp(2 N(0, 1)) times the x30 rows of G below reaches past it at these row counts: the guard trips)
        X = torch.randn((k, cols), generator=g) * torch.exp(torch.randn((k, 1), generator=g))
        G = torch.randn((k, n), generator=g) * 1e-4
        G[::7] *= 30.0
        H = 320 if cols == 1280 else 160
        _TN_OPERANDS[key] = (ops.sp_split_rows(X.to(dev), scale_block=H), ops.sp_split_rows(G.to(dev)), X.double().t() @ G.double(),
                             X.double().abs().t() @ G.double().abs(), H)
    return _TN_OPERANDS[key]


def _flags_set() -> int:
    from tf2_gnn_amd import ops

    torch.cuda.synchronize()
    return int(ops._SPLITK_WS["ws"][:65536].view(torch.int32).count_nonzero()) if "ws" in ops._SPLITK_WS else 0


def check_pair(dev, nt_case, tn_case, ref_ld_form: str):
    """One NT case carrying one TN reduction: every equality the carried pass owes (module docstring)."""
    from tf2_gnn_amd import ops

    what = f"NT {nt_case} carrying TN {tn_case} ({ref_ld_form})"
    cols, n, k, acc, scatter = tn_case
    xs, gs, ref_tn, mag_tn, H = _tn_operands(dev, cols, n, k)
    sc = (H, n * H, 1, H) if scatter else None  # element ((l, h), d) -> dW[l, d, h]
    gen = torch.Generator().manual_seed(k + cols)
    C0 = torch.randn(cols * n, generator=gen).to(dev)

    def fresh():
        return C0.clone().view((cols // H, n, H) if scatter else (cols, n))

    want_dw = ops.sp_gemm_tn(xs, gs, out=fresh(), scatter=sc, accumulate=bool(acc))  # the stand-alone path
    if not acc:  # ... which is itself right: the fp64 bound of the product
        plain = want_dw.cpu().double()
        if scatter:
            plain = plain.permute(0, 2, 1).reshape(cols, n)
        e = float(((plain - ref_tn).abs() / mag_tn.clamp(min=1e-300)).max())
        print(f"{what}: stand-alone TN max err / sum|a||b| = {e:.2e}")
        assert e <= TN_BOUND, (what, e)

    a_op, b_op, kw, ref_nt = _nt_inputs(dev, nt_case)
    N, M, K, _ = nt_case
    _, _, splits_before = ops.sp_gemm_nt_splitk()
    want_nt = ops.sp_gemm_nt(a_op, b_op, **kw)  # the NT product alone
    split = ops.sp_gemm_nt_splitk()[2] - splits_before
    if (M, K) == (257, 960):
        assert split == 1, f"{what}: the product no longer splits K inside its launch"
    scale = max(1.0, 0.05 * float(K) ** 0.5)
    assert_close(want_nt.cpu() / scale, (ref_nt / scale).float(), tol=1e-5, what=what + ": NT alone vs fp64")
    assert _flags_set() == 0

    before = ops.tn_reduce_counts()
    got = []
    for _ in range(2):  # two launches back to back
        dw, job = ops.sp_gemm_tn_product(xs, gs, out=fresh(), scatter=sc, accumulate=bool(acc))
        assert job.num_blocks == max(1, min(1024, -(-cols * n // 512)))  # a function of the reduction's size
        nt = ops.sp_gemm_nt(a_op, b_op, tail=job, **kw)
        got.append((dw, nt))
    assert _flags_set() == 0, what + ": flag words of the K-split workspace left set"
    after = ops.tn_reduce_counts()
    assert (after["own"], after["carried"]) == (before["own"], before["carried"] + 2), what
    for dw, nt in got:
        assert torch.equal(dw, want_dw), what + ": dW differs from the stand-alone path"
        assert torch.equal(nt, want_nt), what + ": NT result differs from the product alone"
    with pytest.raises(RuntimeError):
        ops.tn_reduce_launch(job)  # a job runs once


def pairs():
    """Every TN case on an NT case, every NT case at least once: 48 pairs over 72 NT cases take two rounds"""
    n = max(len(NT_CASES), len(TN_CASES))
    return [(NT_CASES[i % len(NT_CASES)], TN_CASES[(i * 7) % len(TN_CASES)]) for i in range(2 * n)]


def test_the_pairs_cover_every_case():
    ps = pairs()
    assert {p[0] for p in ps} == set(NT_CASES) and {p[1] for p in ps} == set(TN_CASES)


@pytest.mark.parametrize("chunk", range(8))
def test_carried_reduction_equals_the_stand_alone_pass(dev, chunk):
    """factors computed inside the product kernel: one reference scale per (K range, block), ref_ld > 0"""
    ps = pairs()
    for nt_case, tn_case in ps[chunk::8]:
        check_pair(dev, nt_case, tn_case, "one reference scale per K range and block")


def test_carried_reduction_after_the_separate_factor_pass(dev):
    """one reference scale per block (ref_ld == 0): the factor pass form, chosen by TFGNN_TN_FIK=0 - read once per process,
    hence a child process - over every TN case"""
    code = (
        "import torch\n"
        "from tf2_gnn_amd import ops\n"
        "from tests.test_gpu_nt_tail_reduce import NT_CASES, TN_CASES, check_pair\n"
        "dev = torch.device('cuda', 0)\n"
        "ops.set_gemm_mode('f16x2')\n"
        "for i, tn in enumerate(TN_CASES):\n"
        "    check_pair(dev, NT_CASES[(i * 5 + 3) % len(NT_CASES)], tn, 'one reference scale per block')\n"
        "torch.cuda.synchronize()\n"
        "print('CHILD OK')\n"
    )
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, TFGNN_TN_FIK="0", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300, cwd=root)
    assert res.returncode == 0 and "CHILD OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


def test_nt_call_that_launches_nothing_still_reduces(dev):
    """M = 0: no product workgroup exists to stand behind - the pass gets its own launch"""
    from tf2_gnn_amd import ops

    xs, gs, _, _, _ = _tn_operands(dev, 320, 128, 257)
    want = ops.sp_gemm_tn(xs, gs)
    before = ops.tn_reduce_counts()
    dw, job = ops.sp_gemm_tn_product(xs, gs)
    empty = ops.SplitOperand(torch.empty((0, 48 * 4), dtype=torch.uint8, device=dev), torch.empty((0, 1), device=dev), 0, 48, 48)
    b_op = ops.sp_split_rows(torch.randn((128, 48)).to(dev))
    out = ops.sp_gemm_nt(empty, b_op, tail=job)
    assert tuple(out.shape) == (0, 128)
    after = ops.tn_reduce_counts()
    assert (after["own"], after["carried"]) == (before["own"] + 1, before["carried"])
    assert torch.equal(dw, want)
    # and a job run alone
    dw2, job2 = ops.sp_gemm_tn_product(xs, gs)
    assert ops.tn_reduce_launch(job2) is dw2 and torch.equal(dw2, want)


def test_overlapping_workspaces_are_refused(dev):
    """the TN product's workspace is read while the NT product's K split writes its own: a job whose workspace lies inside the
    registered K-split workspace is refused (and runs alone)"""
    import ctypes

    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    a_op, b_op, kw, _ = _nt_inputs(dev, (320, 257, 960, "plain"))
    want_nt = ops.sp_gemm_nt(a_op, b_op)  # (registers the K-split workspace)
    ks = ops._SPLITK_WS["ws"]
    xs, gs, _, _, _ = _tn_operands(dev, 320, 128, 257)
    want = ops.sp_gemm_tn(xs, gs)
    M, N, K = 320, 128, 257
    need = lib.tfgnn_sp_gemm_tn_workspace_bytes(M, N, K, xs.cols, xs.scale_block)
    inside = ks.data_ptr() + (8 << 20)  # behind the flags and the slabs this test's products use
    inside += (-inside) % 256
    assert need and inside + need <= ks.data_ptr() + ks.numel()
    out = torch.empty((M, N), device=dev)
    job = _lib.TnReduceJob()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.tfgnn_sp_gemm_tn_product(M, N, K, xs.data.data_ptr(), xs.data.stride(0), 0, xs.inv_scale.data_ptr(), xs.cols,
                                             xs.scale_block, gs.data.data_ptr(), gs.data.stride(0), 0, gs.inv_scale.data_ptr(),
                                             out.data_ptr(), M, 0, N, 1, 0, ctypes.c_void_p(inside), need, ctypes.byref(job), stream))
    wrapped = ops.TnReduceJob(job, out, None)
    with pytest.raises(Exception, match="overlaps"):
        ops.sp_gemm_nt(a_op, b_op, tail=wrapped)
    ops.tn_reduce_launch(wrapped)  # refused before anything was launched: the job is still the caller's to run
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.equal(ops.sp_gemm_nt(a_op, b_op), want_nt)

    # the layer entry point: tn_workspace inside workspace
    with pytest.raises(Exception, match="overlaps"):
        _mp_backward_with_overlap(dev)


def _mp_backward_with_overlap(dev):
    from tf2_gnn_amd import ops

    V, E, L, H = 300, 2000, 2, 128
    graph = ops.Graph(to_dev(random_graph(V, E, L, seed=1), dev), V, parts=ops.G_PARTS_ALL)
    gen = torch.Generator().manual_seed(2)
    W = (torch.randn((L, H, H), generator=gen) * 0.05).to(dev)
    x_sp = ops.sp_split_rows(torch.randn((V, H), generator=gen).to(dev))
    d_pre = torch.randn((V, H), generator=gen).to(dev)
    real = ops._aligned_workspace

    def shared(device, nbytes, own=False):  # the TN workspace out of the buffer the gather's workspace comes from
        ws = ops._workspace(device, nbytes + 256)
        off = (-ws.data_ptr()) % 256
        return ws.data_ptr() + off, nbytes, ws

    from tf2_gnn_amd import _lib

    lib = _lib.load()
    real_bytes = lib.tfgnn_graph_gather_workspace_bytes
    ops._aligned_workspace = shared
    lib.tfgnn_graph_gather_workspace_bytes = lambda *a: max(4096, real_bytes(*a))  # (a gather without long buckets asks for none)
    try:
        ops._workspace(dev, 64 << 20)
        ops.mp_backward(graph, d_pre, W, x_sp)
    finally:
        ops._aligned_workspace = real
        lib.tfgnn_graph_gather_workspace_bytes = real_bytes
        graph.close()


def _stack(dev, layers=2):
    import bench
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers import GNN, GNNInput
    from tf2_gnn_amd.layers.message_passing import set_seed

    V, E, L, H = 2500, 60000, 4, 320
    set_seed(0)
    gnn = GNN(bench.model_params("rgcn", H, layers, None))
    gen = torch.Generator().manual_seed(5)
    X = torch.randn((V, H), generator=gen).to(dev)
    dOut = torch.randn((V, H), generator=gen).to(dev)
    graph = ops.Graph(to_dev(random_graph(V, E, L, seed=3, hub=(5, 300)), dev), V, parts=ops.G_PARTS_ALL)
    inp = GNNInput(X, graph, torch.zeros(V, dtype=torch.int32, device=dev), 1)

    def step(need_input_grad=False):
        gnn._dropout_calls = 0
        out = gnn(inp, training=False)
        dx = gnn.backward(dOut, need_input_grad=need_input_grad)
        return [out] + ([dx] if dx is not None else []) + [v.grad for v in gnn.trainable_variables]

    return gnn, graph, step


def _snapshot(res):
    torch.cuda.synchronize()
    return [t.clone() for t in res]


def test_layer_stack_carries_every_reduction_but_the_last(dev, monkeypatch):
    """a 2-layer RGCN stack at V = 2500, H = 320 with its Dense layer(s) and the projection: both routes of the layers give the
    same bits; with the one-call layers every weight gradient's reduce pass rides on the input-gradient product behind it,
    except the projection's - the last product of the pass, nothing follows it"""
    from tf2_gnn_amd import ops

    results = {}
    for entry in ("1", "0"):
        monkeypatch.setenv("TFGNN_MP_ENTRY", entry)
        gnn, graph, step = _stack(dev)
        for _ in range(4):  # (the stack's first backward passes are checked synchronously)
            step()
        torch.cuda.synchronize()
        before = ops.tn_reduce_counts()
        results[entry] = _snapshot(step())
        after = ops.tn_reduce_counts()
        own, carried = after["own"] - before["own"], after["carried"] - before["carried"]
        dense = len(gnn._dense_layers)
        if entry == "1":
            assert (own, carried) == (1, len(gnn._mp_layers) + dense), (own, carried)
        else:  # the op-level route of the layers keeps its own launches; the Dense pairs carry theirs
            assert (own, carried) == (1 + len(gnn._mp_layers), dense), (own, carried)
        # asked for the input gradient of the stack, the projection has an NT product behind it too
        before = ops.tn_reduce_counts()
        step(need_input_grad=True)
        after = ops.tn_reduce_counts()
        if entry == "1":
            assert (after["own"] - before["own"], after["carried"] - before["carried"]) == (0, len(gnn._mp_layers) + dense + 1)
        graph.close()
    assert len(results["1"]) == len(results["0"])
    for a, b in zip(results["1"], results["0"]):
        assert torch.equal(a, b)


def test_captured_step_replays_to_the_eager_bits(dev):
    """the same stack, forward and backward captured into one hipGraph: the carried reduce passes replay to the eager bits"""
    from tf2_gnn_amd import CapturedStep, ops

    prev = ops.get_gemm_mode()
    ops.set_gemm_mode("f16x2")
    try:
        gnn, graph, step = _stack(dev)
        for _ in range(4):
            step()
        eager = _snapshot(step())
        cap = CapturedStep(step)
        cap.capture()
        for _ in range(2):
            replayed = _snapshot(cap.replay())
            assert len(replayed) == len(eager)
            for a, b in zip(replayed, eager):
                assert torch.equal(a, b)
        assert not cap.guard_tripped()
        graph.close()
    finally:
        ops.set_gemm_mode(prev)
