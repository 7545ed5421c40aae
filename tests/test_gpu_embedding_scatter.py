"""tfgnn_embedding_scatter_rows (csrc/embedding.hip) through ops.embedding_scatter_rows against numpy, bit for bit: the kernel
only copies rows and fills zeros.  Shapes: the smallest, no ids, a typical one, a full permutation of odd width (the scalar
path), a pitched float4 case with guard columns, and many row tiles (8192 / 4 > 256 rows: 256 rows to a workgroup, 274
workgroups fill, 4 scatter)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

#        N, n, D, pitch
CASES = [(1, 1, 1, 1), (5, 0, 3, 3), (300, 37, 64, 64), (300, 300, 65, 65), (1000, 513, 320, 336), (70000, 1000, 4, 4)]


def _case(N, n, D, pitch, dev, seed=0):
    rng = np.random.default_rng(seed + N + 7 * D)
    rows = rng.standard_normal((n, D)).astype(np.float32)
    ids = rng.permutation(N)[:n].astype(np.int32)
    want = np.full((N, pitch), np.nan, dtype=np.float32)
    want[:, :D] = 0.0
    want[ids, :D] = rows
    buf = torch.full((N, pitch), float("nan"), dtype=torch.float32, device=dev)
    return rows, ids, want, buf


def _same_bits(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("N,n,D,pitch", CASES)
def test_scatter_equals_numpy_bit_for_bit(dev, N, n, D, pitch):
    from tf2_gnn_amd import ops

    rows, ids, want, buf = _case(N, n, D, pitch, dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    before = ops.embedding_launch_count()
    out = ops.embedding_scatter_rows(torch.from_numpy(rows).to(dev), torch.from_numpy(ids).to(dev), N, out=buf[:, :D], bad_flag=flag)
    launches = ops.embedding_launch_count() - before
    torch.cuda.synchronize()
    assert launches == (1 if n == 0 else 2)
    assert out.data_ptr() == buf.data_ptr() and int(flag) == 0
    # every element of the columns < D was written (no NaN of the prefill is left), the guard columns keep theirs
    assert _same_bits(buf, want)
    assert not torch.isnan(buf[:, :D]).any() and (pitch == D or bool(torch.isnan(buf[:, D:]).all()))


def test_pitched_rows_and_allocated_output(dev):
    """``rows`` as a column slice of a wider tensor (pitch 72, float4 path: 72 % 4 == 0; then pitch 67: the scalar path), the
    output allocated by the wrapper"""
    from tf2_gnn_amd import ops

    rng = np.random.default_rng(3)
    for pitch in (72, 67):
        wide = rng.standard_normal((50, pitch)).astype(np.float32)
        ids = rng.permutation(90)[:50].astype(np.int32)
        want = np.zeros((90, 64), dtype=np.float32)
        want[ids] = wide[:, :64]
        out = ops.embedding_scatter_rows(torch.from_numpy(wide).to(dev)[:, :64], torch.from_numpy(ids).to(dev), 90)
        torch.cuda.synchronize()
        assert tuple(out.shape) == (90, 64) and _same_bits(out, want), pitch


@pytest.mark.parametrize("bad", [-1, "N"])
def test_an_id_outside_the_table_sets_the_flag_and_nothing_else(dev, bad):
    from tf2_gnn_amd import ops

    N, n, D = 300, 37, 64
    rows, ids, want, buf = _case(N, n, D, D, dev, seed=5)
    want[ids[11], :] = 0.0  # the row whose id goes bad is skipped: its old target stays zero
    ids[11] = N if bad == "N" else bad
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.embedding_scatter_rows(torch.from_numpy(rows).to(dev), torch.from_numpy(ids).to(dev), N, out=buf, bad_flag=flag)
    torch.cuda.synchronize()
    assert int(flag) == 1 and _same_bits(buf, want)
    # without a flag the row is skipped all the same
    buf.fill_(float("nan"))
    ops.embedding_scatter_rows(torch.from_numpy(rows).to(dev), torch.from_numpy(ids).to(dev), N, out=buf)
    torch.cuda.synchronize()
    assert _same_bits(buf, want)


def test_wrapper_refusals(dev):
    from tf2_gnn_amd import ops

    rows = torch.zeros((4, 8), dtype=torch.float32, device=dev)
    ids = torch.arange(4, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="more rows than the table"):
        ops.embedding_scatter_rows(rows, ids, 3)
    with pytest.raises(ValueError, match="3 ids for 4 rows"):
        ops.embedding_scatter_rows(rows, ids[:3], 10)
    with pytest.raises(ValueError, match=r"out must be a float32 \[10, 8\]"):
        ops.embedding_scatter_rows(rows, ids, 10, out=torch.zeros((10, 4), dtype=torch.float32, device=dev))
    with pytest.raises(TypeError):
        ops.embedding_scatter_rows(rows, ids.long(), 10)
    before = ops.embedding_launch_count()
    assert tuple(ops.embedding_scatter_rows(rows[:0], ids[:0], 0).shape) == (0, 8)  # an empty table: no launch
    assert ops.embedding_launch_count() == before


def test_captured_call_follows_rows_changed_in_place(dev):
    from tf2_gnn_amd import ops

    N, n, D = 300, 37, 64
    rows, ids, want, buf = _case(N, n, D, D, dev, seed=9)
    d_rows, d_ids = torch.from_numpy(rows).to(dev), torch.from_numpy(ids).to(dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # once eagerly: the kernels are loaded before the capture
        ops.embedding_scatter_rows(d_rows, d_ids, N, out=buf, bad_flag=flag)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    buf.fill_(float("nan"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):  # no allocation, copy or synchronisation inside: the call is capturable
        ops.embedding_scatter_rows(d_rows, d_ids, N, out=buf, bad_flag=flag)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(buf, want)
    d_rows.mul_(-3.0).add_(1.0)  # new rows, in place
    buf.fill_(float("nan"))
    want[ids] = d_rows.cpu().numpy()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(buf, want) and int(flag) == 0
