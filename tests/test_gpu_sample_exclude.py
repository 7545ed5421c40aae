"""tfgnn_sample_exclude_edges on the device against the numpy restatement of its contract (tests/sample_exclude_reference.py):
the kept edges, the new counts in the sampler's meta words, ``removed`` and the status word must be EQUAL, and nothing at or
beyond a list's old count may change.  Hand-built target-sorted lists with L = 3 first, then the call behind the real
sampler (``ops.neighbor_sample(exclude=...)``) on a graph of 500 nodes with a tied and two untied relations."""
import numpy as np
import pytest
import torch

from tests import sample_exclude_reference as ref

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A
SLACK = 7  # canary rows behind every list's old count


def _arr(rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 2)


def _exclude(dev, lists, positives, fwd, inv, S):
    """the op on copies of ``lists`` at capacity len + SLACK -> (full buffers, meta, record), all numpy"""
    from tf2_gnn_amd import _lib, ops

    lists = [_arr(a) for a in lists]
    L = len(lists)
    bufs = []
    for a in lists:
        b = torch.full((a.shape[0] + SLACK, 2), GUARD, dtype=torch.int32, device=dev)
        b[:a.shape[0]] = torch.from_numpy(a).to(dev)
        bufs.append(b)
    meta = np.full(_lib.sample_meta_words(L, 1), 1000, dtype=np.int32)  # the words around the counts must survive
    meta[_lib.SAMPLE_META_STATUS] = _lib.SAMPLE_REPEATED_SEED  # a bit the sampler might have set stays
    meta[_lib.SAMPLE_META_EDGES:_lib.SAMPLE_META_EDGES + L] = [a.shape[0] for a in lists]
    meta_dev = torch.from_numpy(meta).to(dev)
    pos = torch.from_numpy(np.asarray(positives, dtype=np.int32).reshape(-1, 3)).to(dev)
    before = ops.sample_exclude_launch_counts()
    record = ops.sample_exclude_edges(bufs, meta_dev, S, pos, fwd, inv)
    assert ops.sample_exclude_launch_counts() - before == _lib.SAMPLE_EXCLUDE_LAUNCHES == ref.LAUNCHES
    assert record.dtype == torch.int32 and tuple(record.shape) == (L + 1,) and record.is_cuda
    return [b.cpu().numpy() for b in bufs], meta_dev.cpu().numpy(), record.cpu().numpy(), meta


def _check(dev, lists, positives, fwd, inv, S, what=""):
    """run the op and compare everything with the restatement -> (kept lists, removed, status)"""
    from tf2_gnn_amd import _lib

    lists = [_arr(a) for a in lists]
    L = len(lists)
    want, removed, status = ref.exclude(lists, positives, fwd, inv, S)
    bufs, meta, record, meta_in = _exclude(dev, lists, positives, fwd, inv, S)
    assert record[:L].tolist() == removed.tolist(), (what, record, removed)
    assert int(record[L]) == status, (what, record[L], status)
    e0 = _lib.SAMPLE_META_EDGES
    assert meta[e0:e0 + L].tolist() == [a.shape[0] for a in want], what
    assert meta[_lib.SAMPLE_META_STATUS] == meta_in[_lib.SAMPLE_META_STATUS] | status, what
    assert meta[_lib.SAMPLE_META_NODES] == 1000 and (meta[e0 + L:] == 1000).all(), what
    for t, (buf, old, new) in enumerate(zip(bufs, lists, want)):
        assert np.array_equal(buf[:new.shape[0]], new), (what, t)
        assert (buf[old.shape[0]:] == np.int32(GUARD)).all(), (what, t, "the canary behind the old count")
    return want, removed, status


def _untied():
    loops = [[0, 0], [1, 1], [2, 2], [3, 3]]
    fwd = [[1, 0], [2, 0], [0, 1], [0, 1], [3, 1], [1, 2], [-1, 2], [0, 3]]  # (0, 1) twice: a multi-edge; a source of -1
    bwd = [[1, 0], [1, 0], [3, 0], [0, 1], [0, 2], [1, 3]]
    return [_arr(a) for a in (loops, fwd, bwd)]


def test_nothing_matches(dev):
    lists = _untied()
    want, removed, status = _check(dev, lists, [[2, 0, 3], [3, 0, 2]], [1], [2], 4)
    assert status == 0 and removed.tolist() == [0, 0, 0]
    bufs, _, record, _ = _exclude(dev, lists, [[2, 0, 3], [3, 0, 2]], [1], [2], 4)
    for buf, a in zip(bufs, lists):  # bit-identical, the whole old range
        assert np.array_equal(buf[:a.shape[0]], a)
    assert record.tolist() == [0, 0, 0, 0]


def test_every_edge_of_one_type_goes(dev):
    lists = _untied()
    every = [[s, 0, d] for s, d in lists[1].tolist() if s >= 0]
    want, removed, status = _check(dev, lists, every, [1], [-1], 4)
    assert status == 0 and removed.tolist() == [0, 7, 0] and want[1].tolist() == [[-1, 2]]  # the source -1 is kept
    one = [_arr([[0, 0]]), _arr([[2, 1], [2, 1], [2, 1]]), _arr([])]
    want, removed, _ = _check(dev, one, [[2, 0, 1]], [1], [2], 3)
    assert removed.tolist() == [0, 3, 0] and want[1].shape == (0, 2) and want[0].tolist() == [[0, 0]]


def test_multi_edges_and_a_repeated_positive(dev):
    want, removed, status = _check(dev, _untied(), [[0, 0, 1], [0, 0, 1], [0, 0, 1]], [1], [2], 4)
    assert status == 0 and removed.tolist() == [0, 2, 2]
    assert want[1].tolist() == [[1, 0], [2, 0], [3, 1], [1, 2], [-1, 2], [0, 3]]
    assert want[2].tolist() == [[3, 0], [0, 1], [0, 2], [1, 3]]


def test_tied_untied_and_no_inverse(dev):
    tied = _arr([[1, 0], [0, 1], [1, 1], [1, 1], [2, 1], [1, 2]])
    lists = [tied, _untied()[1], _untied()[2]]
    # relation 0 is tied (list 0 both ways), relation 1 untied (lists 1 and 2), relation 2 has no inverse (list 1 only)
    fwd, inv = [0, 1, 1], [0, 2, -1]
    want, removed, _ = _check(dev, lists, [[0, 0, 1]], fwd, inv, 4, "tied")
    assert removed.tolist() == [2, 0, 0] and want[0].tolist() == [[1, 1], [1, 1], [2, 1], [1, 2]]
    want, removed, _ = _check(dev, lists, [[3, 1, 1]], fwd, inv, 4, "untied")
    assert removed.tolist() == [0, 1, 1]
    want, removed, _ = _check(dev, lists, [[3, 2, 1]], fwd, inv, 4, "no inverse")
    assert removed.tolist() == [0, 1, 0] and want[2].tolist() == lists[2].tolist()
    want, removed, _ = _check(dev, lists, [[1, 0, 1]], fwd, inv, 4, "u == v on a tied type")
    assert removed.tolist() == [2, 0, 0] and want[0].tolist() == [[1, 0], [0, 1], [2, 1], [1, 2]]


def test_skipped_rows_and_status_bits(dev):
    from tf2_gnn_amd import _lib

    lists = _untied()
    _, removed, status = _check(dev, lists, [[-1, -1, -1]], [1], [2], 4)
    assert status == 0 and removed.tolist() == [0, 0, 0]
    _, removed, status = _check(dev, lists, [[-1, -1, -1], [0, 0, 1]], [1], [2], 4)
    assert status == 0 and removed.tolist() == [0, 2, 2]
    _, removed, status = _check(dev, lists, [[0, 1, 1]], [1], [2], 4, "a relation of T")
    assert status == _lib.SAMPLE_EXCLUDE_BAD_RELATION and removed.tolist() == [0, 0, 0]
    _, removed, status = _check(dev, lists, [[0, 0, 4]], [1], [2], 4, "an endpoint of S")
    assert status == _lib.SAMPLE_EXCLUDE_BAD_ENDPOINT and removed.tolist() == [0, 0, 0]
    _, removed, status = _check(dev, lists, [[0, 0, 3], [0, 0, 1]], [1], [2], 3, "S = 3: node 3 is no seed")
    assert status == _lib.SAMPLE_EXCLUDE_BAD_ENDPOINT and removed.tolist() == [0, 2, 2]
    _, removed, status = _check(dev, lists, [[9, -2, 1], [-1, 0, 1], [1, 0, 2]], [1], [2], 4)
    assert status == _lib.SAMPLE_EXCLUDE_BAD_RELATION | _lib.SAMPLE_EXCLUDE_BAD_ENDPOINT and removed.tolist() == [0, 1, 0]


def _random_lists(n, S, rng):
    """three target-sorted lists of n, n and max(n - 1, 0) edges over S nodes (many repeats), a few sources of -1"""
    out = []
    for m in (n, n, max(n - 1, 0)):
        a = np.stack([rng.integers(-1, S, m), np.sort(rng.integers(0, S, m))], axis=1).astype(np.int32).reshape(-1, 2)
        out.append(a)
    return out


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, 3000])
def test_list_lengths_around_the_chunk(dev, n):
    rng = np.random.default_rng(n)
    S = 12
    lists = _random_lists(n, S, rng)
    positives = np.stack([rng.integers(0, S, 9), rng.integers(0, 2, 9), rng.integers(0, S, 9)], axis=1)
    # relation 0: lists 1 and 2; relation 1: tied on list 2; list 0 is named by nobody
    want, removed, status = _check(dev, lists, positives, [1, 2], [2, 2], S, n)
    assert status == 0 and removed[0] == 0 and want[0].shape[0] == n
    if n >= 1023:
        assert removed[1] > 0 and removed[2] > 0 and want[1].shape[0] > 0


def test_a_row_of_3000_edges_across_three_chunks(dev):
    n, S = 3000, 8
    src = (np.arange(n) % 50 + 10).astype(np.int32)  # no seed among them
    hits = [0, 1023, 1024, 2047, 2048, n - 1]  # the first slot, the last, and both sides of the chunk boundaries
    src[hits] = 3
    hub = np.stack([src, np.full(n, 5, dtype=np.int32)], axis=1)
    around = [_arr([[3, 4]] * 5), hub, _arr([[5, 3]] * 2 + [[3, 6]] * 4)]
    for lead in (0, 1, 1020):  # the row's first slot at 0, at 1, and with its chunk boundaries elsewhere
        front = np.stack([np.full(lead, 3, dtype=np.int32), np.full(lead, 2, dtype=np.int32)], axis=1).reshape(-1, 2)
        back = _arr([[3, 7]] * 3)
        lists = [around[0], np.concatenate([front, hub, back]), around[2]]
        want, removed, status = _check(dev, lists, [[3, 0, 5]], [1], [2], S, lead)
        assert status == 0 and removed.tolist() == [0, len(hits), 2]
        assert want[1].shape[0] == lead + n - len(hits) + 3 and not ((want[1][:, 0] == 3) & (want[1][:, 1] == 5)).any()
    # hundreds of positives pointing at the one row: each a strided walk of its own
    many = [[u, 0, 5] for u in range(S)] * 40
    _check(dev, [around[0], hub, around[2]], many, [1], [2], S, "320 positives")


def test_two_calls_give_equal_bits(dev):
    rng = np.random.default_rng(77)
    S = 10
    lists = _random_lists(2500, S, rng)
    positives = np.stack([rng.integers(0, S, 300), rng.integers(0, 2, 300), rng.integers(0, S, 300)], axis=1)
    a = _exclude(dev, lists, positives, [1, 2], [2, 2], S)
    b = _exclude(dev, lists, positives, [1, 2], [2, 2], S)
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("B", [1, 2048])
def test_the_launch_count_does_not_depend_on_the_batch(dev, B):
    from tf2_gnn_amd import ops

    rng = np.random.default_rng(B)
    S = 40
    lists = _random_lists(500, S, rng)
    positives = np.stack([rng.integers(0, S, B), rng.integers(0, 2, B), rng.integers(0, S, B)], axis=1)
    before = ops.sample_exclude_launch_counts()
    _check(dev, lists, positives, [1, 2], [2, 2], S, B)  # one call inside
    assert ops.sample_exclude_launch_counts() - before == ref.LAUNCHES == 4


# ---- behind the real sampler ------------------------------------------------------------------------------------------------
V_G, T_G = 500, 3
FWD_G, INV_G = [1, 2, 3], [4, 2, 5]  # self loops 0; relation 1 tied; the backward types of relations 0 and 2 behind the forward ones


@pytest.fixture(scope="module")
def sampled():
    """(store, raw edges per relation): 500 nodes, 700 edges per relation, relation 1 tied, self loops"""
    from tf2_gnn_amd.data import NeighborStore, PackedFold

    if not torch.cuda.is_available():
        pytest.skip("no ROCm device")
    rng = np.random.default_rng(5)
    raw = [rng.integers(0, V_G, size=(700, 2)).astype(np.int32) for _ in range(T_G)]
    fold = PackedFold.from_raw_graphs([np.zeros((V_G, 2), np.float32)], [raw], T_G, add_self_loop_edges=True,
                                      tied_fwd_bkwd_edge_types={1}, feature_dim=2)
    assert fold.num_edge_types == 6
    return NeighborStore(fold, torch.device("cuda", 0)), raw


@pytest.mark.parametrize("fanouts", [[-1, -1], [3, 2]])
def test_through_the_sampler(dev, sampled, fanouts):
    from tf2_gnn_amd import ops

    store, raw = sampled
    rng = np.random.default_rng(len(fanouts) + fanouts[0])
    rows = [(int(raw[r][i, 0]), r, int(raw[r][i, 1])) for r in range(T_G) for i in rng.choice(700, 24, replace=False)]
    positives = np.array(rows + rows[:3], dtype=np.int32)  # three of them twice
    seeds = np.unique(positives[:, [0, 2]]).astype(np.int32)
    local = positives.copy()
    local[:, 0], local[:, 2] = np.searchsorted(seeds, positives[:, 0]), np.searchsorted(seeds, positives[:, 2])
    seeds_dev = torch.from_numpy(seeds).to(dev)
    plain = ops.neighbor_sample(store, seeds_dev, fanouts, seed=99)
    assert plain.status == 0 and plain.removed is None
    plain_lists = [a.cpu().numpy() for a in plain.adjacency_lists]
    want, removed, status = ref.exclude(plain_lists, local, FWD_G, INV_G, len(seeds))  # asserts the sampler's lists are sorted
    sample_before, exclude_before = ops.sample_launch_counts()[0], ops.sample_exclude_launch_counts()
    got = ops.neighbor_sample(store, seeds_dev, fanouts, seed=99, exclude=(torch.from_numpy(local).to(dev), FWD_G, INV_G))
    assert ops.sample_launch_counts()[0] - sample_before == 3 + 6 * len(fanouts)
    assert ops.sample_exclude_launch_counts() - exclude_before == ref.LAUNCHES
    assert status == 0 and got.status == 0
    assert torch.equal(got.nodes, plain.nodes) and got.hop_ptr.tolist() == plain.hop_ptr.tolist()
    assert got.removed.is_cuda and got.removed.cpu().numpy().tolist() == removed.tolist()
    for t, (a, b) in enumerate(zip(got.adjacency_lists, want)):
        assert tuple(a.shape) == b.shape and np.array_equal(a.cpu().numpy(), b), (fanouts, t)
    assert removed[0] == 0 and np.array_equal(want[0], plain_lists[0])  # the self loops
    if fanouts[0] < 0:  # every positive was drawn, in both directions
        assert removed[1] >= 24 and removed[3] >= 24 and removed[4] >= 24 and removed[5] >= 24 and removed[2] >= 48
        for u, r, v in local.tolist():
            assert not ((want[FWD_G[r]][:, 0] == u) & (want[FWD_G[r]][:, 1] == v)).any()
            assert not ((want[INV_G[r]][:, 0] == v) & (want[INV_G[r]][:, 1] == u)).any()
    print(f"fanouts {fanouts}: {len(seeds)} seeds, {plain.nodes.shape[0]} nodes, edges {[a.shape[0] for a in plain_lists]}, "
          f"removed {removed.tolist()}")
    assert bool((store.local_id_table() == -1).all())
