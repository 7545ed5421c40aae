"""tfgnn_triple_batch_build on the device against tests/triple_batch_reference.py: every output bit for bit, the id table all -1
after every call, 6 launches per call.  Sizes: V at the edges of the 1024-id chunks and one beyond 256 chunks (the scan's
carry across rounds), B around one 256-thread workgroup, K in {0, 1, 3}; a hub, a self triple, identical positives, repeated
ids; a seed capacity one short; a bad id and a bad endpoint."""
import numpy as np
import pytest
import torch

from tests import triple_batch_reference as ref

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A


def _positives(V, P, rng, T=5):
    return np.stack([rng.integers(0, V, P), rng.integers(0, T, P), rng.integers(0, V, P)], axis=1).astype(np.int32)


def _run(dev, pos, ids, K, V, seed, capacity=None, workspace=None):
    """one call on canaried buffers -> (outputs as numpy, the workspace); asserts the table, the canaries, the launches"""
    from tf2_gnn_amd import ops

    N = len(ids) * (1 + K)
    cap = min(2 * N, V) if capacity is None else capacity
    guard = 8
    bufs = [torch.full((n + guard,), CANARY, dtype=torch.int32, device=dev) for n in (3 * N, 3 * N, cap)]
    out = (bufs[0][:3 * N].view(N, 3), bufs[1][:3 * N].view(N, 3), bufs[2][:cap])
    ws = ops.triple_batch_workspace(V, dev) if workspace is None else workspace
    before = ops.triple_batch_launch_counts()
    triples, local, seeds, S, status = ops.triple_batch(torch.from_numpy(pos).to(dev), torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(dev),
                                                        K, V, seed, ws, out=out)
    torch.cuda.synchronize()
    assert ops.triple_batch_launch_counts() - before == 6
    assert bool((ws[:V] == -1).all()), "the id table is not all -1 after the call"
    for b, n in zip(bufs, (3 * N, 3 * N, cap)):
        assert bool((b[n:] == CANARY).all()), "a word behind an output was written"
    assert seeds.shape[0] == S
    return (triples.cpu().numpy(), local.cpu().numpy(), seeds.cpu().numpy(), S, status), bufs[2].cpu().numpy(), ws


def _check(got, want):
    for g, w, name in zip(got[:3], want[:3], ("triples", "local_triples", "seeds")):
        assert g.dtype == np.int32 and g.shape == w.shape and np.array_equal(g, w), name
    assert got[3:] == want[3:]


@pytest.mark.parametrize("V", [2, 1023, 1024, 1025, 2049])
@pytest.mark.parametrize("B,K", [(1, 0), (1, 3), (255, 1), (257, 0), (257, 3)])
def test_outputs_equal_the_restatement(dev, V, B, K):
    rng = np.random.default_rng(V * 7 + B + K)
    P = 300
    pos = _positives(V, P, rng)
    if V > 2:  # the last id and the ids around a chunk edge are endpoints
        pos[0] = (V - 1, 0, 0)
        pos[1] = (min(1023, V - 1), 1, min(1024, V - 1))
    ids = rng.permutation(P)[:B]
    ids[0] = 0
    if B > 1:
        ids[1] = 1
    seed = (9 << 32) | B
    got, _, ws = _run(dev, pos, ids, K, V, seed)
    want = ref.build(pos, ids, K, V, seed, min(2 * B * (1 + K), V))
    _check(got, want)
    assert got[4] == 0
    # a second call on the same workspace, another seed: the table was left as the next call needs it
    got2, _, _ = _run(dev, pos, ids, K, V, seed + 1, workspace=ws)
    _check(got2, ref.build(pos, ids, K, V, seed + 1, min(2 * B * (1 + K), V)))
    if K:
        assert not np.array_equal(got2[0], got[0]) and np.array_equal(got2[0][:B], got[0][:B])


def test_more_than_256_chunks_of_ids(dev):
    """V = 263 000 is 257 chunks of 1024 ids: the one-workgroup scan carries across its rounds of 256 chunks.  N stays small;
    endpoints sit in the first, the 256th, the 257th and the last chunk."""
    V, K = 263_000, 1
    rng = np.random.default_rng(11)
    pos = _positives(V, 64, rng)
    pos[0] = (0, 0, V - 1)
    pos[1] = (256 * 1024 - 1, 1, 256 * 1024)
    pos[2] = (255 * 1024, 2, 262_999)
    ids = np.arange(64)
    got, _, _ = _run(dev, pos, ids, K, V, 77)
    want = ref.build(pos, ids, K, V, 77, 2 * 128)
    _check(got, want)
    assert got[4] == 0 and (got[2] >= 256 * 1024).sum() >= 3


@pytest.mark.parametrize("case", ["hub", "self", "identical", "repeats"])
def test_degenerate_batches(dev, case):
    V, K = 700, 3
    rng = np.random.default_rng(5)
    pos = _positives(V, 80, rng)
    ids = np.arange(80)
    if case == "hub":  # one node is an endpoint of every positive (a negative may replace it)
        pos[::2, 0] = 13
        pos[1::2, 2] = 13
    elif case == "self":
        pos[:] = np.stack([pos[:, 0], pos[:, 1], pos[:, 0]], axis=1)
    elif case == "identical":
        pos[:] = (41, 2, 97)
    else:
        ids = rng.integers(0, 6, size=80)
    got, _, _ = _run(dev, pos, ids, K, V, 123)
    want = ref.build(pos, ids, K, V, 123, min(2 * 80 * 4, V))
    _check(got, want)
    assert got[4] == 0
    if case == "identical":
        assert (got[1][:80] == got[1][0]).all() and got[2][got[1][0, [0, 2]]].tolist() == [41, 97]


def test_a_seed_capacity_one_short(dev):
    V, K = 1500, 1
    rng = np.random.default_rng(2)
    pos = _positives(V, 200, rng)
    ids = rng.permutation(200)[:90]
    full, _, _ = _run(dev, pos, ids, K, V, 31)
    S = full[3]
    assert full[4] == 0 and S > 10
    got, seed_buffer, _ = _run(dev, pos, ids, K, V, 31, capacity=S - 1)
    want = ref.build(pos, ids, K, V, 31, S - 1)
    _check(got, want)
    assert got[4] == ref.SEED_OVERFLOW and got[3] == S - 1
    assert np.array_equal(got[2], full[2][:S - 1]) and (seed_buffer[S - 1:] == CANARY).all()
    assert (got[1] == -1).sum() == (full[0][:, [0, 2]] == full[2][S - 1]).sum() >= 1
    assert np.array_equal(got[0], full[0])


def test_a_bad_id_and_a_bad_endpoint(dev):
    V, K = 1100, 3
    rng = np.random.default_rng(3)
    pos = _positives(V, 50, rng)
    pos[7] = (V + 4, 1, 20)  # a source outside [0, V)
    pos[9] = (30, 2, -6)     # a target outside, negative
    ids = np.arange(40)
    ids[3] = 50              # outside [0, P)
    ids[5] = -2
    got, _, _ = _run(dev, pos, ids, K, V, 8)
    want = ref.build(pos, ids, K, V, 8, min(2 * 160, V))
    _check(got, want)
    triples, local, seeds, S, status = got
    assert status == ref.BAD_POSITIVE_ID | ref.BAD_ENDPOINT
    for i in (3, 5):
        rows = [i] + [40 + K * i + k for k in range(K)]
        assert (triples[rows] == -1).all() and (local[rows] == -1).all()
    assert triples[7].tolist() == [V + 4, 1, 20] and local[7, 0] == -1 and seeds[local[7, 2]] == 20
    assert triples[9].tolist() == [30, 2, -6] and local[9, 2] == -1 and seeds[local[9, 0]] == 30
    assert seeds.min() >= 0 and seeds.max() < V
    # each bit alone
    only_id, _, _ = _run(dev, np.delete(pos, [7, 9], axis=0), np.where(ids > 47, 48, np.minimum(ids, 30)), K, V, 8)
    assert only_id[4] == ref.BAD_POSITIVE_ID
    only_end, _, _ = _run(dev, pos, np.arange(12), K, V, 8)
    assert only_end[4] == ref.BAD_ENDPOINT


def test_default_outputs_and_a_sampler_workspace(dev):
    """Without ``out`` the seeds buffer is min(2 N, V); the call runs on a NeighborStore's workspace and leaves it usable."""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import NeighborStore, PackedFold

    V = 300
    rng = np.random.default_rng(4)
    edges = rng.integers(0, V, size=(900, 2)).astype(np.int32)
    store = NeighborStore(PackedFold([V], np.zeros((V, 1), np.float32), [[900]], [edges]), dev)
    ws = store.workspace(V)
    pos = _positives(V, 60, rng)
    ids = np.arange(60, dtype=np.int32)
    triples, local, seeds, S, status = ops.triple_batch(torch.from_numpy(pos).to(dev), torch.from_numpy(ids).to(dev), 2, V, 6, ws)
    want = ref.build(pos, ids, 2, V, 6, min(360, V))
    _check((triples.cpu().numpy(), local.cpu().numpy(), seeds.cpu().numpy(), S, status), want)
    assert bool((store.local_id_table() == -1).all())
    sample = ops.neighbor_sample(store, seeds, [2], 1)
    assert sample.status == 0 and torch.equal(sample.nodes[:S], seeds)
    assert bool((store.local_id_table() == -1).all())
