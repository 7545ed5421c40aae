"""tests/distmult_reference.py - the float64 restatement of the tfgnn_distmult_* contracts (include/tfgnn.h) that the GPU
tests compare the kernels with - pinned to independent computations: loss, dH and dR to torch's float64 autograd of the same
loss, the ranking counts to a dense [Q, V] score matrix, and ops.build_triple_tables to a brute-force loop.  CPU-only."""
import numpy as np
import pytest
import torch

from tests import distmult_reference as ref


def _case(seed, V=23, T=4, D=9, N=140, integer=False):
    rng = np.random.default_rng(seed)
    if integer:
        H, R = rng.integers(-2, 3, size=(V, D)).astype(np.float64), rng.integers(-2, 3, size=(T, D)).astype(np.float64)
    else:
        H, R = rng.standard_normal((V, D)), rng.standard_normal((T, D))
    triples = np.stack([rng.integers(0, V, N), rng.integers(0, T - 1, N), rng.integers(0, V, N)], axis=1)  # relation T-1: none
    triples[::17, 2] = triples[::17, 0]  # self triples
    labels = rng.integers(0, 2, N).astype(np.float64)
    weights = rng.uniform(0.5, 2.0, N)
    labels[3], labels[5], labels[8] = 2.0, 0.5, np.nan  # uncounted
    weights[11], weights[12], weights[13] = 0.0, -1.0, np.nan
    return H, R, triples, labels, weights


def _torch_loss(H, R, triples, labels, weights):
    Ht, Rt = torch.tensor(H, requires_grad=True), torch.tensor(R, requires_grad=True)
    t = torch.tensor(triples)
    s = (Ht[t[:, 0]] * Rt[t[:, 1]] * Ht[t[:, 2]]).sum(dim=1)
    y, w = torch.tensor(labels), torch.tensor(weights)
    keep = (w > 0) & ((y == 0) | (y == 1))
    per = torch.nn.functional.binary_cross_entropy_with_logits(s[keep], y[keep], reduction="none")
    loss = (w[keep] * per).sum() / w[keep].sum()
    return Ht, Rt, s, keep, loss


@pytest.mark.parametrize("seed", [0, 1])
def test_loss_and_gradients_against_torch_autograd(seed):
    H, R, triples, labels, weights = _case(seed)
    Ht, Rt, s, keep, loss = _torch_loss(H, R, triples, labels, weights)
    s.retain_grad()
    loss.backward()
    r = ref.distmult_ce(H, R, triples, labels, weights)
    assert np.array_equal(r.counted, keep.numpy()) and r.counted.sum() == len(labels) - 6
    np.testing.assert_allclose(r.scores, s.detach().numpy(), rtol=1e-13, atol=1e-13)
    assert abs(r.loss - float(loss.detach())) <= 1e-13 * max(1.0, abs(float(loss.detach())))
    np.testing.assert_allclose(r.gscore, s.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert np.all(r.gscore[~r.counted] == 0.0)
    dH, dR, bH, bR = ref.distmult_backward(H, R, triples, r.gscore, ref.gscore_error(r, weights))
    np.testing.assert_allclose(dH, Ht.grad.numpy(), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(dR, Rt.grad.numpy(), rtol=1e-11, atol=1e-14)
    assert np.all(dR[-1] == 0.0) and np.all(bR[-1] == 0.0)  # the relation without a triple
    assert np.all(bH >= 0) and np.all(bR >= 0) and np.all(r.score_bound >= 0)
    sc = r.scores[r.counted]
    y = labels[r.counted]
    assert r.counts == (int(((sc > 0) & (y == 1)).sum()), int(((sc > 0) & (y == 0)).sum()),
                        int(((sc <= 0) & (y == 0)).sum()), int(((sc <= 0) & (y == 1)).sum()))
    assert r.accuracy == (r.counts[0] + r.counts[2]) / r.counted.sum()


def test_nothing_counted_and_unweighted():
    H, R, triples, labels, _ = _case(2)
    r = ref.distmult_ce(H, R, triples, labels, np.zeros(len(labels)))
    assert r.W == 0 and r.loss == 0.0 and np.all(r.gscore == 0) and r.counts == (0, 0, 0, 0) and np.isnan(r.accuracy)
    r1 = ref.distmult_ce(H, R, triples, labels)
    r2 = ref.distmult_ce(H, R, triples, labels, np.ones(len(labels)))
    assert r1.loss == r2.loss and np.array_equal(r1.gscore, r2.gscore)


def test_exact_zero_score_predicts_zero():
    H = np.array([[1.0, 1.0], [1.0, -1.0]])
    R = np.array([[1.0, 1.0]])
    r = ref.distmult_ce(H, R, [[0, 0, 1], [0, 0, 0]], [1.0, 1.0])
    assert r.scores.tolist() == [0.0, 2.0] and r.counts == (1, 0, 0, 1)
    assert r.gscore[0] == 0.5 * (0.5 - 1.0)


@pytest.mark.parametrize("corrupt", ["dst", "src"])
@pytest.mark.parametrize("integer", [True, False])
def test_ranks_against_a_dense_score_matrix(corrupt, integer):
    H, R, triples, _, _ = _case(3, integer=integer)
    queries = triples[:31]
    V = H.shape[0]
    rng = np.random.default_rng(4)
    lists = [np.unique(np.concatenate([rng.integers(0, V, rng.integers(0, 6)), [q[2] if corrupt == "dst" else q[0]] * (i % 2)]))
             for i, q in enumerate(queries)]
    offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
    ids = np.concatenate(lists).astype(np.int64)
    Ht, Rt = torch.tensor(H), torch.tensor(R)
    q = torch.tensor(queries)
    if corrupt == "dst":
        dense = torch.einsum("qd,vd->qv", Ht[q[:, 0]] * Rt[q[:, 1]], Ht).numpy()
        truth = queries[:, 2]
    else:
        dense = torch.einsum("vd,qd->qv", Ht, Rt[q[:, 1]] * Ht[q[:, 2]]).numpy()
        truth = queries[:, 0]
    for filtered in (False, True):
        g, e, lo, hi = ref.distmult_rank(H, R, queries, corrupt, offsets if filtered else None, ids if filtered else None)
        for i in range(len(queries)):
            cands = [c for c in range(V) if c != truth[i] and not (filtered and c in set(lists[i].tolist()))]
            s = dense[i, truth[i]]
            if integer:  # exact: ties included
                assert g[i] == sum(dense[i, c] > s for c in cands) and e[i] == sum(dense[i, c] == s for c in cands)
            else:
                assert g[i] == sum(dense[i, c] > s + 1e-12 for c in cands) and e[i] == 0
            assert lo[i] <= g[i] <= g[i] + e[i] <= hi[i]
    if integer:
        assert ref.distmult_rank(H, R, queries, corrupt)[1].sum() > 0  # the exact family does produce ties


@pytest.mark.parametrize("V,T,N", [(1, 1, 1), (7, 3, 40), (50, 2, 300)])
def test_build_triple_tables_against_a_loop(V, T, N):
    from tf2_gnn_amd import ops

    rng = np.random.default_rng(N)
    triples = np.stack([rng.integers(0, V, N), rng.integers(0, T, N), rng.integers(0, V, N)], axis=1)
    got, want = ops.build_triple_tables(triples, V, T), ref.triple_tables_by_loop(triples, V, T)
    assert sorted(got) == sorted(want) == sorted(ops.TRIPLE_TABLE_NAMES)
    for name in want:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), name
    assert got["node_offsets"][-1] == 2 * N and got["rel_offsets"][-1] == N
    for bad in ([[V, 0, 0]], [[0, T, 0]], [[0, 0, -1]]):
        with pytest.raises(ValueError, match="outside"):
            ops.build_triple_tables(np.array(bad), V, T)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        ops.build_triple_tables(np.zeros((2, 2), dtype=np.int64), V, T)
    with pytest.raises(ValueError, match=r"\[N, 3\]"):
        ops.build_triple_tables(np.zeros((2, 3)), V, T)
