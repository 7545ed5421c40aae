"""tests/complex_reference.py - the float64 restatement of the tfgnn_complex_* contracts (include/tfgnn.h) that the GPU tests
compare the kernels with - pinned to independent computations: scores, loss, dH and dR to torch's float64 COMPLEX arithmetic
and autograd (torch.view_as_complex on [.., m, 2] views, s = (a r conj(b)).sum(-1).real), the ranking counts to a dense
[Q, V] score matrix, and - with R_im = 0 - everything to tests/distmult_reference.py on R' = [R_re ; R_re].  CPU-only."""
import numpy as np
import pytest
import torch

from tests import complex_reference as ref
from tests import distmult_reference as dref


def _case(seed, V=23, T=4, D=10, N=140, integer=False):
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


def _as_complex(x):
    """[.., D] halves -> complex [.., m]"""
    m = x.shape[-1] // 2
    return torch.view_as_complex(torch.stack([x[..., :m], x[..., m:]], dim=-1).contiguous())


def _torch_scores(Ht, Rt, t):
    a, r, b = _as_complex(Ht[t[:, 0]]), _as_complex(Rt[t[:, 1]]), _as_complex(Ht[t[:, 2]])
    return (a * r * b.conj()).sum(-1).real


@pytest.mark.parametrize("seed", [0, 1])
def test_loss_and_gradients_against_torch_complex_autograd(seed):
    H, R, triples, labels, weights = _case(seed)
    Ht, Rt = torch.tensor(H, requires_grad=True), torch.tensor(R, requires_grad=True)
    s = _torch_scores(Ht, Rt, torch.tensor(triples))
    y, w = torch.tensor(labels), torch.tensor(weights)
    keep = (w > 0) & ((y == 0) | (y == 1))
    per = torch.nn.functional.binary_cross_entropy_with_logits(s[keep], y[keep], reduction="none")
    loss = (w[keep] * per).sum() / w[keep].sum()
    s.retain_grad()
    loss.backward()
    r = ref.complex_ce(H, R, triples, labels, weights)
    assert np.array_equal(r.counted, keep.numpy()) and r.counted.sum() == len(labels) - 6
    np.testing.assert_allclose(r.scores, s.detach().numpy(), rtol=1e-13, atol=1e-13)
    assert abs(r.loss - float(loss.detach())) <= 1e-13 * max(1.0, abs(float(loss.detach())))
    np.testing.assert_allclose(r.gscore, s.grad.numpy(), rtol=1e-12, atol=1e-15)
    assert np.all(r.gscore[~r.counted] == 0.0)
    dH, dR, bH, bR = ref.complex_backward(H, R, triples, r.gscore, ref.gscore_error(r, weights))
    np.testing.assert_allclose(dH, Ht.grad.numpy(), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(dR, Rt.grad.numpy(), rtol=1e-11, atol=1e-14)
    assert np.all(dR[-1] == 0.0) and np.all(bR[-1] == 0.0)  # the relation without a triple
    assert np.all(bH >= 0) and np.all(bR >= 0) and np.all(r.score_bound >= 0)
    sc, yc = r.scores[r.counted], labels[r.counted]
    assert r.counts == (int(((sc > 0) & (yc == 1)).sum()), int(((sc > 0) & (yc == 0)).sum()),
                        int(((sc <= 0) & (yc == 0)).sum()), int(((sc <= 0) & (yc == 1)).sum()))
    assert r.accuracy == (r.counts[0] + r.counts[2]) / r.counted.sum()


def test_score_bound_is_the_sum_of_the_2d_absolute_products():
    H, R, triples, _, _ = _case(5)
    D = H.shape[1]
    m = D // 2
    s, ds = ref.scores_and_bounds(H, R, triples)
    for e in (0, 17, 99):
        u, t, v = triples[e]
        a, r, b = H[u], R[t], H[v]
        P = sum(abs(r[k]) * (abs(a[k] * b[k]) + abs(a[m + k] * b[m + k])) + abs(r[m + k]) * (abs(a[k] * b[m + k]) + abs(a[m + k] * b[k]))
                for k in range(m))
        assert ds[e] == pytest.approx((2 * D + 3) * 2.0 ** -24 * P, rel=1e-13)
    with pytest.raises(ValueError, match="even"):
        ref.scores_and_bounds(H[:, :9], R[:, :9], triples)


def test_antisymmetry_and_self_triples():
    H, R, triples, _, _ = _case(6, integer=True)
    m = H.shape[1] // 2
    R[0, :m] = 0.0   # r_re = 0: purely imaginary relation -> antisymmetric score
    R[1, m:] = 0.0   # r_im = 0: symmetric score
    fwd = np.array([[u, t, v] for u, t, v in triples if t < 2])
    rev = fwd[:, ::-1].copy()
    s_f, s_r = ref.scores_and_bounds(H, R, fwd)[0], ref.scores_and_bounds(H, R, rev)[0]
    anti = fwd[:, 1] == 0
    assert np.array_equal(s_f[anti], -s_r[anti]) and np.array_equal(s_f[~anti], s_r[~anti])
    assert np.abs(s_f[anti]).max() > 0
    self_triples = anti & (fwd[:, 0] == fwd[:, 2])
    assert self_triples.any() and np.all(s_f[self_triples] == 0.0)


def test_zero_imaginary_relation_equals_distmult_on_doubled_relation():
    H, R, triples, labels, weights = _case(7)
    m = H.shape[1] // 2
    R[:, m:] = 0.0
    R2 = np.concatenate([R[:, :m], R[:, :m]], axis=1)
    r, d = ref.complex_ce(H, R, triples, labels, weights), dref.distmult_ce(H, R2, triples, labels, weights)
    np.testing.assert_allclose(r.scores, d.scores, rtol=1e-13, atol=1e-13)
    assert abs(r.loss - d.loss) <= 1e-13 and r.counts == d.counts
    np.testing.assert_allclose(r.gscore, d.gscore, rtol=1e-12, atol=1e-15)
    dH, dR, _, _ = ref.complex_backward(H, R, triples, r.gscore)
    dH2, dR2, _, _ = dref.distmult_backward(H, R2, triples, r.gscore)
    np.testing.assert_allclose(dH, dH2, rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(dR[:, :m], dR2[:, :m] + dR2[:, m:], rtol=1e-11, atol=1e-14)  # d / d r_re; r_re feeds both halves of R'
    for corrupt in ("dst", "src"):
        got, want = ref.complex_rank(H, R, triples[:20], corrupt), dref.distmult_rank(H, R2, triples[:20], corrupt)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


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
    Hc, Rc = _as_complex(torch.tensor(H)), _as_complex(torch.tensor(R))
    q = torch.tensor(queries)
    if corrupt == "dst":
        dense = torch.einsum("qk,vk->qv", Hc[q[:, 0]] * Rc[q[:, 1]], Hc.conj()).real.numpy()
        truth = queries[:, 2]
    else:
        dense = torch.einsum("vk,qk->qv", Hc, Rc[q[:, 1]] * Hc[q[:, 2]].conj()).real.numpy()
        truth = queries[:, 0]
    # the query vector: the score is linear in the candidate's row
    x = H[queries[:, 0]] if corrupt == "dst" else H[queries[:, 2]]
    np.testing.assert_allclose(ref.query_vector(x, R[queries[:, 1]], corrupt) @ H.T, dense, rtol=1e-12, atol=1e-12)
    for filtered in (False, True):
        g, e, lo, hi = ref.complex_rank(H, R, queries, corrupt, offsets if filtered else None, ids if filtered else None)
        for i in range(len(queries)):
            cands = [c for c in range(V) if c != truth[i] and not (filtered and c in set(lists[i].tolist()))]
            s = dense[i, truth[i]]
            if integer:  # exact: ties included
                assert g[i] == sum(dense[i, c] > s for c in cands) and e[i] == sum(dense[i, c] == s for c in cands)
            else:
                assert g[i] == sum(dense[i, c] > s + 1e-12 for c in cands) and e[i] == 0
            assert lo[i] <= g[i] <= g[i] + e[i] <= hi[i]
    if integer:
        assert ref.complex_rank(H, R, queries, corrupt)[1].sum() > 0  # the exact family does produce ties
