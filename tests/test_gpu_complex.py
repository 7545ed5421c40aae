"""tfgnn_complex_ce_metrics, tfgnn_complex_backward and tfgnn_complex_rank on the device against
tests/complex_reference.py, the float64 restatement of their contracts (include/tfgnn.h; pinned against torch's complex
arithmetic in tests/test_complex_reference_host.py).  Not run per GEMM mode: no product is involved.

Two input families, as in tests/test_gpu_distmult.py.  EXACT: H and R integer-valued in [-2, 2], D <= 64 - every product is an
integer of at most 8 and every score an integer of at most 2 D * 8 = 1024 in magnitude, exact in fp32 in any order - so
scores, confusion counts and ranking counts must equal the reference's, exact-zero scores and ties included.  FLOAT: randn
inputs, every figure inside the bound the reference derives next to its value (the module docstring of
tests/complex_reference.py); the seeds are such that no counted triple has a score within its bound of 0 (asserted on the
CPU when a case is built), so the confusion counts must match exactly as well.

The relations of every case: 0 general (most triples), 1 an all-zero row (scores exactly 0: predicted 0), 2 with r_im = 0 (a
symmetric score), 3 with r_re = 0 (an antisymmetric score: in the EXACT family s(u, t, v) == -s(v, t, u) and a self triple
scores exactly 0; in the FLOAT family a self triple of this relation would have an exact score of 0 inside a positive bound,
so those take relation 0 there), 4 without a triple.  Every case has self triples, labels outside {0, 1} (2, 0.5, -1, NaN)
and - in the weighted runs - zero, negative and NaN weights; the cases with V >= 50 have a node without an entry, the hub
cases a node with >= 2000 entries among 50 nodes.  D: 2 is one complex column, 64 half a wave, 128 exactly one column per
lane, 130 gives one lane a second column, 514 is one complex column past the 256-column register tile of the backward walk,
1024 the limit.  N = 255, 256, 257 straddle the chunk size of both backward passes (relation 0 holds most triples), 513 and
2300 give several chunks.  H sits inside a wider array, dH is written into one; their other columns must stay as they were."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import complex_reference as ref
from tests import distmult_reference as dref

pytestmark = pytest.mark.gpu

T_REL = 5
# (family, V, D, N, hub)
CASES = [
    ("exact", 1, 2, 1, False), ("exact", 2, 6, 255, False), ("exact", 50, 64, 256, False), ("exact", 50, 64, 257, False),
    ("exact", 50, 6, 2300, True), ("exact", 3001, 64, 513, False),
    ("float", 1, 2, 1, False), ("float", 2, 6, 257, False), ("float", 50, 2, 513, False), ("float", 50, 128, 256, False),
    ("float", 50, 130, 255, False), ("float", 50, 320, 256, False), ("float", 50, 514, 513, False), ("float", 50, 1024, 257, False),
    ("float", 50, 130, 2300, True), ("float", 3001, 64, 2300, False), ("float", 3001, 320, 513, False),
]
# FLOAT cases whose first seed puts a counted score within its bound of 0 (found on the CPU, from the reference alone)
SEED_SHIFT = {(50, 1024, 257): 1}
PAD_LEFT, PAD_RIGHT = 2, 3


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(family, V, D, N, hub):
    rng = np.random.default_rng(7919 * V + 31 * D + N + 1000003 * SEED_SHIFT.get((V, D, N), 0))
    m = D // 2
    if family == "exact":
        H = rng.integers(-2, 3, size=(V, D)).astype(np.float32)
        R = rng.integers(-2, 3, size=(T_REL, D)).astype(np.float32)
    else:
        H = rng.standard_normal((V, D)).astype(np.float32)
        R = rng.standard_normal((T_REL, D)).astype(np.float32)
    R[1] = 0.0
    R[2, m:] = 0.0
    R[3, :m] = 0.0
    hi = V - 1 if V >= 50 else V  # node V - 1 has no entry
    triples = np.stack([rng.integers(0, hi, N), np.zeros(N, dtype=np.int64), rng.integers(0, hi, N)], axis=1)
    triples[4::5, 1] = 1
    triples[7::11, 1] = 2
    triples[2::7, 1] = 3
    triples[::17, 2] = triples[::17, 0]  # self triples
    if hub:
        triples[:1100, 0] = 0
        triples[1100:2200, 2] = 0
    if family == "exact":
        triples[17::34, 1] = 3  # self triples of the antisymmetric relation: exactly 0
    else:
        triples[(triples[:, 0] == triples[:, 2]) & (triples[:, 1] == 3), 1] = 0
    labels = rng.integers(0, 2, N).astype(np.float32)
    weights = rng.uniform(0.25, 2.0, N).astype(np.float32)
    for i, bad in zip((3, 9, 14, 20), (2.0, 0.5, -1.0, np.nan)):
        if i < N:
            labels[i] = bad
    for i, bad in zip((6, 12, 18), (0.0, -1.0, np.nan)):
        if i < N:
            weights[i] = bad
    out = {"H": H, "R": R, "triples": triples.astype(np.int32), "labels": labels, "weights": weights, "ref": {}}
    for kind, w in (("none", None), ("weighted", weights)):
        r = ref.complex_ce(H, R, triples, labels, w)
        close = r.counted & (np.abs(r.scores) <= r.score_bound) & (r.score_bound > 0)
        assert family == "exact" or not close.any(), f"seed of {family, V, D, N}: a counted score within its bound of 0"
        out["ref"][kind] = (r, ref.complex_backward(H, R, triples, r.gscore, ref.gscore_error(r, w)))
    return out


def test_case_seeds_keep_counted_scores_away_from_zero():
    """builds every case on the CPU: the assertion in _case"""
    for case in CASES:
        _case(*case)


def _ratio(err, bound):
    """the largest error / bound; an error where the bound is 0 must be 0"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    assert np.all(err[bound == 0] == 0), "an error where the bound is exactly 0"
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if nz.any() else 0.0


def _device_inputs(c, dev):
    from tf2_gnn_amd import ops

    V, D = c["H"].shape
    wide = torch.full((V, PAD_LEFT + D + PAD_RIGHT), 7.5)
    wide[:, PAD_LEFT:PAD_LEFT + D] = torch.from_numpy(c["H"])
    wide = wide.to(dev)
    tables = ops.build_triple_tables(c["triples"], V, T_REL)
    return (wide, wide[:, PAD_LEFT:PAD_LEFT + D], torch.from_numpy(c["R"]).to(dev), torch.from_numpy(c["triples"]).to(dev),
            torch.from_numpy(c["labels"]).to(dev), torch.from_numpy(c["weights"]).to(dev),
            {k: torch.from_numpy(v).to(dev) for k, v in tables.items()}, tables)


@pytest.mark.parametrize("kind", ["none", "weighted"])
@pytest.mark.parametrize("family,V,D,N,hub", CASES)
def test_complex_forward_and_backward(dev, family, V, D, N, hub, kind):
    from tf2_gnn_amd import ops

    c = _case(family, V, D, N, hub)
    r, (dH64, dR64, bH, bR) = c["ref"][kind]
    wide, H, R, triples, labels, weights, tables, host_tables = _device_inputs(c, dev)
    w = weights if kind == "weighted" else None
    # labels and weights by element stride: the two columns of one [N, 2] array
    yw = torch.stack([labels, weights], dim=1)
    y_col, w_col = yw[:, 0], (yw[:, 1] if w is not None else None)

    before, d_before = ops.complex_launch_counts(), ops.link_launch_counts()
    metrics, counts, scores, gscore = ops.complex_ce_metrics(H, R, triples, y_col, w_col)
    mid = ops.complex_launch_counts()
    assert mid["complex_fwd"] - before["complex_fwd"] == 3 and mid["complex_bwd"] == before["complex_bwd"]
    m2, c2, s2, g2 = ops.complex_ce_metrics(H, R, triples, labels, w)  # contiguous columns, second run
    m3, c3, s3, g3 = ops.complex_ce_metrics(H, R, triples, labels, w, need_grad=False, want_scores=False)
    m4, c4, _, _ = ops.complex_ce_metrics(H, R, triples, labels, w, need_grad=False, want_scores=False, want_counts=False)
    assert s3 is None and g3 is None and c4 is None
    for m in (m2, m3, m4):
        assert torch.equal(_bits(m), _bits(metrics))  # bit-identical, with or without the outputs
    assert torch.equal(c2, counts) and torch.equal(c3, counts)
    assert torch.equal(_bits(s2), _bits(scores)) and torch.equal(_bits(g2), _bits(gscore))
    assert torch.equal(wide[:, :PAD_LEFT], torch.full_like(wide[:, :PAD_LEFT], 7.5))

    s, g = scores.cpu().numpy().astype(np.float64), gscore.cpu().numpy().astype(np.float64)
    if family == "exact":
        assert np.array_equal(s, r.scores)
        assert np.abs(r.scores).max() <= 1024
    rel = c["triples"][:, 1]
    assert np.all(s[rel == 1] == 0.0)  # the zero relation: exactly 0
    ratios = {"score": _ratio(np.abs(s - r.scores), r.score_bound)}
    assert [int(x) for x in counts.cpu()] == list(r.counts)
    assert sum(r.counts) == int(r.counted.sum())
    loss, acc = float(metrics[0]), float(metrics[1])
    ratios["loss"] = abs(loss - r.loss) / r.loss_bound
    if r.counted.any():
        assert abs(acc - r.accuracy) <= 1e-6
    else:
        assert math.isnan(acc) and loss == 0.0
    assert np.all(g[~r.counted] == 0.0)
    g_bound = ref.gscore_error(r, c["weights"] if kind == "weighted" else None)
    ratios["gscore"] = _ratio(np.abs(g - r.gscore), g_bound)

    # backward: into a wider, pre-filled array; then accumulate on top of it
    dwide = torch.full((V, PAD_LEFT + D + PAD_RIGHT), -3.25, device=dev)
    out = dwide[:, PAD_LEFT:PAD_LEFT + D]
    dH, dR = ops.complex_backward(H, R, triples, gscore, tables, out=out)
    after = ops.complex_launch_counts()
    assert after["complex_bwd"] - mid["complex_bwd"] == 4 and after["complex_fwd"] == mid["complex_fwd"] + 3 * 3
    assert dH is out
    pads = torch.cat([dwide[:, :PAD_LEFT], dwide[:, PAD_LEFT + D:]], dim=1)
    assert torch.equal(pads, torch.full_like(pads, -3.25))
    dH2, dR2 = ops.complex_backward(H, R, triples, gscore, tables)  # run to run
    assert torch.equal(_bits(dH2), _bits(out)) and torch.equal(_bits(dR2), _bits(dR))
    only_dR = ops.complex_backward(H, R, triples, gscore, tables, want_dH=False)
    only_dH = ops.complex_backward(H, R, triples, gscore, tables, want_dR=False)
    assert only_dR[0] is None and only_dH[1] is None
    assert torch.equal(_bits(only_dR[1]), _bits(dR)) and torch.equal(_bits(only_dH[0]), _bits(dH2))
    ratios["dH"] = _ratio(np.abs(dH2.cpu().numpy() - dH64), bH)
    ratios["dR"] = _ratio(np.abs(dR.cpu().numpy() - dR64), bR)
    no_entry = np.diff(host_tables["node_offsets"].view(np.uint32).astype(np.int64)) == 0
    no_triple = np.diff(host_tables["rel_offsets"].view(np.uint32).astype(np.int64)) == 0
    assert no_triple[T_REL - 1] and (V < 50 or no_entry[V - 1])
    assert not dH2[torch.from_numpy(no_entry).to(dev)].any() and not dR[torch.from_numpy(no_triple).to(dev)].any()
    if hub:
        assert np.diff(host_tables["node_offsets"].astype(np.int64))[0] >= 2000

    prefill = torch.randn((V, D), generator=torch.Generator().manual_seed(5)).to(dev)
    out.copy_(prefill)
    ops.complex_backward(H, R, triples, gscore, tables, want_dR=False, accumulate=True, out=out)
    assert torch.equal(out, prefill + dH2)  # dH = dH + sum, one fp32 addition per element
    assert torch.equal(pads, torch.cat([dwide[:, :PAD_LEFT], dwide[:, PAD_LEFT + D:]], dim=1))
    with pytest.raises(ValueError, match="out="):
        ops.complex_backward(H, R, triples, gscore, tables, accumulate=True)
    # not one launch of all this came from the DistMult entries
    assert ops.link_launch_counts() == d_before

    print(f"complex {family} V={V} D={D} N={N} {kind}: error / bound " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


@pytest.mark.parametrize("V,D,N", [(2, 6, 255), (50, 64, 257), (3001, 64, 513)])
def test_exact_antisymmetric_relation(dev, V, D, N):
    """r_re = 0 (relation 3) in the EXACT family: s(u, t, v) == -s(v, t, u) and self triples score exactly 0; r_im = 0
    (relation 2): s(u, t, v) == s(v, t, u)."""
    from tf2_gnn_amd import ops

    c = _case("exact", V, D, N, False)
    _, H, R, triples, labels, _, _, _ = _device_inputs(c, dev)
    reverse = triples[:, [2, 1, 0]].contiguous()
    s_fwd = ops.complex_ce_metrics(H, R, triples, labels, need_grad=False)[2].cpu().numpy()
    s_rev = ops.complex_ce_metrics(H, R, reverse, labels, need_grad=False)[2].cpu().numpy()
    rel, self_triple = c["triples"][:, 1], c["triples"][:, 0] == c["triples"][:, 2]
    assert (rel == 3).sum() > 10 and (self_triple & (rel == 3)).any() and np.abs(s_fwd[rel == 3]).max() > 0
    assert np.array_equal(s_fwd[rel == 3], -s_rev[rel == 3])
    assert np.all(s_fwd[self_triple & (rel == 3)] == 0.0)
    assert np.array_equal(s_fwd[rel == 2], s_rev[rel == 2])
    assert not np.array_equal(s_fwd[rel == 0], s_rev[rel == 0])


def test_asymmetry_where_distmult_is_symmetric(dev):
    """For a relation with r_im != 0 the ComplEx score of (u, t, v) differs from that of (v, t, u) by more than the sum of the
    two scores' bounds, on every triple of a seeded case; tfgnn_distmult_ce_metrics gives equal BITS for the two.  The
    relation's entries are signed powers of two, so that DistMult's H[u, d] * R[t, d] is exact and its per-column
    fma(H[u] R, H[v], p) rounds the same number whichever end comes first: its symmetry is then exact in fp32, not only in
    exact arithmetic.  The seed is such that the float64 scores differ by more than four times the summed bounds (asserted
    from the reference alone)."""
    from tf2_gnn_amd import ops

    V, D, N = 40, 128, 64
    rng = np.random.default_rng(2016)
    H = rng.standard_normal((V, D)).astype(np.float32)
    R = (rng.choice([-1.0, 1.0], size=(1, D)) * rng.choice([0.5, 1.0, 2.0], size=(1, D))).astype(np.float32)
    u = rng.integers(0, V, N)
    v = (u + 1 + rng.integers(0, V - 1, N)) % V  # no self triple
    fwd = np.stack([u, np.zeros(N, dtype=np.int64), v], axis=1).astype(np.int32)
    rev = fwd[:, ::-1].copy()
    (s_f, b_f), (s_r, b_r) = ref.scores_and_bounds(H, R, fwd), ref.scores_and_bounds(H, R, rev)
    assert np.all(np.abs(s_f - s_r) > 4 * (b_f + b_r)), "seed: a pair of float64 scores too close to tell apart"
    Hd, Rd, y = torch.from_numpy(H).to(dev), torch.from_numpy(R).to(dev), torch.zeros(N, device=dev)
    c_f = ops.complex_ce_metrics(Hd, Rd, fwd, y, need_grad=False)[2].cpu().numpy().astype(np.float64)
    c_r = ops.complex_ce_metrics(Hd, Rd, rev, y, need_grad=False)[2].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(c_f - s_f) <= b_f) and np.all(np.abs(c_r - s_r) <= b_r)
    assert np.all(np.abs(c_f - c_r) > b_f + b_r)
    d_f = ops.distmult_ce_metrics(Hd, Rd, fwd, y, need_grad=False)[2]
    d_r = ops.distmult_ce_metrics(Hd, Rd, rev, y, need_grad=False)[2]
    assert torch.equal(_bits(d_f), _bits(d_r)) and bool(d_f.abs().max() > 0)


@pytest.mark.parametrize("V,D,N,hub", [(50, 130, 255, False), (50, 320, 256, False), (50, 130, 2300, True)])
def test_zero_imaginary_relations_agree_with_the_distmult_kernels(dev, V, D, N, hub):
    """R_im = 0: ops.complex_* on (H, R) against ops.distmult_* on (H, [R_re ; R_re]) - the same mathematical values - within
    the sum of the two references' bounds (by bound, not bit for bit: the operation orders differ)."""
    from tf2_gnn_amd import ops

    c = _case("float", V, D, N, hub)
    m = D // 2
    Rc = c["R"].copy()
    Rc[:, m:] = 0.0
    Rd = np.concatenate([Rc[:, :m], Rc[:, :m]], axis=1)
    rc = ref.complex_ce(c["H"], Rc, c["triples"], c["labels"], c["weights"])
    rd = dref.distmult_ce(c["H"], Rd, c["triples"], c["labels"], c["weights"])
    np.testing.assert_allclose(rc.scores, rd.scores, rtol=1e-12, atol=1e-12)
    _, _, bHc, bRc = ref.complex_backward(c["H"], Rc, c["triples"], rc.gscore, ref.gscore_error(rc, c["weights"]))
    _, _, bHd, bRd = dref.distmult_backward(c["H"], Rd, c["triples"], rd.gscore, dref.gscore_error(rd, c["weights"]))
    _, H, _, triples, labels, weights, tables, _ = _device_inputs(c, dev)
    Rc_dev, Rd_dev = torch.from_numpy(Rc).to(dev), torch.from_numpy(Rd).to(dev)
    mc, cc, sc, gc = ops.complex_ce_metrics(H, Rc_dev, triples, labels, weights)
    md, cd, sd, gd = ops.distmult_ce_metrics(H, Rd_dev, triples, labels, weights)
    f64 = lambda t: t.cpu().numpy().astype(np.float64)
    assert np.all(np.abs(f64(sc) - f64(sd)) <= rc.score_bound + rd.score_bound)
    assert abs(float(mc[0]) - float(md[0])) <= rc.loss_bound + rd.loss_bound
    dHc, dRc = ops.complex_backward(H, Rc_dev, triples, gc, tables)
    dHd, dRd = ops.distmult_backward(H, Rd_dev, triples, gd, tables)
    assert np.all(np.abs(f64(dHc) - f64(dHd)) <= bHc + bHd)
    dRd64 = f64(dRd)
    # d / d r_re: r_re feeds both halves of [R_re ; R_re]
    assert np.all(np.abs(f64(dRc)[:, :m] - (dRd64[:, :m] + dRd64[:, m:])) <= bRc[:, :m] + bRd[:, :m] + bRd[:, m:])
    queries = c["triples"][:40]
    for corrupt in ("dst", "src"):
        g_c, e_c = (f64(t) for t in ops.complex_rank(H, Rc_dev, queries, corrupt))
        g_d, e_d = (f64(t) for t in ops.distmult_rank(H, Rd_dev, queries, corrupt))
        _, _, lo_c, hi_c = ref.complex_rank(c["H"], Rc, queries, corrupt)
        _, _, lo_d, hi_d = dref.distmult_rank(c["H"], Rd, queries, corrupt)
        lo, hi = np.minimum(lo_c, lo_d), np.maximum(hi_c, hi_d)
        assert np.all(lo <= g_c) and np.all(g_c + e_c <= hi) and np.all(lo <= g_d) and np.all(g_d + e_d <= hi)


def test_nothing_counted_and_nan_scores(dev):
    from tf2_gnn_amd import ops

    c = _case("float", 50, 130, 255, False)
    _, H, R, triples, labels, _, _, _ = _device_inputs(c, dev)
    N = triples.shape[0]
    metrics, counts, _, gscore = ops.complex_ce_metrics(H, R, triples, labels, torch.zeros(N, device=dev))
    assert float(metrics[0]) == 0.0 and math.isnan(float(metrics[1])) and not counts.any() and not gscore.any()
    # a NaN in a node row: NaN loss when a counted triple reads it, a finite loss when only uncounted ones do
    u = int(c["triples"][0, 0])
    touched = torch.from_numpy((c["triples"][:, 0] == u) | (c["triples"][:, 2] == u)).to(dev)
    Hn = H.contiguous().clone()
    Hn[u, 0] = float("nan")
    m_nan, _, s_nan, _ = ops.complex_ce_metrics(Hn, R, triples, labels)
    assert math.isnan(float(m_nan[0])) and bool(torch.isnan(s_nan[touched]).all())  # NaN * 0 is NaN: the zero relation too
    w = torch.ones(N, device=dev)
    w[touched] = 0.0
    m_ok, _, _, g_ok = ops.complex_ce_metrics(Hn, R, triples, labels, w)
    assert math.isfinite(float(m_ok[0])) and bool(torch.isfinite(g_ok).all()) and not g_ok[touched].any()


# ---- ranking ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rank_case(family, V, Q, D):
    rng = np.random.default_rng(104729 * V + 13 * Q + D)
    m = D // 2
    if family == "exact":
        H = rng.integers(-2, 3, size=(V, D)).astype(np.float32)
        R = rng.integers(-2, 3, size=(4, D)).astype(np.float32)
    else:
        H = rng.standard_normal((V, D)).astype(np.float32)
        R = rng.standard_normal((4, D)).astype(np.float32)
    R[1, m:] = 0.0  # r_im = 0
    R[2, :m] = 0.0  # r_re = 0
    R[3] = 0.0      # every candidate ties with the true entity
    queries = np.stack([rng.integers(0, V, Q), rng.integers(0, 4, Q), rng.integers(0, V, Q)], axis=1).astype(np.int32)
    if family == "float":
        queries[queries[:, 1] == 3, 1] = 0  # exact ties of NaN-free zeros belong to the exact family
    if V >= 65:  # query 0: another entity with the true entity's row, bit for bit, on either side
        queries[0] = (5, 0, 9)
        H[V - 1], H[V - 2] = H[9], H[5]
    filters = {}
    for corrupt, slot in (("dst", 2), ("src", 0)):
        lists = [np.unique(np.concatenate([rng.integers(0, V, rng.integers(0, min(V, 6) + 1)), [q[slot]] * (i % 2 == 0)])).astype(np.int64)
                 for i, q in enumerate(queries)]  # every second filter holds the true entity
        offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
        ids = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
        filters[corrupt] = (offsets, ids)
    want = {(corrupt, filtered): ref.complex_rank(H, R, queries, corrupt, *(filters[corrupt] if filtered else (None, None)))
            for corrupt in ("dst", "src") for filtered in (False, True)}
    return H, R, queries, filters, want


@pytest.mark.parametrize("D", [2, 64, 128, 130])
@pytest.mark.parametrize("Q", [1, 17, 300])
@pytest.mark.parametrize("V", [1, 2, 65, 1000])
def test_complex_rank(dev, V, Q, D):
    from tf2_gnn_amd import ops

    d_before = ops.link_launch_counts()
    for family in (["exact", "float"] if D <= 64 else ["float"]):
        H, R, queries, filters, want = _rank_case(family, V, Q, D)
        wide = torch.zeros((V, D + 3))
        wide[:, :D] = torch.from_numpy(H)
        Hd, Rd = wide.to(dev)[:, :D], torch.from_numpy(R).to(dev)
        for (corrupt, filtered), (g64, e64, lo, hi) in want.items():
            before = ops.complex_launch_counts()["complex_rank"]
            fo, fi = filters[corrupt] if filtered else (None, None)
            greater, equal = ops.complex_rank(Hd, Rd, queries, corrupt, fo, fi)
            assert ops.complex_launch_counts()["complex_rank"] - before == 2
            assert greater.dtype == equal.dtype == torch.int32 and tuple(greater.shape) == tuple(equal.shape) == (Q,)
            g, e = greater.cpu().numpy().astype(np.int64), equal.cpu().numpy().astype(np.int64)
            what = (family, V, Q, D, corrupt, filtered)
            assert g.min() >= 0 and e.min() >= 0, what
            if family == "exact":
                assert np.array_equal(g, g64) and np.array_equal(e, e64), what
            else:
                assert np.all(lo <= g) and np.all(g <= hi) and np.all(lo <= g + e) and np.all(g + e <= hi), what
            if V >= 65 and not filtered:
                assert e64[0] >= 1 and e[0] >= 1, what  # the duplicated row counts as equal, in fp32 as in float64
            again = ops.complex_rank(Hd, Rd, queries, corrupt, fo, fi)
            assert torch.equal(again[0], greater) and torch.equal(again[1], equal)
        if family == "exact" and V >= 65 and Q >= 17:
            assert want[("dst", False)][1].sum() > 0  # ties do occur
    assert ops.link_launch_counts() == d_before
