"""tfgnn_distmult_ce_metrics, tfgnn_distmult_backward and tfgnn_distmult_rank on the device against
tests/distmult_reference.py, the float64 restatement of their contracts (include/tfgnn.h; pinned against torch in
tests/test_distmult_reference_host.py).  Not run per GEMM mode: no product is involved.

Two input families.  EXACT: H and R integer-valued in [-2, 2], D <= 64 - every score is exact in fp32 in any order
(|s| <= 512), so scores, confusion counts and ranking counts must equal the reference's, exact-zero scores and ties
included.  FLOAT: randn inputs, every figure inside the bound the reference derives next to its value (the module docstring of
tests/distmult_reference.py); the seeds are such that no counted triple has a score within its bound of 0 (asserted), so the
confusion counts must match exactly as well.

Every case has: relation 1 with an all-zero embedding (scores exactly 0: predicted 0), the last relation without a triple,
self triples, labels outside {0, 1} (2, 0.5, -1, NaN), and - in the weighted runs - zero, negative and NaN weights; the cases
with V >= 50 have a node without an entry, and the hub cases a node with >= 2000 entries among 50 nodes (8 chunks of the node
pass).  N = 255, 256, 257 straddle the chunk size of both backward passes (256; relation 0 holds most triples), 513 and 2300
give several chunks.  H sits inside a wider array, dH is written into one; their other columns must stay as they were."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import distmult_reference as ref

pytestmark = pytest.mark.gpu

T_REL = 4  # relation 0: most triples; 1: zero embedding; 2: a few; 3: none
# (family, V, D, N, hub)
CASES = [
    ("exact", 1, 1, 1, False), ("exact", 2, 3, 255, False), ("exact", 50, 64, 256, False), ("exact", 50, 64, 257, False),
    ("exact", 50, 3, 2300, True), ("exact", 3001, 64, 513, False),
    ("float", 1, 1, 1, False), ("float", 2, 3, 257, False), ("float", 50, 65, 255, False), ("float", 50, 320, 256, False),
    ("float", 50, 1024, 257, False), ("float", 50, 65, 2300, True), ("float", 3001, 64, 2300, False), ("float", 3001, 320, 513, False),
    ("float", 50, 1, 513, False),
]
PAD_LEFT, PAD_RIGHT = 2, 3


@functools.lru_cache(maxsize=None)
def _case(family, V, D, N, hub):
    rng = np.random.default_rng(7919 * V + 31 * D + N)
    if family == "exact":
        H = rng.integers(-2, 3, size=(V, D)).astype(np.float32)
        R = rng.integers(-2, 3, size=(T_REL, D)).astype(np.float32)
    else:
        H = rng.standard_normal((V, D)).astype(np.float32)
        R = rng.standard_normal((T_REL, D)).astype(np.float32)
    R[1] = 0.0
    hi = V - 1 if V >= 50 else V  # node V - 1 has no entry
    triples = np.stack([rng.integers(0, hi, N), np.zeros(N, dtype=np.int64), rng.integers(0, hi, N)], axis=1)
    triples[4::5, 1] = 1
    triples[7::11, 1] = 2
    triples[::17, 2] = triples[::17, 0]  # self triples
    if hub:
        triples[:1100, 0] = 0
        triples[1100:2200, 2] = 0
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
        r = ref.distmult_ce(H, R, triples, labels, w)
        close = r.counted & (np.abs(r.scores) <= r.score_bound) & (r.score_bound > 0)
        assert family == "exact" or not close.any(), f"seed of {family, V, D, N}: a counted score within its bound of 0"
        out["ref"][kind] = (r, ref.distmult_backward(H, R, triples, r.gscore, ref.gscore_error(r, w)))
    return out


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
def test_distmult_forward_and_backward(dev, family, V, D, N, hub, kind):
    from tf2_gnn_amd import ops

    c = _case(family, V, D, N, hub)
    r, (dH64, dR64, bH, bR) = c["ref"][kind]
    wide, H, R, triples, labels, weights, tables, host_tables = _device_inputs(c, dev)
    w = weights if kind == "weighted" else None
    # labels and weights by element stride: the two columns of one [N, 2] array
    yw = torch.stack([labels, weights], dim=1)
    y_col, w_col = yw[:, 0], (yw[:, 1] if w is not None else None)

    before = ops.link_launch_counts()
    metrics, counts, scores, gscore = ops.distmult_ce_metrics(H, R, triples, y_col, w_col)
    mid = ops.link_launch_counts()
    assert mid["distmult_fwd"] - before["distmult_fwd"] == 3 and mid["distmult_bwd"] == before["distmult_bwd"]
    m2, c2, s2, g2 = ops.distmult_ce_metrics(H, R, triples, labels, w)  # contiguous columns, second run
    m3, c3, s3, g3 = ops.distmult_ce_metrics(H, R, triples, labels, w, need_grad=False, want_scores=False)
    m4, c4, _, _ = ops.distmult_ce_metrics(H, R, triples, labels, w, need_grad=False, want_scores=False, want_counts=False)
    assert s3 is None and g3 is None and c4 is None
    for m in (m2, m3, m4):
        assert torch.equal(m.view(torch.int32), metrics.view(torch.int32))  # bit-identical, with or without the outputs
    assert torch.equal(c2, counts) and torch.equal(c3, counts)
    assert torch.equal(s2.view(torch.int32), scores.view(torch.int32)) and torch.equal(g2.view(torch.int32), gscore.view(torch.int32))
    assert torch.equal(wide[:, :PAD_LEFT], torch.full_like(wide[:, :PAD_LEFT], 7.5))

    s, g = scores.cpu().numpy().astype(np.float64), gscore.cpu().numpy().astype(np.float64)
    if family == "exact":
        assert np.array_equal(s, r.scores)
        assert np.abs(r.scores).max() <= 512
    zero = c["triples"][:, 1] == 1
    assert np.all(s[zero] == 0.0)  # the zero relation: exactly 0
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
    dH, dR = ops.distmult_backward(H, R, triples, gscore, tables, out=out)
    after = ops.link_launch_counts()
    assert after["distmult_bwd"] - mid["distmult_bwd"] == 4 and after["distmult_fwd"] == mid["distmult_fwd"] + 3 * 3
    assert dH is out
    pads = torch.cat([dwide[:, :PAD_LEFT], dwide[:, PAD_LEFT + D:]], dim=1)
    assert torch.equal(pads, torch.full_like(pads, -3.25))
    dH2, dR2 = ops.distmult_backward(H, R, triples, gscore, tables)
    assert torch.equal(dH2.view(torch.int32), out.contiguous().view(torch.int32)) and torch.equal(dR2.view(torch.int32), dR.view(torch.int32))
    only_dR = ops.distmult_backward(H, R, triples, gscore, tables, want_dH=False)
    only_dH = ops.distmult_backward(H, R, triples, gscore, tables, want_dR=False)
    assert only_dR[0] is None and only_dH[1] is None
    assert torch.equal(only_dR[1].view(torch.int32), dR.view(torch.int32)) and torch.equal(only_dH[0].view(torch.int32), dH2.view(torch.int32))
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
    ops.distmult_backward(H, R, triples, gscore, tables, want_dR=False, accumulate=True, out=out)
    assert torch.equal(out, prefill + dH2)  # dH = dH + sum, one fp32 addition per element
    assert torch.equal(pads, torch.cat([dwide[:, :PAD_LEFT], dwide[:, PAD_LEFT + D:]], dim=1))
    with pytest.raises(ValueError, match="out="):
        ops.distmult_backward(H, R, triples, gscore, tables, accumulate=True)

    print(f"distmult {family} V={V} D={D} N={N} {kind}: error / bound " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(v <= 1.0 for v in ratios.values()), ratios


def test_nothing_counted_and_nan_scores(dev):
    from tf2_gnn_amd import ops

    c = _case("float", 50, 65, 255, False)
    _, H, R, triples, labels, _, _, _ = _device_inputs(c, dev)
    N = triples.shape[0]
    metrics, counts, _, gscore = ops.distmult_ce_metrics(H, R, triples, labels, torch.zeros(N, device=dev))
    assert float(metrics[0]) == 0.0 and math.isnan(float(metrics[1])) and not counts.any() and not gscore.any()
    # a NaN in a node row: NaN loss when a counted triple reads it, a finite loss when only uncounted ones do
    u = int(c["triples"][0, 0])
    touched = torch.from_numpy((c["triples"][:, 0] == u) | (c["triples"][:, 2] == u)).to(dev)
    Hn = H.contiguous().clone()
    Hn[u, 0] = float("nan")
    m_nan, _, s_nan, _ = ops.distmult_ce_metrics(Hn, R, triples, labels)
    assert math.isnan(float(m_nan[0])) and bool(torch.isnan(s_nan[touched & torch.from_numpy(c["triples"][:, 1] != 1).to(dev)]).all())
    w = torch.ones(N, device=dev)
    w[touched] = 0.0
    m_ok, _, _, g_ok = ops.distmult_ce_metrics(Hn, R, triples, labels, w)
    assert math.isfinite(float(m_ok[0])) and bool(torch.isfinite(g_ok).all()) and not g_ok[touched].any()


# ---- ranking ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rank_case(family, V, Q, D):
    rng = np.random.default_rng(104729 * V + 13 * Q + D)
    if family == "exact":
        H = rng.integers(-2, 3, size=(V, D)).astype(np.float32)
        R = rng.integers(-2, 3, size=(3, D)).astype(np.float32)
    else:
        H = rng.standard_normal((V, D)).astype(np.float32)
        R = rng.standard_normal((3, D)).astype(np.float32)
    queries = np.stack([rng.integers(0, V, Q), rng.integers(0, 3, Q), rng.integers(0, V, Q)], axis=1).astype(np.int32)
    filters = {}
    for corrupt, slot in (("dst", 2), ("src", 0)):
        lists = [np.unique(np.concatenate([rng.integers(0, V, rng.integers(0, min(V, 6) + 1)), [q[slot]] * (i % 2 == 0)])).astype(np.int64)
                 for i, q in enumerate(queries)]  # every second filter holds the true entity
        offsets = np.concatenate([[0], np.cumsum([len(l) for l in lists])])
        ids = np.concatenate(lists) if lists else np.zeros(0, dtype=np.int64)
        filters[corrupt] = (offsets, ids)
    want = {(corrupt, filtered): ref.distmult_rank(H, R, queries, corrupt, *(filters[corrupt] if filtered else (None, None)))
            for corrupt in ("dst", "src") for filtered in (False, True)}
    return H, R, queries, filters, want


@pytest.mark.parametrize("D", [1, 64, 65])
@pytest.mark.parametrize("Q", [1, 17, 300])
@pytest.mark.parametrize("V", [1, 2, 65, 1000])
def test_distmult_rank(dev, V, Q, D):
    from tf2_gnn_amd import ops

    for family in (["exact", "float"] if D <= 64 else ["float"]):
        H, R, queries, filters, want = _rank_case(family, V, Q, D)
        wide = torch.zeros((V, D + 3))
        wide[:, :D] = torch.from_numpy(H)
        Hd, Rd = wide.to(dev)[:, :D], torch.from_numpy(R).to(dev)
        for (corrupt, filtered), (g64, e64, lo, hi) in want.items():
            before = ops.link_launch_counts()["distmult_rank"]
            fo, fi = filters[corrupt] if filtered else (None, None)
            greater, equal = ops.distmult_rank(Hd, Rd, queries, corrupt, fo, fi)
            assert ops.link_launch_counts()["distmult_rank"] - before == 2
            assert greater.dtype == equal.dtype == torch.int32 and tuple(greater.shape) == tuple(equal.shape) == (Q,)
            g, e = greater.cpu().numpy().astype(np.int64), equal.cpu().numpy().astype(np.int64)
            what = (family, V, Q, D, corrupt, filtered)
            assert g.min() >= 0 and e.min() >= 0, what
            if family == "exact":
                assert np.array_equal(g, g64) and np.array_equal(e, e64), what
            else:
                assert np.all(lo <= g) and np.all(g + e <= hi), what
            again = ops.distmult_rank(Hd, Rd, queries, corrupt, fo, fi)
            assert torch.equal(again[0], greater) and torch.equal(again[1], equal)
        if family == "exact" and V >= 65 and Q >= 17:
            assert want[("dst", False)][1].sum() > 0  # ties do occur
