"""tests/pool_reference.py and tests/pool_cases.py, checked without a device.

1. The reference is independent of the kernels AND of hand-written calculus: its forward restated in torch float64 ops, with
   torch.autograd.grad producing dT and dS, agrees with its hand-written backward to 1e-12.
2. The comparison of tests/test_gpu_pool_reference.py can fail: a numpy float32 restatement of the chunked scheme that the
   header describes (tiles of C nodes, per-chunk max / sum / weighted sums in two workspace slots per tile, combined in
   ascending chunk order) passes that comparison on that test's own inputs, and each planted defect fails it - without ever
   making a kernel wrong on a GPU."""
import numpy as np
import pytest
import torch

from tests import pool_cases as pc
from tests import pool_reference as ref

C = pc.C
F = np.float32
LOWEST = F(-3.402823466e38)


def test_chunk_size_is_the_librarys():
    from tf2_gnn_amd import _lib

    assert pc.C == _lib.POOL_CHUNK_NODES


# ---- 0. the reference on numbers small enough to do by hand -------------------------------------------------------------
def test_reference_by_hand():
    ptr = [0, 2, 2, 3]
    T = np.array([[1.0, -2.0], [3.0, 0.5], [np.nan, 4.0]])
    S = np.array([[0.0], [np.log(3.0)], [5.0]])
    dOut = np.array([[1.0, 10.0], [7.0, 7.0], [2.0, -1.0]])
    out, w = ref.forward("softmax", ptr, T, S, 1, -1.0, 2.0)
    z = 1.0 / 3.0 + 1.0 + 1e-7
    assert np.allclose(w[:, 0], [1.0 / 3.0 / z, 1.0 / z, 1.0 / (1.0 + 1e-7)], rtol=1e-15)
    assert np.allclose(out[0], [w[0, 0] * 1.0 + w[1, 0] * 2.0, w[0, 0] * -1.0 + w[1, 0] * 0.5], rtol=1e-15)
    assert (out[1] == 0).all() and np.isnan(out[2, 0]) and out[2, 1] == w[2, 0] * 2.0
    dT, dS = ref.backward("softmax", ptr, dOut, T, w, 1, -1.0, 2.0)
    assert dT[0, 0] == w[0, 0] * 1.0 and dT[0, 1] == 0.0 and dT[1, 0] == 0.0 and dT[1, 1] == w[1, 0] * 10.0
    assert dT[2, 0] == 0.0 and dT[2, 1] == 0.0  # with bounds the mask is false at a NaN
    dw = np.array([1.0 * 1.0 + -1.0 * 10.0, 2.0 * 1.0 + 0.5 * 10.0])
    t = w[0, 0] * dw[0] + w[1, 0] * dw[1]
    assert np.allclose(dS[:2, 0], [w[0, 0] * (dw[0] - t), w[1, 0] * (dw[1] - t)], rtol=1e-14) and np.isnan(dS[2, 0])
    # no bounds: no clip and no mask at all
    out, w = ref.forward("average", ptr, T, None, 1, None, None)
    assert np.allclose(out[0], [2.0, -0.75]) and np.isnan(out[2, 0]) and out[2, 1] == 4.0
    dT, dS = ref.backward("average", ptr, dOut, T, None, 1, None, None)
    assert dS is None and np.allclose(dT, [[0.5, 5.0], [0.5, 5.0], [2.0, -1.0]])
    # +inf clips to a bound and stays without one; ties pass the gradient
    assert ref.clip(np.array([np.inf, -np.inf, np.nan]), -1.0, 2.0).tolist()[:2] == [2.0, -1.0]
    assert np.isposinf(ref.clip(np.array([np.inf]), -1.0, None)[0])
    assert ref.pass_mask(np.array([-1.0, 2.0, 2.5, np.nan]), -1.0, 2.0).tolist() == [True, True, False, False]


# ---- 1. independence from hand-written calculus ---------------------------------------------------------------------------
def _torch_forward(kind, ptr, T, S, heads, lo, hi, detach_max=True):
    V, GD = T.shape
    G = len(ptr) - 1
    ph = GD // heads
    ids = torch.from_numpy(np.repeat(np.arange(G), np.diff(ptr))).long()
    R = T
    if lo is not None:
        R = torch.clamp(R, min=lo)
    if hi is not None:
        R = torch.clamp(R, max=hi)
    if kind == "softmax":
        m = torch.full((G, heads), -torch.inf, dtype=torch.float64).scatter_reduce(0, ids[:, None].expand(-1, heads), S, "amax")
        if detach_max:
            m = m.detach()
        e = torch.exp(S - m[ids])
        z = torch.zeros((G, heads), dtype=torch.float64).index_add_(0, ids, e)
        w = e / (z[ids] + 1e-7)
    elif kind == "sigmoid":
        w = S
    else:
        w = torch.ones((V, heads), dtype=torch.float64)
        if kind == "average":
            cnt = torch.from_numpy(np.maximum(np.diff(ptr), 1)).double()
            w = w / cnt[ids][:, None]
    weighted = (w[:, :, None] * R.reshape(V, heads, ph)).reshape(V, GD)
    return torch.zeros((G, GD), dtype=torch.float64).index_add_(0, ids, weighted), w


AUTOGRAD_BOUNDS = [(None, None), pc.TIE_BOUNDS, (pc.TIE_BOUNDS[0], None), (None, pc.TIE_BOUNDS[1])]


@pytest.mark.parametrize("bounds", AUTOGRAD_BOUNDS, ids=["nobounds", "both", "lower", "upper"])
@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("name", ["ties", "layout_long", "heads_130_65"])
def test_hand_written_backward_is_autograds(name, kind, bounds):
    case = pc.by_name(name)
    T32, S32, dOut32 = pc.inputs(case)
    if not case.ties:  # ties in all of them: T on the grid of eighths; empty graphs are in all three layouts
        T32 = (np.round(4.0 * T32) / 8.0).astype(np.float32)
    lo, hi = bounds
    Sk = pc.scores_for(kind, S32)
    T = torch.from_numpy(T32.astype(np.float64)).requires_grad_(True)
    S = None if Sk is None else torch.from_numpy(Sk.astype(np.float64)).requires_grad_(True)
    dOut = torch.from_numpy(dOut32.astype(np.float64))
    assert float((T32 == pc.TIE_BOUNDS[0]).mean()) > 0.02 and float((T32 == pc.TIE_BOUNDS[1]).mean()) > 0.02 and 0 in case.sizes
    out, w = _torch_forward(kind, case.ptr, T, S, case.heads, lo, hi)
    r_out, r_w = ref.forward(kind, case.ptr, T32, Sk, case.heads, lo, hi)
    r_dT, r_dS = ref.backward(kind, case.ptr, dOut32, T32, r_w if kind == "softmax" else Sk, case.heads, lo, hi)
    grads = torch.autograd.grad((out * dOut).sum(), [T] + ([S] if S is not None else []))

    def close(a, b, what, tol=1e-12):
        err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
        assert err.max(initial=0.0) <= tol, (what, float(err.max()))

    close(out.detach().numpy(), r_out, "out")
    close(w.detach().numpy(), r_w, "w")
    close(grads[0].numpy(), r_dT, "dT")
    if S is None:
        assert r_dS is None
    else:
        close(grads[1].numpy(), r_dS, "dS")
    if kind == "softmax":
        # The contract's dS holds the graph's maximum m constant.  Differentiating through m as well adds
        # -(sum w dw) * 1e-7 / (sum exp + 1e-7) at the node that holds the maximum (the 1e-7 breaks the shift invariance):
        # at most 1e-7 of sum w dw, below fp32 resolution.  Measured here so that the choice is on record.
        S2 = torch.from_numpy(Sk.astype(np.float64)).requires_grad_(True)
        out2, _ = _torch_forward(kind, case.ptr, T.detach(), S2, case.heads, lo, hi, detach_max=False)
        g2 = torch.autograd.grad((out2 * dOut).sum(), [S2])[0].numpy()
        _, dw = ref.backward("sigmoid", case.ptr, dOut32, T32, r_w, case.heads, lo, hi)
        close(g2, r_dS, "dS through the maximum", tol=1.01e-7 * max(1.0, float(np.abs(dw).max())))
        assert float(np.abs(g2 - r_dS).max()) > 1e-12  # and the term is there: the two are different functions


# ---- 2. the chunked scheme in numpy float32, with planted defects ---------------------------------------------------------
DEFECTS = ["no_rescale", "max_of_chunk0", "slots_swapped", "one_slot", "head_of_first_column", "strict_mask", "fmax_clip"]


def chunked_readout(case, kind, lo, hi, T, S, dOut, defect=None):
    """tfgnn_pool_forward + tfgnn_pool_backward as the header describes them, float32 -> dict(out, w, dT, dS).
    defect: None, or
      no_rescale            the combine adds the chunks' sums without exp(m_chunk - m)
      max_of_chunk0         the combine takes chunk 0's maximum for the graph's
      slots_swapped         a tile's partial results are written to the other slot than the combine reads
      one_slot              both chunks of a tile use slot 0
      head_of_first_column  on the float4 path the head of a column is that of the first column of its float4
      strict_mask           lo < T < hi in place of lo <= T <= hi
      fmax_clip             the clip as fmin(fmax(x, lo), hi), which returns the bound for a NaN"""
    ptr, heads, GD, V, G = case.ptr, case.heads, case.GD, case.V, case.G
    ph = GD // heads
    lo32, hi32 = F(-np.inf if lo is None else lo), F(np.inf if hi is None else hi)
    cols = np.arange(GD)
    hcol = cols // ph
    hcol_k = (cols // 4 * 4) // ph if (defect == "head_of_first_column" and case.vec4) else hcol
    weighted = kind in pc.WEIGHTED
    T = np.asarray(T, dtype=F)
    S = None if S is None else np.asarray(S, dtype=F)
    dOut = np.asarray(dOut, dtype=F)
    old = np.seterr(invalid="ignore", over="ignore")

    def clip32(x):
        if defect == "fmax_clip":
            return np.fmin(np.fmax(x, lo32), hi32)
        return np.where(x < lo32, lo32, np.where(x > hi32, hi32, x)).astype(F)

    def segments(g):
        a, b = int(ptr[g]), int(ptr[g + 1])
        if b - a <= C:
            return [(a, b, None)]
        return [(s, min(s + C, b), (s // C, 1 if k == 0 else 0)) for k, s in enumerate(range(a, b, C))]

    ws = {}
    empty = {"m": np.zeros(heads, F), "s": np.zeros(heads, F), "sums": np.zeros(GD, F), "t": np.zeros(heads, F)}

    def put(where, **kw):
        tile, slot = where
        if defect == "slots_swapped":
            slot = 1 - slot
        if defect == "one_slot":
            slot = 0
        ws.setdefault((tile, slot), dict(empty)).update(kw)

    def get(where):
        tile, slot = where
        if defect == "one_slot":
            slot = 0
        return ws.get((tile, slot), empty)

    out = np.zeros((G, GD), F)
    w = np.zeros((V, heads), F) if kind == "softmax" else None
    # forward, first launch
    for g in range(G):
        cnt = F(max(int(ptr[g + 1] - ptr[g]), 1))
        for a, b, where in segments(g):
            R = clip32(T[a:b])
            if kind == "softmax":
                m = np.fmax.reduce(S[a:b], axis=0, initial=LOWEST)  # fmaxf skips a NaN
                e = np.exp(S[a:b] - m).astype(F)
                s = e.sum(axis=0, dtype=F)
                if where is None:
                    inv = (F(1) / (s + F(1e-7))).astype(F)
                    w[a:b] = e * inv
                    out[g] = ((e * inv)[:, hcol_k] * R).sum(axis=0, dtype=F)
                else:
                    put(where, m=m, s=s, sums=(e[:, hcol_k] * R).sum(axis=0, dtype=F))
            else:
                wt = S[a:b][:, hcol_k] if kind == "sigmoid" else F(1)
                sums = (wt * R).sum(axis=0, dtype=F)
                if where is None:
                    out[g] = sums / cnt if kind == "average" else sums
                else:
                    put(where, sums=sums)
    # forward, second launch
    for g in range(G):
        segs = segments(g)
        if segs[0][2] is None:
            continue
        recs = [get(where) for _, _, where in segs]
        if kind == "softmax":
            m = np.fmax.reduce(np.stack([r["m"] for r in recs]), axis=0, initial=LOWEST)
            scale = [np.ones(heads, F) if defect == "no_rescale" else np.exp(r["m"] - m).astype(F) for r in recs]
            s = np.zeros(heads, F)
            for r, sc in zip(recs, scale):
                s = s + r["s"] * sc
            inv = (F(1) / (s + F(1e-7))).astype(F)
            if defect == "max_of_chunk0":  # the sum of exponentials is right, the weights are taken relative to chunk 0's maximum
                m = recs[0]["m"]
                scale = [np.exp(r["m"] - m).astype(F) for r in recs]
            a, b = int(ptr[g]), int(ptr[g + 1])
            w[a:b] = np.exp(S[a:b] - m).astype(F) * inv
            acc = np.zeros(GD, F)
            for r, sc in zip(recs, scale):
                acc = acc + r["sums"] * sc[hcol]
            out[g] = acc * inv[hcol]
        else:
            acc = np.zeros(GD, F)
            for r in recs:
                acc = acc + r["sums"]
            out[g] = acc / F(ptr[g + 1] - ptr[g]) if kind == "average" else acc
    # backward, first launch
    w_used = w if kind == "softmax" else S
    dT = np.zeros((V, GD), F)
    dS = np.zeros((V, heads), F) if weighted else None
    for g in range(G):
        cnt = F(max(int(ptr[g + 1] - ptr[g]), 1))
        for a, b, where in segments(g):
            x = T[a:b]
            mask = (x > lo32) & (x < hi32) if defect == "strict_mask" else (x >= lo32) & (x <= hi32)
            wt = w_used[a:b][:, hcol_k] if weighted else (F(1) / cnt if kind == "average" else F(1))
            dT[a:b] = np.where(mask, wt * dOut[g], F(0))
            if weighted:
                dw = (clip32(x) * dOut[g]).reshape(b - a, heads, ph).sum(axis=2, dtype=F)
                dS[a:b] = dw
                if kind == "softmax":
                    t = (w[a:b] * dw).sum(axis=0, dtype=F)
                    if where is None:
                        dS[a:b] = w[a:b] * (dw - t)
                    else:
                        put(where, t=t)
    # backward, second launch
    if kind == "softmax":
        for g in range(G):
            segs = segments(g)
            if segs[0][2] is None:
                continue
            t = np.zeros(heads, F)
            for _, _, where in segs:
                t = t + get(where)["t"]
            a, b = int(ptr[g]), int(ptr[g + 1])
            dS[a:b] = w[a:b] * (dS[a:b] - t)
    np.seterr(**old)
    return {"out": out, "w": w, "dT": dT, "dS": dS}


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.fixture(scope="module")
def verdicts():
    """{defect or None: set of (case name, kind, bounds) at which the comparison fails}: every case, kind and pair of bounds of
    the GPU test; the cases of 1024 columns are left to the clean restatement and the defect that depends on the width"""
    failed = {d: set() for d in [None] + DEFECTS}
    for case in pc.cases():
        T, S, dOut = pc.inputs(case)
        for kind in case.kinds:
            for lo, hi in case.bounds:
                pc.assert_conditions(case, kind, lo, hi)
                for d in [None] + DEFECTS:
                    if d is not None and case.GD >= 1024 and d != "head_of_first_column":
                        continue
                    got = chunked_readout(case, kind, lo, hi, T, pc.scores_for(kind, S), dOut, defect=d)
                    if _fails(lambda: pc.compare(case, kind, lo, hi, got)):
                        failed[d].add((case.name, kind, (lo, hi)))
    return failed


def test_the_clean_restatement_passes_everywhere(verdicts):
    assert verdicts[None] == set()


@pytest.mark.parametrize("defect", [d for d in DEFECTS if d != "fmax_clip"])
def test_each_planted_defect_is_caught(verdicts, defect):
    caught = verdicts[defect]
    assert caught, defect
    names = {n for n, _, _ in caught}
    by = {c.name: c for c in pc.cases()}
    if defect == "one_slot":  # only a tile that owns both slots can tell: the layout cases meant to have one do, no other does
        assert all(pc.both_slot_tiles(by[n].ptr) for n in names), names
        assert {"layout_two_large", "layout_long", "layout_long_wide"} <= names
        for kind in pc.KINDS:
            assert ("layout_two_large", kind, (None, None)) in caught
    if defect in ("no_rescale", "max_of_chunk0"):
        assert all(k == "softmax" for _, k, _ in caught)
        assert {"scores_chunk3", "scores_chunk100", "layout_long"} <= names
    if defect == "slots_swapped":
        assert {n for n in by if n.startswith("layout_") and max(by[n].sizes) > C} <= names
    if defect == "head_of_first_column":  # a float4 that spans two or four heads
        assert all(by[n].vec4 and (by[n].GD // by[n].heads) % 4 != 0 for n in names), names
        assert {"heads_12_4", "heads_12_6", "heads_12_2", "heads_12_12", "heads_4_4", "heads_64_64", "heads_96_96",
                "heads_128_128"} <= names  # heads of 3, 2, 6 and 1 features
    if defect == "strict_mask":
        assert names == {"ties"}
        assert {(k, b) for _, k, b in caught} == {(k, b) for k in pc.KINDS for b in by["ties"].bounds}


def test_fmax_clip_passes_every_finite_case(verdicts):
    """fmin(fmax(x, lo), hi) differs from the contract's clip at a NaN only: no finite case can tell, the plants below do"""
    assert verdicts["fmax_clip"] == set()


PLANT_IDS = [f"{what}_{'nan' if np.isnan(value) else 'inf'}" for what, value, _ in pc.PLANTS]


@pytest.mark.parametrize("where", list(pc.PLANT_SPOTS))
@pytest.mark.parametrize("bounds", pc.BOUNDS, ids=["nobounds", "clipped"])
@pytest.mark.parametrize("plant", pc.PLANTS, ids=PLANT_IDS)
def test_nonfinite_plants_on_the_restatement(plant, bounds, where):
    what, value, kinds = plant
    case = pc.NONFINITE_CASE
    _, _, dOut = pc.inputs(case)
    lo, hi = bounds
    for kind in kinds:
        def run(T, S, defect=None):
            return chunked_readout(case, kind, lo, hi, T, S, dOut, defect=defect)

        pc.check_planted(case, kind, lo, hi, what, value, where, run)
        wrong = _fails(lambda: pc.check_planted(case, kind, lo, hi, what, value, where, lambda T, S: run(T, S, "fmax_clip")))
        # the clip that swallows a NaN is caught by the NaN in T where a bound is finite: out[g, c] is then a finite number.
        # Without bounds fmax(NaN, -inf) = -inf, not finite either: the pattern alone cannot tell there.
        if what == "T" and np.isnan(value) and lo is not None:
            assert wrong, (kind, where)
