"""The chosen inputs of the graph-readout reference tests, and the one comparison both of them use.

tests/test_gpu_pool_reference.py feeds these inputs to tfgnn_pool_forward / tfgnn_pool_backward and compares with
tests/pool_reference.py through ``compare``; tests/test_pool_reference_host.py feeds the same inputs to a numpy restatement
of the chunked scheme with planted defects and requires ``compare`` to pass the clean restatement and to fail every defect.
Nothing here needs a device.  Inputs are float32 (the common starting point); the reference casts them up.

Bounds.  A finite result is held to |got - ref| <= 1e-5 * max(1, |ref|), the bound of tests/test_gpu_pool_entry.py for these
kernels at these sizes.  Two things were considered for more:
  * scores offset by up to 1e4: none needed.  S and the graph's maximum m are fp32 numbers within a factor of two of each
    other, so S - m is exact in fp32 (Sterbenz), and the reference starts from the same fp32 S.
  * long sums.  An n-term fp32 sum of O(1) terms added one after the other collects about n roundings of partial sums of
    size sqrt(k): an error of roughly 2.5e-8 * n, a third of 1e-5 at n = 130 and all of it at n = 400.  The widest sum the
    1e-5 of test_gpu_pool_entry.py has covered is 64 terms.  Cases flagged ``long_sums`` (GD > 256: a head of more than 128
    features, and, per the header's mapping, one lane per column, which then adds a chunk's 128 nodes one after the other)
    therefore add, for out and dS, sqrt(n) roundings of the sum: sqrt(n) * 2^-24 * (sum of |terms|), each rounding being
    at most 2^-24 of a partial sum and a partial sum at most the sum of the magnitudes.  w and dT are no sums over GD and
    keep the plain bound.  (For softmax dS = w * (dw - sum w dw) the allowance of dw carries over times w, and once more
    for the weighted sum: w * (excess(dw) + sum w excess(dw)).)  Measured afterwards, in units of the plain bound: dS of the
    sigmoid at 1024 columns 1.55 (0.87 at 260), out at most 0.88; the GPU test logs both figures for these cases.
Non-finite results are compared as a pattern: non-finite exactly where the reference is, to the element."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from tests import pool_reference as ref

C = 128  # TFGNN_POOL_CHUNK_NODES; the tests assert it against the library's constant
TOL = 1e-5
U = 2.0 ** -24
KINDS = ref.KINDS
WEIGHTED = ("softmax", "sigmoid")
TIE_BOUNDS = (-0.5, 0.75)
BOUNDS = [(None, None), TIE_BOUNDS]


@dataclass
class Case:
    name: str
    sizes: list
    GD: int
    heads: int
    kinds: tuple = KINDS
    bounds: list = field(default_factory=lambda: list(BOUNDS))
    col0: int = 4               # T and dT are columns [col0, col0 + GD) of a wider buffer; 1 = not 16-byte aligned
    scores: str = "randn"       # how S is drawn
    ties: bool = False          # T on a grid of eighths, many of them exactly on the bounds
    both_slots: Optional[bool] = None  # the layout must (True) / must not (False) have a tile that owns both workspace slots
    score_condition: bool = False      # every (graph, head) has >= 3 nodes of reference weight > 1e-3
    long_sums: bool = False

    @property
    def V(self):
        return int(sum(self.sizes))

    @property
    def G(self):
        return len(self.sizes)

    @property
    def ptr(self):
        return np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)

    @property
    def vec4(self):
        """whether the kernels may take their float4 path (rows of a multiple of four floats on 16-byte addresses)"""
        return self.GD % 4 == 0 and self.col0 % 4 == 0


LONG_LAYOUT = [C + 1, C + 1, 0, 2 * C, 0, 0, 2 * C + 1, 3, C, 0]
MIXED = [5, 0, C + 1, C + 1, 9]

LAYOUTS = [
    ("two_large", [C + 1, C + 1], True),
    ("long", LONG_LAYOUT, True),
    ("empty_around_large", [0, 0, C + 1, 0], False),
    ("large_on_tile_edge", [C, 2 * C + 1], False),
    ("large_ends_on_tile_edge", [5, 2 * C - 5], False),
    ("full_tile_then_empty", [C, 0, 0, 3], False),
    ("full_tiles_around_empty", [C, 0, C], False),
    ("one_node", [1], False),
    ("no_nodes", [0, 0, 0], False),
]
# heads that are no power of two, more than 64 of them, and heads of 1, 2, 3 and 6 features (a float4 across several heads)
HEADS = [(12, 3), (12, 6), (12, 2), (12, 12), (12, 4), (4, 4), (64, 64), (96, 96), (128, 128), (130, 65), (5, 5), (7, 1)]


def cases():
    out = []
    for name, sizes, both in LAYOUTS:
        out.append(Case(f"layout_{name}", sizes, 16, 4, both_slots=both))
    out.append(Case("layout_long_wide", LONG_LAYOUT, 128, 8, both_slots=True))
    for GD, heads in HEADS:
        out.append(Case(f"heads_{GD}_{heads}", MIXED, GD, heads, kinds=WEIGHTED, both_slots=True))
    for GD in (1, 3, 4, 68, 260, 1024):
        out.append(Case(f"width_{GD}", MIXED, GD, 1, long_sums=GD > 256))
    out.append(Case("width_1024_heads_256", MIXED, 1024, 256, long_sums=True))
    out.append(Case("width_128_unaligned", MIXED, 128, 8, col0=1))
    out.append(Case("width_65_unaligned", MIXED, 65, 5, col0=1))
    for s in ("const", "const_cycle", "chunk3"):
        out.append(Case(f"scores_{s}", LONG_LAYOUT, 16, 4, kinds=("softmax",), scores=s, score_condition=True, both_slots=True))
    # a graph of C + 1 nodes has ONE node in its +100 chunk, which then holds all the weight: no score condition here
    out.append(Case("scores_chunk100", LONG_LAYOUT, 16, 4, kinds=("softmax",), scores="chunk100", both_slots=True))
    out.append(Case("ties", MIXED, 16, 4, ties=True, bounds=[TIE_BOUNDS, (TIE_BOUNDS[0], None), (None, TIE_BOUNDS[1])]))
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


def chunk_index(case):
    """per node: the index of its chunk of C nodes inside its graph"""
    ptr = case.ptr
    k = np.zeros(case.V, dtype=np.int64)
    for g in range(case.G):
        a, b = int(ptr[g]), int(ptr[g + 1])
        k[a:b] = (np.arange(a, b) - a) // C
    return k


def node_graph(case):
    return np.repeat(np.arange(case.G), case.sizes)


_INPUTS = {}


def inputs(case):
    """-> (T [V, GD], S [V, heads] raw scores, dOut [G, GD]) float32, a pure function of the case's name; do not modify"""
    if case.name in _INPUTS:
        return _INPUTS[case.name]
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    V, G, GD, heads = case.V, case.G, case.GD, case.heads
    T = rng.standard_normal((V, GD))
    if case.ties:
        T = np.round(4.0 * T) / 8.0
    S = rng.standard_normal((V, heads))
    g_of = node_graph(case)
    if case.scores == "const":
        off = rng.choice([-1e4, -90.0, 0.0, 90.0, 1e4], size=(G, heads))
        S = S + off[g_of]
    elif case.scores == "const_cycle":  # every value turns up in every graph or its neighbour
        vals = np.array([-1e4, -90.0, 0.0, 90.0, 1e4])
        off = vals[(np.arange(G)[:, None] + np.arange(heads)[None, :]) % 5]
        S = S + off[g_of]
    elif case.scores in ("chunk3", "chunk100"):
        a = 3.0 if case.scores == "chunk3" else 100.0
        S = S + np.array([0.0, a, -a])[chunk_index(case) % 3][:, None]
    else:
        assert case.scores == "randn", case.scores
    dOut = rng.standard_normal((G, GD))
    res = tuple(np.ascontiguousarray(x, dtype=np.float32) for x in (T, S, dOut))
    for x in res:
        x.setflags(write=False)
    _INPUTS[case.name] = res
    return res


def scores_for(kind, S):
    """what the kernels get as S: the raw scores (softmax), sigmoid weights in fp32 (sigmoid), nothing otherwise"""
    if kind == "softmax":
        return S
    if kind == "sigmoid":
        return (1.0 / (1.0 + np.exp(-S.astype(np.float64)))).astype(np.float32)
    return None


def slot_owners(ptr, chunk=C):
    """{tile: set of workspace slots in use}, from the header's description alone: a graph of more than ``chunk`` nodes is cut
    into chunks from its first node on; a chunk belongs to the tile its first node lies in; slot 1 for a graph's first chunk,
    slot 0 for a later one"""
    owners = {}
    for g in range(len(ptr) - 1):
        a, b = int(ptr[g]), int(ptr[g + 1])
        if b - a <= chunk:
            continue
        for k, s in enumerate(range(a, b, chunk)):
            slot = 1 if k == 0 else 0
            tile = s // chunk
            assert slot not in owners.setdefault(tile, set()), "two chunks in one slot: the header's 'at most one' is wrong"
            owners[tile].add(slot)
    return owners


def both_slot_tiles(ptr, chunk=C):
    return sorted(t for t, s in slot_owners(ptr, chunk).items() if s == {0, 1})


_REFERENCE = {}


def reference(case, kind, lo, hi, T=None, S=None):
    """-> dict(out, w, dT, dS) in float64 from tests/pool_reference.py (w: the weights of every kind; dS None without scores).
    ``T`` / ``S`` (what the kernels get: ``scores_for`` applied) replace the case's own inputs and are not remembered."""
    key = (case.name, kind, lo, hi)
    own = T is None and S is None
    if own and key in _REFERENCE:
        return _REFERENCE[key]
    T0, S0, dOut = inputs(case)
    T = T0 if T is None else T
    S = scores_for(kind, S0) if S is None else S
    out, w = ref.forward(kind, case.ptr, T, S, case.heads, lo, hi)
    dT, dS = ref.backward(kind, case.ptr, dOut, T, w if kind == "softmax" else S, case.heads, lo, hi)
    res = {"out": out, "w": w, "dT": dT, "dS": dS}
    if own:
        _REFERENCE[key] = res
    return res


def assert_conditions(case, kind, lo, hi):
    """What keeps a case from being vacuous, on the inputs and the reference alone."""
    T, S, dOut = inputs(case)
    if case.both_slots is not None:
        tiles = both_slot_tiles(case.ptr)
        assert bool(tiles) == case.both_slots, (case.name, tiles)
    if case.ties:
        for bound, on, beyond in ((lo, T == lo, T < (lo if lo is not None else 0)), (hi, T == hi, T > (hi if hi is not None else 0))):
            if bound is not None:
                assert on.mean() >= 0.02 and beyond.mean() >= 0.02, (case.name, bound, on.mean(), beyond.mean())
    if case.score_condition and kind == "softmax":
        w = reference(case, kind, lo, hi)["w"]
        ptr = case.ptr
        for g in range(case.G):
            if ptr[g + 1] > ptr[g]:
                n = (w[ptr[g]:ptr[g + 1]] > 1e-3).sum(axis=0)
                assert n.min() >= 3, (case.name, g, n)


def excess(case, kind, lo, hi, r, T=None, S=None):
    """The allowance of a ``long_sums`` case on top of 1e-5 * max(1, |ref|) (module docstring) -> {"out": [G, GD], "dS": [V, heads]}"""
    T0, S0, dOut = inputs(case)
    T = T0 if T is None else T
    ph = case.GD // case.heads
    ptr = case.ptr
    R = np.abs(ref.clip(T, lo, hi))
    wf = np.abs(np.repeat(r["w"], ph, axis=1))
    ex_out = np.zeros((case.G, case.GD))
    ex_dw = np.zeros((case.V, case.heads))
    for g in range(case.G):
        a, b = int(ptr[g]), int(ptr[g + 1])
        if b > a:
            ex_out[g] = np.sqrt(b - a) * U * np.sum(wf[a:b] * R[a:b], axis=0)
            ex_dw[a:b] = np.sqrt(ph) * U * np.sum((R[a:b] * np.abs(dOut[g].astype(np.float64))).reshape(b - a, case.heads, ph), axis=2)
    ex_dS = ex_dw
    if kind == "softmax":
        w = np.abs(r["w"])
        ex_dS = np.zeros_like(ex_dw)
        for g in range(case.G):
            a, b = int(ptr[g]), int(ptr[g + 1])
            ex_dS[a:b] = w[a:b] * (ex_dw[a:b] + np.sum(w[a:b] * ex_dw[a:b], axis=0))
    return {"out": ex_out, "dS": ex_dS}


def compare(case, kind, lo, hi, got, r=None, skip_dT=None, T=None, S=None):
    """THE comparison: ``got`` = dict(out, w, dT, dS) of arrays (w None unless softmax, dS None without scores) against the
    float64 reference ``r`` (default: of the case's own inputs).  Non-finite exactly where the reference is; finite values
    within 1e-5 * max(1, |ref|) (+ the allowance of a long_sums case).  ``skip_dT``: (node, column) left out of dT.
    -> {name: worst error / bound}; raises AssertionError naming the first quantity that misses."""
    if r is None:
        r = reference(case, kind, lo, hi, T=T, S=S)
    extra = excess(case, kind, lo, hi, r, T=T, S=S) if case.long_sums else {}
    worst = {}
    for name in ("out", "w", "dT", "dS"):
        g, e = got.get(name), r[name]
        if name == "w" and kind != "softmax":
            continue  # not an output of the other kinds
        if e is None:
            assert g is None, f"{case.name} {kind} {name}: not expected"
            continue
        assert g is not None and g.shape == e.shape, f"{case.name} {kind} {name}: shape {None if g is None else g.shape} vs {e.shape}"
        g = np.asarray(g, dtype=np.float64)
        keep = np.ones(e.shape, dtype=bool)
        if name == "dT" and skip_dT is not None:
            keep[skip_dT] = False
        fin_g, fin_e = np.isfinite(g), np.isfinite(e)
        assert np.array_equal(fin_g[keep], fin_e[keep]), (
            f"{case.name} {kind} {name}: non-finite in {int((~fin_g & keep).sum())} places, the reference in {int((~fin_e & keep).sum())}; "
            f"first difference at {tuple(np.argwhere((fin_g != fin_e) & keep)[0])}")
        both = fin_g & fin_e & keep
        if not both.any():
            worst[name] = 0.0
            continue
        bound = TOL * np.maximum(1.0, np.abs(np.where(fin_e, e, 0.0))) + extra.get(name, 0.0)
        with np.errstate(invalid="ignore"):
            ratio = np.where(both, np.abs(g - e) / bound, 0.0)
        worst[name] = float(ratio.max())
        if name in extra:  # a figure for the log: the same error in units of the plain bound
            with np.errstate(invalid="ignore"):
                plain = np.where(both, np.abs(g - e) / (TOL * np.maximum(1.0, np.abs(np.where(fin_e, e, 0.0)))), 0.0)
            worst[name + " (in units of the plain 1e-5)"] = float(plain.max())
        at = np.unravel_index(int(ratio.argmax()), ratio.shape)
        assert worst[name] <= 1.0, f"{case.name} {kind} ({lo}, {hi}) {name}: error / bound {worst[name]:.3g} at {at}: {g[at]!r} vs {e[at]!r}"
    return worst


# ---- non-finite plants ---------------------------------------------------------------------------------------------------
NONFINITE_CASE = Case("nonfinite", MIXED, 16, 4)
# (what, value, kinds); each with BOUNDS and in a chunked and an unchunked graph
PLANTS = [("T", np.nan, KINDS), ("T", np.inf, KINDS), ("S", np.nan, WEIGHTED), ("S", np.inf, WEIGHTED)]
PLANT_SPOTS = {"chunked": (3, 7), "unchunked": (4, 2)}  # (graph of MIXED, node inside it); graph 3 shares a tile with graph 2's tail
PLANT_COLUMN = {"T": 6, "S": 1}  # feature 6 lies in head 1


def check_planted(case, kind, lo, hi, what, value, where, run):
    """One pair of runs, clean and planted, through ``run(T, S) -> dict(out, w, dT, dS)`` of float32 arrays (S as the kernels
    get it).  In the planted graph: non-finite exactly where the reference of the planted inputs is, finite values within the
    bound.  Everywhere else: bit-equal to the clean run.  -> compare's result"""
    T0, S0, dOut = inputs(case)
    Tp, Sp, v, c, g = planted(case, kind, what, value, where)
    clean = run(T0.copy(), scores_for(kind, S0))
    dirty = run(Tp, Sp)
    a, b = int(case.ptr[g]), int(case.ptr[g + 1])
    r = reference(case, kind, lo, hi, T=Tp, S=Sp)
    # the plant is not vacuous, and stays inside its graph, in the reference already
    clipped_away = what == "T" and np.isposinf(value) and hi is not None
    bad_out = ~np.isfinite(r["out"])
    if clipped_away:
        assert not bad_out.any() and all(np.isfinite(x).all() for x in r.values() if x is not None)  # +inf clips to hi
    else:
        assert bad_out[g].any() and not np.delete(bad_out, g, axis=0).any(), (case.name, kind, what, value, where)
    for name, rows in (("out", slice(g, g + 1)), ("w", slice(a, b)), ("dT", slice(a, b)), ("dS", slice(a, b))):
        x, y = clean.get(name), dirty.get(name)
        if x is None or y is None:
            assert x is None and y is None, name
            continue
        assert x.dtype == np.float32 and y.dtype == np.float32
        same = np.delete(x, rows, axis=0).view(np.uint32) == np.delete(y, rows, axis=0).view(np.uint32)
        assert same.all(), f"{case.name} {kind} {what}={value} {where}: {name} changed outside the planted graph in {int((~same).sum())} places"
    # dT AT a planted NaN is not compared: without bounds the contract has no mask (w * dOut there) while the kernels always
    # evaluate lo <= T <= hi (0 there); what consumes dT multiplies it by the activation's derivative at that NaN next
    skip = (v, c) if what == "T" and np.isnan(value) else None
    return compare(case, kind, lo, hi, dirty, r=r, skip_dT=skip, T=Tp, S=Sp)


def planted(case, kind, what, value, where):
    """-> (T, S as the kernels get them, node, column, graph) with one element replaced"""
    T, S, dOut = inputs(case)
    T, S = T.copy(), scores_for(kind, S)
    g, local = PLANT_SPOTS[where]
    v = int(case.ptr[g]) + local
    c = PLANT_COLUMN[what]
    if what == "T":
        T[v, c] = value
    else:
        S = S.copy()
        S[v, c] = value
    return T, S, v, c, g
