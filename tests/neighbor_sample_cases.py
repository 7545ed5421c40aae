"""Small graphs for the neighbour sampling tests, built from a seed: the host tests and the GPU tests use the same ones."""
import numpy as np

from tests.neighbor_sample_reference import build_in_csr

SPECIAL_DEGREES = (4, 5, 16, 17, 64, 65, 256, 257)  # nodes 0..7: across the Feistel widths and the wave boundaries
HUB, HUB_DEGREE = 8, 300
ISOLATED = 9  # in-degree 0 in every type
# seeds in this order: the hub, the special rows, the isolated node, then the others; 7 and 8 are each other's neighbours
SEED_ORDER = [HUB, 7, 6, 5, 4, 3, 2, 1, 0, ISOLATED] + list(range(10, 200))


def device_test_graph(V=200, seed=0):
    """-> (edge lists [E_t, 2] of 3 processed types, the third empty; in_ptr, in_src per type).  Type 0: nodes 0..7 with the
    SPECIAL_DEGREES, the hub with 300 in-edges - more than V, so sources repeat: duplicate edges -, node 9 with none,
    nodes 10..17 with in-degrees 2, 3, 4 (f and f + 1 for the fanouts 2 and 3) and 5, 6 (for 5), the rest 0..6; the list is
    shuffled, so the in-CSR's stable sort matters.  Type 1: 700 random edges, none into node 9, plus 7 -> 8 and 8 -> 7."""
    rng = np.random.default_rng(seed)
    degree = rng.integers(0, 7, size=V)
    degree[:8] = SPECIAL_DEGREES
    degree[HUB] = HUB_DEGREE
    degree[ISOLATED] = 0
    degree[10:18] = [2, 3, 4, 2, 3, 4, 5, 6]
    targets = np.repeat(np.arange(V), degree)
    e0 = np.stack([rng.integers(0, V, size=targets.shape[0]), targets], axis=1)
    e0 = e0[rng.permutation(e0.shape[0])]
    e1 = rng.integers(0, V, size=(700, 2))
    e1 = e1[e1[:, 1] != ISOLATED]
    e1 = np.concatenate([e1, [[7, 8], [8, 7]], e1[:5]])  # and five exact duplicates
    edges = [e0.astype(np.int32), e1.astype(np.int32), np.zeros((0, 2), dtype=np.int32)]
    csr = [build_in_csr(e, V) for e in edges]
    return edges, [c[0] for c in csr], [c[1] for c in csr]


def exact_hop_graph(V=300, seed=1):
    """V = 300, three processed types: self loops, random edges with a 400-edge hub (node 5), an empty type."""
    rng = np.random.default_rng(seed)
    loops = np.stack([np.arange(V), np.arange(V)], axis=1)
    rand = rng.integers(0, V, size=(900, 2))
    hub = np.stack([rng.integers(0, V, size=400), np.full(400, 5)], axis=1)
    e1 = np.concatenate([rand, hub])
    e1 = e1[rng.permutation(e1.shape[0])]
    return [loops.astype(np.int32), e1.astype(np.int32), np.zeros((0, 2), dtype=np.int32)]
