"""The neighbour sampling contract of include/tfgnn.h ("Neighbour sampling") in numpy and plain loops, literally: the
in-CSR, the keyed positions (splitmix64 step, lowbias32, 8-round balanced Feistel network, cycle walk, rotation) and the
K-hop subgraph in its fixed order.  Independent of the library: tests compare the device sampler against it exactly."""
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
GOLDEN = 0x9E3779B9


def lowbias32(x: int) -> int:
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def seed_words(seed: int) -> Tuple[int, int]:
    """(s0, s1): the low and the high word of one splitmix64 step of the call's 64-bit seed"""
    z = (seed + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z & M32, z >> 32


def row_key(s0: int, s1: int, v: int, t: int) -> int:
    return lowbias32(lowbias32(v ^ s0) + (t + 1) * GOLDEN) ^ s1


def feistel_bits(d: int) -> int:
    b = max(2, (d - 1).bit_length())
    return b + (b & 1)


def permute(k: int, d: int, j: int) -> int:
    """pi(j): the Feistel network on feistel_bits(d) bits, walked until the value is below d"""
    half = feistel_bits(d) // 2
    mask = (1 << half) - 1
    x = j
    while True:
        l, r = x >> half, x & mask
        for i in range(8):
            f = (lowbias32(r ^ ((k + i * GOLDEN) & M32)) >> 7) & mask
            l, r = r, l ^ f
        x = (l << half) | r
        if x < d:
            return x


def positions(k: int, d: int, c: int) -> List[int]:
    """the c positions of a row of in-degree d under row key k"""
    if c == d:
        return list(range(d))
    off = lowbias32(k ^ 0xA5A5A5A5) % d
    return [(permute(k, d, j) + off) % d for j in range(c)]


def lowbias32_many(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint64) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def positions_many(keys: np.ndarray, d: int, c: int) -> np.ndarray:
    """``positions`` for many row keys at once, c < d: int64 [len(keys), c] (the same arithmetic on arrays; the tests hold
    it against the scalar form)"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 1)
    half = np.uint64(feistel_bits(d) // 2)
    mask = np.uint64((1 << int(half)) - 1)
    k = np.broadcast_to(keys, (keys.shape[0], c))
    x = np.broadcast_to(np.arange(c, dtype=np.uint64), k.shape).copy()
    todo = np.ones(k.shape, dtype=bool)
    while todo.any():
        l, r, kk = x[todo] >> half, x[todo] & mask, k[todo]
        for i in range(8):
            f = (lowbias32_many(r ^ ((kk + np.uint64(i * GOLDEN)) & np.uint64(M32))) >> np.uint64(7)) & mask
            l, r = r, l ^ f
        x[todo] = (l << half) | r
        todo &= x >= d
    off = lowbias32_many(keys ^ np.uint64(0xA5A5A5A5)) % np.uint64(d)
    return ((x + off) % np.uint64(d)).astype(np.int64)


def taken(d: int, f: int) -> int:
    return d if f < 0 or d <= f else f


def build_in_csr(edges: np.ndarray, num_nodes: int) -> Tuple[np.ndarray, np.ndarray]:
    """(in_ptr int32 [V + 1], in_src int32 [E]) of one edge list [E, 2] of (source, target): stable sort by target"""
    edges = np.asarray(edges).reshape(-1, 2)
    order = np.argsort(edges[:, 1], kind="stable")
    in_ptr = np.zeros(num_nodes + 1, dtype=np.int64)
    np.cumsum(np.bincount(edges[:, 1], minlength=num_nodes), out=in_ptr[1:])
    return in_ptr.astype(np.int32), edges[order, 0].astype(np.int32)


class Sample(NamedTuple):
    nodes: np.ndarray  # int32 [n], global ids
    hop_ptr: np.ndarray  # int32 [K + 2]
    adjacency_lists: List[np.ndarray]  # int32 [E_t, 2], local ids
    status: int  # bit 4: a repeated seed (the only one the reference knows)
    drawn: dict  # (v, t) -> the global sources drawn for that row, in order


def neighbor_sample(in_ptr: Sequence[np.ndarray], in_src: Sequence[np.ndarray], seeds, fanouts: Sequence[int], seed: int) -> Sample:
    L, K = len(in_ptr), len(fanouts)
    s0, s1 = seed_words(seed)
    nodes = [int(v) for v in seeds]
    status = 4 if len(set(nodes)) != len(nodes) else 0
    local = {v: i for i, v in enumerate(nodes)}
    hop_ptr = [0, len(nodes)]
    edges: List[List[Tuple[int, int]]] = [[] for _ in range(L)]  # (global source, local target)
    drawn = {}
    for h in range(1, K + 1):
        f = int(fanouts[h - 1])
        frontier = nodes[hop_ptr[h - 1]:hop_ptr[h]]
        found = set()
        for t in range(L):  # a type's edges of this hop follow its edges of earlier hops, frontier order within
            for v in frontier:
                first = int(in_ptr[t][v])
                d = int(in_ptr[t][v + 1]) - first
                c = taken(d, f)
                srcs = [int(in_src[t][first + p]) for p in positions(row_key(s0, s1, v, t), d, c)] if c else []
                drawn[(v, t)] = srcs
                for s in srcs:
                    edges[t].append((s, local[v]))
                    if s not in local:
                        found.add(s)
        for s in sorted(found):
            local[s] = len(nodes)
            nodes.append(s)
        hop_ptr.append(len(nodes))
    adjacency = [np.array([(local[s], tgt) for s, tgt in e], dtype=np.int32).reshape(-1, 2) for e in edges]
    return Sample(np.array(nodes, dtype=np.int32), np.array(hop_ptr, dtype=np.int32), adjacency, status, drawn)
