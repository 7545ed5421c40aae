"""The dropout mask generator of include/tfgnn.h ("The dropout mask generator", at tfgnn_dropout_forward) in numpy and plain
Python integers, written from that text: key words, threshold, epoch step, one hash word per aligned group of four elements,
one byte-rotated 24-bit number per element.  Integers only; float32 for the scale alone.  Independent of the library: the GPU
tests compare every kernel that draws a mask against it bit for bit, tests/test_dropout_reference_host.py pins it on the host."""
from fractions import Fraction
from typing import NamedTuple

import numpy as np

from tests.neighbor_sample_reference import M32, M64, lowbias32, lowbias32_many, seed_words

GOLDEN = 0x9E3779B9
EPOCH_S0_ADD = 0x7F4A7C15
EPOCH_S1_MUL = 0x85EBCA6B
RESERVED_SEED = M64  # at the NT product entries: the mask-from-saved form; the flat entries take it as a seed


class Key(NamedTuple):
    s0: int
    s1: int
    threshold: int  # an element is kept iff its 24-bit number is >= threshold
    scale: np.float32  # the value of a kept mask element


def threshold(rate) -> int:
    """ceil(rate * 2^24) of the FLOAT32 rate, in exact rational arithmetic"""
    t = Fraction(float(np.float32(rate))) * (1 << 24)
    return -((-t.numerator) // t.denominator)


def scale(rate) -> np.float32:
    """1 / (1 - rate), both operations in float32"""
    one = np.float32(1.0)
    with np.errstate(divide="ignore"):
        return np.float32(one / np.float32(one - np.float32(rate)))


def key(seed: int, rate, epoch: int = 0) -> Key:
    s0, s1 = seed_words(int(seed) & M64)
    e = int(epoch) & M32
    if e:
        s0 ^= lowbias32((e * GOLDEN + EPOCH_S0_ADD) & M32)
        s1 = (s1 + e * EPOCH_S1_MUL) & M32
    return Key(s0, s1, threshold(rate), scale(rate))


def group_words(k: Key, first_group: int, count: int) -> np.ndarray:
    """uint32 [count]: the hash word of groups first_group .. first_group + count - 1 (group = element index / 4)"""
    group = np.uint64(first_group) + np.arange(count, dtype=np.uint64)
    hi = group >> np.uint64(32)
    s = np.full(count, k.s0, dtype=np.uint64)
    far = hi != 0  # tensors of more than 2^34 elements
    if far.any():
        s[far] ^= lowbias32_many(hi[far] * np.uint64(GOLDEN) + np.uint64(1))
    return (lowbias32_many((group & np.uint64(M32)) ^ s) ^ np.uint64(k.s1)).astype(np.uint32)


def lane_numbers(words: np.ndarray) -> np.ndarray:
    """uint32 [len(words), 4]: element e of a group takes the top 24 bits of the word rotated LEFT by 8 e bits"""
    w = np.asarray(words, dtype=np.uint32)
    out = np.empty((w.shape[0], 4), dtype=np.uint32)
    out[:, 0] = w >> np.uint32(8)
    for e in (1, 2, 3):
        out[:, e] = ((w << np.uint32(8 * e)) | (w >> np.uint32(32 - 8 * e))) >> np.uint32(8)
    return out


def keep(seed: int, rate, epoch: int, start: int, n: int) -> np.ndarray:
    """bool [n]: are the elements of flat index start .. start + n - 1 kept?  (index = row * cols + column of the logical
    tensor)"""
    if n <= 0:
        return np.zeros(0, dtype=bool)
    k = key(seed, rate, epoch)
    first = start >> 2
    count = ((start + n + 3) >> 2) - first
    kept = lane_numbers(group_words(k, first, count)) >= np.uint32(k.threshold)
    off = start - 4 * first
    return kept.reshape(-1)[off:off + n]


def mask(shape, rate, seed: int, epoch: int = 0) -> np.ndarray:
    """float32 [shape]: 0 where dropped, the float32 scale where kept"""
    shape = tuple(int(d) for d in (shape if hasattr(shape, "__len__") else (shape,)))
    n = int(np.prod(shape, dtype=np.int64)) if shape else 1
    k = key(seed, rate, 0)
    return np.where(keep(seed, rate, epoch, 0, n), k.scale, np.float32(0.0)).astype(np.float32).reshape(shape)
