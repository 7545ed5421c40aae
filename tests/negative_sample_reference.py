"""The negatives of tfgnn_triples_draw_negatives (include/tfgnn.h "Negative sampling and triple tables on the device") in numpy,
written from that text on top of tests/dropout_reference.py: negative j copies positive j / K, takes the generator's words 2 j
and 2 j + 1 of (seed, epoch), the top bit of the first as its coin and the multiply-high of the second as its node.  Integers
only.  Independent of the library: the GPU tests compare the kernel against it bit for bit,
tests/test_negative_sample_reference_host.py pins it on the host."""
import numpy as np

from tests import dropout_reference as dref


def words(seed: int, epoch: int, count: int, use_epoch: bool = True) -> np.ndarray:
    """uint32 [count]: word(0) .. word(count - 1) of (seed, epoch); use_epoch False: the key of epoch 0"""
    return dref.group_words(dref.key(seed, 0.0, epoch if use_epoch else 0), 0, count)


def draw(positives, K: int, V: int, seed: int, epoch: int = 0, use_epoch: bool = True) -> np.ndarray:
    """int32 [P K, 3]: the negatives of ``positives`` [P, 3] in np.repeat order"""
    pos = np.asarray(positives, dtype=np.int64).reshape(-1, 3)
    if K > 0 and V < 2:
        raise ValueError("a negative needs a second node")
    neg = np.repeat(pos, K, axis=0)
    n = neg.shape[0]
    if n == 0:
        return neg.astype(np.int32)
    w = words(seed, epoch, 2 * n, use_epoch).astype(np.uint64)
    a, b = w[0::2], w[1::2]
    slot = np.where((a >> np.uint64(31)) != 0, 2, 0)
    d = ((b * np.uint64(V - 1)) >> np.uint64(32)).astype(np.int64)
    rows = np.arange(n)
    old = neg[rows, slot]
    neg[rows, slot] = d + (d >= old)
    return neg.astype(np.int32)


def triples(positives, K: int, V: int, seed: int, epoch: int = 0, use_epoch: bool = True) -> np.ndarray:
    """int32 [P (1 + K), 3]: the positives followed by their negatives - the whole buffer after a draw"""
    pos = np.asarray(positives, dtype=np.int32).reshape(-1, 3)
    return np.concatenate([pos, draw(pos, K, V, seed, epoch, use_epoch)])


def sampler_seed(negative_sampling_seed: int, draws: int) -> int:
    """the 64-bit seed of a DeviceTripleSampler's draw number ``draws`` (counted from 0)"""
    return ((int(negative_sampling_seed) << 32) | (int(draws) & 0xFFFFFFFF)) & dref.M64
