"""tests/negative_sample_reference.py pinned on the host - the properties include/tfgnn.h states for
tfgnn_triples_draw_negatives - and, as far as they go without a device, the new entries: header, symbols and binding, the
argument refusals of the draw and of the table build (all before any launch), the ops wrappers' refusals and the dataset's
``negative_sampling`` hyper-parameter.  CPU-only; the kernels are compared with the reference on the GPU
(tests/test_gpu_negative_sampling.py)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import negative_sample_reference as nref
from tf2_gnn_amd.data import DataFold, LinkPredictionDataset

ROOT = Path(__file__).resolve().parent.parent
NEW = ["tfgnn_triples_draw_negatives", "tfgnn_triple_tables_workspace_bytes", "tfgnn_triple_tables_build",
       "tfgnn_negatives_launch_counts"]


def _positives(P, V, T, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.randint(0, V, P), rng.randint(0, T, P), rng.randint(0, V, P)], axis=1).astype(np.int32)


# ---- the reference --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,K,V", [(1, 1, 2), (257, 3, 50), (513, 2, 3001), (64, 2, 2 ** 31 - 1), (40, 5, 3)])
def test_exactly_one_slot_differs_in_repeat_order(P, K, V):
    pos = _positives(P, V, 7, P)
    pos[0] = (0, 0, 0)  # a self triple
    pos[-1] = (V - 1, 6, V - 1)
    neg = nref.draw(pos, K, V, seed=3, epoch=2)
    of = np.repeat(pos, K, axis=0)  # negative j copies positive j / K
    assert neg.dtype == np.int32 and neg.shape == (P * K, 3)
    assert np.array_equal(neg[:, 1], of[:, 1])  # the relation stays
    changed = neg != of
    assert np.all(changed[:, 0] != changed[:, 2])  # exactly one end replaced, by ANOTHER node: the other slot is kept
    assert neg.min() >= 0 and neg[:, [0, 2]].astype(np.int64).max() < V
    full = nref.triples(pos, K, V, seed=3, epoch=2)
    assert np.array_equal(full[:P], pos) and np.array_equal(full[P:], neg)


def test_no_negatives_and_too_few_nodes():
    pos = _positives(10, 7, 2, 0)
    assert nref.draw(pos, 0, 7, seed=1).shape == (0, 3)
    assert nref.draw(pos, 0, 1, seed=1).shape == (0, 3)  # K = 0 needs no second node
    with pytest.raises(ValueError, match="second node"):
        nref.draw(np.zeros((3, 3), dtype=np.int32), 1, 1, seed=1)


def test_two_nodes_always_yield_the_other_node():
    pos = _positives(300, 2, 3, 4)
    neg = nref.draw(pos, 3, 2, seed=9, epoch=1)
    of = np.repeat(pos, 3, axis=0)
    changed = neg != of
    assert np.all(changed[:, 0] != changed[:, 2])
    assert np.all(neg[changed] == 1 - of[changed])
    assert 0 < changed[:, 0].sum() < len(neg)  # both slots occur


def test_words_by_hand():
    """the definition, in plain Python integers, for one negative: word(2 j), word(2 j + 1) of the header's generator"""
    from tests import dropout_reference as dref

    seed, epoch, V, j = 0x1234_5678_9ABC_DEF0, 7, 1000, 5
    pos = _positives(4, V, 3, 1)
    k = dref.key(seed, 0.0, epoch)
    a = dref.lowbias32(((2 * j) ^ k.s0) & dref.M32) ^ k.s1
    b = dref.lowbias32(((2 * j + 1) ^ k.s0) & dref.M32) ^ k.s1
    u, t, v = (int(x) for x in pos[j // 2])
    d = (b * (V - 1)) >> 32
    want = (u, t, d + (d >= v)) if a >> 31 else (d + (d >= u), t, v)
    assert tuple(int(x) for x in nref.draw(pos, 2, V, seed, epoch)[j]) == want


def test_seed_epoch_and_use_epoch():
    pos = _positives(200, 90, 4, 2)
    base = nref.draw(pos, 2, 90, seed=5, epoch=3)
    assert np.array_equal(base, nref.draw(pos, 2, 90, seed=5, epoch=3))  # deterministic
    assert not np.array_equal(base, nref.draw(pos, 2, 90, seed=6, epoch=3))
    assert not np.array_equal(base, nref.draw(pos, 2, 90, seed=5, epoch=4))
    fixed = nref.draw(pos, 2, 90, seed=5, epoch=3, use_epoch=False)
    assert np.array_equal(fixed, nref.draw(pos, 2, 90, seed=5, epoch=0))  # the key of epoch 0 ...
    assert np.array_equal(fixed, nref.draw(pos, 2, 90, seed=5, epoch=11, use_epoch=False))  # ... whatever the epoch
    assert not np.array_equal(fixed, base)
    # the sampler's seed: the hyper-parameter in the high word, the host counter in the low one
    assert nref.sampler_seed(0, 0) == 0 and nref.sampler_seed(3, 2) == (3 << 32) | 2
    assert nref.sampler_seed(1, 2 ** 32 + 5) == (1 << 32) | 5
    assert len({nref.sampler_seed(s, c) for s in range(3) for c in range(4)}) == 12


def test_uniformity_at_a_fixed_seed():
    """V = 5, P = 10 000, K = 4: 40 000 negatives.  The drawn node's rank among the four OTHER nodes is uniform - each within 5
    standard deviations, sqrt(3 / 16 / 40000) = 0.002165, of 1 / 4 - and the coin within 5 of sqrt(1 / 4 / 40000) = 0.0025 of
    1 / 2.  Seed 0, epoch 0, observed on the host: the four frequencies deviate by -0.20, -1.56, +0.14 and +1.62 standard
    deviations, the coin by +0.35."""
    V, P, K = 5, 10_000, 4
    pos = _positives(P, V, 3, 123)
    neg = nref.draw(pos, K, V, seed=0)
    of = np.repeat(pos, K, axis=0)
    n = P * K
    target = neg[:, 2] != of[:, 2]
    new = np.where(target, neg[:, 2], neg[:, 0]).astype(np.int64)
    old = np.where(target, of[:, 2], of[:, 0]).astype(np.int64)
    rank = new - (new > old)  # position among the other V - 1 nodes
    assert rank.min() == 0 and rank.max() == V - 2
    sd = (0.25 * 0.75 / n) ** 0.5
    dev = [(float((rank == r).mean()) - 0.25) / sd for r in range(4)]
    coin = (float(target.mean()) - 0.5) / (0.25 / n) ** 0.5
    print("uniformity: node deviations", ["%+.2f" % d for d in dev], "coin %+.2f" % coin)
    assert max(abs(d) for d in dev) <= 5.0 and abs(coin) <= 5.0
    # every actual node is reached from every old node
    assert len(set(zip(old.tolist(), new.tolist()))) == V * (V - 1)


# ---- entry points -----------------------------------------------------------------------------------------------------------
def _counts(lib):
    buf = (ctypes.c_int64 * 3)()
    assert lib.tfgnn_negatives_launch_counts(buf, 3) == 0
    assert buf[2] == 0
    return list(buf)[:2]


def test_header_symbols_and_binding_agree():
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tfgnn.h").read_text(), flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    # new symbols, no signature changed
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in header
    assert lib.tfgnn_negatives_launch_counts(None, 1) == -1
    # two key and two payload arrays of 2 N words + the [512][tiles] histogram table, each rounded to 256 bytes
    r256 = lambda b: (b + 255) // 256 * 256
    for N in (1, 4096, 4097, 100_000):
        tiles = -(-2 * N // _lib.TRIPLE_SORT_TILE)
        assert lib.tfgnn_triple_tables_workspace_bytes(N, 5, 2) == r256(512 * ((tiles + 3) // 4 * 4) * 4) + 4 * r256(8 * N)
    assert lib.tfgnn_triple_tables_workspace_bytes(0, 5, 2) == 0 and lib.tfgnn_triple_tables_workspace_bytes(2 ** 30 + 1, 5, 2) == 0
    assert _lib.TRIPLE_SORT_TILE == 8192 and _lib.TRIPLE_SORT_DIGIT_BITS == 9
    # passes(X) = max(1, ceil(ceil(log2 X) / 9))
    assert [ops.triple_table_passes(x) for x in (1, 2, 512, 513, 2 ** 18, 2 ** 18 + 1, 2 ** 27, 2 ** 27 + 1, 2 ** 31 - 1)] == \
        [1, 1, 1, 2, 2, 3, 3, 4, 4]


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    before = _counts(lib)
    P_ = lambda a: ctypes.c_void_p(a)  # never dereferenced: every call below is refused before a launch
    tr, t0, t1, t2, t3, ws = (P_(0x1000 * (i + 1)) for i in range(6))
    big = 1 << 30

    def draw(tr=tr, N=12, P=4, K=2, V=5, seed=1, use_epoch=1):
        return lib.tfgnn_triples_draw_negatives(tr, N, P, K, V, seed, use_epoch, None)

    def build(tr=tr, N=4, V=5, T=2, t0=t0, t1=t1, t2=t2, t3=t3, ws=ws, nbytes=big):
        return lib.tfgnn_triple_tables_build(tr, N, V, T, t0, t1, t2, t3, ws, nbytes, None)

    def refused(status, text):
        assert status == -1
        assert text in lib.tfgnn_last_error(), lib.tfgnn_last_error()

    refused(draw(V=1), b"second node")
    refused(draw(V=0), b"V must be")
    refused(draw(V=2 ** 31), b"V must be")
    refused(draw(N=13), b"P (1 + K)")
    refused(draw(N=8, K=2), b"P (1 + K)")
    refused(draw(K=-1, N=0), b"N must be")
    refused(draw(K=-1, N=4), b"P (1 + K)")
    refused(draw(P=0, N=0), b"empty batch")
    refused(draw(P=-3), b"empty batch")
    refused(draw(N=2 ** 30 + 2, P=2 ** 29 + 1, K=1), b"2^30")
    refused(draw(tr=None), b"NULL")
    assert draw(tr=tr, N=4, P=4, K=0, V=1) == 0  # K = 0: accepted, nothing launched, nothing dereferenced

    refused(build(N=0), b"empty batch")
    refused(build(N=-2), b"empty batch")
    refused(build(N=2 ** 30 + 1), b"2^30")
    refused(build(V=0), b"V and T")
    refused(build(T=0), b"V and T")
    refused(build(V=2 ** 31), b"V and T")
    refused(build(T=2 ** 31), b"V and T")
    refused(build(tr=None), b"NULL")
    refused(build(t0=None, t1=None, t2=None, t3=None), b"NULL")
    refused(build(t0=None), b"pairs")
    refused(build(t1=None), b"pairs")
    refused(build(t3=None), b"pairs")
    refused(build(ws=None), b"workspace")
    refused(build(nbytes=1024), b"workspace")
    refused(build(ws=P_(0x6008)), b"workspace")
    assert _counts(lib) == before  # nothing was launched
    with pytest.raises(ValueError, match="empty batch"):
        _lib.check(build(N=0))


def test_ops_wrappers_refuse_cpu_tensors_and_bad_shapes():
    from tf2_gnn_amd import ops

    tr = torch.zeros((6, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.draw_negative_triples(tr, 3, 5, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.build_triple_tables_device(tr, 5, 2)
    assert ops.negatives_launch_counts().keys() == {"draw_negatives", "triple_tables"}


# ---- dataset ----------------------------------------------------------------------------------------------------------------
def _arrays():
    feats = np.arange(27, dtype=np.float32).reshape(9, 3)
    edges = [np.array([[0, 1], [4, 5], [5, 6], [6, 4], [2, 2]]), np.array([[7, 8], [8, 7], [1, 0]])]
    return feats, edges


def _dataset(**over):
    params = LinkPredictionDataset.get_default_hyperparameters()
    params.update(over)
    return LinkPredictionDataset(params)


def test_dataset_negative_sampling_hyperparameter():
    defaults = LinkPredictionDataset.get_default_hyperparameters()
    assert defaults["negative_sampling"] == "host" and defaults["negative_sampling_seed"] == 0
    for bad in ("gpu", "", None, 1):
        with pytest.raises(ValueError, match="negative_sampling must be 'host' or 'device'"):
            _dataset(negative_sampling=bad)
    for bad in (-1, 2 ** 32, 0.5, "7"):
        with pytest.raises(ValueError, match="negative_sampling_seed"):
            _dataset(negative_sampling_seed=bad)
    # an absent key means "host"
    params = LinkPredictionDataset.get_default_hyperparameters()
    del params["negative_sampling"], params["negative_sampling_seed"]
    feats, edges = _arrays()
    for ds in (LinkPredictionDataset(params), _dataset(negative_sampling="host")):
        ds.load_data_from_arrays(feats, edges)
        np.random.seed(3)
        got = ds.triple_batch(DataFold.TRAIN, "cpu")
        assert "triple_sampler" not in got
        np.random.seed(3)
        assert np.array_equal(got["triples"].numpy(), ds.draw_triples(DataFold.TRAIN))
    # the device route has no CPU fallback
    dev = _dataset(negative_sampling="device", negative_sampling_seed=2 ** 32 - 1)
    dev.load_data_from_arrays(feats, edges)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dev.triple_batch(DataFold.TRAIN, "cpu")
