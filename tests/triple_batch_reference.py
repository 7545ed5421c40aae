"""tfgnn_triple_batch_build (include/tfgnn.h "Triple batches") in numpy, written from that text: gather the batch's positives,
draw their negatives with tests/negative_sample_reference.py (use_epoch = 0), take np.unique of the valid endpoints as the
seeds, searchsorted for the local ids, the status bits and the capacity rule.  Integers only.  Independent of the library:
the GPU tests compare the kernels against it bit for bit, tests/test_triple_batch_host.py pins it against a plain loop."""
import numpy as np

from tests import negative_sample_reference as nref

SEED_OVERFLOW, BAD_POSITIVE_ID, BAD_ENDPOINT = 1, 2, 4


def build(positives, positive_ids, K: int, V: int, seed: int, seed_capacity: int):
    """-> (triples int32 [N, 3], local_triples int32 [N, 3], seeds int32 [S], S, status)"""
    store = np.asarray(positives, dtype=np.int32).reshape(-1, 3)
    ids = np.asarray(positive_ids, dtype=np.int64).reshape(-1)
    P, B = store.shape[0], ids.shape[0]
    status = 0
    good_id = (ids >= 0) & (ids < P)
    if not good_id.all():
        status |= BAD_POSITIVE_ID
    pos = store[np.where(good_id, ids, 0)].astype(np.int64)
    # the draw compares node ids as unsigned 32-bit words: show it a negative endpoint as the kernel sees it (the cast back
    # to int32 wraps it to what the store holds)
    as_words = pos.copy()
    as_words[:, [0, 2]] &= 0xFFFFFFFF
    triples = np.concatenate([as_words, nref.draw(as_words, K, V, seed, use_epoch=False).astype(np.int64) & 0xFFFFFFFF])
    triples = triples.astype(np.uint32).view(np.int32).reshape(-1, 3).astype(np.int64)
    good_row = np.concatenate([good_id, np.repeat(good_id, K)])  # a negative shares its positive's id
    triples[~good_row] = -1
    ends = triples[:, [0, 2]]
    good_end = (ends >= 0) & (ends < V) & good_row[:, None]
    if (~good_end & good_row[:, None]).any():
        status |= BAD_ENDPOINT
    seeds = np.unique(ends[good_end])
    if seeds.shape[0] > seed_capacity:
        status |= SEED_OVERFLOW
        seeds = seeds[:seed_capacity]
    rank = np.searchsorted(seeds, ends)
    found = good_end & (rank < seeds.shape[0])
    found &= seeds[np.minimum(rank, max(seeds.shape[0] - 1, 0))] == ends if seeds.shape[0] else False
    local = triples.copy()
    local[:, [0, 2]] = np.where(found, rank, -1)
    return triples.astype(np.int32), local.astype(np.int32), seeds.astype(np.int32), int(seeds.shape[0]), status


def build_loop(positives, positive_ids, K: int, V: int, seed: int, seed_capacity: int):
    """The same outputs by a plain Python loop over the rows: what tests/test_triple_batch_host.py holds ``build`` against."""
    store = [tuple(int(x) for x in row) for row in np.asarray(positives).reshape(-1, 3)]
    ids = [int(i) for i in np.asarray(positive_ids).reshape(-1)]
    B = len(ids)
    words = nref.words(seed, 0, 2 * B * K, use_epoch=False) if K else []
    status, rows = 0, []
    for e in range(B * (1 + K)):
        pid = ids[e] if e < B else ids[(e - B) // K]
        if not 0 <= pid < len(store):
            status |= BAD_POSITIVE_ID
            rows.append(None)
            continue
        u, t, v = store[pid]
        if e >= B:
            j = e - B
            a, b = int(words[2 * j]), int(words[2 * j + 1])
            old = (v if a >> 31 else u) & 0xFFFFFFFF
            d = (b * (V - 1)) >> 32
            node = d + (1 if d >= old else 0)
            u, v = (u, node) if a >> 31 else (node, v)
        rows.append((u, t, v))
    marked = set()
    for row in rows:
        if row is not None:
            for x in (row[0], row[2]):
                if 0 <= x < V:
                    marked.add(x)
                else:
                    status |= BAD_ENDPOINT
    seeds = sorted(marked)
    if len(seeds) > seed_capacity:
        status |= SEED_OVERFLOW
        seeds = seeds[:seed_capacity]
    rank = {x: i for i, x in enumerate(seeds)}
    triples = [(-1, -1, -1) if r is None else r for r in rows]
    local = [(-1, -1, -1) if r is None else (rank.get(r[0], -1) if 0 <= r[0] < V else -1, r[1],
                                              rank.get(r[2], -1) if 0 <= r[2] < V else -1) for r in rows]
    as32 = lambda a, shape: np.asarray(a, dtype=np.int64).reshape(shape).astype(np.int32)
    return as32(triples, (-1, 3)), as32(local, (-1, 3)), as32(seeds, (-1,)), len(seeds), status


def batch_seed(negative_sampling_seed: int, batches_built: int) -> int:
    """the 64-bit seed of the mini-batch a LinkPredictionDataset builds after ``batches_built`` earlier ones"""
    return nref.sampler_seed(negative_sampling_seed, batches_built)
