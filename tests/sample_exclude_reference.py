"""The contract of tfgnn_sample_exclude_edges (include/tfgnn.h "Excluding a batch's positives") restated in numpy: lists and
positives in, the filtered lists, ``removed`` and the status word out.  Exact and integer: the tests compare bit for bit."""
import numpy as np

BAD_RELATION, BAD_ENDPOINT = 32, 64  # TFGNN_SAMPLE_EXCLUDE_*
LAUNCHES = 4  # TFGNN_SAMPLE_EXCLUDE_LAUNCHES


def exclude(lists, positives, fwd_type, inv_type, num_seeds):
    """``lists``: L arrays int32 [E_t, 2] of (source, target) rows in local ids, each SORTED BY TARGET (asserted: the kernel
    relies on it); ``positives`` int32 [B, 3] rows (u, r, v); ``fwd_type`` / ``inv_type``: per relation the list of its
    forward edges and of their inverses, -1 for none.  -> (filtered lists, removed int32 [L], status)."""
    lists = [np.asarray(a, dtype=np.int32).reshape(-1, 2) for a in lists]
    for a in lists:
        assert (np.diff(a[:, 1]) >= 0).all(), "an adjacency list is not sorted by target"
    positives = np.asarray(positives, dtype=np.int32).reshape(-1, 3)
    T, L = len(fwd_type), len(lists)
    assert len(inv_type) == T and all(-1 <= int(x) < L for x in list(fwd_type) + list(inv_type))
    drop = [set() for _ in range(L)]  # (source, target) pairs that go
    status = 0
    for u, r, v in positives.tolist():
        if (u, r, v) == (-1, -1, -1):
            continue
        bad = (0 if 0 <= r < T else BAD_RELATION) | (0 if 0 <= u < num_seeds and 0 <= v < num_seeds else BAD_ENDPOINT)
        if bad:
            status |= bad
            continue
        if fwd_type[r] >= 0:
            drop[int(fwd_type[r])].add((u, v))
        if inv_type[r] >= 0:
            drop[int(inv_type[r])].add((v, u))
    out, removed = [], np.zeros(L, dtype=np.int32)
    for t, a in enumerate(lists):
        keep = np.array([(s, d) not in drop[t] for s, d in a.tolist()], dtype=bool).reshape(-1)
        out.append(np.ascontiguousarray(a[keep]))
        removed[t] = a.shape[0] - out[-1].shape[0]
    return out, removed, status
