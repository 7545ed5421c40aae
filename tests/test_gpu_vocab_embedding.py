"""Vocabulary embeddings on the device: ops.vocab_embedding_forward / vocab_embedding_backward (csrc/vocab_embedding.hip)
against a float64 host reference - ``table[ids]`` and ``index_add`` over the valid ids - and the task-model route.

The shapes are the smallest at which each mechanism can fail: n around one chunk (255, 256, 257) and five chunks (1025);
N = 600 takes two sort passes; D = 1 and 5 take the scalar columns, 4 and 64 float4, 260 a second slab of 256 columns.

The backward bound is derived, not measured: at most 255 sequential adds in a chunk and one per further chunk, so to first
order  |got - ref| <= (256 + ceil(m / 256)) * 2^-24 * S  with m the rows of the id and S the float64 sum of |d_rows| over them."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = ("i32", "f32", "col0")  # int32 ids, float32 ids, column 0 of a float32 [n, 3] matrix


def _cases():
    dims, cases = (1, 4, 5, 64, 260), []
    for i, (n, N) in enumerate((n, N) for n in (1, 255, 256, 257, 1025) for N in (1, 3, 600)):
        cases.append((n, N, dims[i % 5], "seeded", KINDS[i % 3], False))
    cases += [(1025, 3, D, "hub", KINDS[i % 3], False) for i, D in enumerate(dims)]  # one id over five chunks
    cases += [(n, 600, dims[i], "distinct", KINDS[i % 3], False) for i, n in enumerate((1, 255, 256, 257))]
    cases += [(n, 3, D, "ends_on_256", "i32", False) for n, D in ((257, 4), (1025, 5))]
    cases += [(1025, 3, 64, "seeded", "col0", True), (257, 3, 5, "seeded", "f32", True)]  # row pitches above D
    cases += [(257, 3, D, "invalid", kind, False) for D in (5, 64) for kind in KINDS]
    cases += [(0, 3, 4, "seeded", "i32", False), (0, 3, 5, "seeded", "f32", False)]
    return cases


@functools.lru_cache(maxsize=None)
def _run(n, N, D, pattern, kind, pitched):
    """One case through both ops, twice -> everything the tests compare, on the host."""
    from tf2_gnn_amd import ops

    rng = np.random.default_rng(1000 * n + N + D)
    if pattern == "hub":
        ids = np.full(n, N - 1, dtype=np.float64)
    elif pattern == "distinct":
        ids = rng.permutation(N)[:n].astype(np.float64)
    elif pattern == "ends_on_256":  # the sorted segment of id 0 is the positions [0, 256)
        ids = np.where(np.arange(n) < 256, 0.0, N - 1.0)[rng.permutation(n)]
    else:
        ids = rng.integers(0, N, size=n).astype(np.float64)
    if pattern == "invalid":
        bad = {0: -1, 5: N, 256: -1} if kind == "i32" else {0: 2.5, 3: float("nan"), 5: -0.0, 7: N, 256: float("inf")}
        for i, v in bad.items():
            ids[i] = v
    valid = np.isfinite(ids) & (ids == np.floor(ids)) & (ids >= 0) & (ids < N)  # -0.0 is valid and is id 0
    ids_t = torch.from_numpy(ids)
    if kind == "i32":
        dev_ids = ids_t.to(torch.int32).cuda()
    elif kind == "f32":
        dev_ids = ids_t.to(torch.float32).cuda()
    else:
        matrix = torch.full((n, 3), float("nan"))
        matrix[:, 0] = ids_t.to(torch.float32)
        dev_ids = matrix.cuda()[:, 0]
    pad = (4 if D % 4 == 0 else 3) if pitched else 0  # a pitched float4 case and a pitched scalar case
    g = torch.Generator().manual_seed(n + N + D)
    table = torch.randn(N, D + pad, generator=g).cuda()[:, :D]
    d_rows = torch.randn(n, D + pad, generator=g).cuda()[:, :D]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rows_out = torch.full((n, D + pad), float("nan"), device="cuda")
    rows, plan = ops.vocab_embedding_forward(table, dev_ids, out=rows_out[:, :D], bad_flag=flag)
    grads = []
    for _ in range(2):
        buf = torch.full((N, D + pad), float("nan"), device="cuda")  # the caller does not pre-fill
        ops.vocab_embedding_backward(d_rows, plan, N, out=buf[:, :D])
        grads.append(buf.cpu())
    _, plan2 = ops.vocab_embedding_forward(table, dev_ids, plan=plan)
    torch.cuda.synchronize()
    return dict(ids=ids, valid=valid, table=table.cpu(), d_rows=d_rows.cpu(), rows=rows_out.cpu(), flag=int(flag), grads=grads,
                plan_reused=plan2 is plan)


@pytest.mark.parametrize("n,N,D,pattern,kind,pitched", _cases())
def test_forward(dev, n, N, D, pattern, kind, pitched):
    r = _run(n, N, D, pattern, kind, pitched)
    valid, rows = torch.from_numpy(r["valid"]), r["rows"]
    want = torch.zeros(n, D)
    want[valid] = r["table"][torch.from_numpy(r["ids"][r["valid"]]).long()]
    assert torch.equal(rows[:, :D].view(torch.int32), want.view(torch.int32))  # bit for bit; zero rows for invalid ids
    assert torch.isnan(rows[:, D:]).all()  # the columns beyond D of a pitched row are not touched
    assert r["flag"] == int(not valid.all()) and r["plan_reused"]
    assert (pattern == "invalid") == (not valid.all())


@pytest.mark.parametrize("n,N,D,pattern,kind,pitched", _cases())
def test_backward(dev, n, N, D, pattern, kind, pitched):
    r = _run(n, N, D, pattern, kind, pitched)
    got, again = r["grads"]
    assert torch.equal(got[:, :D].view(torch.int32), again[:, :D].view(torch.int32))  # the same bits from call to call
    assert torch.isnan(got[:, D:]).all() and not torch.isnan(got[:, :D]).any()
    index = torch.from_numpy(r["ids"][r["valid"]]).long()
    d = r["d_rows"][torch.from_numpy(r["valid"])].double()
    ref = torch.zeros(N, D, dtype=torch.float64).index_add_(0, index, d)
    S = torch.zeros(N, D, dtype=torch.float64).index_add_(0, index, d.abs())
    m = torch.bincount(index, minlength=N)
    bound = (256 + torch.ceil(m.double() / 256)).unsqueeze(1) * 2.0 ** -24 * S
    err = (got[:, :D].double() - ref).abs()
    print(f"max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3g}, largest id {int(m.max()) if N else 0} rows")
    assert bool((err <= bound).all())
    assert bool((got[:, :D][m == 0] == 0).all())  # absent ids: exact zeros in a buffer that arrived full of NaN
    single = m == 1  # an id with one row gets that row's bits
    assert torch.equal(got[:, :D][single].view(torch.int32), ref[single].float().view(torch.int32))
    if pattern == "hub":
        assert int(m.max()) == n and math.ceil(n / 256) == 5


# ---- the task-model route -------------------------------------------------------------------------------------------------------
V, L, H, LABELS, VOCAB = 40, 2, 8, 3, 5


def _task(seed, **extra):
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import NodeMulticlassTask

    set_seed(seed)
    params = NodeMulticlassTask.get_default_hyperparameters("rgcn")
    params.update({"gnn_hidden_dim": H, "gnn_num_layers": 2, "gnn_layer_input_dropout_rate": 0.0, "optimizer": "Adam",
                   "learning_rate": 0.01, "node_embedding_dim": H})
    params.update(extra)
    model = NodeMulticlassTask(params, num_edge_types=L, num_node_target_labels=LABELS, num_nodes=V)
    model.build({"node_features": (None, 1)})
    return model


def _step(model, feats, labels):
    out = model(feats, training=True)
    loss = model.compute_task_metrics(feats, out, labels)["loss"]
    model.backward()
    torch.cuda.synchronize()
    return loss


def test_task_model_on_a_tiny_graph(dev):
    from tf2_gnn_amd import CapturedStep, ops

    rng = np.random.default_rng(5)
    feats = {"node_to_graph_map": torch.from_numpy(np.repeat(np.arange(2), V // 2).astype(np.int32)).to(dev),
             "num_graphs_in_batch": 2, "node_features": torch.zeros(V, 1, device=dev)}
    for t in range(L):
        feats[f"adjacency_list_{t}"] = torch.from_numpy(rng.integers(0, V, size=(3 * V, 2)).astype(np.int32)).to(dev)
    labels = {"node_labels": torch.from_numpy(rng.integers(0, 2, size=(V, LABELS)).astype(np.float32)).to(dev)}
    bits = lambda t: t.contiguous().view(torch.int32)
    # (a) distinct ids over a vocabulary of V: the full-batch node_embedding_dim model, bit for bit, on the new kernels
    plain, vocab = _task(3), _task(3, node_vocabulary_size=V)
    assert [v.name for v in vocab.trainable_variables] == [v.name for v in plain.trainable_variables]
    assert vocab.trainable_variables[-1].name == "NodeMulticlassTask/node_embeddings"
    old, new = ops.embedding_launch_count(), ops.vocab_embedding_launch_counts()
    loss_plain = _step(plain, feats, labels)
    loss_vocab = _step(vocab, dict(feats, node_vocabulary_ids=torch.arange(V, dtype=torch.int32, device=dev)), labels)
    assert torch.equal(bits(loss_plain), bits(loss_vocab))
    for a, b in zip(plain.trainable_variables, vocab.trainable_variables):
        assert torch.equal(bits(a.value), bits(b.value)) and torch.equal(bits(a.grad), bits(b.grad)), a.name
    counts = ops.vocab_embedding_launch_counts()
    assert ops.embedding_launch_count() == old and counts[0] > new[0] and counts[1] > new[1]
    # (b) repeated ids: model A has a [V, dim] table set to table[ids]; its gradient is the per-row input gradient
    ids = torch.from_numpy(rng.integers(0, VOCAB - 1, size=V).astype(np.int32)).to(dev)  # id VOCAB - 1 stays absent
    model_a, model_b = _task(4), _task(4, node_vocabulary_size=VOCAB)
    table_a, table_b = model_a.trainable_variables[-1], model_b.trainable_variables[-1]
    assert table_b.shape == (VOCAB, H)
    table_a.assign(table_b.value[ids.long()])
    by_key = dict(feats, node_vocabulary_ids=ids)
    loss_b = _step(model_b, by_key, labels).clone()
    assert torch.equal(bits(_step(model_a, feats, labels)), bits(loss_b))
    d = table_a.grad.double().cpu()
    ref = torch.zeros(VOCAB, H, dtype=torch.float64).index_add_(0, ids.long().cpu(), d)
    S = torch.zeros(VOCAB, H, dtype=torch.float64).index_add_(0, ids.long().cpu(), d.abs())
    assert bool(((table_b.grad.double().cpu() - ref).abs() <= 257 * 2.0 ** -24 * S).all()) and float(S.max()) > 0.0
    assert bool((table_b.grad[VOCAB - 1] == 0).all()) and int(model_b.embedding_bad_index) == 0
    # (d) the ids as column 0 of node_features [V, 1]: the same bits as the key
    grad_by_key = table_b.grad.clone()
    by_column = dict(feats, node_features=ids.to(torch.float32).view(V, 1))
    assert torch.equal(bits(_step(model_b, by_column, labels)), bits(loss_b))
    assert torch.equal(bits(table_b.grad), bits(grad_by_key))
    # (c) one captured training step, replayed, against the eager step of an identically seeded model
    model_c, model_e = _task(6, node_vocabulary_size=VOCAB), _task(6, node_vocabulary_size=VOCAB)
    start = [v.value.clone() for v in model_c.trainable_variables]
    cap = CapturedStep(lambda: model_c._run_step(by_column, labels, training=True)["loss"])
    cap.capture()
    for v, w in zip(model_c.trainable_variables, start):  # back to the start: the warm-up steps trained
        v.assign(w)
        for slot in model_c._optimizer.slots(v):
            slot.zero_()
    model_c._optimizer.iterations = 0
    replayed = cap.replay().clone()
    eager = model_e._run_step(by_column, labels, training=True)["loss"]
    torch.cuda.synchronize()
    assert not cap.guard_tripped() and torch.equal(bits(replayed), bits(eager))
    assert torch.equal(bits(model_c.trainable_variables[-1].value), bits(model_e.trainable_variables[-1].value))
    assert not torch.equal(model_c.trainable_variables[-1].value, start[-1])
