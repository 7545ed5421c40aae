"""LinkPredictionTask with ``link_decoder="complex"`` on the device: the 60-node, 3-relation planted graph, the task and the
helpers of tests/test_gpu_link_prediction.py, hidden width 64, a 2-layer RGCN.  The task against the fp64 oracle stack with a
float64 ComplEx decoder and binary cross-entropy on top, and against the op-level calls bit for bit (those are pinned in
tests/test_gpu_complex.py); which entries launch for which decoder; the torch autograd route; a CapturedStep with the device
negative sampler inside; evaluate_model; a mini-batch with a row-sparse embedding update; and the functional difference: a
direction that ComplEx learns and no symmetric decoder can.  PARITY UNPINNED: the reference has no such task."""
import math

import numpy as np
import pytest
import torch

from tests import complex_reference as cref
from tests import distmult_reference as dref
from tests import test_gpu_link_prediction as lp
from tests.helpers import assert_close
from tests.test_gpu_layers import _gnn_oracle_weights, _to64
from tests.test_gpu_tasks import _check_grads, _gnn_pairs, _leaves, _oracle_gnn

# the library's default mode and bench.py's comparison mode (conftest.py: gemm_modes)
pytestmark = [pytest.mark.gpu, pytest.mark.gemm_modes("f16x2", "bf16x3"), pytest.mark.usefixtures("gemm_mode")]


def _complex_scores64(h64, R64, t):
    m = h64.shape[1] // 2
    a, r, b = h64[t[:, 0]], R64[t[:, 1]], h64[t[:, 2]]
    (ar, ai), (rr, ri), (br, bi) = ((x[:, :m], x[:, m:]) for x in (a, r, b))
    return (rr * (ar * br + ai * bi) + ri * (ar * bi - ai * br)).sum(dim=1)


def _oracle(model, params, ds, labels):
    """tests/test_gpu_link_prediction.py _oracle with the float64 ComplEx decoder on top ->
    (h64, R64, loss64, (variable, float64 leaf) pairs, triples, labels)"""
    from tf2_gnn_amd.data import DataFold

    host = ds.packed_fold(DataFold.TRAIN)
    w64 = _to64(_gnn_oracle_weights(model._gnn))
    R64 = model._relation_embeddings.value.cpu().double().clone()
    _leaves(w64), _leaves(R64)
    h64, _ = _oracle_gnn(params, w64, torch.from_numpy(host.features).double(), host.edges)
    triples = labels["triples"].cpu().numpy()
    s64 = _complex_scores64(h64, R64, torch.from_numpy(triples.astype(np.int64)))
    y = labels["triple_labels"].cpu().double()
    loss64 = torch.nn.functional.binary_cross_entropy_with_logits(s64, y)
    pairs = _gnn_pairs(model._gnn, w64, ds.num_edge_types) + [(model._relation_embeddings, R64)]
    return h64, R64, loss64, pairs, triples, y


def _counts():
    from tf2_gnn_amd import ops

    return {**ops.link_launch_counts(), **ops.complex_launch_counts()}


def _delta(after, before):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def test_complex_task_loss_and_gradients(dev):
    """batch -> scores -> loss / accuracy / counts -> every gradient, against the fp64 oracle stack with the float64 ComplEx
    decoder on top.  Bounds, composed as tests/test_gpu_link_prediction.py composes them: node representations 1e-5
    (assert_close); a score then moves by at most sum |d s / d h_u| e_u + |d s / d h_v| e_v with e = 1e-5 max(1, |h|), the
    derivatives taken term by term in absolute value (tests/complex_reference.py gradient_terms) - first order, 1 % added for
    the second - plus the kernel's own bound; the loss, 1-Lipschitz in every score, by the mean of that plus 2e-6 max(1, loss);
    gradients through _check_grads like every task.  dH / dR of the task path equal the op-level calls bit for bit, and not
    one launch comes from the DistMult entries."""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import DataFold

    ds = lp._dataset()
    model, params = lp._task(ds, 3, link_decoder="complex")
    assert model.link_decoder == "complex"
    with torch.no_grad():
        model._relation_embeddings.value.mul_(3.0)  # scores away from 0
    feats, labels = lp._single_batch(ds, DataFold.TRAIN, dev)
    before = _counts()
    out = model(feats, training=False)
    m = model.compute_task_metrics(feats, out, labels)
    assert _delta(_counts(), before) == {"complex_fwd": 3}  # one fused call for output and metrics
    assert sorted(m) == ["accuracy", "counts", "loss"] and all(isinstance(v, torch.Tensor) and v.is_cuda for v in m.values())
    step = model._step
    d_h, none = model._task_backward()
    assert none is None
    op_dH, op_dR = ops.complex_backward(step["h"], model._relation_embeddings.value, labels["triples"], step["dloss"],
                                        labels["triple_tables"])
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(d_h), bits(op_dH)) and torch.equal(bits(model._relation_embeddings.grad), bits(op_dR))
    op_m, op_c, op_s, op_g = ops.complex_ce_metrics(step["h"], model._relation_embeddings.value, labels["triples"],
                                                    labels["triple_labels"], labels["triple_weights"])
    assert torch.equal(bits(op_s), bits(out[0])) and torch.equal(bits(op_g), bits(step["dloss"]))
    assert torch.equal(bits(op_m[0]), bits(m["loss"])) and torch.equal(op_c, m["counts"])
    model.zero_grad()
    model.backward()
    assert _delta(_counts(), before) == {"complex_fwd": 6, "complex_bwd": 12}  # three fused forward, four backward launches each
    assert torch.equal(bits(model._relation_embeddings.grad), bits(op_dR))

    h64, R64, loss64, pairs, triples, y = _oracle(model, params, ds, labels)
    assert_close(step["h"].cpu(), h64.detach().float(), tol=1e-5, what="final node representations")
    hn, Rn = h64.detach().numpy(), R64.detach().numpy()
    e = 1e-5 * np.maximum(1.0, np.abs(hn))
    u, r, v = triples[:, 0], triples[:, 1], triples[:, 2]
    src, dst, _ = cref.gradient_terms(hn[u], Rn[r], hn[v])
    ds_stack = 1.01 * ((np.abs(src[0]) + np.abs(src[1])) * e[u] + (np.abs(dst[0]) + np.abs(dst[1])) * e[v]).sum(axis=1)
    exact = cref.complex_ce(hn, Rn, triples, y.numpy())
    ds_total = ds_stack + exact.score_bound
    loss = float(loss64.detach())
    assert abs(exact.loss - loss) <= 1e-12
    bound = 2e-6 * max(1.0, loss) + float(ds_total.mean())
    err = abs(float(m["loss"]) - loss)
    print(f"LinkPredictionTask(complex) loss {float(m['loss']):.9g} fp64 {loss:.9g} error / bound {err / bound:.3f}")
    assert err <= bound
    scores = out[0].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(scores - exact.scores) <= ds_total)
    on_hip = cref.complex_ce(hn, Rn, triples, y.numpy(), scores=scores)  # counts from the HIP scores
    assert [int(x) for x in m["counts"].cpu()] == list(on_hip.counts) and sum(on_hip.counts) == len(triples)
    assert abs(float(m["accuracy"]) - on_hip.accuracy) <= 1e-6
    _check_grads(model, pairs, loss64, "LinkPredictionTask(complex)")


def test_default_decoder_launches_nothing_from_the_complex_entries(dev):
    from tf2_gnn_amd.data import DataFold

    ds = lp._dataset()
    feats, labels = lp._single_batch(ds, DataFold.TRAIN, dev)
    test = ds.get_batches(DataFold.TEST, dev)
    for extra, prefix in (({}, "distmult"), ({"link_decoder": "distmult"}, "distmult"), ({"link_decoder": "complex"}, "complex")):
        model, _ = lp._task(ds, 3, optimizer="Adam", learning_rate=0.01, **extra)
        before = _counts()
        model._run_step(feats, labels, training=True)
        assert _delta(_counts(), before) == {f"{prefix}_fwd": 3, f"{prefix}_bwd": 4}, extra
        model.evaluate_model(test)
        assert _delta(_counts(), before) == {f"{prefix}_fwd": 3, f"{prefix}_bwd": 4, f"{prefix}_rank": 4}, extra  # two per side


def test_torch_autograd_route_with_bce(dev):
    from tf2_gnn_amd import TorchGraphTaskModel
    from tf2_gnn_amd.data import DataFold

    ds = lp._dataset()
    model, params = lp._task(ds, 5, link_decoder="complex")
    feats, labels = lp._single_batch(ds, DataFold.TRAIN, dev)
    module = TorchGraphTaskModel(model).eval()
    before = _counts()
    scores = module(feats)
    assert scores.requires_grad and tuple(scores.shape) == (labels["triples"].shape[0],)
    torch.nn.functional.binary_cross_entropy_with_logits(scores, labels["triple_labels"]).backward()
    assert all(p.grad is not None for p in module.parameters())
    assert all(k.startswith("complex_") for k in _delta(_counts(), before))
    _, _, loss64, pairs, _, _ = _oracle(model, params, ds, labels)
    _check_grads(model, pairs, loss64, "TorchGraphTaskModel(LinkPredictionTask, complex)")


def test_captured_step_with_device_negatives_equals_eager(dev):
    """A CapturedStep of three Adam steps with negative_sampling="device" - the sampler's redraw() is inside the capture -
    against three eager steps of a host-route twin whose buffers are overwritten with the reference's negatives for the
    captured draw's key (tests/test_gpu_link_prediction_device_negatives.py, whose construction this follows): every loss, the
    counts and the final weights bit for bit."""
    from tf2_gnn_amd import CapturedStep, ops
    from tf2_gnn_amd.data import DataFold
    from tests import negative_sample_reference as nref
    from tests import test_gpu_link_prediction_device_negatives as dn

    ds_a = dn._dataset(negative_sampling="device", negative_sampling_seed=5)
    ds_b = dn._dataset()  # the host route
    np.random.seed(2)
    feats_a, labels_a = next(iter(ds_a.get_batches(DataFold.TRAIN, dev)))
    feats_b, labels_b = next(iter(ds_b.get_batches(DataFold.TRAIN, dev)))
    sampler = feats_a["triple_sampler"]
    pos = ds_a.positive_triples(DataFold.TRAIN)
    P = len(pos)
    train = {"optimizer": "Adam", "learning_rate": 0.01, "link_decoder": "complex"}
    (model_a, _), (model_b, _) = lp._task(ds_a, 6, **train), lp._task(ds_b, 7, **train)
    for a, b in zip(model_a.trainable_variables, model_b.trainable_variables):
        b.assign(a.value.clone())
    w0 = [v.value.clone() for v in model_a.trainable_variables]

    def step():
        m = model_a._run_step(feats_a, labels_a, training=True)
        return m["loss"], m["accuracy"], m["counts"]

    before = _counts()
    try:
        cap = CapturedStep(step)
        cap.capture()
        seed = sampler.seed_of_last_draw  # the captured draw's seed: every replay passes it
        for v, w in zip(model_a.trainable_variables, w0):
            v.assign(w)
            for slot in model_a._optimizer.slots(v):
                slot.zero_()
        model_a._optimizer.iterations = 0
        ops.dropout_epoch_set(0)
        replayed, drawn = [], []
        for _ in range(3):  # one replay = one epoch with fresh negatives; nothing of the dataset runs in between
            out = cap.replay()
            replayed.append(tuple(t.clone() for t in out))
            drawn.append(labels_a["triples"].clone())
        torch.cuda.synchronize()
        assert not cap.guard_tripped()
        stepped = []
        for i in range(3):
            want = nref.triples(pos, dn.K_DS, dn.V_DS, seed, epoch=i + 1)
            assert np.array_equal(drawn[i].cpu().numpy(), want), f"replay {i}: the negatives are not the reference's"
            dn._overwrite(labels_b, want, dn.V_DS, dn.T_DS)
            m = model_b._run_step(feats_b, labels_b, training=True)
            stepped.append((m["loss"].clone(), m["accuracy"].clone(), m["counts"].clone()))
        torch.cuda.synchronize()
    finally:
        ops.dropout_epoch_set(0)  # every other test draws at epoch 0
        torch.cuda.synchronize()
    assert all(k.startswith("complex_") for k in _delta(_counts(), before))
    assert not torch.equal(drawn[0], drawn[1]) and not torch.equal(drawn[1], drawn[2])
    assert model_a._optimizer.iterations == model_b._optimizer.iterations == 3
    for e, r in zip(stepped, replayed):
        assert all(torch.equal(a, b) for a, b in zip(e, r)), (stepped, replayed)
        assert torch.equal(e[0].view(torch.int32), r[0].view(torch.int32))
    assert all(int(c.sum()) == (1 + dn.K_DS) * P for _, _, c in stepped) and all(math.isfinite(float(l)) for l, _, _ in stepped)
    for a, b, w in zip(model_a.trainable_variables, model_b.trainable_variables, w0):
        assert torch.equal(a.value, b.value) and not torch.equal(a.value, w), a.name


def test_evaluate_model_counts_are_the_op_level_counts(dev):
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.data import DataFold
    from tf2_gnn_amd.utils import eval_metrics

    ds = lp._dataset()
    model, _ = lp._task(ds, 9, link_decoder="complex")
    test = ds.get_batches(DataFold.TEST, dev)
    metrics = model.evaluate_model(test)
    assert list(metrics) == ["mrr", "hits@1", "hits@3", "hits@10"]
    assert all(0.0 <= v <= 1.0 for v in metrics.values()) and metrics["hits@1"] <= metrics["hits@3"] <= metrics["hits@10"]
    feats, labels = lp._single_batch(ds, DataFold.TEST, dev)
    greater, equal = model.rank_counts(feats, labels)
    h = model._final(model.compute_final_node_representations(feats, training=False))
    P = len(ds.positive_triples(DataFold.TEST))
    for i, side in enumerate(("dst", "src")):
        g, e = ops.complex_rank(h, model._relation_embeddings.value, ds.positive_triples(DataFold.TEST), side,
                                *ds.rank_filters(DataFold.TEST)[side])
        assert torch.equal(greater[i * P:(i + 1) * P], g) and torch.equal(equal[i * P:(i + 1) * P], e)
    assert metrics == eval_metrics.ranking_metrics(greater.cpu().numpy(), equal.cpu().numpy())
    # the exact family: integer representations, the float64 reference's filtered counts over both sides exactly
    rng = np.random.default_rng(5)
    H = rng.integers(-2, 3, size=(lp.V_DS, lp.H_DS)).astype(np.float32)
    R = rng.integers(-2, 3, size=(lp.T_DS, lp.H_DS)).astype(np.float32)
    model._relation_embeddings.assign(torch.from_numpy(R).to(dev))
    H_dev = torch.from_numpy(H).to(dev)
    model.compute_final_node_representations = lambda inputs, training: H_dev
    got = model.evaluate_model(test)
    pairs = [cref.complex_rank(H, R, ds.positive_triples(DataFold.TEST), side, *ds.rank_filters(DataFold.TEST)[side])[:2]
             for side in ("dst", "src")]
    want = eval_metrics.ranking_metrics(np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs]))
    assert got == want, (got, want)


def test_mini_batch_with_row_sparse_embedding_update(dev):
    """One sampled batch of a featureless model: its loss inside the reference's bound when evaluated from the batch's own h
    and local triples; the table's gradient is a RowGradient with finite rows; the step applies."""
    from tf2_gnn_amd import RowGradient
    from tf2_gnn_amd.data import DataFold
    from tests.test_gpu_link_prediction_minibatch import _dataset as minibatch_dataset

    ds = minibatch_dataset(featureless=True, neighbor_fanouts=[-1], triples_per_batch=24)
    model, _ = lp._task(ds, 8, optimizer="Adam", learning_rate=0.01, node_embedding_dim=16, node_embedding_update="rows",
                        link_decoder="complex")
    (table,) = [x for x in model.trainable_variables if x.name.endswith("/node_embeddings")]
    np.random.seed(6)
    feats, labels = next(iter(ds.get_batches(DataFold.TRAIN, dev)))
    before = _counts()
    out = model(feats, training=True)
    m = model.compute_task_metrics(feats, out, labels)
    pairs = model.backward()
    assert _delta(_counts(), before) == {"complex_fwd": 3, "complex_bwd": 4}
    h = model._step["h"].cpu().numpy()
    triples = labels["triples"].cpu().numpy()
    assert triples.max() < h.shape[0] < ds.num_nodes  # local ids: rows of the batch's representations
    w = labels.get("triple_weights")
    r = cref.complex_ce(h, model._relation_embeddings.value.cpu().numpy(), triples, labels["triple_labels"].cpu().numpy(),
                        None if w is None else w.cpu().numpy())
    err = abs(float(m["loss"]) - r.loss)
    print(f"mini-batch ComplEx loss {float(m['loss']):.9g} reference {r.loss:.9g} error / bound {err / r.loss_bound:.3f}")
    assert err <= r.loss_bound and [int(x) for x in m["counts"].cpu()] == list(r.counts)
    assert np.all(np.abs(out[0].cpu().numpy() - r.scores) <= r.score_bound)
    grad = dict((v.name, g) for v, g in pairs)[table.name]
    assert isinstance(grad, RowGradient) and grad.ids is feats["sampled_node_ids"]
    assert tuple(grad.rows.shape) == (h.shape[0], 16) and bool(torch.isfinite(grad.rows).all()) and bool(grad.rows.any())
    old = table.value.clone()
    model._apply_gradients(pairs)
    torch.cuda.synchronize()
    assert int(model.embedding_bad_index) == 0 and not torch.equal(table.value, old) and bool(torch.isfinite(table.value).all())


# ---- direction ------------------------------------------------------------------------------------------------------------
V_DIR, D0_DIR, H_DIR, STEPS_DIR = 16, 8, 32, 200


def _direction_batch(dev):
    """16 nodes, one relation.  Positives: 40 ordered pairs u -> v, u != v, none of them the reverse of another; negatives:
    exactly the reversed pairs.  The graph holds the positives as type 0 and - untied - their reverses as type 1."""
    from tf2_gnn_amd import ops

    rng = np.random.default_rng(1609)
    pairs = [(u, v) for u in range(V_DIR) for v in range(u + 1, V_DIR)]
    chosen = [pairs[i] for i in rng.permutation(len(pairs))[:40]]
    pos = np.array([(u, v) if rng.integers(0, 2) else (v, u) for u, v in chosen], dtype=np.int32)
    assert len({(int(u), int(v)) for u, v in pos} & {(int(v), int(u)) for u, v in pos}) == 0
    triples = np.concatenate([np.stack([pos[:, 0], np.zeros(40, dtype=np.int32), pos[:, 1]], axis=1),
                              np.stack([pos[:, 1], np.zeros(40, dtype=np.int32), pos[:, 0]], axis=1)]).astype(np.int32)
    y = np.concatenate([np.ones(40), np.zeros(40)]).astype(np.float32)
    X = rng.standard_normal((V_DIR, D0_DIR)).astype(np.float32)
    feats = {"node_features": torch.from_numpy(X).to(dev), "node_to_graph_map": torch.zeros(V_DIR, dtype=torch.int32, device=dev),
             "num_graphs_in_batch": 1, "adjacency_list_0": torch.from_numpy(pos).to(dev),
             "adjacency_list_1": torch.from_numpy(np.ascontiguousarray(pos[:, ::-1])).to(dev)}
    labels = {"triples": torch.from_numpy(triples).to(dev), "triple_labels": torch.from_numpy(y).to(dev),
              "triple_weights": torch.ones(80, device=dev),
              "triple_tables": {k: torch.from_numpy(t).to(dev) for k, t in ops.build_triple_tables(triples, V_DIR, 1).items()}}
    feats.update(labels)
    return feats, labels, triples, y


def _direction_run(dev, decoder):
    """-> [(loss of the step, the reference's loss bound at that step's h and R)] over STEPS_DIR Adam steps"""
    from tf2_gnn_amd.layers.message_passing import set_seed
    from tf2_gnn_amd.tasks import LinkPredictionTask
    from tests.test_gpu_tasks import _gnn_params

    feats, labels, triples, y = _direction_batch(dev)
    set_seed(11)
    params = _gnn_params(LinkPredictionTask, "rgcn", H_DIR, 2, extra={"gnn_layer_input_dropout_rate": 0.0, "optimizer": "Adam",
                                                                       "learning_rate": 0.02, "link_decoder": decoder})
    model = LinkPredictionTask(params, num_edge_types=2, num_relations=1)
    model.build({"node_features": (None, D0_DIR)})
    ce = cref.complex_ce if decoder == "complex" else dref.distmult_ce
    history = []
    for _ in range(STEPS_DIR):
        R = model._relation_embeddings.value.cpu().numpy()  # before the update of this step
        loss = float(model._run_step(feats, labels, training=True)["loss"])
        r = ce(model._step["h"].cpu().numpy(), R, triples, y)
        assert abs(loss - r.loss) <= r.loss_bound
        history.append((loss, r.loss_bound))
    return history


def test_direction_can_be_learned_by_complex_and_not_by_distmult(dev):
    """Every negative is the reverse of a positive.  For ANY symmetric decoder a positive and its negative score the same s, so
    their two loss elements add up to softplus(-s) + softplus(s) >= 2 ln 2 and the mean loss is >= ln 2 in exact arithmetic,
    whatever the weights: with "distmult" the loss of EVERY step is >= ln 2 minus the reference's loss bound (the kernel's
    distance from exact arithmetic).  The same seeded model with "complex" ends below ln 2 minus that bound.  The kernels are
    bit-reproducible, so the outcome is deterministic; no other threshold is fixed."""
    ln2 = math.log(2.0)
    sym = _direction_run(dev, "distmult")
    asym = _direction_run(dev, "complex")
    print(f"direction: {STEPS_DIR} Adam steps, final loss distmult {sym[-1][0]:.6f} complex {asym[-1][0]:.6f} (ln 2 = {ln2:.6f})")
    for step, (loss, bound) in enumerate(sym):
        assert loss >= ln2 - bound, (step, loss, bound)
    assert asym[-1][0] < ln2 - asym[-1][1], asym[-1]
