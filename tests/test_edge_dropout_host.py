"""Edge dropout on the host: the numpy restatement of tfgnn_graph_scales_edge_dropout (tests/edge_dropout_reference.py) against
direct statements of what it must reduce to, the hyper-parameter's validation, and the new symbol's declaration and binding."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import dropout_reference as dr
from tests import edge_dropout_reference as ref
from tests.helpers import random_graph

ROOT = Path(__file__).resolve().parent.parent
NEW = ["tfgnn_graph_scales_edge_dropout", "tfgnn_edge_dropout_launch_counts"]
COMBOS = [(normalize, mode) for normalize in (False, True) for mode in (0, 1, 2)]


def _graph(seed=3, V=24, L=5):
    adjs = random_graph(V - 1, 400, L, seed=seed, empty_types=(3,), hub=(2, 150))
    adjs[0] = np.concatenate([adjs[0], np.array([[1, V - 1], [2, V - 1], [5, V - 1]], dtype=np.int32)])  # a node fed by type 0 alone
    adjs[1] = np.concatenate([adjs[1], adjs[1][:7], np.array([[4, 4], [4, 4]], dtype=np.int32)])  # duplicates, self loops
    return adjs, V, L


@pytest.mark.parametrize("normalize,mode", COMBOS)
def test_all_zero_rates_reduce_to_todays_scales(normalize, mode):
    adjs, V, L = _graph()
    got = ref.scales(adjs, V, [0.0] * L, seed=11, epoch=4, normalize=normalize, mode=mode)
    assert got.keep.all()
    # today's scales, stated directly with loops
    E = sum(a.shape[0] for a in adjs)
    cnt = np.zeros((V, L), dtype=np.int64)
    for l, a in enumerate(adjs):
        for _, v in a:
            cnt[v, l] += 1
    N = cnt.sum(axis=1)
    one = np.float32(1.0)
    m = np.array([one if mode == 0 else one / np.float32(max(n, 1)) if mode == 1 else one / np.sqrt(np.float32(max(n, 1)))
                  for n in N], dtype=np.float32)
    s, s_src, e = np.zeros(E, np.float32), np.zeros(E, np.float32), 0
    for l, a in enumerate(adjs):
        for _, v in a:
            s[e] = one / (np.float32(cnt[v, l]) + np.float32(1e-7)) if normalize else one
            s_src[e] = s[e] * m[v]
            e += 1
    assert np.array_equal(got.node_scale, m) and np.array_equal(got.s, s) and np.array_equal(got.s_src, s_src)
    pm, ps, pss = ref.plain_scales(adjs, V, normalize, mode)
    assert np.array_equal(pm, m) and np.array_equal(ps, s) and np.array_equal(pss, s_src)
    assert np.array_equal(got.c, cnt) and np.array_equal(got.n, N)


def test_per_type_rates_select_per_type_thresholds():
    adjs, V, L = _graph()
    rates = [0.2, 0.4, 0.0, 0.5, 0.9]
    seed, epoch = 77, 3
    per = [a.shape[0] for a in adjs]
    keep = ref.keep_edges(per, rates, seed, epoch)
    first = 0
    for l, n in enumerate(per):
        k = dr.key(seed, rates[l], epoch)
        assert k.threshold == dr.threshold(rates[l])
        for e in range(first, first + n, max(1, n // 17)):  # element e of the mask drawn for (seed, rate of e's type)
            assert keep[e] == bool(dr.keep(seed, rates[l], epoch, e, 1)[0])
            number = dr.lane_numbers(dr.group_words(k, e >> 2, 1))[0, e & 3]
            assert keep[e] == (int(number) >= k.threshold)
        first += n
    t = ref.edge_types(adjs)
    assert keep[t == 2].all()  # rate 0 keeps every edge of the type
    frac = [keep[t == l].mean() for l in (0, 1, 4)]
    assert abs(frac[0] - 0.8) < 0.15 and abs(frac[1] - 0.6) < 0.15 and frac[2] < 0.3
    # another epoch and another seed are other draws; the same arguments the same draw
    assert not np.array_equal(keep, ref.keep_edges(per, rates, seed, epoch + 1))
    assert not np.array_equal(keep, ref.keep_edges(per, rates, seed + 1, epoch))
    assert np.array_equal(keep, ref.keep_edges(per, rates, seed, epoch))


@pytest.mark.parametrize("normalize,mode", COMBOS)
def test_dropped_steps_count_kept_edges_and_stay_finite(normalize, mode):
    adjs, V, L = _graph()
    rates = [0.999, 0.0, 0.999, 0.999, 0.999]
    r = ref.scales(adjs, V, rates, seed=5, epoch=0, normalize=normalize, mode=mode)
    t, tgt = ref.edge_types(adjs), ref.edge_targets(adjs)
    full = np.zeros((V, L), dtype=np.int64)
    np.add.at(full, (tgt, t), 1)
    assert ((full > 0) & (r.c == 0)).any(), "no bucket lost every edge"
    assert ((full.sum(axis=1) > 0) & (r.n == 0)).any(), "no node lost every edge"
    for a in (r.node_scale, r.s, r.s_src):
        assert a.dtype == np.float32 and np.isfinite(a).all()
    assert np.all(r.node_scale[r.n == 0] == 1.0) and np.all(r.s[~r.keep] == 0.0) and np.all(r.s_src[~r.keep] == 0.0)
    assert np.array_equal(r.s != 0, r.keep) and np.array_equal(r.s_src != 0, r.keep)
    # where a count divides it is the kept count; where none does kept edges carry 1 / (1 - p)
    k = r.keep
    if normalize:
        assert np.array_equal(r.s[k], (np.float32(1) / (r.c[tgt[k], t[k]].astype(np.float32) + np.float32(1e-7))))
    elif mode == 0:
        assert np.array_equal(r.s[k], np.array([dr.scale(x) for x in rates], dtype=np.float32)[t[k]])
        assert dr.scale(0.0) == 1.0
    else:
        assert np.all(r.s[k] == 1.0)
    if mode == 1:
        assert np.array_equal(r.node_scale, np.float32(1) / np.maximum(r.n, 1).astype(np.float32))
    # the kept values are today's scales of the graph made of the kept edges
    filtered, first = [], 0
    for a in adjs:
        filtered.append(a[k[first:first + a.shape[0]]])
        first += a.shape[0]
    m2, s2, ss2 = ref.plain_scales(filtered, V, normalize, mode)
    assert np.array_equal(m2, r.node_scale)
    if normalize or mode != 0:
        assert np.array_equal(s2, r.s[k]) and np.array_equal(ss2, r.s_src[k])


def _params(name, **over):
    from tf2_gnn_amd.layers import get_message_passing_class

    cls = get_message_passing_class(name)
    return cls, dict(cls.get_default_hyperparameters(), **over)


@pytest.mark.parametrize("name", ["rgcn_basis", "rgcn_blockdiag"])
def test_hyperparameter_validation(name):
    from tf2_gnn_amd.layers import MessagePassingInput
    from tf2_gnn_amd.layers.message_passing import set_default_device

    cls, hp = _params(name)
    assert "edge_dropout_rate" not in hp and cls.supports_edge_dropout  # absent = 0.0: no defaults dictionary changes
    for bad in (1.0, -0.1, float("nan"), [0.2, 1.0], [0.2, -1e-3]):
        with pytest.raises(ValueError, match=r"edge_dropout_rate"):
            cls(dict(hp, edge_dropout_rate=bad))
    shapes = MessagePassingInput((None, 8), tuple((None, 2) for _ in range(4)))
    set_default_device("cpu")
    try:
        with pytest.raises(ValueError, match=r"3 rates for 4 edge types"):
            cls(dict(hp, edge_dropout_rate=[0.2, 0.4, 0.4], hidden_dim=8)).build(shapes)
        layer = cls(dict(hp, edge_dropout_rate=[0.2, 0.4, 0.4, 0.0], hidden_dim=8))
        layer.build(shapes)
        assert layer._edge_dropout_rates.dtype.is_floating_point and layer._edge_dropout_rates.tolist() == pytest.approx([0.2, 0.4, 0.4, 0.0])
        assert layer.edge_dropout_seed == 0
        uniform = cls(dict(hp, edge_dropout_rate=0.5, hidden_dim=8))
        uniform.build(shapes)
        assert uniform._edge_dropout_rates.tolist() == [0.5] * 4
        off = cls(dict(hp, hidden_dim=8))
        off.build(shapes)
        assert off._edge_dropout_rates is None
        zeros = cls(dict(hp, edge_dropout_rate=[0.0] * 4, hidden_dim=8))
        zeros.build(shapes)
        assert zeros._edge_dropout_rates is None
        from tf2_gnn_amd import ops

        # the dropped step's part is named with the layer's others, and only by a layer that drops
        assert layer.graph_parts(10, [1] * 4, 8) == off.graph_parts(10, [1] * 4, 8) | ops.G_PART_EDGE_MAPS
        assert not off.graph_parts(10, [1] * 4, 8) & ops.G_PART_EDGE_MAPS
    finally:
        set_default_device(None)


@pytest.mark.parametrize("name", ["rgcn", "rgat", "ggnn", "rgin", "gnn_edge_mlp", "gnn_film"])
def test_layers_that_do_not_support_it_refuse_a_non_zero_rate(name):
    cls, hp = _params(name)
    assert "edge_dropout_rate" not in hp and not cls.supports_edge_dropout
    cls(hp)  # no key: as before
    cls(dict(hp, edge_dropout_rate=0.0))
    cls(dict(hp, edge_dropout_rate=[0.0, 0.0]))
    for rate in (0.4, [0.0, 0.2]):
        with pytest.raises(ValueError, match=r"RGCN_Basis and RGCN_BlockDiag"):
            cls(dict(hp, edge_dropout_rate=rate))


def test_the_rate_reaches_the_layers_of_a_task_model_as_a_gnn_hyperparameter():
    from tf2_gnn_amd.layers import GNN
    from tf2_gnn_amd.tasks import LinkPredictionTask

    for name in ("rgcn_basis", "rgcn_blockdiag"):
        params = LinkPredictionTask.get_default_hyperparameters(name)
        assert "gnn_edge_dropout_rate" not in params  # absent = 0.0
        params["gnn_edge_dropout_rate"] = [0.2, 0.4]
        graph_params = {k[4:]: v for k, v in params.items() if k.startswith("gnn_")}  # what GraphTaskModel hands its GNN
        assert graph_params["edge_dropout_rate"] == [0.2, 0.4]
        layer = GNN(graph_params)._message_passing_class(graph_params)
        assert layer._edge_dropout_rate == (0.2, 0.4)


def test_the_symbol_is_declared_bound_and_refuses_null_arguments_and_the_abi_stays_5():
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name), name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in text
    assert lib.tfgnn_graph_scales_edge_dropout(None, 1, 1, None, 0, None, None, None, None) == -1
    assert "graph is NULL" in lib.tfgnn_last_error().decode()
    buf = (ctypes.c_int64 * 3)(-1, -1, -1)
    assert lib.tfgnn_edge_dropout_launch_counts(buf, 3) == 0 and buf[0] >= 0 and buf[1] == 0 and buf[2] == 0
    assert lib.tfgnn_edge_dropout_launch_counts(None, 1) == -1
    assert set(ops.edge_dropout_launch_counts()) == {"edge_dropout_scales"}
