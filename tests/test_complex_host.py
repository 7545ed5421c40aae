"""The ComplEx decoder (tfgnn_complex_*, LinkPredictionTask link_decoder="complex") as far as it goes without a device:
header, symbols and binding, workspace sizes, the argument checks of the three calls (all before any launch, the DistMult
counters untouched), the ops wrappers' refusals, the task's ValueErrors, its unchanged defaults, the relation variable and a
checkpoint round trip.  CPU-only; the arithmetic is checked on the GPU (tests/test_gpu_complex.py,
tests/test_gpu_link_prediction_complex.py)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tf2_gnn_amd import tasks
from tf2_gnn_amd.layers.message_passing import set_default_device
from tf2_gnn_amd.utils import model_utils as mu

ROOT = Path(__file__).resolve().parent.parent
NEW = ["tfgnn_complex_ce_workspace_bytes", "tfgnn_complex_ce_metrics", "tfgnn_complex_backward_workspace_bytes",
       "tfgnn_complex_backward", "tfgnn_complex_rank_workspace_bytes", "tfgnn_complex_rank", "tfgnn_complex_launch_counts"]


@pytest.fixture
def cpu_params():
    set_default_device("cpu")
    yield
    set_default_device(None)


def _counts(lib):
    """-> (the three ComplEx counters, the three DistMult counters); further slots of either call are 0"""
    c, d = (ctypes.c_int64 * 5)(), (ctypes.c_int64 * 4)()
    assert lib.tfgnn_complex_launch_counts(c, 5) == 0 and lib.tfgnn_link_launch_counts(d, 4) == 0
    assert c[3] == 0 and c[4] == 0 and d[3] == 0
    return list(c)[:3], list(d)[:3]


def test_header_symbols_and_binding_agree():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in header
    # the namesakes' parameter lists, word for word (the rank workspace size also takes D)
    decl = lambda name: re.sub(r"\s+", " ", re.search(rf"\b{name}\s*\(([^)]*)\)", header).group(1))
    for call in ("ce_workspace_bytes", "ce_metrics", "backward_workspace_bytes", "backward", "rank"):
        assert decl(f"tfgnn_complex_{call}") == decl(f"tfgnn_distmult_{call}"), call
    assert decl("tfgnn_complex_rank_workspace_bytes") == "int64_t Q, int64_t D"
    assert decl("tfgnn_complex_launch_counts") == decl("tfgnn_link_launch_counts")
    # the contract is written down: the layout, the operation orders, the query vectors
    for phrase in ("HALVES", "must be even", "fma(r_re, x, p)", "QUERY", "acc_re = fma(gr, y_re, acc_re)", "PARITY"):
        assert phrase in text, phrase
    assert lib.tfgnn_complex_launch_counts(None, 1) == -1


def test_workspace_sizes():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    assert lib.tfgnn_complex_ce_workspace_bytes() == lib.tfgnn_distmult_ce_workspace_bytes() >= 8
    # backward: one wave ("item") per 128 list positions, 2 N node entries and N relation positions, D floats each
    assert lib.tfgnn_complex_backward_workspace_bytes(257, 6) == (5 + 3) * 6 * 4
    assert lib.tfgnn_complex_backward_workspace_bytes(1, 1024) == 2 * 1024 * 4
    for N, D in ((0, 8), (2 ** 30 + 1, 8), (8, 0), (8, 1), (8, 7), (8, 1025), (8, 1026), (8, -2)):
        assert lib.tfgnn_complex_backward_workspace_bytes(N, D) == 0, (N, D)
    # rank: one query vector [D] and one true score per query
    assert lib.tfgnn_complex_rank_workspace_bytes(17, 6) == 17 * 7 * 4
    assert lib.tfgnn_complex_rank_workspace_bytes(1, 2) == 12
    assert lib.tfgnn_complex_rank_workspace_bytes(2 ** 30, 1024) == 2 ** 30 * 1025 * 4
    for Q, D in ((0, 8), (-1, 8), (2 ** 30 + 1, 8), (4, 0), (4, 1), (4, 129), (4, 1026)):
        assert lib.tfgnn_complex_rank_workspace_bytes(Q, D) == 0, (Q, D)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    before = _counts(lib)
    # never dereferenced: every call below is refused before a launch
    P = lambda a: ctypes.c_void_p(a)
    H, R, tr, y, w, m, ws, g, dH, dR, t0, t1, t2, t3 = (P(0x1000 * (i + 1)) for i in range(14))
    big = 1 << 20

    def ce(H=H, ldh=8, R=R, tr=tr, y=y, ldy=1, w=None, ldw=0, V=5, T=2, N=4, D=8, m=m, ws=ws, nbytes=big):
        return lib.tfgnn_complex_ce_metrics(H, ldh, R, tr, y, ldy, w, ldw, V, T, N, D, m, None, None, None, ws, nbytes, None)

    def bwd(H=H, ldh=8, R=R, tr=tr, g=g, t0=t0, t1=t1, t2=t2, t3=t3, V=5, T=2, N=4, D=8, dH=dH, ldd=8, dR=dR, ws=ws, nbytes=big):
        return lib.tfgnn_complex_backward(H, ldh, R, tr, g, t0, t1, t2, t3, V, T, N, D, dH, ldd, 0, dR, ws, nbytes, None)

    def rank(H=H, ldh=8, R=R, q=tr, Q=4, side=0, fo=None, fi=None, V=5, T=2, D=8, gt=dH, eq=dR, ws=ws, nbytes=big):
        return lib.tfgnn_complex_rank(H, ldh, R, q, Q, side, fo, fi, V, T, D, gt, eq, ws, nbytes, None)

    def refused(status, text):
        assert status == -1
        assert text in lib.tfgnn_last_error(), lib.tfgnn_last_error()
        assert b"complex_" in lib.tfgnn_last_error()

    for call in (ce, bwd):
        refused(call(N=0), b"empty batch")
        refused(call(N=-2), b"empty batch")
        refused(call(N=2 ** 30 + 1), b"2^30")
    refused(rank(Q=0), b"empty batch")
    refused(rank(Q=2 ** 30 + 1), b"2^30")
    for call in (ce, bwd, rank):
        refused(call(D=7), b"even")
        refused(call(D=1023, ldh=2048), b"even")
        refused(call(D=0), b"width D")
        refused(call(D=1), b"width D")
        refused(call(D=1026, ldh=2048), b"width D")
        refused(call(V=0), b"V and T")
        refused(call(T=0), b"V and T")
        refused(call(V=2 ** 31), b"V and T")
        refused(call(ldh=7), b"leading dimension of H")
        refused(call(H=None), b"NULL")
        refused(call(R=None), b"NULL")
        refused(call(ws=None), b"workspace")
        refused(call(nbytes=3), b"workspace")
    refused(ce(tr=None), b"NULL")
    refused(ce(y=None), b"NULL")
    refused(ce(m=None), b"NULL")
    refused(ce(ldy=0), b"stride")
    refused(ce(w=w, ldw=0), b"stride")
    refused(ce(ws=P(0x9004)), b"workspace")
    refused(bwd(g=None), b"NULL")
    refused(bwd(dH=None, dR=None), b"NULL")
    refused(bwd(t1=None), b"tables")
    refused(bwd(t2=None), b"tables")
    refused(bwd(ldd=7), b"leading dimension of dH")
    refused(bwd(ws=P(0x9002)), b"workspace")
    refused(rank(side=2), b"side")
    refused(rank(gt=None), b"NULL")
    refused(rank(fo=t0), b"filter")
    refused(rank(fi=t0), b"filter")
    refused(rank(nbytes=4 * 4 * 9 - 1), b"workspace")  # Q (D + 1) floats, not the Q floats of the DistMult call
    assert _counts(lib) == before  # nothing was launched, by either decoder's entries
    with pytest.raises(ValueError, match="even"):
        _lib.check(ce(D=3))


def test_ops_wrappers_refuse_cpu_tensors_odd_widths_and_bad_triples():
    from tf2_gnn_amd import ops

    H, R = torch.zeros(5, 4), torch.zeros(2, 4)
    tr = np.array([[0, 1, 4]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.complex_ce_metrics(H, R, tr, torch.zeros(1))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.complex_backward(H, R, tr, torch.zeros(1), {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.complex_rank(H, R, tr)
    with pytest.raises(ValueError, match="corrupt"):
        ops.complex_rank(H, R, tr, corrupt="both")
    H3, R3 = torch.zeros(5, 3), torch.zeros(2, 3)
    with pytest.raises(ValueError, match="even"):
        ops.complex_ce_metrics(H3, R3, tr, torch.zeros(1))
    with pytest.raises(ValueError, match="even"):
        ops.complex_backward(H3, R3, tr, torch.zeros(1), {})
    with pytest.raises(ValueError, match="even"):
        ops.complex_rank(H3, R3, tr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # DistMult takes any width: it gets as far as the device check
        ops.distmult_ce_metrics(H3, R3, tr, torch.zeros(1))
    assert sorted(ops.complex_launch_counts()) == ["complex_bwd", "complex_fwd", "complex_rank"]
    assert sorted(ops.link_launch_counts()) == ["distmult_bwd", "distmult_fwd", "distmult_rank"]
    assert ops.LINK_DECODERS == ("distmult", "complex")


def test_task_decoder_choice_and_unchanged_defaults():
    defaults = tasks.LinkPredictionTask.get_default_hyperparameters("rgcn")
    assert defaults == tasks.GraphTaskModel.get_default_hyperparameters("rgcn") and "link_decoder" not in defaults
    assert tasks.LinkPredictionTask(defaults, num_edge_types=1, num_relations=1).link_decoder == "distmult"
    p = dict(defaults, gnn_hidden_dim=12, link_decoder="complex")
    assert tasks.LinkPredictionTask(p, num_edge_types=1, num_relations=1).link_decoder == "complex"
    assert tasks.LinkPredictionTask(dict(p, link_decoder="distmult"), num_edge_types=1, num_relations=1).link_decoder == "distmult"
    with pytest.raises(ValueError, match="'distmult' or 'complex'"):
        tasks.LinkPredictionTask(dict(p, link_decoder="transe"), num_edge_types=1, num_relations=1)
    with pytest.raises(ValueError, match="'distmult' or 'complex'"):
        tasks.LinkPredictionTask(dict(p, link_decoder=None), num_edge_types=1, num_relations=1)
    with pytest.raises(ValueError, match="gnn_hidden_dim must be even"):
        tasks.LinkPredictionTask(dict(p, gnn_hidden_dim=13), num_edge_types=1, num_relations=1)
    tasks.LinkPredictionTask(dict(p, gnn_hidden_dim=13, link_decoder="distmult"), num_edge_types=1, num_relations=1)  # any width


def test_relation_embeddings_variable_and_checkpoint_round_trip(cpu_params, tmp_path):
    p = tasks.LinkPredictionTask.get_default_hyperparameters("rgcn")
    p.update(gnn_num_layers=2, gnn_hidden_dim=12, link_decoder="complex")
    model = tasks.LinkPredictionTask(p, num_edge_types=3, num_relations=5)
    model.build({"node_features": (None, 6)})
    names = [v.name for v in model.variables]
    assert len(set(names)) == len(names) and names[-1] == "LinkPredictionTask/relation_embeddings"
    (rel,) = model._task_variables()
    assert tuple(rel.value.shape) == (5, 12) and rel in model.trainable_variables
    limit = (6.0 / (5 + 12)) ** 0.5  # glorot-uniform, as with DistMult
    assert float(rel.value.abs().max()) <= limit and float(rel.value.std()) > 0.2 * limit
    # the same variables as the default decoder: a checkpoint of either loads into the other
    q = dict(p)
    del q["link_decoder"]
    other = tasks.LinkPredictionTask(q, num_edge_types=3, num_relations=5)
    other.build({"node_features": (None, 6)})
    assert [(v.name, tuple(v.value.shape)) for v in other.variables] == [(v.name, tuple(v.value.shape)) for v in model.variables]
    want = {v.name: v.value.clone() for v in model.variables}
    path = str(tmp_path / "link_complex.pkl")
    mu.save_model(path, model)
    saved = mu.load_pickle(path)
    assert saved["model_class"] is tasks.LinkPredictionTask and saved["model_params"]["link_decoder"] == "complex"
    for v in model.variables:
        v.assign(torch.zeros_like(v.value))
    assert sorted(mu.load_weights_verbosely(path, model)) == sorted(names)
    assert all(torch.equal(v.value, want[v.name]) for v in model.variables)
    again = tasks.LinkPredictionTask(saved["model_params"], num_edge_types=3, num_relations=5)
    assert again.link_decoder == "complex"
