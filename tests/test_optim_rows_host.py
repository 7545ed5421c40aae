"""The row-sparse optimizer step as far as it goes without a device: the two new symbols, every host-side rejection of
tfgnn_optimizer_apply_rows through the loaded library with made-up addresses (refused before any HIP call), the validation of
``optim.RowGradient`` and of the hyper-parameter ``node_embedding_update``, and the refusal of ``parallel.allreduce_gradients``.
On the device: tests/test_gpu_optim_rows.py, tests/test_gpu_node_embeddings_rows.py."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
NEW = ("tfgnn_optimizer_rows_workspace_bytes", "tfgnn_optimizer_apply_rows")


def test_symbols_and_abi():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in text
    assert "#define TFGNN_OPT_MAX_ROW_TENSORS 8" in text and _lib.OPT_MAX_ROW_TENSORS == 8
    # the struct, field for field: 11 eight-byte fields on this ABI
    fields = re.search(r"typedef struct tfgnn_opt_row_tensor \{(.*?)\} tfgnn_opt_row_tensor;", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", fields)
    assert names == [f[0] for f in _lib.OptRowTensor._fields_] and ctypes.sizeof(_lib.OptRowTensor) == 88


W, G, IDS, S0, S1, FLAG, STATE, WS = (0x10000 * (i + 1) for i in range(8))  # made-up device addresses: the checks never read them


def _config(kind=2, clip=0, momentum=0.0, workspace=None, workspace_bytes=0, state=STATE):
    from tf2_gnn_amd import _lib

    cfg = _lib.OptConfig()
    cfg.struct_size = ctypes.sizeof(_lib.OptConfig)
    cfg.kind, cfg.clip, cfg.clip_value, cfg.momentum = kind, clip, 1.0, momentum
    cfg.rho, cfg.beta_1, cfg.beta_2, cfg.epsilon, cfg.learning_rate = 0.9, 0.9, 0.999, 1e-7, 0.01
    cfg.state, cfg.workspace, cfg.workspace_bytes = state, workspace, workspace_bytes
    return cfg


def _row_tensor(**over):
    from tf2_gnn_amd import _lib

    good = dict(value=W, ld_value=8, grad_rows=G, ld_grad=8, ids=IDS, n=5, N=10, cols=8, slot0=S0, slot1=S1, bad_flag=FLAG)
    good.update(over)
    t = (_lib.OptRowTensor * 1)()
    for k, v in good.items():
        setattr(t[0], k, v)
    return t


def test_apply_rows_rejections_before_any_hip_call():
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    dense = np.array([[0x90000, 4, 0xA0000, 4, 3, 4, 0xB0000, 0xC0000]], dtype=np.int64)
    before = lib.tfgnn_optimizer_launch_count()

    def refused(match, cfg=None, n_dense=1, n_rows=1, rows=None, **over):
        cfg = cfg if cfg is not None else _config()
        rows = rows if rows is not None else _row_tensor(**over)
        assert lib.tfgnn_optimizer_apply_rows(dense.ctypes.data, n_dense, rows, n_rows, ctypes.byref(cfg), None) == -1, over
        assert match in lib.tfgnn_last_error(), (over, lib.tfgnn_last_error())

    refused(b"negative size", n=-1)
    refused(b"negative size", N=-1, n=0)
    for cols in (0, -3, 2 ** 31):
        refused(b"cols must be in [1, 2^31)", cols=cols, ld_value=2 ** 32, ld_grad=2 ** 31)
    refused(b"2^31 or more table rows", N=2 ** 31)
    refused(b"more rows than the table", n=11)
    refused(b"below the width", ld_value=7)
    refused(b"below the width", ld_grad=7)
    refused(b"below the width", ld_value=-8)
    refused(b"gradient row pitch too large", ld_grad=2 ** 32)
    refused(b"at most 2^31 - 1", n=2 ** 28, N=2 ** 28, cols=8)  # n * cols == 2^31: grad_rows is a tensor of the squared-sum pass
    refused(b"NULL value, gradient rows or ids", value=None)
    refused(b"NULL value, gradient rows or ids", grad_rows=None)
    refused(b"NULL value, gradient rows or ids", ids=None)
    refused(b"NULL slot", slot0=None)  # Adam needs both
    refused(b"NULL slot", slot1=None)
    refused(b"NULL slot", cfg=_config(kind=0, momentum=0.5), slot0=None)  # SGD with momentum: the accumulator
    refused(b"NULL slot", cfg=_config(kind=1, momentum=0.5), slot1=None)  # RMSprop with momentum: both
    refused(b"bad row tensor list", n_rows=-1)
    refused(b"bad row tensor list", n_rows=1, rows=ctypes.c_void_p(None))
    refused(b"row tensors (at most 8", n_rows=9)
    # what tfgnn_optimizer_apply refuses for the config and for the dense tensors
    refused(b"unknown optimizer kind", cfg=_config(kind=7))
    refused(b"NULL or unaligned state", cfg=_config(state=None))
    refused(b"bad tensor list", n_dense=-1)
    bad_dense = dense.copy()
    bad_dense[0, 4] = -3
    dense, good_dense = bad_dense, dense
    refused(b"negative shape")
    dense = good_dense
    # the norm modes: the workspace holds the partial sums of the dense tensors AND of the row gradient
    assert lib.tfgnn_optimizer_rows_workspace_bytes(dense.ctypes.data, 1, _row_tensor(), 1, 0) == 0
    assert lib.tfgnn_optimizer_rows_workspace_bytes(dense.ctypes.data, 1, _row_tensor(), 1, 3) == 2 * 8
    big = _row_tensor(n=3000, N=4000, cols=8)  # 24000 gradient elements: 3 partitions of 8192
    assert lib.tfgnn_optimizer_rows_workspace_bytes(dense.ctypes.data, 1, big, 1, 2) == 4 * 8
    assert lib.tfgnn_optimizer_rows_workspace_bytes(dense.ctypes.data, 1, _row_tensor(n=0), 1, 2) == 1 * 8
    refused(b"workspace of 16 bytes", cfg=_config(clip=3))
    refused(b"workspace of 32 bytes", cfg=_config(clip=2, workspace=WS, workspace_bytes=24), rows=big)
    # slots the kind does not use are nullable, the flag always
    ok_without = _row_tensor(slot0=None, slot1=None, bad_flag=None, n=11, N=10)
    refused(b"more rows than the table", cfg=_config(kind=0), rows=ok_without)  # refused for n > N, not for the slots
    assert lib.tfgnn_optimizer_launch_count() == before


def test_row_gradient_validation():
    from tf2_gnn_amd import RowGradient, optim

    assert optim.RowGradient is RowGradient
    rows, ids = torch.zeros(5, 8), torch.arange(5, dtype=torch.int32)
    g = RowGradient(rows, ids, 10)
    assert g.shape == (10, 8) and g.rows is rows and g.ids is ids and g.num_rows == 10 and g.bad_flag is None
    flag = torch.zeros(1, dtype=torch.int32)
    assert RowGradient(rows, ids, np.int64(5), bad_flag=flag).bad_flag is flag
    assert RowGradient(torch.zeros(0, 3), torch.zeros(0, dtype=torch.int32), 0).shape == (0, 3)
    assert RowGradient(torch.zeros(5, 12)[:, :8], ids, 10).shape == (10, 8)  # pitched rows
    for bad_rows in (torch.zeros(5, 8, dtype=torch.float64), torch.zeros(5), torch.zeros(5, 8, 1), np.zeros((5, 8), np.float32)):
        with pytest.raises(ValueError, match="rows must be a float32"):
            RowGradient(bad_rows, ids, 10)
    for bad_rows in (torch.zeros(8, 5).t(), torch.zeros(5, 0), torch.zeros(1, 8).expand(5, 8)):
        with pytest.raises(ValueError, match="unit stride"):
            RowGradient(bad_rows, torch.arange(bad_rows.shape[0], dtype=torch.int32), 10)
    for bad_ids in (ids.long(), ids.view(5, 1), torch.arange(10, dtype=torch.int32)[::2], [0, 1, 2, 3, 4]):
        with pytest.raises(ValueError, match="ids must be a contiguous int32"):
            RowGradient(rows, bad_ids, 10)
    with pytest.raises(ValueError, match="4 ids for 5 rows"):
        RowGradient(rows, ids[:4], 10)
    for bad_n in (-1, 2 ** 31, 2.5, True, "10"):
        with pytest.raises(ValueError, match="num_rows must be an integer"):
            RowGradient(rows, ids, bad_n)
    with pytest.raises(ValueError, match="5 rows for a table of 4"):
        RowGradient(rows, ids, 4)
    for bad_flag in (torch.zeros(1), torch.zeros(2, dtype=torch.int32), 0):
        with pytest.raises(ValueError, match="bad_flag must be an int32"):
            RowGradient(rows, ids, 10, bad_flag=bad_flag)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the dense form is a device op
        g.to_dense()


def _task_params(task_cls, **over):
    params = task_cls.get_default_hyperparameters("rgcn")
    params.update({"gnn_hidden_dim": 8, "gnn_num_layers": 2})
    params.update(over)
    return params


def test_node_embedding_update_validation():
    from tf2_gnn_amd.tasks import GraphTaskModel, LinkPredictionTask, NodeClassificationTask

    assert "node_embedding_update" not in GraphTaskModel.get_default_hyperparameters()
    assert "node_embedding_update" not in NodeClassificationTask.get_default_hyperparameters("rgcn")
    kw = dict(num_edge_types=2, num_node_classes=3, num_nodes=7)
    make = lambda **over: NodeClassificationTask(_task_params(NodeClassificationTask, **over), **kw)
    assert make(node_embedding_dim=4)._node_embedding_rows is False  # absent: dense
    assert make(node_embedding_dim=4, node_embedding_update=None)._node_embedding_rows is False
    assert make(node_embedding_dim=4, node_embedding_update="dense")._node_embedding_rows is False
    assert make(node_embedding_dim=4, node_embedding_update="rows")._node_embedding_rows is True
    for bad in ("Rows", "sparse", "", 1, True, ["rows"]):
        with pytest.raises(ValueError, match='node_embedding_update must be "dense" or "rows"'):
            make(node_embedding_dim=4, node_embedding_update=bad)
    for value in ("dense", "rows"):
        with pytest.raises(ValueError, match="node_embedding_update is set without node_embedding_dim"):
            make(node_embedding_update=value)
        with pytest.raises(ValueError, match="node_embedding_update is set without node_embedding_dim"):
            LinkPredictionTask(_task_params(LinkPredictionTask, node_embedding_update=value), num_edge_types=3, num_relations=2)


class _Dist:
    """a communicator that fails the test when it is touched"""

    def __getattr__(self, name):
        raise AssertionError(f"dist.{name} was touched")


def test_allreduce_refuses_a_row_gradient_before_any_collective():
    from tf2_gnn_amd import RowGradient
    from tf2_gnn_amd.layers.message_passing.message_passing import Variable
    from tf2_gnn_amd.parallel import allreduce_gradients

    dense, table = Variable("w", torch.zeros(3, 4)), Variable("Task/node_embeddings", torch.zeros(10, 8))
    dense.grad = torch.ones(3, 4)
    table.grad = RowGradient(torch.zeros(5, 8), torch.arange(5, dtype=torch.int32), 10)
    with pytest.raises(ValueError, match=r'Task/node_embeddings.*node_embedding_update="dense"'):
        allreduce_gradients([dense, table], _Dist())
    assert torch.equal(dense.grad, torch.ones(3, 4))  # nothing was scaled or packed
    assert allreduce_gradients([dense, table], None) == 0  # one process: nothing to exchange
