"""Vocabulary embeddings as far as they go without a device: the new symbols, the refusals of the C entries before any HIP
call, and the validation of ``node_vocabulary_size``.  On the device: tests/test_gpu_vocab_embedding.py."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NEW = ("tfgnn_vocab_embedding_workspace_bytes", "tfgnn_vocab_embedding_forward", "tfgnn_vocab_embedding_backward",
       "tfgnn_vocab_embedding_launch_counts")


def test_symbols_and_abi():
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    text = (ROOT / "include" / "tfgnn.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTED_SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    assert _lib.ABI_VERSION == 5 and lib.tfgnn_abi_version() == 5 and "#define TFGNN_ABI_VERSION 5" in text
    assert all(isinstance(c, int) for c in ops.vocab_embedding_launch_counts())
    # one sort pass up to 511 ids, two from 512: the second pass needs no more memory, a longer batch does
    size = lib.tfgnn_vocab_embedding_workspace_bytes
    assert 0 < size(1000, 511) and size(1000, 5) < size(100000, 5) and size(1000, 5) < size(1000, 100000)
    assert size(1000, 0) == 0 and size(2 ** 31, 5) == 0 and size(5, 2 ** 31) == 0
    assert _lib.vocab_embedding_partial_rows(257) == 4


def test_refusals_before_any_hip_call():
    from tf2_gnn_amd import _lib, ops

    lib = _lib.load()
    before = ops.vocab_embedding_launch_counts()
    TABLE, IDS, OUT, WS = 0x10000, 0x20000, 0x30000, 0x40000  # made-up device addresses: the checks never read them
    fwd = dict(n=5, N=10, D=8, table=TABLE, ld_table=8, ids_i32=IDS, ids_f32=None, ids_pitch=1, out=OUT, ld_out=8,
               workspace=WS, workspace_bytes=1 << 20, bad_flag=None)
    bwd = dict(n=5, N=10, D=8, d_rows=TABLE, ld_rows=8, workspace=WS, workspace_bytes=1 << 20, partials=None, partials_bytes=0,
               table_grad=OUT, ld_grad=8)

    def refused(cls, fn, good, match, status=-1, **over):
        a = cls(**dict(good, **over))
        a.struct_size = over.get("struct_size", ctypes.sizeof(cls))
        assert fn(ctypes.byref(a), None) == status, over
        assert match in lib.tfgnn_last_error(), (over, lib.tfgnn_last_error())

    F = (_lib.VocabEmbeddingForwardArgs, lib.tfgnn_vocab_embedding_forward, fwd)
    B = (_lib.VocabEmbeddingBackwardArgs, lib.tfgnn_vocab_embedding_backward, bwd)
    for entry in (F, B):
        refused(*entry, b"struct of another size", struct_size=8)
        refused(*entry, b"negative size", n=-1)
        refused(*entry, b"2^31 or more", N=2 ** 31)
        refused(*entry, b"2^31 or more", n=2 ** 31)
        refused(*entry, b"D must be in [1, 2^31)", D=0)
        refused(*entry, b"empty vocabulary", N=0)
        refused(*entry, b"too small or misaligned", workspace_bytes=16)
    refused(*F, b"pitch below D", ld_out=7)
    refused(*F, b"exactly one of", ids_f32=IDS)
    refused(*F, b"exactly one of", ids_i32=None)
    refused(*F, b"float ids need N <= 2^24", ids_i32=None, ids_f32=IDS, N=2 ** 24 + 1, workspace_bytes=1 << 30)
    refused(*B, b"pitch below D", ld_grad=7)
    refused(*B, b"partials too small", n=257)
    # n == 0 is legal and the forward call launches nothing for it
    a = _lib.VocabEmbeddingForwardArgs(**dict(fwd, n=0, ids_i32=None, workspace=None))
    a.struct_size = ctypes.sizeof(a)
    assert lib.tfgnn_vocab_embedding_forward(ctypes.byref(a), None) == 0 and ops.vocab_embedding_launch_counts() == before


def test_node_vocabulary_size_validation():
    import torch

    from tf2_gnn_amd.layers.message_passing.message_passing import set_default_device
    from tf2_gnn_amd.tasks import GraphTaskModel, NodeMulticlassTask

    def params(**over):
        p = NodeMulticlassTask.get_default_hyperparameters("rgcn")
        p.update({"gnn_hidden_dim": 8, "gnn_num_layers": 2})
        p.update(over)
        return p

    kw = dict(num_edge_types=2, num_node_target_labels=3)
    assert "node_vocabulary_size" not in GraphTaskModel.get_default_hyperparameters()
    with pytest.raises(ValueError, match="node_vocabulary_size is set without node_embedding_dim"):
        NodeMulticlassTask(params(node_vocabulary_size=5), **kw)
    for bad in (0, -1, 2.5, True, "5", 2 ** 31):
        with pytest.raises(ValueError, match="node_vocabulary_size must be an integer"):
            NodeMulticlassTask(params(node_vocabulary_size=bad, node_embedding_dim=4), **kw)
    with pytest.raises(ValueError, match='node_embedding_update="rows" with node_vocabulary_size'):
        NodeMulticlassTask(params(node_vocabulary_size=5, node_embedding_dim=4, node_embedding_update="rows"), **kw)
    set_default_device("cpu")
    try:
        for size in (None, 5):
            over = {"node_vocabulary_size": size}
            if size is None:  # off: the transductive table, which still needs num_nodes
                with pytest.raises(ValueError, match=r"dataset\.num_nodes.*num_nodes="):
                    NodeMulticlassTask(params(node_embedding_dim=4, **over), **kw)
                continue
            model = NodeMulticlassTask(params(node_embedding_dim=4, **over), **kw)  # num_nodes is not asked for
            model.build({"node_features": (None, 1)})
            table = model.trainable_variables[-1]
            assert table.name == "NodeMulticlassTask/node_embeddings" and table.shape == (5, 4)
            batch = {"node_features": torch.zeros(6, 2), "node_to_graph_map": torch.zeros(6, dtype=torch.int32)}
            with pytest.raises(ValueError, match=r"node_features \[V, 1\], not from \(6, 2\)"):
                model.compute_initial_node_features(batch, training=False)
    finally:
        set_default_device(None)
