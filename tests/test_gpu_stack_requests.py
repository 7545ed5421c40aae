"""What the layer stack asks of a message-passing layer - write the output split as well, apply the next layer's input dropout,
write the input gradient split as well - travels as arguments of ``call_with_epilogue`` / ``backward_with_epilogue`` and comes
back as a return value: a step leaves no attribute on a layer, and a layer call that raises leaves no request behind."""
import pytest
import torch

from tests.helpers import random_graph, to_dev

pytestmark = pytest.mark.gpu


def _stack(mp_style, dev, over, V=600, E=7000, L=3, Din=64, seed=17):
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers import GNN, GNNInput
    from tf2_gnn_amd.layers.message_passing import set_seed

    assert ops.get_gemm_mode() == ops.GEMM_F16X2
    p = GNN.get_default_hyperparameters(mp_style)
    p.update({"num_layers": 4, "hidden_dim": 128, "layer_input_dropout_rate": 0.2, "global_exchange_every_num_layers": 10000})
    if mp_style == "rgat":
        p["num_heads"] = 4
    p.update(over)
    set_seed(seed)
    gnn = GNN(p)
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn((V, Din), generator=gen).to(dev)
    dOut = torch.randn((V, 128), generator=gen).to(dev)
    adj = to_dev(random_graph(V, E, L, seed=seed, hub=(2, 100)), dev)
    return gnn, GNNInput(X, adj, torch.zeros(V, dtype=torch.int32, device=dev), 1), dOut


@pytest.mark.parametrize("mp_style", ["rgcn", "ggnn", "rgat", "rgin"])
def test_a_training_step_adds_no_attribute_to_a_layer(dev, mp_style):
    gnn, inp, dOut = _stack(mp_style, dev, {})
    gnn(inp, training=False)  # builds the layers
    before = [set(vars(mp)) for mp in gnn._mp_layers]
    gnn(inp, training=True)
    gnn.backward(dOut, need_input_grad=True)
    torch.cuda.synchronize()
    assert [set(vars(mp)) for mp in gnn._mp_layers] == before


def test_a_failed_layer_call_leaves_no_request_behind(dev, monkeypatch):
    """Layer 1 of this stack (no Dense behind it, no residual sum at layer 2) is asked to apply layer 2's input dropout in its
    product's epilogue.  When its forward pass raises after the stack has formed that request, a later stand-alone call of the
    layer in eval mode must give what it gave before: no dropout."""
    from tf2_gnn_amd import ops
    from tf2_gnn_amd.layers import MessagePassingInput

    gnn, inp, _ = _stack("rgcn", dev, {"residual_every_num_layers": 4, "dense_every_num_layers": 2,
                                       "use_target_state_as_input": False, "num_edge_MLP_hidden_layers": 0})
    gnn(inp, training=False)  # builds the layers
    gnn(inp, training=True)
    fused = [bool(st.get("drop_by_producer")) for st in gnn._ctx["steps"]]
    assert fused[2], fused  # an undisturbed step: layer 1 drops layer 2's input
    assert gnn.dropout_masks()[2] is not None
    layer = gnn._mp_layers[1]
    H = torch.randn((inp.node_features.shape[0], 128), generator=torch.Generator().manual_seed(3)).to(dev)
    alone = MessagePassingInput(H, inp.adjacency_lists)
    before = layer(alone, training=False).clone()

    real, raised = ops.mp_forward, []

    def failing_once(*args, **kwargs):
        if kwargs.get("dropout") is not None and not raised:  # the call that carries the stack's request
            raised.append(1)
            raise RuntimeError("injected failure of the layer's forward product")
        return real(*args, **kwargs)

    monkeypatch.setattr(ops, "mp_forward", failing_once)
    with pytest.raises(RuntimeError, match="injected failure"):
        gnn(inp, training=True)
    assert raised
    after = layer(alone, training=False)
    torch.cuda.synchronize()
    assert torch.equal(after, before)
