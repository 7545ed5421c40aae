"""R-GCN with block-diagonal decomposition (Schlichtkrull et al. 2018, "Modeling Relational Data with Graph Convolutional
Networks", eq. 4) - the paper's regulariser for link prediction on graphs with many relation types (FB15k-237: 5x5 blocks)."""
from typing import Any, Dict

import torch

from ... import ops
from .message_passing import (
    MessagePassing,
    MessagePassingInput,
    default_device,
    get_graph,
    glorot_uniform,
    register_message_passing_implementation,
)

_SUM_LIKE = ("sum", "mean", "sqrt_n")


@register_message_passing_implementation
class RGCN_BlockDiag(MessagePassing):
    """Compute new graph states by neural message passing with block-diagonal kernels:
        h^{t+1}_v := sigma( sum_l sum_{(u,v) in A_l} W_l h^t_u / c_{v,l} ),   W_l = blockdiag(Q_l^0 .. Q_l^{C-1})
    with C = ``num_blocks`` blocks Q_l^c [D/C, H/C] per edge type: L*D*H/C parameters instead of L*D*H.

    The blocks are applied inside the neighbour walk, once per run of one edge type (csrc/blockdiag.hip): no [V, L*D] operand,
    no per-edge message, no product.  That only commutes with sum-like aggregation (sum, mean, sqrt_n) and an activation
    applied after it.  Block widths D/C and H/C of at most 64.

    Weight: ``block_kernels`` [L, D/C, H], the blocks banded: W_l[c*di + i, c*ho + j] = block_kernels[l, i, c*ho + j]."""

    supports_edge_dropout = True

    @classmethod
    def get_default_hyperparameters(cls):
        these_hypers = {
            "num_blocks": 4,
            "normalize_by_num_incoming": True,
        }
        mp_hypers = super().get_default_hyperparameters()
        mp_hypers.update(these_hypers)
        return mp_hypers

    def __init__(self, params: Dict[str, Any], **kwargs):
        super().__init__(params, **kwargs)
        self._num_blocks = int(params["num_blocks"])
        self._normalize_by_num_incoming: bool = bool(params["normalize_by_num_incoming"])
        why = ("applying the blocks after the run sum only commutes with sum-like aggregation (sum, mean, sqrt_n) applied before "
               "the activation")
        if self._aggregation_name not in _SUM_LIKE:
            raise ValueError(f"RGCN_BlockDiag: aggregation_function {self._aggregation_name!r} is not supported: {why}")
        if self._message_activation_before_aggregation:
            raise ValueError(f"RGCN_BlockDiag: message_activation_before_aggregation=True is not supported: {why}")
        if self._num_blocks < 1:
            raise ValueError(f"RGCN_BlockDiag: num_blocks must be at least 1, got {self._num_blocks}: {why}")
        self._qb = None  # [L, di, H]
        self._block_kernels = None
        self._num_edge_types = None
        self._in_dim = None

    def graph_parts(self, num_nodes: int, edges_per_type, in_dim: int) -> int:
        # the node views' plans (csrc/blockdiag.hip) and the edge ids the weight gradient's type-major table inverts; the typed
        # plans stay named as the part every stack builds
        return ops.G_PART_PLAN_TYPED | ops.G_PART_PLAN_NODE | ops.G_PART_EDGE_IDS | self._edge_dropout_parts()

    def build(self, input_shapes: MessagePassingInput):
        D = int(input_shapes.node_embeddings[-1])
        L = len(input_shapes.adjacency_lists)
        H, C = self._hidden_dim, self._num_blocks
        if D % C or H % C:
            raise ValueError(f"RGCN_BlockDiag: num_blocks = {C} must divide the input width {D} and the hidden width {H}")
        di, ho = D // C, H // C
        self._num_edge_types, self._in_dim = L, D
        # Glorot-uniform per block [di, ho]: limit sqrt(6 / (di + ho))
        self._qb = glorot_uniform((L, di, H), fan_in=di, fan_out=ho, device=default_device())
        self._block_kernels = self.add_weight("block_kernels", self._qb)
        self._build_edge_dropout(L)
        super().build(input_shapes)

    def dense_kernels(self) -> torch.Tensor:
        """The composed kernels W_l [L, D, H] (zeros off the blocks), for inspection and tests."""
        L, di, H = self._qb.shape
        C = self._num_blocks
        ho = H // C
        W = self._qb.new_zeros((L, C * di, H))
        for c in range(C):
            W[:, c * di:(c + 1) * di, c * ho:(c + 1) * ho] = self._qb[:, :, c * ho:(c + 1) * ho]
        return W

    def _message_function(self, edge_source_states, edge_target_states, num_incoming_to_node_per_message,
                          edge_type_idx, training):
        raise NotImplementedError(
            "RGCN_BlockDiag applies the blocks inside the neighbour walk on the bucketed graph (csrc/blockdiag.hip); the per-edge "
            "form is RGCN's with W_l = dense_kernels()[l] (oracle/tf2gnn_oracle.py)"
        )

    _message_function._tfgnn_builtin = True

    def call(self, inputs: MessagePassingInput, training: bool = False):
        if not getattr(type(self)._message_function, "_tfgnn_builtin", False):
            raise NotImplementedError(
                f"{type(self).__name__} overrides RGCN_BlockDiag._message_function: the layer never forms per-edge messages, "
                "override call() and backward() as well"
            )
        X = inputs.node_embeddings
        V, D = X.shape
        g = get_graph(inputs.adjacency_lists, V)
        if g.num_edge_types != self._num_edge_types:
            raise ValueError(f"layer was built for {self._num_edge_types} edge types, got {g.num_edge_types}")
        if D != self._in_dim:
            raise ValueError(f"layer was built for inputs of width {self._in_dim}, got {D}")
        scales = self._step_scales(g, self._normalize_by_num_incoming, training)
        pre = ops.blockdiag_forward(g, self._qb, X, self._num_blocks, edge_weight=scales.edge_weight_by_dst,
                                    node_scale=scales.node_scale)
        act = self._activation_name
        out = pre if act is None else ops.activation_forward(act, pre)
        # gelu's derivative needs the raw output, the others the activated one
        self._ctx = {"graph": g, "X": X, "scales": scales, "fused_act": act, "saved": pre if act == "gelu" else out}
        return out

    def activation_backward_spec(self):
        return None  # backward() applies the derivative itself; the stack's generic epilogue handles the rest

    def backward(self, grad_output: torch.Tensor) -> torch.Tensor:
        """d(loss)/d(out) -> d(loss)/d(node_embeddings); fills the block kernels' gradient."""
        ctx = self._ctx
        if ctx is None:
            raise RuntimeError("backward called before a forward pass")
        g, X, scales, act = ctx["graph"], ctx["X"], ctx["scales"], ctx["fused_act"]
        d_pre = grad_output
        if act is not None:
            d_pre = ops.activation_backward(act, grad_output, ctx["saved"])
        dX, dQb = ops.blockdiag_backward(g, self._qb, d_pre, X, self._num_blocks, edge_weight_by_dst=scales.edge_weight_by_dst,
                                         edge_weight_by_src=scales.edge_weight_by_src, node_scale=scales.node_scale)
        self._block_kernels.grad = dQb
        return dX
