"""R-GCN with basis decomposition (Schlichtkrull et al. 2018, "Modeling Relational Data with Graph Convolutional
Networks", eq. 3) - the R-GCN layer for graphs with many relation types (knowledge graphs: tens to hundreds)."""
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
class RGCN_Basis(MessagePassing):
    """Compute new graph states by neural message passing with shared bases:
        h^{t+1}_v := sigma( sum_l sum_{(u,v) in A_l} W_l h^t_u / c_{v,l} ),   W_l = sum_b a[l,b] V_b
    with B = ``num_bases`` kernels V_b [D, H] shared by all L edge types and one coefficient row a[l, :] per type: B*D*H + L*B
    parameters instead of L*D*H.

    Aggregate first, as RGCN's path A, but over the bases instead of the types (csrc/basis.hip):
        Z[v, b, :] = m_v * sum_{e = (u -> v), type l} s_e * a[l,b] * X[u, :]        one gather, [V, B*D]
        out        = act( Z.reshape(V, B*D) @ [V_0; ...; V_{B-1}] )                 one product, K = B*D
    The operand the gather writes and the product reads is L/B times smaller than RGCN's [V, L*D].  The decomposition only
    commutes with sum-like aggregation (sum, mean, sqrt_n) and an activation applied after it.

    Weights: ``basis_{b}/kernel`` - views of one [B*D, H] buffer - and ``relation_coefficients`` [L, B]."""

    supports_edge_dropout = True

    @classmethod
    def get_default_hyperparameters(cls):
        these_hypers = {
            "num_bases": 8,
            "normalize_by_num_incoming": True,
        }
        mp_hypers = super().get_default_hyperparameters()
        mp_hypers.update(these_hypers)
        return mp_hypers

    def __init__(self, params: Dict[str, Any], **kwargs):
        super().__init__(params, **kwargs)
        self._num_bases = int(params["num_bases"])
        self._normalize_by_num_incoming: bool = bool(params["normalize_by_num_incoming"])
        why = "the basis decomposition only commutes with sum-like aggregation (sum, mean, sqrt_n) applied before the activation"
        if self._aggregation_name not in _SUM_LIKE:
            raise ValueError(f"RGCN_Basis: aggregation_function {self._aggregation_name!r} is not supported: {why}")
        if self._message_activation_before_aggregation:
            raise ValueError(f"RGCN_Basis: message_activation_before_aggregation=True is not supported: {why}")
        if self._num_bases < 1:
            raise ValueError(f"RGCN_Basis: num_bases must be at least 1, got {self._num_bases}: {why}")
        self._bases = None   # [B*D, H]
        self._coeff = None   # [L, B]
        self._basis_kernels = []
        self._coefficients = None
        self._num_edge_types = None

    def graph_parts(self, num_nodes: int, edges_per_type, in_dim: int) -> int:
        # the node views' plans (csrc/basis.hip); the typed plans stay named as the part every stack builds
        return ops.G_PART_PLAN_TYPED | ops.G_PART_PLAN_NODE | self._edge_dropout_parts()

    def build(self, input_shapes: MessagePassingInput):
        D = int(input_shapes.node_embeddings[-1])
        L = len(input_shapes.adjacency_lists)
        H, B = self._hidden_dim, self._num_bases
        dev = default_device()
        self._num_edge_types = L
        self._bases = torch.empty((B * D, H), dtype=torch.float32, device=dev)
        for b in range(B):
            self._bases[b * D : (b + 1) * D].copy_(glorot_uniform((D, H), device=dev))
            self._basis_kernels.append(self.add_weight(f"basis_{b}/kernel", self._bases[b * D : (b + 1) * D]))
        self._coeff = glorot_uniform((L, B), device=dev)
        self._coefficients = self.add_weight("relation_coefficients", self._coeff)
        self._build_edge_dropout(L)
        super().build(input_shapes)

    def _message_function(self, edge_source_states, edge_target_states, num_incoming_to_node_per_message,
                          edge_type_idx, training):
        raise NotImplementedError(
            "RGCN_Basis aggregates over the shared bases on the bucketed graph (csrc/basis.hip); the per-edge form is RGCN's "
            "with W_l = sum_b a[l,b] V_b (oracle/tf2gnn_oracle.py)"
        )

    _message_function._tfgnn_builtin = True

    def call(self, inputs: MessagePassingInput, training: bool = False):
        if not getattr(type(self)._message_function, "_tfgnn_builtin", False):
            raise NotImplementedError(
                f"{type(self).__name__} overrides RGCN_Basis._message_function: the layer never forms per-edge messages, "
                "override call() and backward() as well"
            )
        X = inputs.node_embeddings
        V, D = X.shape
        g = get_graph(inputs.adjacency_lists, V)
        if g.num_edge_types != self._num_edge_types:
            raise ValueError(f"layer was built for {self._num_edge_types} edge types, got {g.num_edge_types}")
        if self._bases.shape[0] != self._num_bases * D:
            raise ValueError(f"layer was built for inputs of width {self._bases.shape[0] // self._num_bases}, got {D}")
        scales = self._step_scales(g, self._normalize_by_num_incoming, training)
        Z = ops.basis_gather_forward(g, self._coeff, X, edge_weight=scales.edge_weight_by_dst, node_scale=scales.node_scale)
        act = self._activation_name
        ctx = {"graph": g, "X": X, "Z": Z, "scales": scales, "fused_act": act}
        if act == "gelu":  # its derivative needs the product's raw output
            ctx["pre"] = ops.gemm(Z, self._bases)
            out = ops.activation_forward("gelu", ctx["pre"])
        else:
            out = ops.gemm(Z, self._bases, act=act)
        ctx["out"] = out
        self._ctx = ctx
        return out

    def activation_backward_spec(self):
        return None  # backward() applies the derivative itself; the stack's generic epilogue handles the rest

    def backward(self, grad_output: torch.Tensor) -> torch.Tensor:
        """d(loss)/d(out) -> d(loss)/d(node_embeddings); fills the basis and coefficient gradients."""
        ctx = self._ctx
        if ctx is None:
            raise RuntimeError("backward called before a forward pass")
        g, X, Z, scales, act = ctx["graph"], ctx["X"], ctx["Z"], ctx["scales"], ctx["fused_act"]
        D = X.shape[1]
        d_pre = grad_output
        if act is not None:
            d_pre = ops.activation_backward(act, grad_output, ctx["pre"] if act == "gelu" else ctx["out"])
        d_pre = d_pre.contiguous()
        # both products on ops.gemm in the mode of the moment: the K = V weight gradient never runs on split operands here,
        # so the f16x2 spread guard has nothing to watch
        d_bases = ops.gemm(Z, d_pre, trans_a=True)          # [B*D, H]
        dZ = ops.gemm(d_pre, self._bases, trans_b=True)     # [V, B*D]
        dX, d_coeff = ops.basis_gather_backward(g, self._coeff, dZ, X, edge_weight_by_dst=scales.edge_weight_by_dst,
                                                edge_weight_by_src=scales.edge_weight_by_src, node_scale=scales.node_scale)
        for b, var in enumerate(self._basis_kernels):
            var.grad = d_bases[b * D : (b + 1) * D]
        self._coefficients.grad = d_coeff
        return dX
