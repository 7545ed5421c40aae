"""Task models around the path: what the reference wraps the GNN stack in, on the same
kernels - the computation between a finalised batch and the loss, and back.

Mirrors ``tf2_gnn.models`` for that computation only: ``compute_final_node_representations``,
``compute_task_output``, ``compute_task_metrics`` keep the reference's names, arguments (dicts keyed like the batches
of ``GraphDataset._finalise_batch``: "node_features", "adjacency_list_<i>", "node_to_graph_map",
"num_graphs_in_batch"; labels "node_labels" / "target_value") and result keys.  ``backward()`` stands in for the
``tf.GradientTape`` of ``GraphTaskModel._run_step`` (tf2_gnn/models/graph_task_model.py:327-357): it fills ``.grad``
of every trainable variable with d loss / d variable.  The parameter update of that step (``_make_optimizer``,
``_apply_gradients``: clipping + a Keras optimizer, optim.py) and the step / epoch methods around it (``_run_step``,
``run_one_epoch``) are here too, and so are the prediction loop and the evaluation metrics (``predict``, ``evaluate_model``);
the training CLI, datasets and checkpoint I/O stay out (out of scope).

MLP-input dropout of the heads (``regression_mlp_dropout``, ``graph_aggregation_dropout_rate``; QM9 hands
``out_layer_dropout_keep_prob`` over as a rate) is applied in training mode as in the pooling layers (layers/nodes_to_graph_representation.py MLP).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import time

import numpy as np
import torch

from . import _lib, ops
from .optim import Optimizer, RowGradient, make_optimizer
from .layers.gnn import GNN, GNNInput
from .layers.message_passing.message_passing import Variable, default_device, glorot_uniform
from .layers.nodes_to_graph_representation import (
    prefix_names,
    MLP,
    NodesToGraphRepresentationInput,
    WeightedSumGraphRepresentation,
    segment_offsets,
)
from .utils import eval_metrics


def _feature_width(dataset) -> Optional[int]:
    """the dataset's node feature width, None where it does not say (no such property, or nothing loaded yet)"""
    try:
        return int(dataset.node_feature_shape[-1])
    except (AttributeError, ValueError, TypeError, IndexError, StopIteration):
        return None


class GraphTaskModel:
    """tf2_gnn/models/graph_task_model.py:14-399 without the Keras plumbing."""

    @classmethod
    def get_default_hyperparameters(cls, mp_style: Optional[str] = None) -> Dict[str, Any]:
        """graph_task_model.py:16-33 (the optimizer keys are kept: they are part of the dict callers pass around)."""
        params = {f"gnn_{name}": value for name, value in GNN.get_default_hyperparameters(mp_style).items()}
        params.update(
            {
                "optimizer": "Adam",
                "learning_rate": 0.001,
                "learning_rate_warmup_steps": None,
                "learning_rate_decay_steps": None,
                "momentum": 0.85,
                "rmsprop_rho": 0.98,
                "gradient_clip_value": None,
                "gradient_clip_norm": None,
                "gradient_clip_global_norm": None,
                "use_intermediate_gnn_results": False,
            }
        )
        return params

    def __init__(self, params: Dict[str, Any], dataset: Any = None, name: Optional[str] = None, *,
                 num_edge_types: Optional[int] = None, num_nodes: Optional[int] = None):
        """``dataset``: anything with ``num_edge_types`` (graph_task_model.py:41-43), or pass ``num_edge_types``.

        Learned node embeddings - the hyper-parameter ``node_embedding_dim``: absent or None (it is in no defaults dictionary)
        is off, an integer >= 1 turns it on, anything else raises ValueError.  With it on the model owns one more trainable
        variable, ``<ClassName>/node_embeddings`` [num_nodes, node_embedding_dim] (glorot_uniform; ``num_nodes`` from
        ``dataset.num_nodes`` or the keyword), and its rows REPLACE the node features: the batch's ``node_features`` - the
        dataset's, if it has any - are not read.  The hooks the reference leaves for this, ``get_initial_node_feature_shape``
        and ``compute_initial_node_features`` (graph_task_model.py:133-156), do it: a batch of ``num_nodes`` rows without
        ``sampled_node_ids`` (a transductive full batch) takes the table as it is, a batch that names its nodes in
        ``sampled_node_ids`` (neighbour sampling: distinct ids) looks its rows up with ops.gather_node_rows.  ``backward()``
        asks the stack for its input gradient, which is the table's gradient - through ops.embedding_scatter_rows into a
        dense [num_nodes, node_embedding_dim] buffer on the sampled route - and the update is the optimizer's dense step, what
        Keras does with the IndexedSlices of a lookup: every row is updated, the moments of untouched rows decay.  A
        full-batch step stays capturable.  A dataset without node features (``node_feature_shape == (0,)``) needs the key.

        ``node_embedding_update`` (absent: ``"dense"``; in no defaults dictionary; needs ``node_embedding_dim``) chooses the
        sampled route's update.  ``"dense"`` is the above: its cost is that of the whole table, every step.  ``"rows"`` keeps
        the gradient as the pair it is: ``backward()`` returns ``optim.RowGradient(d_rows, sampled_node_ids, num_nodes)`` for
        the table, no dense buffer is allocated and no embedding kernel runs, and the optimizer updates the batch's rows and
        their slots only (tfgnn_optimizer_apply_rows).  Plain SGD gives the dense result; with momentum, RMSprop or Adam it
        is the LAZY optimizer (LazyAdam): the moments of rows outside the batch do not decay and those rows do not move.  A
        full batch has a gradient for every row and takes the dense route under either value.  Anything else raises
        ValueError."""
        self._params = params
        if num_edge_types is None:
            if dataset is None or not hasattr(dataset, "num_edge_types"):
                raise ValueError("GraphTaskModel needs a dataset with num_edge_types, or num_edge_types=...")
            num_edge_types = dataset.num_edge_types
        self._num_edge_types = int(num_edge_types)
        dim = params.get("node_embedding_dim")
        if dim is not None and (isinstance(dim, bool) or not isinstance(dim, (int, np.integer)) or dim < 1):
            raise ValueError(f"node_embedding_dim must be an integer >= 1 (or None: no learned node embeddings), not {dim!r}")
        self._node_embedding_dim = None if dim is None else int(dim)
        update = params.get("node_embedding_update")
        if update is not None and (not isinstance(update, str) or update not in ("dense", "rows")):
            raise ValueError(f'node_embedding_update must be "dense" or "rows", not {update!r}')
        if update is not None and dim is None:
            raise ValueError("node_embedding_update is set without node_embedding_dim: there is no embedding table to update")
        self._node_embedding_rows = update == "rows"
        self._num_nodes: Optional[int] = None
        self._node_embeddings: Optional[Variable] = None
        self._node_embeddings_grad: Optional[torch.Tensor] = None  # the sampled route's dense [num_nodes, dim] buffer
        self._embedding_ids: Optional[torch.Tensor] = None  # sampled_node_ids of the last forward pass; None: the whole table
        self.embedding_bad_index: Optional[torch.Tensor] = None  # device flag: a sampled id outside the table (read lazily)
        if dim is not None:
            if num_nodes is None:
                if dataset is None or not hasattr(dataset, "num_nodes"):
                    raise ValueError("node_embedding_dim needs the number of nodes: a dataset with num_nodes (dataset.num_nodes), "
                                     "or num_nodes=...")
                num_nodes = dataset.num_nodes
            self._num_nodes = int(num_nodes)
            if not 1 <= self._num_nodes < 2 ** 31:
                raise ValueError(f"node_embedding_dim: num_nodes must be in [1, 2^31), not {num_nodes!r}")
        elif dataset is not None and _feature_width(dataset) == 0:
            raise ValueError(f"{type(dataset).__name__} has no node features (node_feature_shape == (0,)): set the hyper-parameter "
                             "node_embedding_dim, the width of one learned embedding per node")
        self._use_intermediate_gnn_results = params.get("use_intermediate_gnn_results", False)
        self.name = name or self.__class__.__name__
        self._gnn: Optional[GNN] = None
        self.built = False
        self._step = None  # what backward() needs from the last forward / metrics call
        self._optimizer: Optional[Optimizer] = None
        # graph_task_model.py:50: training steps taken by _run_step (host-side; not saved, the reference saves weights only).
        # A replayed CapturedStep does not advance it - the optimizer's device counter ``iterations`` does.
        self._train_step_counter = 0

    # ---- structure (graph_task_model.py:93-131) --------------------------------------------------------------
    def build(self, input_shapes: Dict[str, Any]):
        graph_params = {name[4:]: value for name, value in self._params.items() if name.startswith("gnn_")}
        self._gnn = GNN(graph_params)
        self._gnn.build(
            GNNInput(
                node_features=self.get_initial_node_feature_shape(input_shapes),
                adjacency_lists=tuple((None, 2) for _ in range(self._num_edge_types)),
                node_to_graph_map=(None,),
                num_graphs=(),
            )
        )
        if self._node_embedding_dim is not None:  # created last: the other variables draw what they draw without it
            self._node_embeddings = Variable(f"{self.__class__.__name__}/node_embeddings",
                                             glorot_uniform((self._num_nodes, self._node_embedding_dim), device=default_device()))
        self.built = True

    def get_initial_node_feature_shape(self, input_shapes):
        """graph_task_model.py:133-135; with learned node embeddings (None, node_embedding_dim)."""
        if self._node_embedding_dim is not None:
            return (None, self._node_embedding_dim)
        shape = tuple(input_shapes["node_features"])
        if int(shape[-1]) == 0:
            raise ValueError("the batch has no node features (width 0): set the hyper-parameter node_embedding_dim")
        return shape

    def compute_initial_node_features(self, inputs, training: bool):
        """graph_task_model.py:137-156; with learned node embeddings the rows of the table (see ``__init__``)."""
        table = self._node_embeddings
        if table is None:
            return inputs["node_features"]
        ids = inputs.get("sampled_node_ids") if hasattr(inputs, "get") else None
        self._embedding_ids = ids
        N, dim = table.value.shape
        if ids is None:
            rows = int(inputs["node_to_graph_map"].shape[0])
            if rows != N:
                raise ValueError(f"a batch of {rows} nodes without sampled_node_ids cannot index the {N} node embeddings: only a "
                                 "batch of the whole node set stands for the table's rows in order")
            # the table itself, no launch and no copy.  A view of its own per pass: forms derived from the stack's input are
            # remembered per tensor object (ops.sp_rows_of), and the optimizer rewrites the table between two passes
            return table.value.view(N, dim)
        if self.embedding_bad_index is None:
            self.embedding_bad_index = torch.zeros(1, dtype=torch.int32, device=table.value.device)
        rows, _ = ops.gather_node_rows(ids, int(ids.shape[0]), table.value, bad_flag=self.embedding_bad_index)
        return rows

    @property
    def trainable_variables(self) -> List[Variable]:
        embeddings = [self._node_embeddings] if self._node_embeddings is not None else []
        return list(self._gnn.trainable_variables) + self._task_variables() + embeddings

    def _task_variables(self) -> List[Variable]:
        return []

    @property
    def variables(self) -> List[Variable]:
        """what save_model / load_weights_verbosely walk (utils/model_utils.py); the reference's non-trainable
        training_step counter is not part of the hot path"""
        return self.trainable_variables

    def zero_grad(self):
        for v in self.trainable_variables:
            v.grad = None

    # ---- forward (graph_task_model.py:158-183) -----------------------------------------------------------------
    def compute_final_node_representations(self, inputs, training: bool):
        # An input pipeline may hand over the batch already bucketed - ``bucketed_graph``: the ops.Graph of these adjacency
        # lists, built on a prefetch stream while the previous step trained (the reference prepares batches in a background
        # thread + tf.data prefetch: data/graph_dataset.py:292-295); the caller has ordered the compute stream after it.
        adjacency_lists = inputs.get("bucketed_graph") if hasattr(inputs, "get") else None
        if adjacency_lists is None:
            adjacency_lists = tuple(inputs[f"adjacency_list_{i}"] for i in range(self._num_edge_types))
        gnn_input = GNNInput(
            node_features=self.compute_initial_node_features(inputs, training),
            adjacency_lists=adjacency_lists,
            node_to_graph_map=inputs["node_to_graph_map"],
            num_graphs=inputs["num_graphs_in_batch"],
        )
        return self._gnn(gnn_input, training=training, return_all_representations=self._use_intermediate_gnn_results)

    def __call__(self, inputs, training: bool = False):
        if not self.built:
            self.build({"node_features": tuple(inputs["node_features"].shape)})
        final_node_representations = self.compute_final_node_representations(inputs, training)
        return self.compute_task_output(inputs, final_node_representations, training)

    call = __call__

    def compute_task_output(self, batch_features, final_node_representations, training: bool):
        raise NotImplementedError

    def compute_task_metrics(self, batch_features, task_output, batch_labels) -> Dict[str, torch.Tensor]:
        raise NotImplementedError

    # ---- backward (graph_task_model.py:347-357: tape.gradient(loss, trainable_variables)) -----------------------
    def backward(self) -> List[Tuple[Variable, Optional[torch.Tensor]]]:
        """d loss / d variable for the loss of the last ``compute_task_metrics`` call -> [(variable, grad)]."""
        if self._step is None or "dloss" not in self._step:
            raise RuntimeError("backward() needs a forward pass followed by compute_task_metrics()")
        grad_final, grad_all = self._task_backward()
        table = self._node_embeddings
        if table is None:
            self._gnn.backward(grad_final, grad_all_representations=grad_all)
        else:  # the stack's input gradient is the gradient of the looked-up rows
            d_rows = self._gnn.backward(grad_final, need_input_grad=True, grad_all_representations=grad_all)
            if self._embedding_ids is None:
                table.grad = d_rows
            elif self._node_embedding_rows:  # the pair itself: the optimizer updates these rows and no others
                table.grad = RowGradient(d_rows, self._embedding_ids, table.value.shape[0], bad_flag=self.embedding_bad_index)
            else:
                self._node_embeddings_grad = table.grad = ops.embedding_scatter_rows(
                    d_rows, self._embedding_ids, table.value.shape[0], out=self._node_embeddings_grad,
                    bad_flag=self.embedding_bad_index)
        return [(v, v.grad) for v in self.trainable_variables]

    def _task_backward(self):
        raise NotImplementedError

    # ---- the update (graph_task_model.py:224-324) -------------------------------------------------------------------
    def _make_optimizer(self, learning_rate=None) -> Optimizer:
        """A fresh optimizer from the hyper-parameters (optimizer name, learning rate and its warm-up / decay steps, momentum,
        rmsprop_rho), or with the given learning rate (a float or a PolynomialWarmupAndDecaySchedule)."""
        return make_optimizer(self._params, learning_rate)

    def _apply_gradients(self, gradient_variable_pairs) -> None:
        """Clip and apply gradients - ``(variable, grad)`` pairs as ``backward()`` returns them, or the reference's
        ``(grad, variable)`` - with the model's optimizer (made at the first call).  One library call; no synchronisation."""
        if getattr(self, "_optimizer", None) is None:
            self._optimizer = self._make_optimizer()
        clip_val = self._params.get("gradient_clip_value")
        clip_norm_val = self._params.get("gradient_clip_norm")
        clip_global_norm_val = self._params.get("gradient_clip_global_norm")
        clip = None
        if clip_val is not None:
            if clip_norm_val is not None:
                raise ValueError("Both 'gradient_clip_value' and 'gradient_clip_norm' are set, but can only use one at a time.")
            if clip_global_norm_val is not None:
                raise ValueError("Both 'gradient_clip_value' and 'gradient_clip_global_norm' are set, but can only use one at a time.")
            clip = ("value", clip_val)
        elif clip_norm_val is not None:
            if clip_global_norm_val is not None:
                raise ValueError("Both 'gradient_clip_norm' and 'gradient_clip_global_norm' are set, but can only use one at a time.")
            clip = ("norm", clip_norm_val)
        elif clip_global_norm_val is not None:
            clip = ("global_norm", clip_global_norm_val)
        self._optimizer.apply_gradients(gradient_variable_pairs, clip=clip)

    # ---- training loop (graph_task_model.py:327-399) ------------------------------------------------------------------
    def _run_step(self, batch_features, batch_labels, training: bool) -> Dict[str, Any]:
        """Forward pass and metrics; when ``training``, the gradients and the update too."""
        task_output = self(batch_features, training=training)
        task_metrics = self.compute_task_metrics(batch_features=batch_features, task_output=task_output, batch_labels=batch_labels)
        if training:
            self._apply_gradients(self.backward())
            self._train_step_counter += 1
        return task_metrics

    def run_one_epoch(self, dataset, quiet: bool = False, training: bool = True) -> Tuple[float, float, List[Any]]:
        """One pass over ``dataset`` (an iterable of ``(batch_features, batch_labels)``) -> (average loss per graph, graphs per
        second, the metrics of every step)."""
        epoch_time_start = time.time()
        total_num_graphs = 0
        task_results = []
        total_loss = 0.0
        for step, (batch_features, batch_labels) in enumerate(dataset):
            task_metrics = self._run_step(batch_features, batch_labels, training)
            # task_metrics["loss"] is the batch average loss over graphs
            num_graphs = int(batch_features["num_graphs_in_batch"])
            total_loss = total_loss + task_metrics["loss"] * float(num_graphs)
            total_num_graphs += num_graphs
            task_results.append(task_metrics)
            if not quiet:
                epoch_graph_average_loss = float(total_loss) / float(total_num_graphs)
                batch_graph_average_loss = float(task_metrics["loss"])
                steps_per_second = step / (time.time() - epoch_time_start)
                print(
                    f"   Step: {step:4d}"
                    f"  |  Epoch graph avg. loss = {epoch_graph_average_loss:.5f}"
                    f"  |  Batch graph avg. loss = {batch_graph_average_loss:.5f}"
                    f"  |  Steps per sec = {steps_per_second:.5f}",
                    end="\r",
                )
        if not quiet:
            print("\r\x1b[K", end="")
        total_time = time.time() - epoch_time_start
        return float(total_loss) / float(total_num_graphs), float(total_num_graphs) / total_time, task_results

    # ---- prediction loop (graph_task_model.py:401-420) ------------------------------------------------------------------
    def predict(self, dataset) -> torch.Tensor:
        """The task outputs of every batch of ``dataset`` (an iterable of ``(batch_features, batch_labels)``) in evaluation
        mode, concatenated along axis 0 on the device.  A model whose output is a 1-tuple (NodeMulticlassTask:
        ``(per_node_logits,)``) contributes the tuple's element, so the result is one tensor for every task model."""
        task_outputs = []
        for batch_features, _ in dataset:
            task_output = self(batch_features, training=False)
            task_outputs.append(task_output[0] if isinstance(task_output, tuple) else task_output)
        return torch.cat(task_outputs, dim=0)

    def evaluate_model(self, dataset) -> Dict[str, float]:
        """Metrics that make sense for the model's application area, by name (e.g. "acc", "roc_auc"), over ``dataset`` in the
        format of the training loop; the graph-level tasks implement it."""
        raise NotImplementedError()

    def _predictions_and_target_values(self, dataset) -> Tuple[np.ndarray, np.ndarray]:
        """``predict(dataset)`` and the batches' "target_value" labels, each copied to the host once"""
        predictions = self.predict(dataset)
        labels = torch.cat([batch_labels["target_value"].reshape(-1) for _, batch_labels in dataset], dim=0)
        return predictions.cpu().numpy(), labels.cpu().numpy()


class NodeMulticlassTask(GraphTaskModel):
    """tf2_gnn/models/node_multiclass_task.py:26-76: Dense(num_labels) on the final node representations, sigmoid
    cross entropy summed over labels and averaged over nodes, micro-F1."""

    def __init__(self, params: Dict[str, Any], dataset: Any = None, name: Optional[str] = None, *,
                 num_edge_types: Optional[int] = None, num_node_target_labels: Optional[int] = None,
                 num_nodes: Optional[int] = None):
        super().__init__(params, dataset=dataset, name=name, num_edge_types=num_edge_types, num_nodes=num_nodes)
        if num_node_target_labels is None:
            if not hasattr(dataset, "num_node_target_labels"):
                raise ValueError(
                    f"Provided dataset of type {type(dataset)} does not provide num_node_target_labels information."
                )
            num_node_target_labels = dataset.num_node_target_labels
        self._num_labels = int(num_node_target_labels)

    def build(self, input_shapes):
        H = int(self._params["gnn_hidden_dim"])
        dev = default_device()
        # node_multiclass_task.py:41-43: a Dense built directly under tf.name_scope(<class name>) - Keras adds no layer name
        cls = self.__class__.__name__
        self._kernel = Variable(f"{cls}/kernel", glorot_uniform((H, self._num_labels), device=dev))
        self._bias = Variable(f"{cls}/bias", torch.zeros(self._num_labels, dtype=torch.float32, device=dev))
        super().build(input_shapes)

    def _task_variables(self):
        return [self._kernel, self._bias]

    def compute_task_output(self, batch_features, final_node_representations, training: bool):
        h = final_node_representations[0] if isinstance(final_node_representations, tuple) else final_node_representations
        per_node_logits = ops.gemm(h, self._kernel.value, bias=self._bias.value)
        self._step = {"h": h}
        return (per_node_logits,)

    def compute_task_metrics(self, batch_features, task_output, batch_labels) -> Dict[str, torch.Tensor]:
        (per_node_logits,) = task_output
        metrics, counts, dlogits = ops.sigmoid_ce_metrics(per_node_logits, batch_labels["node_labels"])
        if self._step is not None:
            self._step["dloss"] = dlogits
        return {"loss": metrics[0], "f1_score": metrics[1], "f1_counts": counts}

    def compute_epoch_metrics(self, task_results: List[Any]) -> Tuple[float, str]:
        """node_multiclass_task.py:72-74."""
        avg_microf1 = float(sum(float(r["f1_score"]) for r in task_results) / len(task_results))
        return -avg_microf1, f"Avg MicroF1: {avg_microf1:.3f}"

    def _task_backward(self):
        h, d = self._step["h"], self._step["dloss"]
        self._kernel.grad = ops.gemm(h, d, trans_a=True)
        self._bias.grad = ops.colsum(d)
        return ops.gemm(d, self._kernel.value, trans_b=True), None


class NodeClassificationTask(NodeMulticlassTask):
    """One class per node, labels known for part of the nodes, folds as node masks over the same graph (ogbn-arxiv style);
    the reference has no counterpart.  Dense(num_node_classes) on the final node representations - the head, its variable
    names and its backward pass are NodeMulticlassTask's - and the weighted softmax cross-entropy of include/tfgnn.h
    tfgnn_softmax_ce_metrics: a node is counted iff its ``node_label_weights`` entry (1 when the batch has none) is > 0 and
    its ``node_labels`` entry is an integer in [0, num_node_classes).  Labels and weights are read from device memory by the
    kernel, so a captured step follows in-place changes of either (capture.py)."""

    def __init__(self, params: Dict[str, Any], dataset: Any = None, name: Optional[str] = None, *,
                 num_edge_types: Optional[int] = None, num_node_classes: Optional[int] = None,
                 num_nodes: Optional[int] = None):
        if num_node_classes is None:
            if not hasattr(dataset, "num_node_classes"):
                raise ValueError(f"Provided dataset of type {type(dataset)} does not provide num_node_classes information.")
            num_node_classes = dataset.num_node_classes
        super().__init__(params, dataset=dataset, name=name, num_edge_types=num_edge_types,
                         num_node_target_labels=num_node_classes, num_nodes=num_nodes)

    @property
    def num_node_classes(self) -> int:
        return self._num_labels

    def compute_task_metrics(self, batch_features, task_output, batch_labels) -> Dict[str, torch.Tensor]:
        """-> "loss", "accuracy" (of this batch's counted nodes), "num_correct", "num_labelled" (int64): device tensors."""
        (per_node_logits,) = task_output
        metrics, counts, dlogits, _ = ops.softmax_ce_metrics(per_node_logits, batch_labels["node_labels"],
                                                             batch_labels.get("node_label_weights"))
        if self._step is not None:
            self._step["dloss"] = dlogits
        return {"loss": metrics[0], "accuracy": metrics[1], "num_correct": counts[0], "num_labelled": counts[1]}

    def compute_epoch_metrics(self, task_results: List[Any]) -> Tuple[float, str]:
        """Correct predictions over counted nodes, across steps of different sizes; the smaller the better, so -accuracy."""
        total_correct = sum(int(r["num_correct"]) for r in task_results)
        total_labelled = sum(int(r["num_labelled"]) for r in task_results)
        epoch_acc = float(total_correct) / float(total_labelled) if total_labelled else float("nan")
        return -epoch_acc, f"Accuracy = {epoch_acc:.3f}"

    def evaluate_model(self, dataset) -> Dict[str, float]:
        """-> acc, macro_f1 (utils/eval_metrics.py multiclass_metrics) of the argmax of ``predict(dataset)`` over the counted
        nodes of ``dataset``."""
        predictions = np.argmax(self.predict(dataset).cpu().numpy(), axis=1)  # the lowest index among equal logits, as the kernel
        labels, weights = [], []
        for _, batch_labels in dataset:
            y = batch_labels["node_labels"].reshape(-1)
            w = batch_labels.get("node_label_weights")
            labels.append(y)
            weights.append(torch.ones_like(y) if w is None else w.reshape(-1))
        return eval_metrics.multiclass_metrics(torch.cat(labels).cpu().numpy(), predictions, self._num_labels,
                                               weights=torch.cat(weights).cpu().numpy())


class LinkPredictionTask(GraphTaskModel):
    """Edge-level task: score typed edges (source, relation, target) from the final node representations with a DistMult
    decoder, s = sum_d h_u[d] R[t, d] h_v[d] (the link-prediction experiment of the R-GCN paper); the reference has no
    counterpart.  One task variable, ``relation_embeddings`` [num_relations, gnn_hidden_dim].  Loss: the weighted sigmoid
    cross-entropy of the scores against ``triple_labels`` (1 for a true edge, 0 for a sampled negative) of include/tfgnn.h
    tfgnn_distmult_ce_metrics: a triple is counted iff its ``triple_weights`` entry (1 when absent) is > 0 and its label is
    0 or 1.

    ``params["link_decoder"]`` chooses the decoder: ``"distmult"`` (the default; the key is in no defaults dictionary) or
    ``"complex"``.  DistMult is symmetric - s(u, t, v) == s(v, t, u) whatever the parameters - so it cannot tell a directed
    relation from its reverse.  ComplEx (Trouillon et al. 2016) reads a row of h and of ``relation_embeddings`` as the complex
    vector [re ; im] (two halves, ``gnn_hidden_dim`` even) and scores s = Re sum_k h_u[k] R[t, k] conj(h_v[k]) with the
    tfgnn_complex_* kernels: the same variable, batches, loss, counts and filtered ranking, an asymmetric score.

    The triples travel in BOTH dictionaries of a batch (LinkPredictionDataset puts the same tensors into each): the forward
    pass needs them for its output, ``compute_task_metrics`` takes the labels from ``batch_labels`` like every task.  When
    ``batch_features`` also carries ``triple_labels`` - the dataset's batches do - the forward pass runs the fused kernel once
    (scores, loss, counts, d loss / d score) and ``compute_task_metrics`` on that output with the same label tensor reuses its
    results; otherwise it runs the kernel again on the node representations of the last forward pass.  Triples, labels,
    weights and tables are read from device memory by the kernels, so a captured step follows in-place changes (new
    negatives) of all of them.  A training step on a batch that carries ``triple_sampler`` (LinkPredictionDataset with
    ``negative_sampling = "device"``) first calls its ``redraw()``: the negatives and the node tables are rewritten on the
    device as part of the step, and of every replay of a captured one.  Inference never redraws.

    Mini-batches (LinkPredictionDataset with ``neighbor_fanouts``): a TRAIN batch is a sampled subgraph whose ``triples`` are
    in the batch's LOCAL ids - rows of the node representations - so nothing here changes: the loss is the mean over the
    batch's counted triples, a learned embedding table is read through ``sampled_node_ids`` and, with
    ``node_embedding_update="rows"``, gets a RowGradient.  Such a batch carries no ``triple_sampler`` and cannot be ranked:
    ``evaluate_model`` on it raises ValueError (use VALIDATION or TEST, which stay full-graph batches)."""

    def __init__(self, params: Dict[str, Any], dataset: Any = None, name: Optional[str] = None, *,
                 num_edge_types: Optional[int] = None, num_relations: Optional[int] = None, num_nodes: Optional[int] = None):
        super().__init__(params, dataset=dataset, name=name, num_edge_types=num_edge_types, num_nodes=num_nodes)
        if num_relations is None:
            if not hasattr(dataset, "num_relations"):
                raise ValueError(f"Provided dataset of type {type(dataset)} does not provide num_relations information.")
            num_relations = dataset.num_relations
        self._num_relations = int(num_relations)
        if self._num_relations < 1:
            raise ValueError("LinkPredictionTask needs at least one relation")
        self._decoder = params.get("link_decoder", "distmult")
        if self._decoder not in ops.LINK_DECODERS:
            raise ValueError(f"link_decoder must be 'distmult' or 'complex', not {self._decoder!r}")
        if self._decoder == "complex" and int(self._params["gnn_hidden_dim"]) % 2:
            raise ValueError(f"link_decoder='complex' reads a row as [re ; im] halves: gnn_hidden_dim must be even, not "
                             f"{self._params['gnn_hidden_dim']}")
        self._ce_metrics, self._backward_op, self._rank_op = (
            (ops.complex_ce_metrics, ops.complex_backward, ops.complex_rank) if self._decoder == "complex"
            else (ops.distmult_ce_metrics, ops.distmult_backward, ops.distmult_rank))

    @property
    def num_relations(self) -> int:
        return self._num_relations

    @property
    def link_decoder(self) -> str:
        return self._decoder

    def build(self, input_shapes):
        H = int(self._params["gnn_hidden_dim"])
        self._relation_embeddings = Variable(f"{self.__class__.__name__}/relation_embeddings",
                                             glorot_uniform((self._num_relations, H), device=default_device()))
        super().build(input_shapes)

    def _task_variables(self):
        return [self._relation_embeddings]

    @staticmethod
    def _final(final_node_representations):
        return final_node_representations[0] if isinstance(final_node_representations, tuple) else final_node_representations

    def _fused(self, h, triples, labels, weights, need_grad=True):
        metrics, counts, scores, gscore = self._ce_metrics(h, self._relation_embeddings.value, triples, labels, weights,
                                                           need_grad=need_grad)
        return {"scores": scores, "metrics": metrics, "counts": counts, "gscore": gscore, "triples": triples, "labels": labels,
                "weights": weights}

    def compute_task_output(self, batch_features, final_node_representations, training: bool):
        sampler = batch_features.get("triple_sampler")
        if training and sampler is not None:  # negative_sampling = "device": new negatives and node tables, in place, on this stream
            sampler.redraw()
        h = self._final(final_node_representations)
        triples = batch_features["triples"]
        labels = batch_features.get("triple_labels")
        # triples and tables of the forward pass: what backward() walks when the gradient of the scores comes from elsewhere
        # (TorchGraphTaskModel); compute_task_metrics replaces them with the ones it was given
        self._step = {"h": h, "triples": triples, "tables": batch_features.get("triple_tables")}
        if labels is None:  # scores only: no triple is counted against an all-zero weight column
            zeros = torch.zeros(triples.shape[0], dtype=torch.float32, device=h.device)
            return (self._fused(h, triples, zeros, zeros, need_grad=False)["scores"],)
        self._step["fused"] = self._fused(h, triples, labels, batch_features.get("triple_weights"))
        return (self._step["fused"]["scores"],)

    def compute_task_metrics(self, batch_features, task_output, batch_labels) -> Dict[str, torch.Tensor]:
        """-> "loss", "accuracy" (of this batch's counted triples), "counts" (int64 [4]: tp, fp, tn, fn): device tensors."""
        step = self._step
        if step is None:
            raise RuntimeError("compute_task_metrics() needs the node representations of a forward pass")
        fused = step.get("fused")
        labels, weights = batch_labels["triple_labels"], batch_labels.get("triple_weights")
        if not (fused is not None and task_output[0] is fused["scores"] and labels is fused["labels"]
                and weights is fused["weights"] and batch_labels["triples"] is fused["triples"]):
            fused = self._fused(step["h"], batch_labels["triples"], labels, weights)
        step["dloss"] = fused["gscore"]
        step["triples"], step["tables"] = fused["triples"], batch_labels.get("triple_tables")
        return {"loss": fused["metrics"][0], "accuracy": fused["metrics"][1], "counts": fused["counts"]}

    def compute_epoch_metrics(self, task_results: List[Any]) -> Tuple[float, str]:
        """Correct predictions over counted triples, from the summed confusion counts; the smaller the better: -accuracy."""
        tp, fp, tn, fn = (sum(int(r["counts"][i]) for r in task_results) for i in range(4))
        total = tp + fp + tn + fn
        epoch_acc = float(tp + tn) / float(total) if total else float("nan")
        return -epoch_acc, f"Accuracy = {epoch_acc:.3f}"

    def _task_backward(self):
        s = self._step
        if s.get("tables") is None:
            raise RuntimeError("backward() needs batch_labels['triple_tables'] (ops.build_triple_tables, on the device)")
        d_h, d_r = self._backward_op(s["h"], self._relation_embeddings.value, s["triples"], s["dloss"], s["tables"])
        self._relation_embeddings.grad = d_r
        if self._use_intermediate_gnn_results:
            return d_h, [None] * (int(self._params["gnn_num_layers"]) + 1)
        return d_h, None

    def rank_counts(self, batch_features, batch_labels) -> Tuple[torch.Tensor, torch.Tensor]:
        """(greater, equal) of tfgnn_distmult_rank (tfgnn_complex_rank with that decoder) for the batch's ``positive_triples``,
        filtered by ``rank_filters``: the queries with the target corrupted, then the same queries with the source corrupted
        (int32 [2 P] each, on the device)."""
        if "rank_filters" not in batch_labels or "positive_triples" not in batch_labels:
            raise ValueError("this batch carries no positive_triples / rank_filters: filtered ranking needs every entity's "
                             "representation, which a neighbour-sampled TRAIN mini-batch does not hold; use the VALIDATION or "
                             "TEST batches")
        h = self._final(self.compute_final_node_representations(batch_features, training=False))
        greater, equal = [], []
        for side in ("dst", "src"):
            offsets, ids = batch_labels["rank_filters"][side]
            g, e = self._rank_op(h, self._relation_embeddings.value, batch_labels["positive_triples"], side, offsets, ids)
            greater.append(g)
            equal.append(e)
        return torch.cat(greater), torch.cat(equal)

    def evaluate_model(self, dataset) -> Dict[str, float]:
        """-> mrr, hits@1, hits@3, hits@10 (utils/eval_metrics.py ranking_metrics) of the fold's true triples: filtered ranking
        - every known true triple of the loaded folds is left out of the candidates - with both sides corrupted in turn."""
        if not self.built:
            raise RuntimeError("evaluate_model() needs a built model")
        greater, equal = [], []
        for batch_features, batch_labels in dataset:
            g, e = self.rank_counts(batch_features, batch_labels)
            greater.append(g)
            equal.append(e)
        return eval_metrics.ranking_metrics(torch.cat(greater).cpu().numpy(), torch.cat(equal).cpu().numpy())


def _regression_task_metrics(task, task_output, batch_features, batch_labels):
    """graph_regression_task.py:150-166 / qm9_regression.py:116-130."""
    metrics, dpred = ops.regression_metrics(task_output, batch_labels["target_value"])
    if task._step is not None:
        task._step["dloss"] = dpred
    num_graphs = float(int(batch_features["num_graphs_in_batch"]))
    return {
        "loss": metrics[0],
        "batch_squared_error": metrics[0] * num_graphs,
        "batch_absolute_error": metrics[1] * num_graphs,
        "num_graphs": num_graphs,
    }


def _regression_epoch_metrics(task_results):
    total_num_graphs = sum(r["num_graphs"] for r in task_results)
    epoch_mse = float(sum(float(r["batch_squared_error"]) for r in task_results) / total_num_graphs)
    epoch_mae = float(sum(float(r["batch_absolute_error"]) for r in task_results) / total_num_graphs)
    return epoch_mse, epoch_mae


class QM9RegressionTask(GraphTaskModel):
    """tf2_gnn/models/qm9_regression.py:30-145: per node sigmoid(gate([x0 | h])) * transform(h), summed per graph."""

    @classmethod
    def get_default_hyperparameters(cls, mp_style: Optional[str] = None) -> Dict[str, Any]:
        params = super().get_default_hyperparameters(mp_style)
        params.update({"use_intermediate_gnn_results": False, "out_layer_dropout_keep_prob": 1.0})
        return params

    def __init__(self, params: Dict[str, Any], dataset: Any = None, name: Optional[str] = None, *,
                 num_edge_types: Optional[int] = None, task_id: int = 0):
        super().__init__(params, dataset=dataset, name=name, num_edge_types=num_edge_types)
        self._task_id = int(getattr(dataset, "_params", {}).get("task_id", task_id)) if dataset is not None else int(task_id)
        # qm9_regression.py:49-62: the "keep prob" hyper-parameter is handed over as the dropout RATE; without hidden layers
        # the MLPs never draw a mask (see layers/nodes_to_graph_representation.py MLP)
        rate = float(self._params["out_layer_dropout_keep_prob"])
        self._regression_gate = MLP(out_size=1, hidden_layers=[], use_biases=True, dropout_rate=rate, name="gate")
        self._regression_transform = MLP(out_size=1, hidden_layers=[], use_biases=True, dropout_rate=rate, name="transform")

    def build(self, input_shapes):
        H = int(self._params["gnn_hidden_dim"])
        self._regression_gate.build(int(input_shapes["node_features"][-1]) + H)
        self._regression_transform.build(H)
        cls = self.__class__.__name__  # qm9_regression.py:65-80
        prefix_names(self._regression_gate.variables, f"{cls}/node_gate")
        prefix_names(self._regression_transform.variables, f"{cls}/node_transform")
        super().build(input_shapes)

    def _task_variables(self):
        return self._regression_gate.variables + self._regression_transform.variables

    def compute_task_output(self, batch_features, final_node_representations, training: bool):
        if self._params["use_intermediate_gnn_results"]:
            final_node_representations, _ = final_node_representations
        h = final_node_representations
        x0 = batch_features["node_features"]
        G = int(batch_features["num_graphs_in_batch"])
        per_node_output = self._regression_transform(h, training=training)  # [V, 1]
        per_node_weight = self._regression_gate(torch.cat([x0, h], dim=1), final_act="sigmoid", training=training)  # [V, 1]
        ids = batch_features["node_to_graph_map"].to(torch.int32).contiguous()
        ptr = segment_offsets(ids, G)
        out = torch.empty((G, 1), dtype=torch.float32, device=h.device)
        lib = _lib.load()
        _lib.check(
            lib.tfgnn_segment_weighted_sum(ops._ptr(per_node_output), ops._ptr(per_node_weight), ops._ptr(ptr), G, 1, 1, 0,
                                           ops._ptr(out), ops._stream())
        )
        self._step = {"ids": ids, "ptr": ptr, "R": per_node_output, "w": per_node_weight, "D0": x0.shape[1], "V": h.shape[0]}
        return out.view(G)

    def compute_task_metrics(self, batch_features, task_output, batch_labels):
        return _regression_task_metrics(self, task_output, batch_features, batch_labels)

    def compute_epoch_metrics(self, task_results: List[Any]) -> Tuple[float, str]:
        """qm9_regression.py:132-158."""
        epoch_mse, epoch_mae = _regression_epoch_metrics(task_results)
        return epoch_mae, f"Task {self._task_id} | MSE = {epoch_mse:.3f} | MAE = {epoch_mae:.3f}"

    def evaluate_model(self, dataset) -> Dict[str, float]:
        """The regression metrics of GraphRegressionTask (mae, mse, max_err, expl_var, r2_score) for the task's target; the
        reference's QM9 model leaves this to its base class, which raises."""
        predictions, labels = self._predictions_and_target_values(dataset)
        return eval_metrics.regression_metrics(labels, predictions)

    def _task_backward(self):
        s = self._step
        V = s["V"]
        d_out = s["dloss"].contiguous().view(-1, 1)
        dR = torch.empty((V, 1), dtype=torch.float32, device=d_out.device)
        dw = torch.empty((V, 1), dtype=torch.float32, device=d_out.device)
        lib = _lib.load()
        _lib.check(
            lib.tfgnn_segment_weighted_sum_backward(ops._ptr(d_out), ops._ptr(s["R"]), ops._ptr(s["w"]), ops._ptr(s["ids"]),
                                                    ops._ptr(s["ptr"]), V, 1, 1, 0, ops._ptr(dR), ops._ptr(dw), ops._stream())
        )
        d_cat = self._regression_gate.backward(dw)  # [V, D0 + H]
        d_h = self._regression_transform.backward(dR)
        d_h = ops.add_scale(d_h, d_cat[:, s["D0"]:], 1.0)
        if self._params["use_intermediate_gnn_results"]:
            L = int(self._params["gnn_num_layers"])
            return d_h, [None] * (L + 1)
        return d_h, None


class GraphRegressionTask(GraphTaskModel):
    """tf2_gnn/models/graph_regression_task.py:15-185: softmax- and sigmoid-weighted sums of the node representations
    (the input features next to every layer's output, or the last one), concatenated, through a regression MLP."""

    @classmethod
    def get_default_hyperparameters(cls, mp_style: Optional[str] = None) -> Dict[str, Any]:
        params = super().get_default_hyperparameters(mp_style)
        params.update(
            {
                "use_intermediate_gnn_results": True,
                "graph_aggregation_output_size": 32,
                "graph_aggregation_num_heads": 4,
                "graph_aggregation_layers": [32, 32],
                "graph_aggregation_dropout_rate": 0.1,
                "regression_mlp_layers": [64, 32],
                "regression_mlp_dropout": 0.1,
            }
        )
        return params

    def __init__(self, params: Dict[str, Any], dataset: Any = None, name: Optional[str] = None, *,
                 num_edge_types: Optional[int] = None):
        super().__init__(params, dataset=dataset, name=name, num_edge_types=num_edge_types)

        def pooling(weighting_fun):
            return WeightedSumGraphRepresentation(
                graph_representation_size=params["graph_aggregation_output_size"],
                num_heads=params["graph_aggregation_num_heads"],
                weighting_fun=weighting_fun,
                scoring_mlp_layers=params["graph_aggregation_layers"],
                scoring_mlp_dropout_rate=params["graph_aggregation_dropout_rate"],
                scoring_mlp_activation_fun="elu",
                transformation_mlp_layers=params["graph_aggregation_layers"],
                transformation_mlp_dropout_rate=params["graph_aggregation_dropout_rate"],
                transformation_mlp_activation_fun="elu",
            )

        self._weighted_avg_of_nodes_to_graph_repr = pooling("softmax")
        self._weighted_sum_of_nodes_to_graph_repr = pooling("sigmoid")
        self._regression_mlp = MLP(out_size=1, hidden_layers=params["regression_mlp_layers"], use_biases=True,
                                   activation_fun="relu", dropout_rate=params["regression_mlp_dropout"])  # default name "MLP"
        self.regression_mlp_dropout_masks = None  # tests: masks per Dense layer instead of drawn ones

    def build(self, input_shapes):
        D0 = int(input_shapes["node_features"][-1])
        H = int(self._params["gnn_hidden_dim"])
        if self._params["use_intermediate_gnn_results"]:
            node_repr_size = D0 + H * int(self._params["gnn_num_layers"])
        else:
            node_repr_size = D0 + H
        shapes = NodesToGraphRepresentationInput((None, node_repr_size), (None,), ())
        self._weighted_avg_of_nodes_to_graph_repr.build(shapes)
        self._weighted_sum_of_nodes_to_graph_repr.build(shapes)
        self._regression_mlp.build(2 * int(self._params["graph_aggregation_output_size"]))
        # graph_regression_task.py:91-106: name scopes of the reference's variables
        cls = self.__class__.__name__
        prefix_names(self._weighted_avg_of_nodes_to_graph_repr.trainable_variables, f"{cls}/graph_representation_computation/weighted_avg")
        prefix_names(self._weighted_sum_of_nodes_to_graph_repr.trainable_variables, f"{cls}/graph_representation_computation/weighted_sum")
        prefix_names(self._regression_mlp.variables, cls)
        super().build(input_shapes)

    def _task_variables(self):
        return (
            list(self._weighted_avg_of_nodes_to_graph_repr.trainable_variables)
            + list(self._weighted_sum_of_nodes_to_graph_repr.trainable_variables)
            + self._regression_mlp.variables
        )

    def compute_task_output(self, batch_features, final_node_representations, training: bool):
        x0 = batch_features["node_features"]
        if self._params["use_intermediate_gnn_results"]:
            _, intermediate = final_node_representations
            pieces = (x0,) + tuple(intermediate[1:])  # skip the output of the initial projection (:112-121)
        else:
            pieces = (x0, final_node_representations)
        node_representations = torch.cat(pieces, dim=1)
        pool_in = NodesToGraphRepresentationInput(
            node_representations, batch_features["node_to_graph_map"], batch_features["num_graphs_in_batch"]
        )
        avg = self._weighted_avg_of_nodes_to_graph_repr(pool_in, training=training)
        tot = self._weighted_sum_of_nodes_to_graph_repr(pool_in, training=training)
        graph_representations = torch.cat([avg, tot], dim=1)  # [G, 2 GD]
        per_graph_results = self._regression_mlp(graph_representations, training=training,
                                                 dropout_masks=self.regression_mlp_dropout_masks)  # [G, 1]
        self._step = {"widths": [p.shape[1] for p in pieces], "GD": avg.shape[1]}
        return per_graph_results.view(-1)

    def compute_task_metrics(self, batch_features, task_output, batch_labels):
        return _regression_task_metrics(self, task_output, batch_features, batch_labels)

    def compute_epoch_metrics(self, task_results: List[Any]) -> Tuple[float, str]:
        """graph_regression_task.py:168-185."""
        epoch_mse, epoch_mae = _regression_epoch_metrics(task_results)
        return epoch_mae, f" MSE = {epoch_mse:.3f} | MAE = {epoch_mae:.3f}"

    def evaluate_model(self, dataset) -> Dict[str, float]:
        """graph_regression_task.py:184-203 -> mae, mse, max_err, expl_var, r2_score (utils/eval_metrics.py)."""
        predictions, labels = self._predictions_and_target_values(dataset)
        return eval_metrics.regression_metrics(labels, predictions)

    def _dloss_dresults(self) -> torch.Tensor:
        """d loss / d (per-graph results of the regression MLP) [G]"""
        return self._step["dloss"]

    def _task_backward(self):
        s = self._step
        d_graph = self._regression_mlp.backward(self._dloss_dresults().contiguous().view(-1, 1))  # [G, 2 GD]
        GD = s["GD"]
        d_nodes = ops.add_scale(
            self._weighted_avg_of_nodes_to_graph_repr.backward(d_graph[:, :GD].contiguous()),
            self._weighted_sum_of_nodes_to_graph_repr.backward(d_graph[:, GD:].contiguous()),
            1.0,
        )  # [V, D0 + ...]
        widths = s["widths"]
        if self._params["use_intermediate_gnn_results"]:
            grads: List[Optional[torch.Tensor]] = [None]
            col = widths[0]
            for w in widths[1:]:
                grads.append(d_nodes[:, col : col + w])
                col += w
            return None, grads
        return d_nodes[:, widths[0] :], None


def _float32_epsilon() -> Tuple[float, float]:
    """K.epsilon() and 1 - K.epsilon() as the float32 values Keras clips with"""
    eps = np.float32(1e-7)
    return float(eps), float(np.float32(1.0) - eps)


def _binary_ce_from_probabilities(prob: torch.Tensor, target: torch.Tensor):
    """The arithmetic of tfgnn_binary_ce_metrics (include/tfgnn.h) for probabilities that did not come out of the last
    forward pass, unfused -> (loss, batch accuracy, number of correct predictions, d loss / d probability)."""
    ops._require_dev(prob, torch.float32, "task_output")
    ops._require_dev(target, torch.float32, "target_value")
    p, y = prob.reshape(-1), target.reshape(-1)
    if p.shape != y.shape:
        raise ValueError(f"task_output {tuple(prob.shape)} and target_value {tuple(target.shape)} differ in shape")
    if p.numel() == 0:
        raise ValueError("binary cross-entropy of an empty batch (the reference's reduce_mean gives nan)")
    eps, hi = _float32_epsilon()
    pc = p.clamp(eps, hi)
    a, b = pc + eps, (1.0 - pc) + eps
    loss = -(y * torch.log(a) + (1.0 - y) * torch.log(b)).mean()
    num_correct = (torch.round(p) == y).sum()  # torch.round: half to even, as tf.math.round
    inside = (p >= eps) & (p <= hi)
    dprob = torch.where(inside, (1.0 - y) / b - y / a, torch.zeros_like(p)) / float(p.numel())
    return loss, num_correct.to(torch.float32) / float(p.numel()), num_correct, dprob


class GraphBinaryClassificationTask(GraphRegressionTask):
    """tf2_gnn/models/graph_binary_classification_task.py:11-101: the graph regression model with a sigmoid on its per-graph
    results, binary cross-entropy of the probabilities against "target_value" (0 / 1), accuracy.

    What ``_step`` holds, beside the parent's entries.  After a forward pass: ``"logits"`` (the parent's per-graph results)
    and ``"prob"`` (the task output, sigmoid(logits)).  ``"dloss"`` is, as for every task model, the gradient with respect to
    the task OUTPUT - here the probabilities - or ``None``; ``"dlogits"`` is the gradient with respect to the logits.
    ``compute_task_metrics`` on the output of the last forward pass runs the fused kernel, which differentiates through the
    sigmoid itself: it stores ``"dlogits"`` and sets ``"dloss"`` to ``None``.  Whoever has a gradient with respect to the
    probabilities - ``TorchGraphTaskModel.back``, or ``compute_task_metrics`` on probabilities of the caller's own - stores it
    under ``"dloss"``.  ``backward()`` uses ``"dloss"`` times p (1 - p) when it is not ``None``, and ``"dlogits"`` otherwise:
    the last writer decides."""

    def compute_task_output(self, batch_features, final_node_representations, training: bool):
        logits = super().compute_task_output(batch_features, final_node_representations, training)
        prob = ops.activation_forward("sigmoid", logits)  # :31
        self._step["logits"], self._step["prob"] = logits, prob
        return prob

    def compute_task_metrics(self, batch_features, task_output, batch_labels) -> Dict[str, Any]:
        """:33-58 -> "loss", "batch_acc", "num_correct" (device tensors; the count is int64), "num_graphs" (a float)."""
        target = batch_labels["target_value"]
        step = self._step
        if step is not None and task_output is step.get("prob"):
            metrics, counts, _, dlogits = ops.binary_ce_metrics(step["logits"], target, want_prob=False)
            loss, batch_acc, num_correct = metrics[0], metrics[1], counts[0] + counts[2]
            step["dlogits"], step["dloss"] = dlogits, None
        else:
            loss, batch_acc, num_correct, dprob = _binary_ce_from_probabilities(task_output, target)
            if step is not None:
                step["dloss"] = dprob
        return {
            "loss": loss,
            "batch_acc": batch_acc,
            "num_correct": num_correct,
            "num_graphs": float(int(batch_features["num_graphs_in_batch"])),
        }

    def compute_epoch_metrics(self, task_results: List[Any]) -> Tuple[float, str]:
        """:60-68."""
        total_num_graphs = sum(r["num_graphs"] for r in task_results)
        total_num_correct = sum(int(r["num_correct"]) for r in task_results)
        epoch_acc = float(total_num_correct) / float(total_num_graphs)
        return -epoch_acc, f"Accuracy = {epoch_acc:.3f}"

    def evaluate_model(self, dataset) -> Dict[str, float]:
        """:70-101 -> acc, balanced_acc, precision, recall, f1_score, roc_auc, average_precision (utils/eval_metrics.py)."""
        predictions, labels = self._predictions_and_target_values(dataset)
        return eval_metrics.binary_classification_metrics(labels, predictions)

    def _dloss_dresults(self) -> torch.Tensor:
        s = self._step
        if s["dloss"] is not None:  # with respect to the probabilities: through the sigmoid
            return ops.activation_backward("sigmoid", s["dloss"].reshape(-1), s["prob"])
        return s["dlogits"]
