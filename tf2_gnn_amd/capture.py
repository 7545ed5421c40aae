"""A step on a STATIC batch as one hipGraph: capture once, replay per step.

Why.  A step on a batch of BASELINE configs[0]'s size (PPI: 7 110 nodes, ~200 k edges after finalisation) is ~190 library
calls - 50 kernels of 5-70 microseconds for forward + loss + backward, the rest batch preparation; driven from Python through
ctypes it costs 1.4 ms of HOST time for 1.3 ms of device time (``bench.py --workload ppi``, VERDICT r4 missing 2).  The reference has the same problem and the same answer: it traces the
step into one ``tf.function`` graph (``tf2_gnn/models/graph_task_model.py:327-357``: ``_run_step`` under
``tf.function(input_signature=...)``) and replays that.  Here the step is captured into a hipGraph - every kernel the
library launches on the capturing stream becomes a node - and ``replay()`` is one ``hipGraphLaunch``.

What is static.  A hipGraph freezes kernel arguments: pointers, sizes, launch grids.  The launch grids of the gather
kernels depend on the ADJACENCY (long-row plans, non-empty buckets), so a captured step is valid for the batch it was
captured on - the same ``GNNInput`` tensors (contents of ``node_features``, labels and weights may change IN PLACE between
replays; the adjacency may not).  That is full-batch training / inference on one graph (ogbn-arxiv-style), an epoch that
revisits the same finalised batches (capture one step per batch), and the benchmark's protocol (one batch, K steps).
A stream of NEW batches runs eagerly, as before.

What a replay does NOT freeze.
  * Weights: they are read from their buffers by every replay; an optimizer that updates them in place is seen.  The
    capture starts from an EMPTY derived-weight cache, so the conversions of the weights into operand form
    (``ops.sp_weight_operand``) are nodes of the graph and run per replay.
  * Dropout: masks are a function of (seed, element, EPOCH); the first node of the captured step advances the epoch word in
    device memory (``tfgnn_dropout_epoch_advance``), so every replay draws fresh masks and the forward and backward
    kernels of one replay the same ones (include/tfgnn.h "dropout EPOCH").
  * The spread guard of the f16x2 mode (guard.py): its flag is host-mapped memory and keeps working; a replay cannot re-route
    itself to other kernels (``GuardPolicy.begin_backward`` never checks a pass that is being captured), so ``replay()`` reports a trip (``guard_tripped``) instead of demoting anything.  For a model whose
    gradients trip it, either capture in ``bf16x3`` or arm the in-stream repair BEFORE building the step
    (``ops.set_guard_repair(True)``): the weight-gradient products of all five layer kinds - the grouped per-relation
    product of RGIN and the compact-row route included, K range by K range - then repair themselves on the device in every
    replay (a memset node, the product, a repair kernel that returns at once unless the product tripped, the reduce pass -
    all nodes of the graph), the flag stays down and the replayed gradients are the repaired ones.

PyTorch supplies the capture machinery (``torch.cuda.CUDAGraph`` is hipGraph on ROCm: stream capture, a private memory
pool for what the step allocates); nothing of the step's arithmetic runs in torch.
"""
from __future__ import annotations

from typing import Any, Callable, Optional

import torch

from . import ops


class CapturedStep:
    """``step = CapturedStep(fn); step.capture(); for _ in range(K): out = step.replay()``

    ``fn()``: a step on static inputs - e.g. ``lambda: (model(batch, training=True), model.compute_task_metrics(...),
    model.backward())`` - that launches its work through this package on the current stream and returns tensors (or any
    structure of them); the structure returned by ``capture()`` / ``replay()`` is the one ``fn`` returned while being
    captured, its tensors are rewritten by every replay - RETURN whatever a replay is run for (outputs, metrics, the
    ``.grad`` tensors): attributes ``fn`` assigns on the way (``variable.grad = ...``) are Python state of the captured run
    and are re-bound by any later eager call.  ``fn`` must not synchronise with the device (no ``.item()``,
    no new adjacency: ``ops.Graph`` construction reads sizes back) - run it eagerly first (``warmup``) so that every
    lazily built piece exists: weights, the batch's bucketed ``Graph`` (cached on the adjacency tensors), workspaces, the
    synchronous guard passes of a new ``GNN`` (``TFGNN_GUARD_SYNC_PASSES``, ``gnn.guard.sync_passes_left``)."""

    def __init__(self, fn: Callable[[], Any], warmup: int = 4, advance_dropout_epoch: bool = True):
        self._fn = fn
        self._warmup = int(warmup)
        self._advance = bool(advance_dropout_epoch)
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._out = None
        self._stream: Optional[torch.cuda.Stream] = None
        self.replays = 0

    @property
    def captured(self) -> bool:
        return self._graph is not None

    def capture(self):
        if self._graph is not None:
            raise RuntimeError("already captured (make a new CapturedStep for another batch)")
        if not torch.cuda.is_available():
            raise RuntimeError("tf2_gnn_amd: CapturedStep needs a ROCm device (there is no CPU fallback)")
        ops.dropout_epoch()  # the epoch word must exist before the capture (its allocation cannot be captured)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(self._warmup):
                self._fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if ops.get_gemm_mode() == ops.GEMM_F16X2 and ops.f16x2_guard_flag_async():
            raise RuntimeError("the spread guard of the f16x2 mode tripped during the warm-up steps; capture this step in "
                               "ops.set_gemm_mode('bf16x3'), or arm ops.set_guard_repair(True) before building it")
        # every derived form of the weights is rebuilt INSIDE the capture: replays follow in-place weight updates
        ops.clear_weight_operand_cache()
        # the graph-owned gather operands (ops.Graph.gather_operand) count as unfilled: the first gather of each direction
        # inside the captured sequence writes the empty buckets' rows, the later ones keep them, and a replay repeats that
        ops.gather_operands_touched()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            if self._advance:
                ops.dropout_epoch_advance()
            out = self._fn()
        ops.gather_operands_touched()
        self._graph, self._out, self._stream = graph, out, side
        # the derived-weight forms made during the capture live in the graph's memory pool and are rewritten by replays the
        # library's cache cannot see: eager calls after this must rebuild their own
        ops.clear_weight_operand_cache()
        return out

    def replay(self):
        if self._graph is None:
            self.capture()
        self._graph.replay()
        ops.gather_operands_touched()  # (a replay rewrites them: an eager call behind it fills its operand again)
        self.replays += 1
        return self._out

    __call__ = replay

    def guard_tripped(self) -> bool:
        """Has a replayed (or any other) f16x2 product reported operand rows spread over more than 2^20 so far?  Reads the
        host-mapped flag as it stands (call ``torch.cuda.synchronize()`` first to cover the replays enqueued so far)."""
        return bool(ops.f16x2_guard_flag_async())
