"""The optimizer step of the training loop: ``GraphTaskModel._make_optimizer`` / ``_apply_gradients``
(tf2_gnn/models/graph_task_model.py:224-324) and ``PolynomialWarmupAndDecaySchedule``
(tf2_gnn/utils/polynomial_warmup_and_decay_schedule.py) on one HIP entry point, ``tfgnn_optimizer_apply`` (csrc/optim.hip).

The arithmetic is that of the TF 2.x Keras optimizers the reference's hyper-parameters were tuned with (SGD / RMSprop / Adam,
epsilon 1e-7, lr inside the momentum buffers) - not torch.optim's: include/tfgnn.h "Optimizer step" states it.  One call
updates every variable: clipping, the slot updates and the weight write are one launch per 32 tensors (plus one for the
norm modes).  The learning rate is computed on the device from the step counter ``iterations``, which the call advances on
the device: a step captured with ``CapturedStep`` (forward + metrics + backward + ``apply_gradients``) is one complete training
iteration per replay and follows the schedule.

A gradient may also be a ``RowGradient`` - the rows of a lookup and their ids, the counterpart of ``tf.IndexedSlices`` - and then
the call is ``tfgnn_optimizer_apply_rows``: the listed rows of the variable and of its slots get the dense step's arithmetic,
every other row is neither read nor written (the LAZY variant of the optimizer: see ``RowGradient``).
"""
from __future__ import annotations

import ctypes
from typing import Any, Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops

OPT_SGD, OPT_RMSPROP, OPT_ADAM = 0, 1, 2
CLIP_NONE, CLIP_VALUE, CLIP_NORM, CLIP_GLOBAL_NORM = 0, 1, 2, 3
_CLIP_MODES = {None: CLIP_NONE, "value": CLIP_VALUE, "norm": CLIP_NORM, "global_norm": CLIP_GLOBAL_NORM}


class PolynomialWarmupAndDecaySchedule:
    """utils/polynomial_warmup_and_decay_schedule.py: the learning rate rises from ``initial_learning_rate`` to ``learning_rate``
    over ``warmup_steps`` steps (polynomial of degree ``power``), then falls to ``final_learning_rate`` over ``decay_steps``
    steps and stays there.  The optimizer evaluates it on the device; ``__call__`` is the same formula on the host, in fp32
    like the device (and like the float32 step Keras hands a schedule)."""

    def __init__(self, learning_rate: float, warmup_steps: int, decay_steps: int, initial_learning_rate: float,
                 final_learning_rate: float, power: float = 1.0, name: Optional[str] = None):
        self.learning_rate = learning_rate
        self.initial_learning_rate = initial_learning_rate
        self.final_learning_rate = final_learning_rate
        self.warmup_steps = warmup_steps
        self.decay_steps = decay_steps
        self.power = power
        self.name = name

    def get_config(self) -> Dict[str, Any]:
        return {
            "learning_rate": self.learning_rate,
            "initial_learning_rate": self.initial_learning_rate,
            "final_learning_rate": self.final_learning_rate,
            "warmup_steps": self.warmup_steps,
            "decay_steps": self.decay_steps,
            "power": self.power,
            "name": self.name,
        }

    def __call__(self, step) -> float:
        f = np.float32
        step, warmup, decay = f(step), f(self.warmup_steps), f(self.decay_steps)
        lr, power = f(self.learning_rate), f(self.power)
        with np.errstate(divide="ignore", invalid="ignore"):
            if step <= warmup:
                lr0 = f(self.initial_learning_rate)
                return float((lr - lr0) * np.power(step / warmup, power) + lr0)
            lr1 = f(self.final_learning_rate)
            effective_step = np.minimum(step - warmup, decay)
            return float((lr - lr1) * np.power(f(1) - effective_step / decay, power) + lr1)


def _rows(t: torch.Tensor) -> Optional[Tuple[int, int, int]]:
    """(rows, cols, row stride) of a tensor as a row-major 2-D view with unit inner stride, or None."""
    if t.dim() == 0:
        return 1, 1, 1
    if t.dim() == 1:
        return (1, t.shape[0], t.shape[0]) if t.stride(0) == 1 or t.shape[0] <= 1 else None
    if t.stride(-1) != 1 and t.shape[-1] > 1:
        return None
    for i in range(t.dim() - 2):  # leading dimensions must collapse into one
        if t.shape[i] > 1 and t.stride(i) != t.stride(i + 1) * t.shape[i + 1]:
            return None
    cols = t.shape[-1]
    return t.numel() // max(cols, 1), cols, t.stride(-2)


class RowGradient:
    """The gradient of a row lookup ``table[ids]`` (``ops.gather_node_rows``) against a table of ``num_rows`` rows, kept as the
    pair it is: ``rows`` float32 [n, D] (unit inner stride, any row pitch >= D) and ``ids`` int32 [n], DISTINCT by precondition
    (the neighbour sampler guarantees it).  It stands for the dense [num_rows, D] gradient that is ``rows[i]`` at row
    ``ids[i]`` and zero elsewhere - ``tf.IndexedSlices`` without repeated indices.

    ``Optimizer.apply_gradients`` updates the listed rows only (tfgnn_optimizer_apply_rows): their values and slots get exactly
    the dense step's arithmetic, all other rows and their slots are not touched.  For plain SGD (momentum 0) that IS the dense
    step.  For SGD with momentum, RMSprop and Adam it is the lazy variant (LazyAdam / SparseAdam): the moments of rows without
    a gradient do not decay and those rows do not move, where the dense step would keep moving them along their old moments.
    An id outside [0, num_rows) skips its row and sets ``bad_flag`` (a zeroed int32 [1] on the device, optional)."""

    def __init__(self, rows: torch.Tensor, ids: torch.Tensor, num_rows: int, bad_flag: Optional[torch.Tensor] = None):
        if not isinstance(rows, torch.Tensor) or rows.dtype != torch.float32 or rows.dim() != 2:
            raise ValueError("RowGradient: rows must be a float32 [n, D] tensor")
        if rows.shape[1] < 1 or (rows.shape[1] > 1 and rows.stride(1) != 1) or (rows.shape[0] > 1 and rows.stride(0) < rows.shape[1]):
            raise ValueError(f"RowGradient: rows must have D >= 1 columns at unit stride and a row pitch >= D (shape "
                             f"{tuple(rows.shape)}, strides {tuple(rows.stride())})")
        if not isinstance(ids, torch.Tensor) or ids.dtype != torch.int32 or ids.dim() != 1 or (ids.shape[0] > 1 and ids.stride(0) != 1):
            raise ValueError("RowGradient: ids must be a contiguous int32 [n] tensor")
        if ids.shape[0] != rows.shape[0]:
            raise ValueError(f"RowGradient: {int(ids.shape[0])} ids for {int(rows.shape[0])} rows")
        if ids.device != rows.device:
            raise ValueError(f"RowGradient: rows on {rows.device}, ids on {ids.device}")
        if isinstance(num_rows, bool) or not isinstance(num_rows, (int, np.integer)) or not 0 <= num_rows < 2 ** 31:
            raise ValueError(f"RowGradient: num_rows must be an integer in [0, 2^31), not {num_rows!r}")
        if rows.shape[0] > num_rows:
            raise ValueError(f"RowGradient: {int(rows.shape[0])} rows for a table of {int(num_rows)} (the ids are distinct)")
        if bad_flag is not None and (not isinstance(bad_flag, torch.Tensor) or bad_flag.dtype != torch.int32 or bad_flag.numel() != 1
                                     or bad_flag.device != rows.device):
            raise ValueError("RowGradient: bad_flag must be an int32 tensor of one element on the device of rows")
        self.rows, self.ids, self.num_rows, self.bad_flag = rows, ids, int(num_rows), bad_flag

    @property
    def shape(self) -> Tuple[int, int]:
        """the shape of the dense gradient it stands for"""
        return (self.num_rows, int(self.rows.shape[1]))

    @property
    def device(self):
        return self.rows.device

    def to_dense(self, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the dense [num_rows, D] gradient (ops.embedding_scatter_rows: a fill and a scatter)"""
        return ops.embedding_scatter_rows(self.rows, self.ids, self.num_rows, out=out, bad_flag=self.bad_flag)


class Optimizer:
    """A Keras optimizer (SGD, RMSprop, Adam) over this package's ``Variable``s.  ``learning_rate``: a float or a
    ``PolynomialWarmupAndDecaySchedule``.  Slots are allocated at the first update of a variable and start at zero."""

    def __init__(self, kind: str, learning_rate=0.001, momentum: float = 0.0, rho: float = 0.9, beta_1: float = 0.9,
                 beta_2: float = 0.999, epsilon: float = 1e-7):
        kinds = {"sgd": OPT_SGD, "rmsprop": OPT_RMSPROP, "adam": OPT_ADAM}
        if kind.lower() not in kinds:
            raise ValueError(f'Unknown optimizer "{kind}".')
        if not 0.0 <= float(momentum) <= 1.0:
            raise ValueError("`momentum` must be between [0, 1].")
        self.kind = kind.lower()
        self.learning_rate = learning_rate
        self.momentum, self.rho = float(momentum), float(rho)
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        self._kind_id = kinds[self.kind]
        self._nslots = {OPT_SGD: 1 if self.momentum > 0 else 0, OPT_RMSPROP: 2 if self.momentum > 0 else 1, OPT_ADAM: 2}[self._kind_id]
        self._slots: Dict[int, Tuple[Any, list]] = {}  # id(variable) -> (variable, [slot tensors])
        self._state: Optional[torch.Tensor] = None    # int64 [2] on the device: iterations, ticket
        self._workspace: Optional[torch.Tensor] = None
        cfg = _lib.OptConfig()
        cfg.struct_size = ctypes.sizeof(_lib.OptConfig)
        cfg.kind = self._kind_id
        cfg.momentum, cfg.rho, cfg.beta_1, cfg.beta_2, cfg.epsilon = self.momentum, self.rho, self.beta_1, self.beta_2, self.epsilon
        lr = learning_rate
        if isinstance(lr, PolynomialWarmupAndDecaySchedule):
            cfg.schedule = 1
            cfg.learning_rate, cfg.initial_learning_rate, cfg.final_learning_rate = lr.learning_rate, lr.initial_learning_rate, lr.final_learning_rate
            cfg.power, cfg.warmup_steps, cfg.decay_steps = lr.power, int(lr.warmup_steps), int(lr.decay_steps)
        else:
            cfg.schedule, cfg.learning_rate = 0, float(lr)
        self._cfg = cfg

    def slots(self, variable) -> list:
        """the slot tensors of a variable ([] before its first update): SGD [accumulator]; RMSprop [mean square(, momentum)];
        Adam [m, v] - flat fp32 arrays of the variable's size"""
        hit = self._slots.get(id(variable))
        return list(hit[1]) if hit is not None else []

    def _ensure_state(self, device):
        if self._state is None:
            self._state = torch.zeros(2, dtype=torch.int64, device=device)
        return self._state

    @property
    def iterations(self) -> int:
        """The number of updates applied so far (the device counter the learning rate is computed from).  Reading it
        synchronises with the current stream."""
        if self._state is None:
            return 0
        out = torch.empty(1, dtype=torch.int64, device=self._state.device)
        _lib.check(_lib.load().tfgnn_optimizer_iterations_get(ops._ptr(self._state), ops._ptr(out), ops._stream()))
        return int(out.item())

    @iterations.setter
    def iterations(self, value: int):
        if self._state is None:
            raise RuntimeError("the optimizer has no device state before its first update")
        _lib.check(_lib.load().tfgnn_optimizer_iterations_set(ops._ptr(self._state), int(value), ops._stream()))

    def apply_gradients(self, pairs: Iterable[Tuple[Any, Optional[torch.Tensor]]], clip: Optional[Tuple[str, float]] = None) -> None:
        """Update every variable of ``pairs`` - ``(variable, grad)`` as ``GraphTaskModel.backward()`` returns them, or Keras'
        ``(grad, variable)`` - in one library call on the current stream.  Pairs whose gradient is None are dropped (no slot
        update, not part of the global norm).  A gradient may be a ``RowGradient``: its variable's listed rows are updated and
        no others, in the same call (tfgnn_optimizer_apply_rows; without one the call is tfgnn_optimizer_apply).  ``clip``:
        None, ``("value", c)``, ``("norm", c)`` or ``("global_norm", c)``, applied to the gradients first
        (graph_task_model.py:296-322).  Does not synchronise: it can be captured."""
        from .layers.message_passing.message_passing import Variable

        mode = _CLIP_MODES.get(clip[0] if clip is not None else None)
        if mode is None:
            raise ValueError(f"unknown clip mode {clip[0]!r} (value, norm, global_norm)")
        live = []
        for a, b in pairs:
            var, grad = (a, b) if isinstance(a, Variable) else (b, a)
            if grad is not None:
                live.append((var, grad))
        if not live:
            raise ValueError("No gradients provided for any variable.")
        dev = live[0][0].value.device
        state = self._ensure_state(dev)
        dense = [(var, grad) for var, grad in live if not isinstance(grad, RowGradient)]
        sparse = [(var, grad) for var, grad in live if isinstance(grad, RowGradient)]
        rows = np.empty((len(dense), 8), dtype=np.int64)
        bases = {}

        def slots_of(var, w):
            hit = self._slots.get(id(var))
            if hit is None or hit[0] is not var:
                hit = (var, [torch.zeros(w.numel(), dtype=torch.float32, device=dev) for _ in range(self._nslots)])
                self._slots[id(var)] = hit
            base = w._base if w._base is not None else w
            bases.setdefault(base.data_ptr(), w)
            return hit[1] + [None, None]

        for i, (var, grad) in enumerate(dense):
            w = var.value
            if tuple(grad.shape) != tuple(w.shape):
                raise ValueError(f"gradient of {var.name} has shape {tuple(grad.shape)}, the variable {tuple(w.shape)}")
            ops._require_dev(w, torch.float32, var.name)
            ops._require_dev(grad, torch.float32, f"gradient of {var.name}")
            lw, lg = _rows(w), _rows(grad)
            if lw is None or lg is None or lw[:2] != lg[:2]:
                raise ValueError(f"{var.name}: value and gradient must be row-major views with unit inner stride")
            s = slots_of(var, w)
            rows[i] = (w.data_ptr(), lw[2], grad.data_ptr(), lg[2], lw[0], lw[1],
                       s[0].data_ptr() if s[0] is not None else 0, s[1].data_ptr() if s[1] is not None else 0)
        lib = _lib.load()
        cfg = self._cfg
        cfg.clip, cfg.clip_value = mode, float(clip[1]) if clip is not None else 0.0
        cfg.state = state.data_ptr()
        if sparse:
            if len(sparse) > _lib.OPT_MAX_ROW_TENSORS:
                raise ValueError(f"{len(sparse)} row gradients in one call (at most {_lib.OPT_MAX_ROW_TENSORS})")
            row_tensors = (_lib.OptRowTensor * len(sparse))()
            for r, (var, grad) in zip(row_tensors, sparse):
                w = var.value
                if w.dim() != 2 or tuple(grad.shape) != tuple(w.shape) or (w.shape[1] > 1 and w.stride(1) != 1) or (
                        w.shape[0] > 1 and w.stride(0) < w.shape[1]):
                    raise ValueError(f"row gradient of {var.name} stands for shape {tuple(grad.shape)}, the variable is "
                                     f"{tuple(w.shape)} (a 2-D row-major table with unit inner stride)")
                ops._require_dev(w, torch.float32, var.name)
                ops._require_dev(grad.rows, torch.float32, f"row gradient of {var.name}")
                ops._require_dev(grad.ids, torch.int32, f"ids of the row gradient of {var.name}")
                s = slots_of(var, w)
                n, cols = int(grad.rows.shape[0]), int(w.shape[1])
                r.value, r.ld_value = w.data_ptr(), max(int(w.stride(0)), cols) if w.shape[0] > 1 else cols
                r.grad_rows, r.ld_grad = (grad.rows.data_ptr() if n else None), (int(grad.rows.stride(0)) if n > 1 else cols)
                r.ids, r.n, r.N, r.cols = (grad.ids.data_ptr() if n else None), n, int(w.shape[0]), cols
                r.slot0 = s[0].data_ptr() if s[0] is not None else None
                r.slot1 = s[1].data_ptr() if s[1] is not None else None
                r.bad_flag = grad.bad_flag.data_ptr() if grad.bad_flag is not None else None
            ws_bytes = lib.tfgnn_optimizer_rows_workspace_bytes(rows.ctypes.data, len(dense), row_tensors, len(sparse), mode)
        else:
            ws_bytes = lib.tfgnn_optimizer_workspace_bytes(rows.ctypes.data, len(dense), mode)
        if ws_bytes and (self._workspace is None or self._workspace.numel() < ws_bytes):
            self._workspace = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        cfg.workspace = self._workspace.data_ptr() if ws_bytes else None
        cfg.workspace_bytes = self._workspace.numel() if ws_bytes else 0
        if sparse:
            _lib.check(lib.tfgnn_optimizer_apply_rows(rows.ctypes.data, len(dense), row_tensors, len(sparse), ctypes.byref(cfg),
                                                      ops._stream()))
        else:
            _lib.check(lib.tfgnn_optimizer_apply(rows.ctypes.data, len(dense), ctypes.byref(cfg), ops._stream()))
        for w in bases.values():  # the weights changed behind torch's version counter: drop their derived forms, once per buffer
            ops.notify_weights_changed(w)


def make_optimizer(params: Dict[str, Any], learning_rate=None) -> Optimizer:
    """GraphTaskModel._make_optimizer (graph_task_model.py:224-277), rule for rule."""
    if learning_rate is None:
        learning_rate = params["learning_rate"]
        num_warmup_steps = params.get("learning_rate_warmup_steps")
        num_decay_steps = params.get("learning_rate_decay_steps")
        if num_warmup_steps is not None or num_decay_steps is not None:
            initial_learning_rate = 0.00001
            final_learning_rate = 0.00001
            if num_warmup_steps is None:
                num_warmup_steps = -1  # no warm-up phase
                initial_learning_rate = learning_rate
            if num_decay_steps is None:
                num_decay_steps = 1  # value does not matter, but must be non-zero
                final_learning_rate = learning_rate
            learning_rate = PolynomialWarmupAndDecaySchedule(
                learning_rate=learning_rate,
                warmup_steps=num_warmup_steps,
                decay_steps=num_decay_steps,
                initial_learning_rate=initial_learning_rate,
                final_learning_rate=final_learning_rate,
                power=1.0,
            )
    optimizer_name = params["optimizer"].lower()
    if optimizer_name == "sgd":
        return Optimizer("sgd", learning_rate=learning_rate, momentum=params["momentum"])
    elif optimizer_name == "rmsprop":
        return Optimizer("rmsprop", learning_rate=learning_rate, momentum=params["momentum"], rho=params["rmsprop_rho"])
    elif optimizer_name == "adam":
        return Optimizer("adam", learning_rate=learning_rate)
    else:
        raise Exception('Unknown optimizer "%s".' % (params["optimizer"]))
