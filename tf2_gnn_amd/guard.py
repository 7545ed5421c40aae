"""The spread guard of the f16x2 mode on the host: the mode and its queries (process-wide; ``ops`` re-exports the public names) and
the staged demotion policy of a layer stack (``GuardPolicy``, one per ``GNN``).  DESIGN.md "the spread guard" says what the policy
is for, NOTEBOOK section 27 draws its states.  The library raises the flag WITHOUT a stream synchronisation: a pass that trips it
has produced its gradients by the time the host notices - hence checked passes (``GNN.backward`` waits and recomputes) and, for
the others, late trips (a later query of the mode notices).
"""
from __future__ import annotations

import ctypes
import warnings
import weakref
from types import SimpleNamespace
from typing import Optional

import torch

from . import _lib

GEMM_FP32, GEMM_BF16X3, GEMM_BF16X3_EXACT, GEMM_F16X2 = 0, 6, 9, 3
_GEMM_MODE_NAMES = {"fp32": GEMM_FP32, "bf16x3": GEMM_BF16X3, "bf16x3_9": GEMM_BF16X3_EXACT, "f16x2": GEMM_F16X2}

_S = SimpleNamespace(
    f16x2=False,         # the library's mode as of the last query (it only serves to notice a demotion)
    hold=0,              # depth of hold_spread_guard
    in_late_trip=False,  # the stacks' policies are being asked: their own queries must not dispatch again
    warned=False,        # the warning about the demoted mode is issued once per process
    epoch=0,             # times the f16x2 mode was (re-)armed by set_gemm_mode("f16x2")
    policies=weakref.WeakValueDictionary())  # id -> GuardPolicy of every living stack, in order of construction


def stream_wait() -> None:
    torch.cuda.current_stream().synchronize()


def capturing() -> bool:
    """Is the current stream being captured into a hipGraph (``capture.CapturedStep``)?  Host synchronisation is illegal then."""
    return bool(torch.cuda.is_current_stream_capturing())


def get_gemm_mode() -> int:
    """The mode in force.  When this query is the one that notices that the library has demoted f16x2 for a raised flag, the
    stacks' policies are asked first (a late trip); if none moves, the demotion is announced."""
    s = _S
    if not s.f16x2:
        mode = _lib.load().tfgnn_gemm_get_mode()
        s.f16x2 = mode == GEMM_F16X2
        return mode
    if s.hold or s.in_late_trip:
        return GEMM_F16X2  # a caller that checks the guard synchronously at the end of its pass decides what a trip demotes
    lib = _lib.load()
    mode = lib.tfgnn_gemm_get_mode()  # ONE read of the flag decides, the library's: a second one here could straddle its raising
    if mode != GEMM_F16X2:
        if lib.tfgnn_sp_spread_flag(0):
            if s.policies and not capturing() and _dispatch_late_trip(lib):
                return GEMM_F16X2
            _warn_mode_demoted()
        s.f16x2 = False
    return mode


def _dispatch_late_trip(lib) -> bool:
    """If a stack that ran unchecked passes has a stage to give, the mode goes back on (tfgnn_gemm_set_mode waits for the device
    and clears the flag).  -> did any policy move?"""
    _S.in_late_trip = True
    try:
        handled = [w for w in (p.on_late_trip() for p in list(_S.policies.values())) if w]
        if handled:
            _lib.check(lib.tfgnn_gemm_set_mode(GEMM_F16X2))
            warnings.warn("tf2_gnn_amd: operand rows of a weight-gradient product spread beyond the range of the split-operand "
                          "product that ran, in a pass that was not checked synchronously (its gradients may have lost "
                          "low-order rows): " + "; ".join(handled) + "; the next passes are checked again")
        return bool(handled)
    finally:
        _S.in_late_trip = False


def _warn_mode_demoted() -> None:
    if not _S.warned:
        _S.warned = True
        warnings.warn("tf2_gnn_amd: operand rows of a weight-gradient product spread over more than 2^20 in magnitude; "
                      "the f16x2 layer paths are switched to the exact bf16x3 kernels (ops.set_gemm_mode('f16x2') re-arms them)")


def warn_recomputed(what: str) -> None:
    warnings.warn(f"tf2_gnn_amd: operand rows of a weight-gradient product of this GNN are spread beyond the range "
                  f"of the split-operand product that ran: {what}; the pass was recomputed")


def reset_warned() -> None:  # (tests: the once-per-process warning may be issued again)
    _S.warned = False


def forget_policies() -> None:  # (tests: with no stack's policy registered a late trip demotes the mode on sight)
    _S.policies.clear()


def set_gemm_mode(mode) -> int:
    """Select how the Dense products are evaluated: "fp32" (fp32 MFMA), "bf16x3" (exact 3-way bf16 split of both operands,
    6 piece products), "bf16x3_9" (all 9) or "f16x2": the layers hand the hot products pre-split SP16 operands
    (tfgnn_sp_gemm_*: 2-way fp16 split, 3 piece products, the gather writes the operand) and every other product runs as in
    "bf16x3" - include/tfgnn.h, tfgnn_gemm_set_mode.  "f16x2" is the DEFAULT of the library (environment TFGNN_GEMM_MODE
    overrides); its spread guard (tfgnn_sp_spread_flag) demotes it to "bf16x3" when an operand's row scales spread over more
    than 2^20; setting "f16x2" again re-arms the guard (waits for the device) and every stack's policy
    (``GuardPolicy.sync_with_rearm_epoch``).  Returns the previous mode id."""
    prev = get_gemm_mode()
    mode = _GEMM_MODE_NAMES.get(mode, mode)
    _lib.check(_lib.load().tfgnn_gemm_set_mode(mode))
    _S.f16x2 = mode == GEMM_F16X2
    if _S.f16x2:
        _S.epoch += 1
    return prev


def demote_gemm_mode() -> int:
    """Let the library act on a set spread flag NOW, also inside ``hold_spread_guard`` -> the mode in force afterwards."""
    held, _S.hold = _S.hold, 0
    try:
        return get_gemm_mode()
    finally:
        _S.hold = held


class hold_spread_guard:
    """Inside this context a tripped spread flag does not demote the mode on sight: the caller reads the flag itself
    (``f16x2_guard_tripped_sync``) when its pass is complete and decides what to demote (``GNN.backward``)."""

    def __enter__(self):
        get_gemm_mode()
        _S.hold += 1
        return self

    def __exit__(self, *exc):
        _S.hold -= 1
        return False


def rearm_spread_guard() -> None:
    """Clear the spread flag WITHOUT demoting the mode (the caller has dealt with the product that tripped it).  Waits for the
    stream first: a factor computation still in flight must not set it again."""
    stream_wait()
    _lib.load().tfgnn_sp_spread_flag(1)


def f16x2_guard_flag_async() -> bool:
    """The spread flag as the host sees it NOW, without waiting for the device (what earlier products have reported so far)."""
    return bool(_lib.load().tfgnn_sp_spread_flag(0))


def f16x2_guard_tripped_sync() -> bool:
    """Wait for the current stream, then read the spread guard: True if a split weight-gradient product enqueued so far met
    operand rows spread over more than 2^20 (its result may have lost low-order rows)."""
    stream_wait()
    return f16x2_guard_flag_async()


def set_guard_repair(on: bool) -> bool:
    """Arm (True) or disarm the in-stream repair of tripped split-operand weight-gradient products (include/tfgnn.h,
    tfgnn_sp_guard_repair) -> the previous state.  While armed, ``sp_gemm_tn`` (both forms), the product inside
    ``mp_backward`` and ``sp_gemm_tn_grouped`` recompute what their spread guard reports in fp32 from the SP16 operands, on
    the stream and before their reduce pass - the plain products whole, the grouped product the K ranges that tripped: the
    pass's own gradients are right, the host flag stays down, the mode stays ``f16x2`` and no stack's ``GuardPolicy`` takes a
    stage - also in a replayed ``capture.CapturedStep`` (arm before building it; arming allocates, so not while capturing).
    Off by default (environment TFGNN_GUARD_REPAIR=1 arms at start)."""
    if capturing():
        raise RuntimeError("tf2_gnn_amd: set_guard_repair is not legal while the stream is capturing (arm before the capture)")
    rc = _lib.load().tfgnn_sp_guard_repair(1 if on else 0)
    if rc < 0:
        _lib.check(rc)
    return bool(rc)


def guard_repair() -> bool:
    """Is the in-stream repair of tripped weight-gradient products armed (``set_guard_repair``)?"""
    return bool(_lib.load().tfgnn_sp_guard_repair(-1))


def repair_stats(reset: bool = False) -> dict:
    """{"armed_products": products enqueued with repair armed (host counter), "repaired_products": products the device
    repaired}; waits for the device (not legal while capturing).  ``reset`` clears both."""
    buf = (ctypes.c_int64 * 2)()
    _lib.check(_lib.load().tfgnn_sp_repair_stats(buf, int(bool(reset))))
    return {"armed_products": int(buf[0]), "repaired_products": int(buf[1])}


class GuardPolicy:
    """One stack's part.  ``dense``: split -> wide (stage 1a: the Dense / projection weight gradients on the two-factor TN
    product, 2^22 per operand) -> exact (1b: the Dense products on the bf16x3 kernels); ``grouped_tn``: split -> exact (2: the
    per-relation MLP weight gradients of the layers that ran one on the bf16x3 kernels, ``layer._grouped_tn_split_ok``).
    ``step``: a bound method of the stack, held weakly, that walks one stage (``GNN._advance_guard``).  ``tripped_last_backward``:
    after a checked pass, was it recomputed; for an unchecked one the flag as it stood when the pass was enqueued."""

    def __init__(self, step, sync_passes: int = 3, check_every: int = 0):
        self._step = weakref.WeakMethod(step) if step is not None else (lambda: None)
        self.dense, self.grouped_tn = "split", "split"
        self.dense_epoch = self.grouped_tn_epoch = -1  # _S.epoch when each was last demoted
        self.sync_passes_init = self.sync_passes_left = sync_passes
        self.check_every = check_every
        self.backward_passes = 0
        self.unchecked_epoch = -1  # _S.epoch at the last f16x2 pass that was not checked, -1: none since the last checked one
        self.late_trip_pass = -1  # the backward pass whose late trip moved the policy (one stage per pass)
        self.tripped_last_backward: Optional[bool] = None
        _S.policies[id(self)] = self

    @property
    def stage(self) -> str:
        return "2" if self.grouped_tn == "exact" else {"split": "none", "wide": "1a", "exact": "1b"}[self.dense]

    def state(self) -> dict:
        """-> ``GNN.guard_state()``; stage "3": the whole mode went"""
        stage = self.stage
        if self.backward_passes and get_gemm_mode() != GEMM_F16X2 and (stage != "none" or f16x2_guard_flag_async()):
            stage = "3"
        return {"tripped": self.tripped_last_backward, "stage": stage, "checked_passes_left": self.sync_passes_left}

    def sync_with_rearm_epoch(self, forward_layers=None) -> None:
        """The mode was re-armed after this stack demoted something: it tries the split operands again, with its checked first
        passes.  A Dense query (no argument) restores ``dense``; the start of a forward pass (the stack's layers) restores
        ``grouped_tn`` - never inside a backward pass: the layers read ``_grouped_tn_split_ok`` when they choose their route."""
        if forward_layers is None:
            if self.dense == "split" or self.dense_epoch == _S.epoch:
                return
            self.dense = "split"
        else:
            if self.grouped_tn == "split" or self.grouped_tn_epoch == _S.epoch:
                return
            self.grouped_tn = "split"
            for mp in forward_layers:
                mp._grouped_tn_split_ok = True
        self.sync_passes_left = max(self.sync_passes_left, self.sync_passes_init)

    def begin_backward(self, mode_is_f16x2: bool, capturing: bool) -> bool:
        """Count a backward pass -> is it a checked one?"""
        self.backward_passes += 1
        periodic = self.check_every > 0 and self.backward_passes % self.check_every == 0
        if capturing:  # a step being captured into a hipGraph cannot wait for the device: never a checked pass
            if mode_is_f16x2 and self.sync_passes_left > 0:
                raise RuntimeError("tf2_gnn_amd: this GNN's first backward passes are checked synchronously "
                                   f"(TFGNN_GUARD_SYNC_PASSES, {self.sync_passes_left} left); run them eagerly before "
                                   "capturing the step (capture.CapturedStep warmup)")
            periodic = False
        checked = mode_is_f16x2 and (self.sync_passes_left > 0 or periodic)
        if checked:
            self.sync_passes_left = max(self.sync_passes_left - 1, 0)
            self.unchecked_epoch = -1
        elif mode_is_f16x2:
            self.unchecked_epoch = _S.epoch
        self.tripped_last_backward = bool(mode_is_f16x2 and not checked and f16x2_guard_flag_async())
        return checked

    def advance(self, layers, dense_possible: bool) -> Optional[str]:
        """One stage: the weight-gradient products whose operand ROWS are un-normalised sums change kernels; the message
        products keep their split operands.  ``dense_possible``: the stack runs its Dense products on split operands now.
        -> what was demoted, None: nothing is left."""
        if dense_possible:
            self.dense_epoch = _S.epoch
            if self.dense == "split":
                self.dense = "wide"
                return "the Dense / projection weight gradients (now on the two-factor split-operand product)"
            self.dense = "exact"
            return "the Dense / projection products (now on the exact bf16x3 kernels)"
        used = [mp for mp in layers if mp._grouped_tn_used and mp._grouped_tn_split_ok]
        for mp in used:
            mp._grouped_tn_split_ok = False
        if not used:
            return None
        self.grouped_tn, self.grouped_tn_epoch = "exact", _S.epoch
        return "the per-relation MLP weight gradients (now on the exact bf16x3 kernels)"

    def on_late_trip(self) -> Optional[str]:
        """-> what changed kernels for the trip of an unchecked pass, None: nothing left / not this stack's pass"""
        if self.unchecked_epoch != _S.epoch:
            return None  # (no unchecked pass of this stack since the mode was last armed: somebody else's products)
        if self.late_trip_pass == self.backward_passes:
            return "(this stack's policy has moved a step for that pass already)"
        step = self._step()
        what = step() if step is not None else None
        if what:
            self.late_trip_pass = self.backward_passes
            self.sync_passes_left = max(self.sync_passes_left, self.sync_passes_init)
            self.tripped_last_backward = True
        return what
