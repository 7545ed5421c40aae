"""The row-sparse ("lazy") optimizer step in fp64: tests/optim_model64.Optimizer64, unchanged, applied to the gathered rows of a
table and of its slots (include/tfgnn.h "The row-sparse step": listed rows get the dense arithmetic, all others are not touched)."""
from __future__ import annotations

import numpy as np

from tests.optim_model64 import Optimizer64


class LazyRows64:
    """``table`` float64 [N, D], updated in place by ``step(ids, rows)``; the slots [N, D] start at zero."""

    def __init__(self, table: np.ndarray, kind, lr, momentum=0.0, rho=0.9, clip=None):
        self.table = table
        self.slots = [np.zeros_like(table), np.zeros_like(table)]
        self.opt = Optimizer64(kind, lr, momentum=momentum, rho=rho, clip=clip)

    def step(self, ids: np.ndarray, rows: np.ndarray) -> None:
        w = self.table[ids].copy()
        self.opt.slots[0] = [s[ids].copy() for s in self.slots]
        self.opt.step([w], [np.asarray(rows, dtype=np.float64)])
        self.table[ids] = w
        for s, new in zip(self.slots, self.opt.slots[0]):
            s[ids] = new
