"""An independent fp64 restatement of the optimizer step the library runs (include/tfgnn.h "Optimizer step"): the TF 2.x Keras
optimizer_v2 update rules, the gradient clipping of GraphTaskModel._apply_gradients (graph_task_model.py:296-322) and the
polynomial warm-up / decay schedule (utils/polynomial_warmup_and_decay_schedule.py:90-111).  Hyper-parameters enter as the
float32 numbers TF computes with (its hyper-parameters are float32 tensors); everything else is float64."""
from __future__ import annotations

import math

import numpy as np


def f32(x: float) -> float:
    return float(np.float32(x))


def schedule64(step: int, learning_rate, warmup_steps, decay_steps, initial_learning_rate, final_learning_rate, power=1.0):
    step = float(step)
    lr, lr0, lr1 = f32(learning_rate), f32(initial_learning_rate), f32(final_learning_rate)
    if step <= warmup_steps:
        return (lr - lr0) * (step / warmup_steps) ** power + lr0
    effective = min(step - warmup_steps, decay_steps)
    return (lr - lr1) * (1.0 - effective / decay_steps) ** power + lr1


def clip64(grads, clip):
    """grads: list of float64 arrays -> clipped copies."""
    if clip is None:
        return [g.copy() for g in grads]
    mode, c = clip[0], f32(clip[1])
    if mode == "value":
        return [np.clip(g, -c, c) for g in grads]
    if mode == "norm":
        return [g * c / max(math.sqrt(float((g * g).sum())), c) for g in grads]
    assert mode == "global_norm"
    norm = math.sqrt(sum(float((g * g).sum()) for g in grads))
    scale = c * min(1.0 / norm, 1.0 / c) if math.isfinite(norm) else float("nan")
    return [g * scale for g in grads]


class Optimizer64:
    """kind "sgd" | "rmsprop" | "adam"; lr: a float or a function step -> lr.  ``step(weights, grads)`` updates float64 weight
    arrays in place; slots are kept per index of the list."""

    def __init__(self, kind, lr, momentum=0.0, rho=0.9, clip=None):
        self.kind, self.lr, self.clip = kind, lr, clip
        self.mu, self.rho = f32(momentum), f32(rho)
        self.b1, self.b2, self.eps = f32(0.9), f32(0.999), f32(1e-7)
        self.iterations = 0
        self.slots = {}

    def step(self, weights, grads):
        lr = self.lr(self.iterations) if callable(self.lr) else f32(self.lr)
        gs = clip64(grads, self.clip)
        for i, (w, g) in enumerate(zip(weights, gs)):
            s = self.slots.setdefault(i, [np.zeros_like(w), np.zeros_like(w)])
            if self.kind == "sgd":
                if self.mu > 0:
                    s[0][...] = s[0] * self.mu - lr * g
                    w += s[0]
                else:
                    w -= lr * g
            elif self.kind == "rmsprop":
                if self.mu > 0:
                    s[0] += (g * g - s[0]) * (1.0 - self.rho)
                    s[1][...] = s[1] * self.mu + lr * g / np.sqrt(s[0] + self.eps)
                    w -= s[1]
                else:
                    s[0][...] = self.rho * s[0] + (1.0 - self.rho) * g * g
                    w -= lr * g / (np.sqrt(s[0]) + self.eps)
            else:
                t = self.iterations + 1
                alpha = lr * math.sqrt(1.0 - self.b2 ** t) / (1.0 - self.b1 ** t)
                s[0] += (g - s[0]) * (1.0 - self.b1)
                s[1] += (g * g - s[1]) * (1.0 - self.b2)
                w -= s[0] * alpha / (np.sqrt(s[1]) + self.eps)
        self.iterations += 1
