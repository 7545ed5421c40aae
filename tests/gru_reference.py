"""fp64 host reference of the GRUCell gate math (csrc/elementwise.hip: ``ops.gru_gates_forward``, ``ops.gru_gates_backward``,
``ops.gru_gates_backward_sp``; [ext] tf.keras.layers.GRUCell, reset_after=True).  Plain torch on the CPU, closed form, no
device code.  mx, mh are [V, 3H] in gate order z | r | c:
    z = sigmoid(mx_z + mh_z);  r = sigmoid(mx_r + mh_r);  c = tanh(mx_c + r * mh_c);  h' = z * h + (1 - z) * c
tests/test_gru_reference_host.py pins these functions to torch.autograd so that a mistake here is not read as a kernel bug."""
from __future__ import annotations

import torch


def _f64(t):
    return torch.as_tensor(t).detach().cpu().double()


def gru_forward(mx, mh, h):
    """-> (h_new [V, H], gates [V, 3H] = z | r | c) in fp64 from the given inputs cast up"""
    mx, mh, h = _f64(mx), _f64(mh), _f64(h)
    H = h.shape[1]
    assert mx.shape == mh.shape == (h.shape[0], 3 * H)
    z = torch.sigmoid(mx[:, :H] + mh[:, :H])
    r = torch.sigmoid(mx[:, H:2 * H] + mh[:, H:2 * H])
    c = torch.tanh(mx[:, 2 * H:] + r * mh[:, 2 * H:])
    return z * h + (1.0 - z) * c, torch.cat([z, r, c], dim=1)


def gru_backward(dh_new, gates, mh, h, factor=None):
    """Gradients of sum(h' * dh_new) from the SAVED gates (the kernels receive the fp32 gates: cast up, their rounding is not
    part of a comparison) -> (dmx [V, 3H], dmh [V, 3H], dh_direct [V, H], bias_grad [2, 3H]) in fp64.
    dh_direct = dh_new * z (* factor: the dropout mask of the layer input); bias_grad = the column sums of dmx and dmh."""
    g, gates, mh, h = _f64(dh_new), _f64(gates), _f64(mh), _f64(h)
    H = h.shape[1]
    assert gates.shape == mh.shape == (h.shape[0], 3 * H) and g.shape == h.shape
    z, r, c = gates[:, :H], gates[:, H:2 * H], gates[:, 2 * H:]
    hh = mh[:, 2 * H:]
    dpc = g * (1.0 - z) * (1.0 - c * c)   # d pre-activation of the candidate
    dpz = g * (h - c) * z * (1.0 - z)     # ... of the update gate
    dpr = dpc * hh * r * (1.0 - r)        # ... of the reset gate
    dmx = torch.cat([dpz, dpr, dpc], dim=1)
    dmh = torch.cat([dpz, dpr, dpc * r], dim=1)
    dh_direct = g * z
    if factor is not None:
        dh_direct = dh_direct * _f64(factor)
    return dmx, dmh, dh_direct, torch.stack([dmx.sum(dim=0), dmh.sum(dim=0)], dim=0)
