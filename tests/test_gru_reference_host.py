"""tests/gru_reference.py against torch.autograd in fp64 (CPU only): a bug in the closed-form reference of
tests/test_gpu_gru_gates.py must not be read as a kernel bug."""
import pytest
import torch

from tests import gru_reference as gru


def _autograd(mx, mh, h, dout):
    mx, mh, h = (t.clone().requires_grad_(True) for t in (mx, mh, h))
    H = h.shape[1]
    z = torch.sigmoid(mx[:, :H] + mh[:, :H])
    r = torch.sigmoid(mx[:, H:2 * H] + mh[:, H:2 * H])
    c = torch.tanh(mx[:, 2 * H:] + r * mh[:, 2 * H:])
    out = z * h + (1 - z) * c
    return (out.detach(), torch.cat([z, r, c], dim=1).detach()) + torch.autograd.grad((out * dout).sum(), [mx, mh, h])


@pytest.mark.parametrize("V,H", [(50, 12), (37, 128)])
def test_closed_form_equals_autograd(V, H):
    g = torch.Generator().manual_seed(V + H)
    mx = torch.randn((V, 3 * H), generator=g, dtype=torch.float64) * 2.0
    mh = torch.randn((V, 3 * H), generator=g, dtype=torch.float64) * 2.0
    h = torch.randn((V, H), generator=g, dtype=torch.float64)
    dout = torch.randn((V, H), generator=g, dtype=torch.float64)
    out, gates, gmx, gmh, gh = _autograd(mx, mh, h, dout)
    h_new, got_gates = gru.gru_forward(mx, mh, h)
    torch.testing.assert_close(h_new, out, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(got_gates, gates, rtol=1e-13, atol=1e-13)
    dmx, dmh, dh, bias = gru.gru_backward(dout, got_gates, mh, h)
    assert dmx.dtype == dmh.dtype == dh.dtype == bias.dtype == torch.float64 and tuple(bias.shape) == (2, 3 * H)
    torch.testing.assert_close(dmx, gmx, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dmh, gmh, rtol=1e-12, atol=1e-13)
    # d h through the gates' own path only: the part through mh = h U + b belongs to the product that follows
    torch.testing.assert_close(dh, dout * gates[:, :H], rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(bias, torch.stack([gmx.sum(0), gmh.sum(0)]), rtol=1e-12, atol=1e-12)


def test_direct_state_gradient_and_its_factor():
    """autograd's d h with mh held fixed is dh_new * z; the optional factor multiplies that term alone"""
    V, H = 9, 12
    g = torch.Generator().manual_seed(3)
    mx, mh = (torch.randn((V, 3 * H), generator=g, dtype=torch.float64) for _ in range(2))
    h, dout = (torch.randn((V, H), generator=g, dtype=torch.float64) for _ in range(2))
    _, gates, _, _, gh = _autograd(mx, mh, h, dout)
    factor = (torch.rand((V, H), generator=g) > 0.3).double() / 0.7
    plain = gru.gru_backward(dout, gates, mh, h)
    with_factor = gru.gru_backward(dout, gates, mh, h, factor=factor)
    torch.testing.assert_close(plain[2], gh, rtol=1e-13, atol=1e-13)
    assert torch.equal(with_factor[2], plain[2] * factor)
    for a, b in zip(plain[:2] + plain[3:], with_factor[:2] + with_factor[3:]):
        assert torch.equal(a, b)


def test_inputs_are_cast_up_not_rounded():
    """fp32 inputs give the fp64 result of exactly those values"""
    g = torch.Generator().manual_seed(5)
    mx, mh = (torch.randn((4, 36), generator=g) for _ in range(2))
    h, dout = (torch.randn((4, 12), generator=g) for _ in range(2))
    h_new, gates = gru.gru_forward(mx, mh, h)
    ref, ref_gates = gru.gru_forward(mx.double(), mh.double(), h.double())
    assert h_new.dtype == torch.float64 and torch.equal(h_new, ref) and torch.equal(gates, ref_gates)
    got = gru.gru_backward(dout, gates.float(), mh, h)
    want = gru.gru_backward(dout.double(), gates.float().double(), mh.double(), h.double())
    assert all(torch.equal(a, b) for a, b in zip(got, want))
