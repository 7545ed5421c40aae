"""tests/sp16_reference.py (the numpy model of the SP16 format the GPU tests of the split-operand gather compare with) on the
host: its scales, its reconstruction bound and its byte layout.  No device."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import sp16_reference as sp
from tests.helpers import decode_sp16

FLT_MAX = float(np.finfo(np.float32).max)


def _roundtrip(x, scale_block):
    h, l, inv = sp.encode(x, scale_block)
    return h, l, inv, sp.decode(h, l, inv, scale_block)


def _assert_within_format_bound(x, rec, scale_block):
    ref = x.astype(np.float64)
    bound = sp.format_bound(ref, sp.blockmax(ref, scale_block))
    err = np.abs(rec - ref)
    assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))


def _assert_powers_of_two(inv):
    m, _ = np.frexp(inv)
    assert np.all(m == 0.5), "scales must be exact powers of two"


@pytest.mark.parametrize("R,C,sb", [(64, 320, 320), (40, 128, 16), (33, 96, 32), (7, 512, 512)])
def test_random_rows_spread_over_sixty_binades(R, C, sb):
    rng = np.random.default_rng(R + C)
    x = (rng.standard_normal((R, C)) * np.exp2(rng.uniform(-30, 30, size=(R, 1)))).astype(np.float32)
    h, l, inv, rec = _roundtrip(x, sb)
    _assert_powers_of_two(inv)
    _assert_within_format_bound(x, rec, sb)
    scaled = np.abs(x.astype(np.float64)).reshape(R, C // sb, sb).max(axis=2) / inv.astype(np.float64)
    assert np.all((scaled >= sp.SCALED_LO) & (scaled < sp.SCALED_HI))
    assert h.dtype == np.float16 and l.dtype == np.float16 and inv.dtype == np.float32 and inv.shape == (R, C // sb)


def test_all_zero_row_carries_the_marker():
    x = np.zeros((3, 64), dtype=np.float32)
    x[1, :] = 1.0
    x[2, 5] = -0.0
    h, l, inv, rec = _roundtrip(x, 64)
    assert inv[0, 0] == sp.MARKER_INV == np.float32(2.0 ** -126) and inv[2, 0] == sp.MARKER_INV and inv[1, 0] != sp.MARKER_INV
    assert not sp.pack(h, l)[0].any()  # zero bytes
    assert np.all(rec[0] == 0) and np.all(rec[2] == 0)  # (+0 and -0)
    assert np.all(rec[1] == 1.0)
    # per block: an all-zero block beside a block that holds something
    x = np.concatenate([np.zeros((1, 16), dtype=np.float32), np.full((1, 16), 3.0, dtype=np.float32)], axis=1)
    _, _, inv, rec = _roundtrip(x, 16)
    assert inv[0, 0] == sp.MARKER_INV and inv[0, 1] == np.float32(2.0 ** -13) and np.array_equal(rec, x.astype(np.float64))


def test_rows_below_the_exponent_cap_and_subnormal_rows():
    rng = np.random.default_rng(5)
    small = (rng.standard_normal((8, 64)) * np.exp2(rng.uniform(-126, -113, size=(8, 1)))).astype(np.float32)
    small[:, 0] = np.exp2(rng.integers(-126, -112, size=8)).astype(np.float32)  # a maximum in [2^-126, 2^-112)
    small = np.clip(small, -small[:, :1], small[:, :1])
    assert np.all((np.abs(small).max(axis=1) >= 2.0 ** -126) & (np.abs(small).max(axis=1) < 2.0 ** -112))
    h, l, inv, rec = _roundtrip(small, 64)
    assert np.all(inv == np.float32(2.0 ** -126))  # e capped at 126 (the marker's value, with bytes that are not zero)
    assert sp.pack(h, l).any(axis=1).all()
    _assert_within_format_bound(small, rec, 64)
    sub = (rng.integers(-(2 ** 22), 2 ** 22, size=(4, 64)).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    sub[0, :] = np.float32(1e-42)
    assert np.all(np.abs(sub) < 2.0 ** -126) and np.abs(sub).max() > 0
    _, _, inv, rec = _roundtrip(sub, 64)
    assert np.all(inv == np.float32(2.0 ** -126))  # scaled as the smallest normal exponent
    assert np.array_equal(rec, sub.astype(np.float64))  # multiples of 2^-149 times 2^126: h + l holds them exactly
    _assert_within_format_bound(sub, rec, 64)


def test_powers_of_two_at_both_ends_of_the_scale_interval():
    ks = np.arange(-112, 127)
    x = np.zeros((2 * ks.size, 16), dtype=np.float32)
    x[: ks.size, 3] = np.exp2(ks.astype(np.float64)).astype(np.float32)  # 2^k: scaled to 2^14 exactly
    x[ks.size:, 3] = -np.nextafter(np.exp2(ks + 1.0).astype(np.float32), np.float32(0))  # the float below 2^(k+1): below 2^15
    x[:, 7] = x[:, 3] * np.float32(0.3)
    h, l, inv, rec = _roundtrip(x, 16)
    _assert_powers_of_two(inv)
    scaled = np.abs(x[:, 3].astype(np.float64)) / inv[:, 0].astype(np.float64)
    assert np.all(scaled[: ks.size] == sp.SCALED_LO)
    assert np.all((scaled[ks.size:] >= sp.SCALED_LO) & (scaled[ks.size:] < sp.SCALED_HI))
    assert np.array_equal(inv[: ks.size, 0].astype(np.float64), np.exp2(ks - 14.0))
    assert np.array_equal(inv[ks.size:, 0], inv[: ks.size, 0])
    _assert_within_format_bound(x, rec, 16)
    assert np.array_equal(rec[: ks.size, 3], x[: ks.size, 3].astype(np.float64))


def test_flt_max_inf_and_nan():
    rng = np.random.default_rng(9)
    x = rng.standard_normal((5, 32)).astype(np.float32)
    x[0, 4], x[0, 9] = FLT_MAX, -FLT_MAX
    x[1, 4] = np.inf
    x[2, 4] = -np.inf
    x[3, 4] = np.nan
    x[4, :16] = np.nan  # a block that holds nothing but nan beside an ordinary block
    h, l, inv, rec = _roundtrip(x, 16)
    assert inv[0, 0] == np.float32(2.0 ** 113) and rec[0, 4] == FLT_MAX and rec[0, 9] == -FLT_MAX
    _assert_within_format_bound(x[:1], rec[:1], 16)
    assert np.all(inv[1:5, 0] == 1.0)  # inf or nan in the block: no scaling
    assert rec[1, 4] == np.inf and rec[2, 4] == -np.inf and np.isnan(rec[3, 4]) and np.all(np.isnan(rec[4, :16]))
    bad = ~np.isfinite(x)
    assert np.all(l[bad] == 0) and np.array_equal(np.isnan(h), np.isnan(x)) and np.array_equal(np.isinf(h), np.isinf(x))
    # the blocks beside them are ordinary blocks
    assert np.all(inv[1:, 1] != 1.0)
    _assert_powers_of_two(inv)
    _assert_within_format_bound(x[:, 16:], rec[:, 16:], 16)
    finite_neighbours = np.isfinite(rec[1:4, :16]) & ~bad[1:4, :16]
    assert finite_neighbours.sum() == 3 * 15  # finite entries beside an inf / nan stay finite


def test_fixed_inverse_scale():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((6, 48)).astype(np.float32)
    x[2] = 0.0
    bound = 2.0 * float(np.abs(x).max())
    _, fixed = sp.scale_for_max(np.array([bound], dtype=np.float32))
    h, l, inv = sp.encode(x, 48, fixed_inv=fixed[0])
    assert np.all(inv == fixed[0]) and inv.shape == (6, 1)
    rec = sp.decode(h, l, inv, 48)
    err = np.abs(rec - x.astype(np.float64))
    assert np.all(err <= sp.format_bound(x.astype(np.float64), bound))
    assert np.all(rec[2] == 0)


def test_pack_unpack_and_the_byte_layout():
    rng = np.random.default_rng(3)
    R, C = 5, 48
    x = (rng.standard_normal((R, C)) * 100).astype(np.float32)
    h, l, inv = sp.encode(x, 16)
    data = sp.pack(h, l)
    assert data.shape == (R, 4 * C) and data.dtype == np.uint8
    for r, c in ((0, 0), (1, 15), (2, 16), (3, 31), (4, 47)):  # row r, column c -> byte (c / 16) * 64 + plane * 32 + (c % 16) * 2
        for plane, val in ((0, h[r, c]), (1, l[r, c])):
            at = (c // 16) * 64 + plane * 32 + (c % 16) * 2
            assert data[r, at:at + 2].tobytes() == np.float16(val).tobytes()
    h2, l2 = sp.unpack(data, C)
    assert np.array_equal(h2.view(np.uint16), h.view(np.uint16)) and np.array_equal(l2.view(np.uint16), l.view(np.uint16))
    padded = np.concatenate([data, np.full((R, 64), 0xA5, dtype=np.uint8)], axis=1)  # bytes behind a row: ignored
    h3, l3 = sp.unpack(padded, C)
    assert np.array_equal(h3.view(np.uint16), h.view(np.uint16)) and np.array_equal(l3.view(np.uint16), l.view(np.uint16))
    # a hand-built operand: helpers.decode_sp16 (what the product tests decode with) reads the same matrix
    op = SimpleNamespace(data=torch.from_numpy(data), inv_scale=torch.from_numpy(inv), rows=R, cols=C, scale_block=16)
    assert np.array_equal(decode_sp16(op), sp.decode(h2, l2, inv, 16))
    hand = np.zeros((1, 64), dtype=np.uint8)
    hand[0, 2 * 3:2 * 3 + 2] = np.frombuffer(np.float16(1.5).tobytes(), dtype=np.uint8)        # h of column 3
    hand[0, 32 + 2 * 3:32 + 2 * 3 + 2] = np.frombuffer(np.float16(2.0 ** -12).tobytes(), dtype=np.uint8)  # l of column 3
    hh, hl = sp.unpack(hand, 16)
    assert hh[0, 3] == 1.5 and hl[0, 3] == 2.0 ** -12 and np.count_nonzero(hh) == 1 and np.count_nonzero(hl) == 1
    op = SimpleNamespace(data=torch.from_numpy(hand), inv_scale=torch.tensor([[0.25]]), rows=1, cols=16, scale_block=16)
    want = np.zeros((1, 16))
    want[0, 3] = (1.5 + 2.0 ** -12) * 0.25
    assert np.array_equal(decode_sp16(op), want) and np.array_equal(sp.decode(hh, hl, np.array([[0.25]]), 16), want)


def test_without_zero_signs_changes_nothing_but_the_sign_of_a_zero():
    x = np.array([[-0.0, 0.0, -1.5, 1.5, -2.0 ** -30, 3.0, -0.0, 7.0] + [0.0] * 8], dtype=np.float32)
    h, l, inv = sp.encode(x, 16)
    data = sp.pack(h, l)
    assert data[0, 1] == 0x80 and data[0, 13] == 0x80  # the model's h of a -0
    clean = sp.without_zero_signs(data)
    assert clean.shape == data.shape and clean.dtype == np.uint8 and data[0, 1] == 0x80  # (a copy)
    differ = np.flatnonzero(clean != data)
    assert differ.tolist() == [1, 13]
    h2, l2 = sp.unpack(clean, 16)
    assert np.array_equal(sp.decode(h2, l2, inv, 16), sp.decode(h, l, inv, 16))
    device = data.copy()  # what a device producer writes for a -0: h = +0, l = -0
    device[0, [1, 13]] = 0
    device[0, [33, 45]] = 0x80
    assert np.array_equal(sp.without_zero_signs(device), clean)
