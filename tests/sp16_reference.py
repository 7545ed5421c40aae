"""Plain numpy model of the SP16 split-operand format, written from the format description at the head of csrc/gemm_sp.hip
and from csrc/sp16.hpp (sp_scale_for_max, sp_split, sp_store4).  No device code: tests/test_sp16_reference_host.py pins the
model on the host so that a mistake here is not read as a kernel bug.

One scale block = ``scale_block`` consecutive columns of one row.  With mx = max |x| over the block:
  s = 2^e with mx * s in [2^14, 2^15), e capped at 126; a subnormal mx is scaled as the smallest normal exponent
  an all-zero block: s = 1, inv = 2^-126 (the marker csrc/sp16.hpp sp_row_too_small / sp_row_holds recognise)
  an inf or nan in the block: s = inv = 1
  h = fp16(x * s) (round to nearest even), l = fp16(x * s - h); l = 0 where x * s is inf or nan
x * s is an fp32 product and x * s - h an fp32 difference, as on the device (both are exact for finite values that do not
underflow).  Byte layout: row r, column c -> byte (c / 16) * 64 + plane * 32 + (c % 16) * 2 of the row, plane 0 = h, 1 = l.
The SIGN OF A ZERO in h or l is not part of the format (the value is (h + l) * inv, and a product adds nothing for either zero):
where x * s is -0 this model writes h = -0, l = +0, while a device producer may write h = +0, l = -0 - the compiler contracts
fp16(x * s) and fp16(x * s - h) into fused multiply-adds (v_fma_mixlo_f16) whose +0 addend takes the sign off a zero product.
Byte comparisons against a tensor that holds -0 go through ``without_zero_signs``."""
from __future__ import annotations

import numpy as np

MARKER_INV = np.float32(2.0 ** -126)  # inverse scale of an all-zero block
SCALED_LO, SCALED_HI = 2.0 ** 14, 2.0 ** 15  # the scaled block maximum lies in [SCALED_LO, SCALED_HI)
# |decode(encode(x)) - x| <= max(|x| * REL_TERM, block maximum * ABS_TERM): two fp16 roundings leave 2^-22 of an element whose
# l is a normal fp16; below that l is a multiple of 2^-24 in units where the block maximum is >= 2^14 (2^-25 / 2^14 = 2^-39 of
# the block maximum).  tests/test_gpu_gemm_sp.py asserts 2^-22 / 2^-38 for the split pass (test_split_rows_reconstructs) and
# 2^-22 / 2^-37 for the gather (test_gather_sp_matches_fp32_gather); format_bound is the latter.
REL_TERM = 2.0 ** -22
ABS_TERM = 2.0 ** -37


def scale_for_max(mx):
    """block maxima (fp32, any shape; nan = a block that holds one) -> (s, inv), both fp32 powers of two"""
    mx = np.ascontiguousarray(mx, dtype=np.float32)
    ex = ((mx.view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    nonfinite = ex == 255
    zero = mx == 0
    e = np.minimum(14 - (np.maximum(ex, 1) - 127), 126)
    s = np.ldexp(np.float32(1.0), e).astype(np.float32)
    inv = np.ldexp(np.float32(1.0), -e).astype(np.float32)
    s[nonfinite | zero] = 1.0
    inv[nonfinite] = 1.0
    inv[zero] = MARKER_INV
    return s, inv


def encode(x32, scale_block: int, fixed_inv=None):
    """fp32 [R, C] -> (h fp16 [R, C], l fp16 [R, C], inv fp32 [R, C / scale_block]).
    fixed_inv: one caller-chosen 2^-e for the whole tensor (the producers' fixed_inv_scale; s = 1 / fixed_inv)."""
    x = np.ascontiguousarray(x32, dtype=np.float32)
    assert x.ndim == 2 and scale_block % 16 == 0 and x.shape[1] % scale_block == 0, (x.shape, scale_block)
    R, C = x.shape
    blocks = x.reshape(R, C // scale_block, scale_block)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if fixed_inv is None:
            s, inv = scale_for_max(np.abs(blocks).max(axis=2))  # (np.max hands a nan on)
        else:
            inv = np.full((R, C // scale_block), fixed_inv, dtype=np.float32)
            s = (np.float32(1.0) / inv).astype(np.float32)
        xs = (blocks * s[:, :, None]).astype(np.float32)
        h = xs.astype(np.float16)
        l = (xs - h.astype(np.float32)).astype(np.float16)
    l[~np.isfinite(xs)] = 0
    return h.reshape(R, C), l.reshape(R, C), inv


def decode(h, l, inv, scale_block: int):
    """-> float64 [R, C] = (h + l) * inv of the element's block"""
    h, l = np.asarray(h), np.asarray(l)
    inv = np.asarray(inv, dtype=np.float64).reshape(h.shape[0], -1)
    return (h.astype(np.float64) + l.astype(np.float64)) * np.repeat(inv, scale_block, axis=1)


def pack(h, l):
    """(h, l) fp16 [R, C], C % 16 == 0 -> uint8 [R, 4 * C]: per 16 columns one 64-byte granule [16 x h | 16 x l]"""
    h = np.ascontiguousarray(h, dtype=np.float16)
    l = np.ascontiguousarray(l, dtype=np.float16)
    R, C = h.shape
    assert l.shape == (R, C) and C % 16 == 0
    gran = np.stack([h.reshape(R, C // 16, 16), l.reshape(R, C // 16, 16)], axis=2)  # [R, C / 16, plane, 16]
    return np.ascontiguousarray(gran).view(np.uint8).reshape(R, 4 * C)


def unpack(data, cols: int):
    """uint8 [R, >= 4 * cols] (bytes behind 4 * cols of a row: padding, ignored) -> (h, l) fp16 [R, cols]"""
    data = np.asarray(data, dtype=np.uint8)
    R = data.shape[0]
    assert cols % 16 == 0 and data.shape[1] >= 4 * cols
    gran = np.ascontiguousarray(data[:, : 4 * cols]).view(np.float16).reshape(R, cols // 16, 2, 16)
    return gran[:, :, 0, :].reshape(R, cols).copy(), gran[:, :, 1, :].reshape(R, cols).copy()


def without_zero_signs(data):
    """packed SP16 bytes (uint8 [R, 4 * C]) with every fp16 -0 (0x8000) written as +0: nothing else changes"""
    words = np.ascontiguousarray(data, dtype=np.uint8).view(np.uint16).copy()
    words[words == 0x8000] = 0
    return words.view(np.uint8)


def blockmax(ref, scale_block: int):
    """max |ref| of every element's scale block, as an array of ref's shape"""
    ref = np.asarray(ref, dtype=np.float64)
    R, C = ref.shape
    with np.errstate(invalid="ignore"):
        m = np.abs(ref).reshape(R, C // scale_block, scale_block).max(axis=2)
    return np.repeat(m, scale_block, axis=1)


def format_bound(ref, block_max):
    """what the format may lose of ``ref``: max(|ref| * 2^-22, block maximum * 2^-37)"""
    with np.errstate(invalid="ignore"):
        return np.maximum(np.abs(np.asarray(ref, dtype=np.float64)) * REL_TERM, np.asarray(block_max, dtype=np.float64) * ABS_TERM)
