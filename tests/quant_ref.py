"""A plain reference of the quantizer and dequantizer, in numpy int64.

Written from quantize.cpp as oracle/evx_oracle.c:341-410 cites it: rounded
division is the truncating division of n -/+ d/2 (half away from zero), the
two matrices, the two DC scales, the inter dead zone qf - sign(qf) * qp with
qf narrowed to int16, the dequantizer's truncating / 16, and the final int16
narrowings.  No reciprocals, no tricks: every division is a division.

Macroblocks are (n, 384) int16, block-major (Y TL, TR, BL, BR, U, V; 64 each),
the layout of cairo_kat_transform and cairo_kat_quant.
tests/test_mb_cases.py pins this file to the oracle.
"""
from __future__ import annotations

import numpy as np

QSCALE = 16  # EVX_QUANTIZER_SCALE_FACTOR, quantize.cpp:9
INTRA, MOTION = 1, 2

# default_intra_8x8_qm / default_inter_8x8_qm, quantize.cpp:13-35
QM_INTRA = np.array([
    8, 17, 18, 19, 21, 23, 25, 27,
    17, 18, 19, 21, 23, 25, 27, 28,
    20, 21, 22, 23, 24, 26, 28, 30,
    21, 22, 23, 24, 26, 28, 30, 32,
    22, 23, 24, 26, 28, 30, 32, 35,
    23, 24, 26, 28, 30, 32, 35, 38,
    25, 26, 28, 30, 32, 35, 38, 41,
    27, 28, 30, 32, 35, 38, 41, 45], np.int64)
QM_INTER = np.array([
    16, 17, 18, 19, 20, 21, 22, 23,
    17, 18, 19, 20, 21, 22, 23, 24,
    18, 19, 20, 21, 22, 23, 24, 25,
    19, 20, 21, 22, 23, 24, 26, 27,
    20, 21, 22, 23, 25, 26, 27, 28,
    21, 22, 23, 24, 26, 27, 28, 30,
    22, 23, 24, 26, 27, 28, 30, 31,
    23, 24, 25, 27, 28, 30, 31, 33], np.int64)


def luma_dc_scale(qp: int) -> int:
    """compute_luma_dc_scale, quantize.cpp:37-46."""
    if qp < 5:
        return 8
    if qp < 9:
        return 2 * qp
    if qp < 25:
        return qp + 8
    return 2 * qp - 16


def chroma_dc_scale(qp: int) -> int:
    """compute_chroma_dc_scale, quantize.cpp:48-55."""
    if qp < 5:
        return 8
    if qp < 25:
        return (qp + 13) >> 1
    return qp - 6


def tdiv(n, d):
    """C's division: truncation toward zero (d > 0)."""
    n = np.asarray(n, np.int64)
    return np.sign(n) * (np.abs(n) // d)


def rdiv(n, d):
    """rounded_div, math.h:224-232, for d > 0: (n - d/2) / d below zero,
    (n + d/2) / d otherwise, both truncating."""
    n = np.asarray(n, np.int64)
    return np.where(n < 0, tdiv(n - d // 2, d), tdiv(n + d // 2, d))


def i16(x):
    """The (int16_t) cast: the low 16 bits, two's complement."""
    return ((np.asarray(x, np.int64) + 32768) & 0xFFFF) - 32768


def intra_path(typ: int) -> bool:
    """quantize.cpp:256-354: the intra matrices and DC scales for an intra
    type without motion, the inter quantizer for everything else."""
    return bool(typ & INTRA) and not (typ & MOTION)


def _dc_scales(qp: int) -> np.ndarray:
    return np.array([luma_dc_scale(qp)] * 4 + [chroma_dc_scale(qp)] * 2, np.int64)[None, :]


def quantize(coef: np.ndarray, typ: int, qp: int) -> np.ndarray:
    """quantize_macroblock (quantize.cpp:79-163, 357-367) -> (n, 384) int16."""
    c = np.asarray(coef, np.int64).reshape(-1, 6, 64)
    if intra_path(typ):
        q = i16(rdiv(rdiv(c * QSCALE, QM_INTRA), 2 * qp))
        q[:, :, 0] = i16(rdiv(c[:, :, 0], _dc_scales(qp)))
    else:
        qf = i16(rdiv(c * QSCALE, QM_INTER))
        q = i16(rdiv(qf - np.sign(qf) * qp, 2 * qp))
    return q.reshape(-1, 384).astype(np.int16)


def dequantize(quant: np.ndarray, typ: int, qp: int) -> np.ndarray:
    """inverse_quantize_macroblock (quantize.cpp:182-243, 369-379) -> (n, 384) int16."""
    v = np.asarray(quant, np.int64).reshape(-1, 6, 64)
    if intra_path(typ):
        d = i16(tdiv(2 * v * QM_INTRA * qp, QSCALE))
        d[:, :, 0] = i16(v[:, :, 0] * _dc_scales(qp))
    else:
        d = i16(tdiv(2 * v * QM_INTER * qp, QSCALE))
    return d.reshape(-1, 384).astype(np.int16)
