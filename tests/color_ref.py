"""Numpy restatement of the colour descriptions (include/cairo_amd.h
CAIRO_RANGE_*, CAIRO_MATRIX_*), shared by tests/test_color.py and
tests/test_gpu_color.py: the derivation of the integer coefficients from Kr
and Kb in exact rationals, the maps on 8-bit sample planes, and the byte-frame
maps built on tests/pixfmt_ref.py's views.

Written from the header's text, not from the library's code: a description is
(range, matrix); dir 0 maps described YUV to the codec's full-range BT.601,
dir 1 the codec's to described YUV.
"""
from __future__ import annotations

from fractions import Fraction as F

import numpy as np

from tests import pixfmt_ref as pf

FULL, LIMITED = 0, 1
BT601, BT709 = 0, 1
KR_KB = {BT601: (F(299, 1000), F(114, 1000)), BT709: (F(2126, 10000), F(722, 10000))}
DESCRIPTIONS = ((FULL, BT601), (LIMITED, BT601), (FULL, BT709), (LIMITED, BT709))
NON_IDENTITY = DESCRIPTIONS[1:]
SHIFT = 14
# every coefficient is off by at most 2^-15; |d0| <= 255, |d1|, |d2| <= 128
BOUND = F(1, 2) + F(511, 32768)


def rgb_to_ycc(kr: F, kb: F):
    """A(Kr, Kb): the RGB -> YCbCr matrix, rows of Fractions."""
    kg = 1 - kr - kb
    return [[kr, kg, kb],
            [-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), (1 - kb) / (2 * (1 - kb))],
            [(1 - kr) / (2 * (1 - kr)), -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))]]


def _mul(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def _inv(m):
    """Inverse of a 3x3 matrix of Fractions (adjugate over determinant)."""
    (a, b, c), (d, e, f), (g, h, i) = m
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e],
           [f * g - d * i, a * i - c * g, c * d - a * f],
           [d * h - e * g, b * g - a * h, a * e - b * d]]
    return [[x / det for x in row] for row in adj]


def real_matrix(direction: int, rng: int, matrix: int):
    """The real-valued 3x3 map with the range factors applied (Fractions), and
    the luma offset oy."""
    a601 = rgb_to_ycc(*KR_KB[BT601])
    am = rgb_to_ycc(*KR_KB[matrix])
    sy, sc, oy = (F(255, 219), F(255, 224), 16) if rng == LIMITED else (F(1), F(1), 0)
    if direction == 0:
        c = _mul(a601, _inv(am))
        c = [[row[0] * sy, row[1] * sc, row[2] * sc] for row in c]
    else:
        c = _mul(am, _inv(a601))
        c = [[x / sy for x in c[0]], [x / sc for x in c[1]], [x / sc for x in c[2]]]
    assert c[1][0] == 0 and c[2][0] == 0  # the shape [1 a b; 0 c d; 0 e f] times the range factors
    return c, oy


def coefs(direction: int, rng: int, matrix: int):
    """-> (k: 9 ints, row-major; oy): k_ij = floor(2^14 c_ij + 1/2)."""
    c, oy = real_matrix(direction, rng, matrix)
    return [int((x * (1 << SHIFT) + F(1, 2)).__floor__()) for row in c for x in row], oy


def map_luma(y8, u8, v8, direction: int, rng: int, matrix: int) -> np.ndarray:
    """The integer luma map on sample arrays of one shape (chroma already
    brought to the luma's positions), in int32 as the rule says it fits."""
    k, oy = coefs(direction, rng, matrix)
    acc = np.asarray(y8).astype(np.int32)
    if direction == 0:
        acc -= oy
    acc *= k[0]
    if k[1]:
        acc += k[1] * (np.asarray(u8).astype(np.int32) - 128)
    if k[2]:
        acc += k[2] * (np.asarray(v8).astype(np.int32) - 128)
    acc += ((oy << SHIFT) if direction == 1 else 0) + (1 << (SHIFT - 1))
    acc >>= SHIFT
    return np.clip(acc, 0, 255).astype(np.uint8)


def map_chroma(u8, v8, direction: int, rng: int, matrix: int):
    """The integer chroma maps: -> (u', v') uint8."""
    k, _ = coefs(direction, rng, matrix)
    d1 = np.asarray(u8).astype(np.int32) - 128
    d2 = np.asarray(v8).astype(np.int32) - 128
    bias = (128 << SHIFT) + (1 << (SHIFT - 1))
    uu = (k[4] * d1 + k[5] * d2 + bias) >> SHIFT
    vv = (k[7] * d1 + k[8] * d2 + bias) >> SHIFT
    return np.clip(uu, 0, 255).astype(np.uint8), np.clip(vv, 0, 255).astype(np.uint8)


def map_samples(y8, u8, v8, direction: int, rng: int, matrix: int):
    """The integer map on sample arrays of one shape: -> (y', u', v') uint8."""
    return (map_luma(y8, u8, v8, direction, rng, matrix),) + map_chroma(u8, v8, direction, rng, matrix)


def real_samples(y8, u8, v8, direction: int, rng: int, matrix: int):
    """The same map in real arithmetic (float64), clamped to 0..255, unrounded."""
    c, oy = real_matrix(direction, rng, matrix)
    c = [[float(x) for x in row] for row in c]
    y = np.asarray(y8).astype(np.float64)
    d1 = np.asarray(u8).astype(np.float64) - 128
    d2 = np.asarray(v8).astype(np.float64) - 128
    if direction == 0:
        yy = c[0][0] * (y - oy) + c[0][1] * d1 + c[0][2] * d2
    else:
        yy = c[0][0] * y + c[0][1] * d1 + c[0][2] * d2 + oy
    uu = c[1][1] * d1 + c[1][2] * d2 + 128
    vv = c[2][1] * d1 + c[2][2] * d2 + 128
    return tuple(np.clip(a, 0.0, 255.0) for a in (yy, uu, vv))


def map_planes(y8, u8, v8, direction: int, rng: int, matrix: int):
    """4:2:0 planes (y: (h, w), u and v: (h/2, w/2)) -> mapped planes: a luma
    sample at (x, y) uses the chroma sample at (x >> 1, y >> 1)."""
    up = lambda c: np.repeat(np.repeat(np.asarray(c), 2, axis=0), 2, axis=1)  # noqa: E731
    return (map_luma(y8, up(u8), up(v8), direction, rng, matrix),) + map_chroma(u8, v8, direction, rng, matrix)


def map_frame(frame: np.ndarray, fmt: int, w: int, h: int, pitch: int, direction: int, rng: int,
              matrix: int) -> np.ndarray:
    """A copy of the frame buffer with the samples of an I420 / NV12 image
    mapped; the pitch padding and RGB24 / BGR24 frames keep their bytes."""
    out = frame.copy()
    if fmt in (pf.RGB24, pf.BGR24):
        return out
    vin, vout = pf.views(frame, fmt, w, h, pitch), pf.views(out, fmt, w, h, pitch)
    if fmt == pf.I420:
        yy, uu, vv = map_planes(vin[0], vin[1], vin[2], direction, rng, matrix)
        vout[0][...], vout[1][...], vout[2][...] = yy, uu, vv
    else:
        yy, uu, vv = map_planes(vin[0], vin[1][..., 0], vin[1][..., 1], direction, rng, matrix)
        vout[0][...] = yy
        vout[1][..., 0], vout[1][..., 1] = uu, vv
    return out
