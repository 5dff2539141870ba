"""Numpy restatement of the scaled submit's rule (include/cairo_amd.h,
cairo_source), shared by tests/test_scale.py and tests/test_gpu_scale.py.

Per axis, S source samples map onto D output samples: g = gcd(S, D), L = S / g,
P = D / g; output sample o covers the units [o L, (o + 1) L), source sample s
the units [s P, (s + 1) P), and w(o, s) is the length of their overlap.  With
the weight matrices Wx (Dx x Sx) and Wy (Dy x Sy) of the two axes,

    out = (Wy @ src @ Wx.T + ((Lx Ly) >> 1)) // (Lx Ly)

in exact integers, for every 8-bit sample plane of the frame as its format
stores it (R, G, B; Y, U, V with the chroma planes at half size).
"""
from __future__ import annotations

from math import gcd

import numpy as np

from tests import pixfmt_ref as pf

RGB24, BGR24, I420, NV12 = pf.RGB24, pf.BGR24, pf.I420, pf.NV12


def axis(S: int, D: int):
    """(L, P) of one axis."""
    g = gcd(S, D)
    return S // g, D // g


def weights(S: int, D: int) -> np.ndarray:
    """The D x S matrix of overlap lengths w(o, s), int64."""
    L, P = axis(S, D)
    o = np.arange(D, dtype=np.int64)[:, None]
    s = np.arange(S, dtype=np.int64)[None, :]
    return np.maximum(np.minimum((o + 1) * L, (s + 1) * P) - np.maximum(o * L, s * P), 0)


def valid(fmt: int, pitch: int, src_size, crop, dw: int, dh: int) -> bool:
    """The constraints of include/cairo_amd.h, restated."""
    sw, sh = src_size
    if fmt not in (RGB24, BGR24, I420, NV12):
        return False
    if min(sw, sh, dw, dh) <= 0 or (sw | sh | dw | dh) & 1 or max(sw, sh) > 32768:
        return False
    tight = 3 * sw if fmt in (RGB24, BGR24) else sw
    if pitch and (pitch < tight or (fmt == I420 and pitch & 1)):
        return False
    cx, cy, cw, ch = crop if crop else (0, 0, sw, sh)
    if min(cx, cy) < 0 or min(cw, ch) <= 0 or (cx | cy | cw | ch) & 1:
        return False
    if cx + cw > sw or cy + ch > sh:
        return False
    if not (dw <= cw <= 8 * dw and dh <= ch <= 8 * dh):
        return False
    return 255 * axis(cw, dw)[0] * axis(ch, dh)[0] < 2 ** 31


def scale_plane(p: np.ndarray, dw: int, dh: int, order: str = "yx") -> np.ndarray:
    """One (sh, sw) uint8 plane to (dh, dw).  order names the axis that is
    summed first; the result does not depend on it (no intermediate rounding)."""
    sh, sw = p.shape
    wx, wy = weights(sw, dw), weights(sh, dh)
    n = axis(sw, dw)[0] * axis(sh, dh)[0]
    assert 255 * n < 2 ** 31
    a = p.astype(np.int64)
    acc = (wy @ a) @ wx.T if order == "yx" else wy @ (a @ wx.T)
    out = (acc + (n >> 1)) // n
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def scaled_frame(frame: np.ndarray, fmt: int, pitch: int, src, dw: int, dh: int) -> np.ndarray:
    """The tight dw x dh frame of format fmt that scaling `frame` gives.  frame
    is a flat uint8 buffer of pixfmt_ref.layout(fmt, sw, sh, pitch) bytes; src is
    ((sw, sh), crop) with crop (x, y, w, h) or None for the whole frame."""
    (sw, sh), crop = src
    assert valid(fmt, pitch, (sw, sh), crop, dw, dh)
    cx, cy, cw, ch = crop if crop else (0, 0, sw, sh)
    vw = pf.views(np.ascontiguousarray(frame), fmt, sw, sh, pitch)
    out = np.zeros(pf.layout(fmt, dw, dh)[0], np.uint8)
    ow = pf.views(out, fmt, dw, dh)
    if fmt in (RGB24, BGR24):
        for c in range(3):
            ow[0][..., c] = scale_plane(vw[0][cy:cy + ch, cx:cx + cw, c], dw, dh)
        return out
    ow[0][...] = scale_plane(vw[0][cy:cy + ch, cx:cx + cw], dw, dh)
    hx, hy, hw, hh = cx // 2, cy // 2, cw // 2, ch // 2
    if fmt == I420:
        for k in (1, 2):
            ow[k][...] = scale_plane(vw[k][hy:hy + hh, hx:hx + hw], dw // 2, dh // 2)
    else:
        for c in range(2):
            ow[1][..., c] = scale_plane(vw[1][hy:hy + hh, hx:hx + hw, c], dw // 2, dh // 2)
    return out


# The KAT's cases (tests/test_gpu_scale.py): source size -> output size.
KAT_SIZES = (
    ((64, 48), (64, 48)),      # copy
    ((140, 68), (70, 34)),     # 2:1, strips cut by the right edge
    ((210, 102), (70, 34)),    # 3:1
    ((96, 72), (64, 48)),      # 3:2, fractional weights
    ((70, 34), (34, 18)),      # L = 35 / 17, nearly coprime
    ((272, 144), (34, 18)),    # 8:1, the maximum tap count
    ((3840, 16), (1918, 8)),   # the largest Lx a 4K source allows
)
