"""Numpy restatement of the capture and 10-bit layouts (include/cairo_amd.h,
CAIRO_FMT_YUY2 / UYVY / P010), written from the header's text: the layouts, and
the two maps onto NV12 that define them.  Shared by tests/test_capfmt.py and
tests/test_gpu_capfmt.py.

    YUY2   per pixel pair the bytes Y0 U Y1 V, rows of `pitch` bytes
    UYVY   per pixel pair the bytes U Y0 V Y1
    P010   little-endian 16-bit words, the sample in the high ten bits: h rows
           of Y words, then h/2 rows of interleaved U, V words

fold:   YUY2 / UYVY  Y8 = Y; U8(cx, cy) = (U(cx, 2cy) + U(cx, 2cy+1) + 1) >> 1
        P010         s8 = min(((word >> 6) + 2) >> 2, 255)
unfold: YUY2 / UYVY  Y = Y8; rows 2cy and 2cy+1 both carry U8(cx, cy), V8(cx, cy)
        P010         word = s8 << 8
"""
from __future__ import annotations

import numpy as np

from tests import pixfmt_ref

NV12 = pixfmt_ref.NV12
YUY2, UYVY, P010 = 8, 9, 10
CAP_FMTS = (YUY2, UYVY, P010)
FMT_NAMES = {YUY2: "yuy2", UYVY: "uyvy", P010: "p010"}


def layout(fmt: int, w: int, h: int, pitch: int = 0):
    """(bytes, tight pitch, pitch in use) by the header's table."""
    tight = 2 * w
    p = pitch or tight
    return (p * h + p * (h // 2) if fmt == P010 else p * h), tight, p


def pitched(fmt: int, w: int) -> int:
    """A pitch 3 bytes wider than tight (P010, whose pitch is even: 2)."""
    return 2 * w + (2 if fmt == P010 else 3)


def views(buf: np.ndarray, fmt: int, w: int, h: int, pitch: int = 0):
    """Writable views of the image's samples inside a flat uint8 frame buffer.
    YUY2 / UYVY: (y (h, w), u (h, w/2), v (h, w/2)) bytes.  P010: (y (h, w),
    uv (h/2, w/2, 2)) as (h, w, 2) and (h/2, w/2, 2, 2) bytes, low byte first."""
    nb, _, p = layout(fmt, w, h, pitch)
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.size == nb
    st = np.lib.stride_tricks.as_strided
    if fmt == P010:
        return st(buf, (h, w, 2), (p, 2, 1)), st(buf[p * h:], (h // 2, w // 2, 2, 2), (p, 4, 2, 1))
    o = 1 if fmt == UYVY else 0
    return st(buf[o:], (h, w), (p, 2)), st(buf[1 - o:], (h, w // 2), (p, 4)), st(buf[3 - o:], (h, w // 2), (p, 4))


def image_mask(fmt: int, w: int, h: int, pitch: int = 0) -> np.ndarray:
    """True for the bytes of a frame buffer that belong to the image."""
    m = np.zeros(layout(fmt, w, h, pitch)[0], np.uint8)
    for v in views(m, fmt, w, h, pitch):
        v[...] = 1
    return m.astype(bool)


def _words(v: np.ndarray) -> np.ndarray:
    """A (..., 2) byte view of little-endian words as integers."""
    return v[..., 0].astype(np.int32) | (v[..., 1].astype(np.int32) << 8)


def fold(frame: np.ndarray, fmt: int, w: int, h: int, pitch: int = 0, nv12_pitch: int = 0, fill: int = 0) -> np.ndarray:
    """A YUY2 / UYVY / P010 frame -> the NV12 frame (padding bytes: fill)."""
    out = np.full(pixfmt_ref.layout(NV12, w, h, nv12_pitch)[0], fill, np.uint8)
    y8, uv8 = pixfmt_ref.views(out, NV12, w, h, nv12_pitch)
    vw = views(frame, fmt, w, h, pitch)
    if fmt == P010:
        s8 = lambda words: np.minimum(((words >> 6) + 2) >> 2, 255).astype(np.uint8)  # noqa: E731
        y8[...] = s8(_words(vw[0]))
        uv8[...] = s8(_words(vw[1]))
        return out
    y, u, v = vw
    y8[...] = y
    for c, plane in enumerate((u, v)):
        p = plane.astype(np.int32)
        uv8[..., c] = ((p[0::2] + p[1::2] + 1) >> 1).astype(np.uint8)
    return out


def unfold(nv12: np.ndarray, fmt: int, w: int, h: int, pitch: int = 0, nv12_pitch: int = 0, fill: int = 0,
           into: np.ndarray | None = None) -> np.ndarray:
    """An NV12 frame -> the YUY2 / UYVY / P010 frame (padding bytes: fill, or
    what `into` holds)."""
    out = np.full(layout(fmt, w, h, pitch)[0], fill, np.uint8) if into is None else into
    y8, uv8 = pixfmt_ref.views(nv12, NV12, w, h, nv12_pitch)
    vw = views(out, fmt, w, h, pitch)
    if fmt == P010:
        vw[0][..., 0], vw[0][..., 1] = 0, y8  # word = s8 << 8: low byte zero, high byte the sample
        vw[1][..., 0], vw[1][..., 1] = 0, uv8
        return out
    y, u, v = vw
    y[...] = y8
    for c, plane in enumerate((u, v)):
        plane[0::2] = uv8[..., c]
        plane[1::2] = uv8[..., c]
    return out


def exhaustive_422(fmt: int, rng) -> tuple:
    """A 1024x256 YUY2 / UYVY frame whose two chroma rows of each row pair carry
    every one of the 65 536 (row 0, row 1) byte pairs once per plane (512 x 128
    pairs per plane); luma is random.  -> (frame, w, h)."""
    w, h = 1024, 256
    frame = rng.integers(0, 256, layout(fmt, w, h)[0], dtype=np.uint8)
    _, u, v = views(frame, fmt, w, h)
    pairs = np.arange(65536, dtype=np.int64)
    for plane, order in ((u, pairs), (v, rng.permutation(pairs))):
        g = order.reshape(h // 2, w // 2)
        plane[0::2] = (g >> 8).astype(np.uint8)
        plane[1::2] = (g & 255).astype(np.uint8)
    return frame, w, h


def exhaustive_p010(rng) -> tuple:
    """A 4100x4 P010 frame in which every one of the 1024 ten-bit values
    appears, with random low six bits, at both half-word positions of a dword;
    the rest is random 16-bit words.  -> (frame, w, h)."""
    w, h = 4100, 4
    frame = rng.integers(0, 256, layout(P010, w, h)[0], dtype=np.uint8)
    y, uv = views(frame, P010, w, h)
    v10 = np.arange(1024)

    def put(row, values):  # row: (n, 2) bytes
        assert np.shares_memory(row, frame)
        words = (values << 6) | rng.integers(0, 64, values.size)
        row[:values.size, 0], row[:values.size, 1] = words & 255, words >> 8

    put(y[0], np.repeat(v10, 2))                     # each value at an even and an odd column
    put(y[3], np.repeat(v10[::-1], 2))
    put(uv[0].reshape(-1, 2), np.repeat(v10, 2))     # each value as U (low half-word) and as V (high)
    put(uv[1].reshape(-1, 2), np.repeat(v10[::-1], 2))
    return frame, w, h


def covers_all_positions(frame: np.ndarray, fmt: int, w: int, h: int, pitch: int = 0) -> bool:
    """Whether every one of the 256 sample values appears at every byte
    position of a dword of a row (YUY2, UYVY) or in the high byte of both
    half-word positions (P010), counted from the row's start."""
    _, _, p = layout(fmt, w, h, pitch)
    rows = frame.reshape(-1, p)[:, :2 * w]
    lanes = (1, 3) if fmt == P010 else (0, 1, 2, 3)
    return all(np.unique(rows[:, k::4]).size == 256 for k in lanes)
