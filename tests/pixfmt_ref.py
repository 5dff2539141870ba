"""Numpy restatement of the pixel formats (include/cairo_amd.h CAIRO_FMT_*),
shared by tests/test_pixfmt.py and tests/test_gpu_pixfmt.py, and the list of
frames the GPU tests feed in as I420 / NV12.

I420 and NV12 carry the codec's own planes: Y8 = Y - 16, U8 = U, V8 = V.  A
frame built that way from the oracle's input planes reproduces them exactly
only where they fit 8 bits (luma 16..271, chroma 0..255);
test_pixfmt.py::test_gpu_inputs_fit_8_bits checks that for every entry of
GPU_INPUTS, so the GPU tests may compare against the oracle's RGB run.
"""
from __future__ import annotations

import numpy as np

RGB24, BGR24, I420, NV12 = range(4)
FMT_NAMES = {RGB24: "rgb24", BGR24: "bgr24", I420: "i420", NV12: "nv12"}


def layout(fmt: int, w: int, h: int, pitch: int = 0):
    """(bytes, tight pitch, pitch in use) by the header's formulas."""
    tight = 3 * w if fmt in (RGB24, BGR24) else w
    p = pitch or tight
    return (p * h if fmt in (RGB24, BGR24) else p * h + p * (h // 2)), tight, p


def views(buf: np.ndarray, fmt: int, w: int, h: int, pitch: int = 0):
    """Writable views of the image's samples inside a flat frame buffer:
    (pixels (h, w, 3),) / (y, u, v) / (y, uv (h/2, w/2, 2))."""
    nb, tight, p = layout(fmt, w, h, pitch)
    assert buf.dtype == np.uint8 and buf.ndim == 1 and buf.size == nb
    if fmt in (RGB24, BGR24):
        return (np.lib.stride_tricks.as_strided(buf, (h, w, 3), (p, 3, 1)),)
    y = buf[:p * h].reshape(h, p)[:, :w]
    if fmt == I420:
        cp, ch = p // 2, h // 2
        return (y, buf[p * h:p * h + cp * ch].reshape(ch, cp)[:, :w // 2],
                buf[p * h + cp * ch:].reshape(ch, cp)[:, :w // 2])
    return y, buf[p * h:].reshape(h // 2, p)[:, :w].reshape(h // 2, w // 2, 2)


def image_mask(fmt: int, w: int, h: int, pitch: int = 0) -> np.ndarray:
    """True for the bytes of a frame buffer that belong to the image (the rest
    is pitch padding)."""
    nb = layout(fmt, w, h, pitch)[0]
    m = np.zeros(nb, np.uint8)
    for v in views(m, fmt, w, h, pitch):
        v[...] = 1
    return m.astype(bool)


def rgb_to_frame(rgb: np.ndarray, fmt: int, pitch: int = 0, fill: int = 0) -> np.ndarray:
    """An (h, w, 3) RGB888 image as an RGB24 / BGR24 frame buffer."""
    h, w = rgb.shape[:2]
    buf = np.full(layout(fmt, w, h, pitch)[0], fill, np.uint8)
    views(buf, fmt, w, h, pitch)[0][...] = rgb if fmt == RGB24 else rgb[..., ::-1]
    return buf


def planes_to_frame(y, u, v, fmt: int, w: int, h: int, pitch: int = 0, fill: int = 0, into=None) -> np.ndarray:
    """Internal int16 planes (any pitch >= w) as an I420 / NV12 frame:
    clamp(Y - 16), clamp(U), clamp(V) to 0..255 -- the output side's rule, and
    on 8-bit-clean planes the exact inverse of frame_to_planes."""
    buf = np.full(layout(fmt, w, h, pitch)[0], fill, np.uint8) if into is None else into
    y8 = np.clip(y[:h, :w].astype(np.int32) - 16, 0, 255).astype(np.uint8)
    u8 = np.clip(u[:h // 2, :w // 2].astype(np.int32), 0, 255).astype(np.uint8)
    v8 = np.clip(v[:h // 2, :w // 2].astype(np.int32), 0, 255).astype(np.uint8)
    vw = views(buf, fmt, w, h, pitch)
    vw[0][...] = y8
    if fmt == I420:
        vw[1][...] = u8
        vw[2][...] = v8
    else:
        vw[1][..., 0] = u8
        vw[1][..., 1] = v8
    return buf


def frame_to_planes(buf: np.ndarray, fmt: int, w: int, h: int, pitch: int = 0):
    """A frame as tight internal planes.  I420 / NV12: Y8 + 16, U8, V8.
    RGB24 / BGR24: the codec's own rule (cairo_amd/csrc/rgb_pixel.h restated):
    a luma sample per pixel, a chroma sample the rounded mean of the four
    chroma terms of a 2 x 2 quad, `/ 256` truncating towards zero."""
    vw = views(buf, fmt, w, h, pitch)
    if fmt in (RGB24, BGR24):
        px = vw[0].astype(np.int32)
        r, g, b = (px[..., 0], px[..., 1], px[..., 2]) if fmt == RGB24 else (px[..., 2], px[..., 1], px[..., 0])
        trunc256 = lambda x: np.where(x < 0, -((-x) // 256), x // 256)  # noqa: E731
        quad = lambda t: (t.reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3)) + 2) >> 2  # noqa: E731
        y = ((77 * r + 150 * g + 29 * b + 128) >> 8) + 16
        u = quad(trunc256(-43 * r - 85 * g + 128 * b + 128) + 128)
        v = quad(trunc256(128 * r - 107 * g - 21 * b + 128) + 128)
        return y.astype(np.int16), u.astype(np.int16), v.astype(np.int16)
    y = vw[0].astype(np.int16) + 16
    if fmt == I420:
        return y, vw[1].astype(np.int16), vw[2].astype(np.int16)
    return y, vw[1][..., 0].astype(np.int16), vw[1][..., 1].astype(np.int16)


def make_frame(kind: str, w: int, h: int, t: int) -> np.ndarray:
    """RGB888 content by name: band4 (the oracle's generator) or tests/content.py."""
    if kind == "band4":
        from oracle import oracle

        return oracle.make_frame(w, h, t)
    from tests import content

    return content.make(kind, w, h, t)


def oracle_input_planes(orc, rgb: np.ndarray):
    """The oracle encoder's planes(0) for an RGB frame (orc_convert_rgb into
    zeroed wa x ha planes), without running an encode."""
    h, w = rgb.shape[:2]
    wa, ha = (w + 15) & ~15, (h + 15) & ~15
    y = np.zeros((ha, wa), np.int16)
    u = np.zeros((ha // 2, wa // 2), np.int16)
    v = np.zeros_like(u)
    rgb = np.ascontiguousarray(rgb)
    orc.lib().orc_convert_rgb(rgb.ctypes.data, w, h, y.ctypes.data, u.ctypes.data, v.ctypes.data, wa, ha)
    return y, u, v


# Encoder parity (tests/test_gpu_pixfmt.py): sizes, contents, I + 3 P.
ENC_SIZES = ((64, 48), (70, 34), (352, 288))
ENC_KINDS = ("band4", "noise", "pan", "gradient")
ENC_FRAMES = 4
# Decoder: (content, quality) at each of DEC_SIZES, 4 frames.
DEC_SIZES = ((64, 48), (200, 120))
DEC_CASES = (("band4", 16), ("black", 16), ("noise", 16), ("noise", 31))
DEC_FRAMES = 4
STREAM_CASE = ("band4", 352, 288, 6)
BIG_CASE = ("band4", 1280, 720, 2)


def gpu_inputs():
    """(kind, w, h, t) of every frame a GPU test turns into I420 / NV12."""
    seen = set()
    for w, h in ENC_SIZES:
        for kind in ENC_KINDS:
            for t in range(max(ENC_FRAMES, 6)):  # the mixed-format launch takes 6 frames
                seen.add((kind, w, h, t))
    for kind, w, h, n in (STREAM_CASE, BIG_CASE):
        for t in range(n):
            seen.add((kind, w, h, t))
    return sorted(seen)
