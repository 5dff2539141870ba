"""Numpy restatement of the per-frame metrics (include/cairo_amd.h
cairo_frame_metrics), shared by tests/test_metrics.py and
tests/test_gpu_metrics.py: int64 sums, num / den in float64.

Both sides are first mapped to the 8-bit samples the I420 output defines
(Y8 = clamp(Y - 16), U8 = clamp(U), V8 = clamp(V)) over the nominal picture.
"""
from __future__ import annotations

import numpy as np

C1, C2 = 416, 235963  # (0.01 * 255)^2 * 64 and (0.03 * 255)^2 * 64 * 63, rounded


def samples8(plane: np.ndarray, pw: int, ph: int, luma: bool) -> np.ndarray:
    """The nominal pw x ph part of an internal int16 plane as 8-bit samples (int64)."""
    p = plane[:ph, :pw].astype(np.int64)
    return np.clip(p - 16 if luma else p, 0, 255)


def window_count(pw: int, ph: int) -> int:
    bw, bh = pw // 4, ph // 4
    return (bw - 1) * (bh - 1) if bw >= 2 and bh >= 2 else 0


def sse8(a: np.ndarray, b: np.ndarray) -> int:
    d = a.astype(np.int64) - b.astype(np.int64)
    return int((d * d).sum())


def ssim_windows(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The window values of two planes of 8-bit samples (any integer dtype),
    shape (bh - 1, bw - 1), float64: 4x4 blocks from the origin, leftover
    columns and rows ignored, a window = 2x2 blocks at block stride 1."""
    ph, pw = a.shape
    bw, bh = pw // 4, ph // 4
    if bw < 2 or bh < 2:
        return np.zeros((0, 0), np.float64)
    a = a[:4 * bh, :4 * bw].astype(np.int64)
    b = b[:4 * bh, :4 * bw].astype(np.int64)

    def blocks(x):  # 4x4 block sums
        return x.reshape(bh, 4, bw, 4).sum(axis=(1, 3))

    def windows(x):  # 2x2 blocks at block stride 1
        return x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:]

    s1, s2 = windows(blocks(a)), windows(blocks(b))
    ss, s12 = windows(blocks(a * a + b * b)), windows(blocks(a * b))
    var = 64 * ss - s1 * s1 - s2 * s2
    covar = 64 * s12 - s1 * s2
    num = (2 * s1 * s2 + C1) * (2 * covar + C2)
    den = (s1 * s1 + s2 * s2 + C1) * (var + C2)
    assert num.dtype == np.int64 and den.dtype == np.int64
    return num.astype(np.float64) / den.astype(np.float64)


def plane_metrics(a8: np.ndarray, b8: np.ndarray) -> dict:
    win = ssim_windows(a8, b8)
    return {"sse": sse8(a8, b8), "ssim_sum": float(win.sum()), "ssim_windows": int(win.size),
            "samples": int(a8.size)}


def frame_metrics(a, b, w: int, h: int) -> dict:
    """a, b: (y, u, v) internal int16 planes of any pitch >= w (chroma w / 2)
    -> the fields of cairo_frame_metrics as lists over Y, U, V."""
    out = {"sse": [], "ssim_sum": [], "ssim_windows": [], "samples": []}
    for k in range(3):
        pw, ph = (w, h) if k == 0 else (w // 2, h // 2)
        m = plane_metrics(samples8(a[k], pw, ph, k == 0), samples8(b[k], pw, ph, k == 0))
        for key in out:
            out[key].append(m[key])
    return out


def psnr(sse: int, samples: int) -> float:
    return float("inf") if sse == 0 else 10.0 * float(np.log10(255.0 ** 2 * samples / sse))
