"""Colour descriptions without a GPU: the library's coefficient table against
the derivation from Kr / Kb in exact rationals, the integer maps against real
arithmetic within the derived bound, the grey axis, and the identity
(tests/color_ref.py; include/cairo_amd.h CAIRO_RANGE_*, CAIRO_MATRIX_*).
"""
from fractions import Fraction as F

import numpy as np
import pytest

from tests import color_ref as cr
from tests import pixfmt_ref as pf

_cid = lambda c: f"{'limited' if c[0] else 'full'}-{'709' if c[1] else '601'}"  # noqa: E731
CASES = [(d, r, m) for d in (0, 1) for r, m in cr.NON_IDENTITY]


def test_coefs_equal_the_derivation(cairo):
    """cairo_color_coefs for all 2 x 2 x 2 combinations equals the Fraction
    derivation; the identity is 16384 I with offset 0."""
    for d in (0, 1):
        for r, m in cr.DESCRIPTIONS:
            k, oy = cairo.color_coefs(d, r, m)
            want, woy = cr.coefs(d, r, m)
            assert k.reshape(-1).tolist() == want and oy == woy, (d, r, m)
        k, oy = cairo.color_coefs(d, cairo.RANGE_FULL, cairo.MATRIX_BT601)
        assert np.array_equal(k, 16384 * np.eye(3, dtype=np.int32)) and oy == 0


def test_derivation_shape():
    """Both real matrices have the shape [x a b; 0 c d; 0 e f], the BT.601 ones
    are diagonal, and dir 1 inverts dir 0."""
    for r, m in cr.DESCRIPTIONS:
        cin, _ = cr.real_matrix(0, r, m)
        cout, _ = cr.real_matrix(1, r, m)
        prod = [[sum(cout[i][k] * cin[k][j] for k in range(3)) for j in range(3)] for i in range(3)]
        assert prod == [[F(int(i == j)) for j in range(3)] for i in range(3)]
        if m == cr.BT601:
            assert all(cin[i][j] == 0 for i in range(3) for j in range(3) if i != j)


def test_unknown_values_are_refused(cairo):
    L = cairo.lib()
    k = np.zeros(9, np.int32)
    import ctypes

    oy = ctypes.c_int32()
    for bad in ((2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 2), (1, 1, -1)):
        assert L.cairo_color_coefs(*bad, k.ctypes.data, ctypes.byref(oy)) == cairo.EVX_ERROR_INVALID_ARGS, bad
        with pytest.raises(ValueError):
            cairo.color_coefs(*bad)
    assert L.cairo_color_coefs(0, 1, 1, None, ctypes.byref(oy)) == cairo.EVX_ERROR_INVALID_ARGS


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"dir{c[0]}-{_cid(c[1:])}")
def test_integer_map_within_the_bound(case):
    """Every (U8, V8) pair for chroma and every Y8 against every (U8, V8) pair
    for luma: the integer map is within 0.5 + 511/32768 of the real-arithmetic
    value (float64, whose own error here is below 1e-10)."""
    d, r, m = case
    bound = float(cr.BOUND) + 1e-9
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    _, ui, vi = cr.map_samples(np.zeros_like(u), u, v, d, r, m)
    _, ur, vr = cr.real_samples(np.zeros_like(u), u, v, d, r, m)
    worst = max(np.abs(ui - ur).max(), np.abs(vi - vr).max())
    assert worst <= bound, f"chroma: {worst}"
    for y in range(256):
        yi, _, _ = cr.map_samples(np.full_like(u, y), u, v, d, r, m)
        yr, _, _ = cr.real_samples(np.full_like(u, y), u, v, d, r, m)
        worst = max(worst, np.abs(yi - yr).max())
    assert worst <= bound, f"luma: {worst}"


def test_grey_axis_limited_bt601_input():
    f = lambda y: int(cr.map_samples(np.array([y]), np.array([128]), np.array([128]), 0, cr.LIMITED, cr.BT601)[0][0])  # noqa: E731
    assert (f(16), f(235), f(126)) == (0, 255, 128)
    assert [f(y) for y in (0, 5, 15)] == [0, 0, 0] and [f(y) for y in (236, 250, 255)] == [255, 255, 255]
    _, u, v = cr.map_samples(np.array([77]), np.array([128]), np.array([128]), 0, cr.LIMITED, cr.BT601)
    assert (int(u[0]), int(v[0])) == (128, 128)
    # the nominal chroma extremes sit at 0.5 and 255.5 in real arithmetic: they land within the bound of them
    _, u, v = cr.map_samples(np.array([0, 0]), np.array([16, 240]), np.array([240, 16]), 0, cr.LIMITED, cr.BT601)
    assert u.tolist() == [1, 255] and v.tolist() == [255, 1]


@pytest.mark.parametrize("fmt", (pf.I420, pf.NV12), ids=lambda f: pf.FMT_NAMES[f])
def test_identity_maps_a_frame_to_itself(fmt):
    rng = np.random.default_rng(5)
    for w, h in ((2, 2), (70, 34)):
        tight = pf.layout(fmt, w, h)[1]
        for pitch in (0, tight + (2 if fmt == pf.I420 else 3)):
            frame = rng.integers(0, 256, pf.layout(fmt, w, h, pitch)[0], dtype=np.uint8)
            for d in (0, 1):
                assert np.array_equal(cr.map_frame(frame, fmt, w, h, pitch, d, cr.FULL, cr.BT601), frame)


def test_map_frame_touches_the_image_only():
    """A non-identity map changes image bytes, keeps the pitch padding, and
    gives the same samples for I420 and NV12 frames of the same planes; an RGB
    frame is returned as it is."""
    rng = np.random.default_rng(6)
    w, h = 70, 34
    y = rng.integers(0, 256, (h, w)).astype(np.int16) + 16
    u = rng.integers(0, 256, (h // 2, w // 2)).astype(np.int16)
    v = rng.integers(0, 256, (h // 2, w // 2)).astype(np.int16)
    for r, m in cr.NON_IDENTITY:
        for d in (0, 1):
            outs = []
            for fmt, pitch in ((pf.I420, 72), (pf.NV12, 73)):
                frame = pf.planes_to_frame(y, u, v, fmt, w, h, pitch, fill=0xA5)
                out = cr.map_frame(frame, fmt, w, h, pitch, d, r, m)
                mask = pf.image_mask(fmt, w, h, pitch)
                assert (out[~mask] == 0xA5).all() and not np.array_equal(out[mask], frame[mask])
                outs.append(pf.frame_to_planes(out, fmt, w, h, pitch))
            for a, b in zip(*outs):
                assert np.array_equal(a, b)
    rgb = rng.integers(0, 256, 3 * w * h, dtype=np.uint8)
    assert np.array_equal(cr.map_frame(rgb, pf.RGB24, w, h, 0, 0, cr.LIMITED, cr.BT709), rgb)
