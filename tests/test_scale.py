"""The scaled submit without a GPU: cairo_scale_check against the rule's
constraints (include/cairo_amd.h, cairo_source), the binding's struct, the new
symbols, and the properties of the numpy restatement (tests/scale_ref.py) that
the GPU tests compare the kernel against."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import pixfmt_ref as pf
from tests import scale_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMTS = (ref.RGB24, ref.BGR24, ref.I420, ref.NV12)
SCALE_SYMBOLS = ("cairo_source_size", "cairo_scale_check", "cairo_ctx_submit_scaled", "cairo_stream_submit_scaled",
                 "cairo_kat_scale")

# (format, pitch, source size, crop, output size) -> accepted?
CHECK_CASES = [
    # the renditions of a 4K master, a copy, a crop
    (ref.RGB24, 0, (3840, 2160), None, (1920, 1080), True),
    (ref.NV12, 0, (3840, 2160), None, (1280, 720), True),
    (ref.I420, 4096, (3840, 2160), None, (480, 270), True),
    (ref.BGR24, 0, (64, 48), None, (64, 48), True),
    (ref.NV12, 0, (160, 80), (6, 4, 140, 68), (70, 34), True),
    (ref.I420, 0, (356, 288), (0, 0, 354, 288), (118, 96), True),
    # odd sizes
    (ref.RGB24, 0, (141, 68), None, (70, 34), False),
    (ref.RGB24, 0, (140, 67), None, (70, 34), False),
    (ref.RGB24, 0, (140, 68), None, (71, 34), False),
    (ref.RGB24, 0, (140, 68), None, (70, 33), False),
    (ref.NV12, 0, (160, 80), (5, 4, 140, 68), (70, 34), False),
    (ref.NV12, 0, (160, 80), (6, 3, 140, 68), (70, 34), False),
    (ref.NV12, 0, (160, 80), (6, 4, 139, 68), (70, 34), False),
    (ref.NV12, 0, (160, 80), (6, 4, 140, 67), (70, 34), False),
    (ref.RGB24, 0, (0, 68), None, (70, 34), False),
    (ref.RGB24, 0, (140, 68), None, (0, 34), False),
    # a crop outside the source
    (ref.NV12, 0, (160, 80), (22, 4, 140, 68), (70, 34), False),
    (ref.NV12, 0, (160, 80), (6, 14, 140, 68), (70, 34), False),
    (ref.NV12, 0, (160, 80), (20, 12, 140, 68), (70, 34), True),  # flush with the far corner
    (ref.NV12, 0, (160, 80), (2 ** 32 - 2, 0, 4, 4), (4, 4), False),  # x + w wraps in 32 bits
    (ref.NV12, 0, (160, 80), (6, 4, 0, 68), (70, 34), False),  # crop_w 0 means no crop at all
    # upscaling
    (ref.RGB24, 0, (70, 34), None, (72, 34), False),
    (ref.RGB24, 0, (70, 34), None, (70, 36), False),
    (ref.RGB24, 0, (160, 80), (0, 0, 68, 34), (70, 34), False),
    # 8:1 accepted, 8:1 + 2 samples refused
    (ref.I420, 0, (272, 144), None, (34, 18), True),
    (ref.I420, 0, (274, 144), None, (34, 18), False),
    (ref.I420, 0, (272, 146), None, (34, 18), False),
    # 255 Lx Ly < 2^31
    (ref.RGB24, 0, (8192, 8192), None, (4098, 4098), False),
    (ref.RGB24, 0, (3840, 2160), None, (1918, 1078), True),
    # an unknown format
    (4, 0, (140, 68), None, (70, 34), False),
    (-1, 0, (140, 68), None, (70, 34), False),
    # a short pitch (the pitch is the source's), an odd I420 pitch
    (ref.RGB24, 3 * 140 - 1, (140, 68), None, (70, 34), False),
    (ref.RGB24, 3 * 70, (140, 68), None, (70, 34), False),
    (ref.NV12, 139, (140, 68), None, (70, 34), False),
    (ref.NV12, 141, (140, 68), None, (70, 34), True),
    (ref.I420, 141, (140, 68), None, (70, 34), False),
    (ref.I420, 142, (140, 68), None, (70, 34), True),
]


@pytest.mark.parametrize("case", CHECK_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}-{c[3]}-{c[4][0]}x{c[4][1]}")
def test_scale_check(cairo, case):
    fmt, pitch, size, crop, (dw, dh), want = case
    assert cairo.scale_check(fmt, size, dw, dh, crop=crop, pitch=pitch) is want
    if 0 <= fmt <= 3 and (crop is None or all(v < 2 ** 31 for v in crop)):
        assert ref.valid(fmt, pitch, size, crop, dw, dh) is want, "the restatement's own constraints disagree"


def test_scale_check_every_4k_rendition(cairo):
    """3840x2160 to any even size from 480x270 up passes the 2^31 bound (the
    header's promise): the restatement over all of them, the library on a
    sample of them."""
    for dw in range(480, 3841, 2):
        lx = ref.axis(3840, dw)[0]
        for dh in (270, 1078, 1080, 2158, 2160):
            assert 255 * lx * ref.axis(2160, dh)[0] < 2 ** 31
    worst = max(ref.axis(3840, dw)[0] for dw in range(480, 3841, 2)) * max(ref.axis(2160, dh)[0]
                                                                           for dh in range(270, 2161, 2))
    assert 255 * worst < 2 ** 31
    for dw, dh in ((480, 270), (482, 272), (1918, 1078), (1280, 720), (3838, 2158), (3840, 2160)):
        assert cairo.scale_check(cairo.FMT_NV12, (3840, 2160), dw, dh)


def test_scale_check_reserved_and_null(cairo):
    L = cairo.lib()
    s = cairo._Source(140, 68, 0, 0, 0, 0)
    assert L.cairo_scale_check(cairo.FMT_RGB24, 0, ctypes.byref(s), 70, 34) == 0
    s.reserved[1] = 1
    assert L.cairo_scale_check(cairo.FMT_RGB24, 0, ctypes.byref(s), 70, 34) == cairo.EVX_ERROR_INVALID_ARGS
    assert L.cairo_scale_check(cairo.FMT_RGB24, 0, None, 70, 34) == cairo.EVX_ERROR_INVALID_ARGS


def test_source_struct_size(cairo):
    assert cairo.lib().cairo_source_size() == ctypes.sizeof(cairo._Source) == 32


def test_scale_symbols_exported(cairo):
    """The header declares the scaled submit's entry points, the library
    exports them and the API version stays 4 (entry points only)."""
    text = open(os.path.join(ROOT, "include", "cairo_amd.h")).read()
    declared = set(re.findall(r"CAIRO_API\s+[\w\s\*]+?\b((?:cairo|evx)_\w+)\s*\(", text))
    L = cairo.lib()
    for n in SCALE_SYMBOLS:
        assert n in declared, n
        assert hasattr(L, n), n
    assert L.cairo_api_version() == 4
    assert int(re.search(r"#define CAIRO_KAT_SCALE_GUARD (\d+)", text).group(1)) == cairo.KAT_SCALE_GUARD


def test_kat_refuses_invalid_arguments_without_a_device(cairo):
    """Arguments that fail cairo_scale_check never reach the device: the
    known-answer entry point refuses them first."""
    s = cairo._Source(70, 34, 0, 0, 0, 0)
    src, out = np.zeros(70 * 34 * 3, np.uint8), np.zeros(140 * 68 * 3 + cairo.KAT_SCALE_GUARD, np.uint8)
    st = cairo.lib().cairo_kat_scale(cairo.FMT_RGB24, 0, ctypes.byref(s), src.ctypes.data, 140, 68, out.ctypes.data, 0)
    assert st == cairo.EVX_ERROR_INVALID_ARGS  # upscaling


# ---------------------------------------------------------------------------
# The restatement's own properties
# ---------------------------------------------------------------------------

AXES = [(s, d) for (sz, dz) in ref.KAT_SIZES for (s, d) in zip(sz, dz)] + [(354, 118), (528, 264), (528, 176), (8, 2)]


@pytest.mark.parametrize("S,D", sorted(set(AXES)))
def test_weights_sum_to_L(S, D):
    L, P = ref.axis(S, D)
    w = ref.weights(S, D)
    assert w.shape == (D, S) and (w >= 0).all()
    assert (w.sum(axis=1) == L).all()
    assert (w.sum(axis=0) == P).all()  # every source sample is used exactly once
    assert (np.count_nonzero(w, axis=1) <= 9).all()  # at most 8 + 1 taps per output sample


def test_same_size_is_identity():
    rng = np.random.default_rng(7)
    p = rng.integers(0, 256, (48, 64), dtype=np.uint8)
    np.testing.assert_array_equal(ref.scale_plane(p, 64, 48), p)
    for fmt in FMTS:
        f = rng.integers(0, 256, pf.layout(fmt, 64, 48)[0], dtype=np.uint8)
        np.testing.assert_array_equal(ref.scaled_frame(f, fmt, 0, ((64, 48), None), 64, 48), f)


@pytest.mark.parametrize("value", [0, 1, 254, 255])
def test_constant_stays_constant(value):
    for (sw, sh), (dw, dh) in ref.KAT_SIZES:
        out = ref.scale_plane(np.full((sh, sw), value, np.uint8), dw, dh)
        assert (out == value).all(), f"{sw}x{sh} -> {dw}x{dh}"


def test_two_to_one_is_the_rounded_up_mean():
    rng = np.random.default_rng(8)
    p = rng.integers(0, 256, (68, 140), dtype=np.uint8)
    p[0:2, 0:2] = [[0, 0], [0, 2]]   # 0.5 -> 1
    p[0:2, 2:4] = [[255, 255], [255, 254]]  # 254.75 -> 255
    p[0:2, 4:6] = [[1, 0], [0, 0]]   # 0.25 -> 0
    a = p.astype(np.int64)
    want = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
    got = ref.scale_plane(p, 70, 34)
    np.testing.assert_array_equal(got, want)
    assert tuple(got[0, :3]) == (1, 255, 0)


def test_axis_order_does_not_matter():
    rng = np.random.default_rng(9)
    for (sw, sh), (dw, dh) in ref.KAT_SIZES[:6]:
        p = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
        np.testing.assert_array_equal(ref.scale_plane(p, dw, dh, "yx"), ref.scale_plane(p, dw, dh, "xy"))


def test_scaled_frame_layouts():
    """scaled_frame scales each plane of each format on its own: the four
    formats of one picture agree plane by plane, a pitch changes nothing, and a
    crop equals scaling the cropped picture."""
    rng = np.random.default_rng(10)
    sw, sh, dw, dh = 160, 80, 70, 34
    crop = (6, 4, 140, 68)
    y = rng.integers(0, 256, (sh, sw), dtype=np.uint8)
    u = rng.integers(0, 256, (sh // 2, sw // 2), dtype=np.uint8)
    v = rng.integers(0, 256, (sh // 2, sw // 2), dtype=np.uint8)

    def build(fmt, pitch):
        buf = np.full(pf.layout(fmt, sw, sh, pitch)[0], 0xEE, np.uint8)
        vw = pf.views(buf, fmt, sw, sh, pitch)
        vw[0][...] = y
        if fmt == ref.I420:
            vw[1][...], vw[2][...] = u, v
        else:
            vw[1][..., 0], vw[1][..., 1] = u, v
        return buf

    wy = ref.scale_plane(y[4:72, 6:146], dw, dh)
    wu = ref.scale_plane(u[2:36, 3:73], dw // 2, dh // 2)
    wv = ref.scale_plane(v[2:36, 3:73], dw // 2, dh // 2)
    for fmt in (ref.I420, ref.NV12):
        for pitch in (0, sw + 6):
            got = pf.views(ref.scaled_frame(build(fmt, pitch), fmt, pitch, ((sw, sh), crop), dw, dh), fmt, dw, dh)
            np.testing.assert_array_equal(got[0], wy)
            if fmt == ref.I420:
                np.testing.assert_array_equal(got[1], wu)
                np.testing.assert_array_equal(got[2], wv)
            else:
                np.testing.assert_array_equal(got[1][..., 0], wu)
                np.testing.assert_array_equal(got[1][..., 1], wv)
    rgb = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    a = ref.scaled_frame(pf.rgb_to_frame(rgb, ref.RGB24), ref.RGB24, 0, ((sw, sh), crop), dw, dh)
    b = ref.scaled_frame(pf.rgb_to_frame(rgb, ref.BGR24, 3 * sw + 3, 0xEE), ref.BGR24, 3 * sw + 3, ((sw, sh), crop), dw, dh)
    np.testing.assert_array_equal(a.reshape(dh, dw, 3), b.reshape(dh, dw, 3)[..., ::-1])
    for c in range(3):
        np.testing.assert_array_equal(a.reshape(dh, dw, 3)[..., c], ref.scale_plane(rgb[4:72, 6:146, c], dw, dh))
