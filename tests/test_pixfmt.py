"""Pixel formats without a GPU: the frame layout, the constants, the wrapper's
checks before any native call, and the condition the GPU tests rest on -- every
frame they feed in as I420 / NV12 fits 8 bits, so that it reproduces the
oracle's input planes exactly."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import pixfmt_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fmt", [ref.RGB24, ref.BGR24, ref.I420, ref.NV12], ids=lambda f: ref.FMT_NAMES[f])
def test_frame_layout(cairo, fmt):
    w, h = 70, 34
    rgb = fmt in (ref.RGB24, ref.BGR24)
    tight = 3 * w if rgb else w
    assert cairo.frame_layout(fmt, w, h) == (tight * h if rgb else tight * h * 3 // 2, tight)
    assert cairo.frame_layout(fmt, w, h, tight) == cairo.frame_layout(fmt, w, h)
    pitch = 224 if rgb else 96
    assert cairo.frame_layout(fmt, w, h, pitch) == (pitch * h if rgb else pitch * h + pitch * (h // 2), tight)
    assert cairo.frame_layout(fmt, w, h, pitch)[0] == ref.layout(fmt, w, h, pitch)[0]


def test_frame_layout_refusals(cairo):
    for fmt, w, h, pitch in [(4, 70, 34, 0), (-1, 70, 34, 0), (cairo.FMT_RGB24, 71, 34, 0), (cairo.FMT_NV12, 70, 33, 0),
                             (cairo.FMT_I420, 0, 34, 0), (cairo.FMT_I420, 70, 34, 69), (cairo.FMT_NV12, 70, 34, 69),
                             (cairo.FMT_I420, 70, 34, 71), (cairo.FMT_RGB24, 70, 34, 209),
                             (cairo.FMT_BGR24, 70, 34, 209)]:
        with pytest.raises(ValueError):
            cairo.frame_layout(fmt, w, h, pitch)
        nb = ctypes.c_uint64()
        assert cairo.lib().cairo_frame_layout(fmt, w, h, pitch, ctypes.byref(nb), None) == cairo.EVX_ERROR_INVALID_ARGS
    assert cairo.frame_layout(cairo.FMT_NV12, 70, 34, 71) == (71 * 51, 70)  # an odd pitch is fine for NV12
    assert cairo.frame_layout(cairo.FMT_RGB24, 70, 34, 211) == (211 * 34, 210)


def test_format_constants_match_header(cairo):
    """The CAIRO_FMT_* values as the header and the binding name them, and the
    ABI version that introduced them."""
    text = open(os.path.join(ROOT, "include", "cairo_amd.h")).read()
    fmts = {k: int(v) for k, v in re.findall(r"#define CAIRO_FMT_(\w+)\s+(\d+)", text)}
    assert fmts == {"RGB24": cairo.FMT_RGB24, "BGR24": cairo.FMT_BGR24, "I420": cairo.FMT_I420,
                    "NV12": cairo.FMT_NV12}
    assert sorted(fmts.values()) == [0, 1, 2, 3]
    assert (ref.RGB24, ref.BGR24, ref.I420, ref.NV12) == (0, 1, 2, 3)
    assert int(re.search(r"#define CAIRO_AMD_API_VERSION (\d+)", text).group(1)) == cairo.API_VERSION == 4
    assert cairo.lib().cairo_api_version() == 4


def test_encoder_checks_frame_before_native_call(cairo):
    """After set_input_format, encode() refuses a buffer of the wrong size,
    dtype or contiguity before the native call (no device is touched)."""
    e = cairo.Encoder()
    try:
        e.set_input_format(cairo.FMT_NV12, 0)
        nb = cairo.frame_layout(cairo.FMT_NV12, 64, 48)[0]
        for bad in (np.zeros(nb - 1, np.uint8), np.zeros(nb + 1, np.uint8), np.zeros(nb, np.int8),
                    np.zeros(2 * nb, np.uint8)[::2], np.zeros((48, 64, 3), np.uint8)):
            with pytest.raises(ValueError):
                e.encode(bad, None, 64, 48)
        with pytest.raises(ValueError):
            e.encode(np.zeros(nb, np.uint8), None)  # a flat buffer does not tell its size
        with pytest.raises(cairo.CairoError):
            e.set_input_format(4, 0)
        e.set_input_format(cairo.FMT_I420, 66)
        with pytest.raises(ValueError):
            e.encode(np.zeros(64 * 48 * 3 // 2, np.uint8), None, 64, 48)  # tight bytes for a pitched format
    finally:
        e.close()
    d = cairo.Decoder()
    try:
        with pytest.raises(cairo.CairoError):
            d.set_output_format(7, 0)
        d.set_output_format(cairo.FMT_NV12, 0)
    finally:
        d.close()


def test_split_frame(cairo):
    w, h, p = 6, 4, 8
    for fmt in (cairo.FMT_I420, cairo.FMT_NV12, cairo.FMT_RGB24, cairo.FMT_BGR24):
        pitch = 3 * w + 5 if fmt in (cairo.FMT_RGB24, cairo.FMT_BGR24) else p
        buf = np.arange(cairo.frame_layout(fmt, w, h, pitch)[0], dtype=np.uint8)
        got = cairo.split_frame(buf, fmt, w, h, pitch)
        want = ref.views(buf, fmt, w, h, pitch)
        got = got if isinstance(got, tuple) else (got,)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError):
        cairo.split_frame(np.zeros(10, np.uint8), cairo.FMT_NV12, w, h)


def test_reference_round_trip_and_mask():
    """The helper itself: 8-bit-clean planes survive planes -> frame -> planes,
    pitch padding keeps the fill, and the clamp fires outside 8 bits."""
    rng = np.random.default_rng(5)
    w, h = 70, 34
    y = rng.integers(16, 272, (h, w)).astype(np.int16)
    u = rng.integers(0, 256, (h // 2, w // 2)).astype(np.int16)
    v = rng.integers(0, 256, (h // 2, w // 2)).astype(np.int16)
    for fmt, pitch in ((ref.I420, 0), (ref.I420, 72), (ref.NV12, 0), (ref.NV12, 73)):
        buf = ref.planes_to_frame(y, u, v, fmt, w, h, pitch, fill=0xFF)
        for a, b in zip(ref.frame_to_planes(buf, fmt, w, h, pitch), (y, u, v)):
            np.testing.assert_array_equal(a, b)
        m = ref.image_mask(fmt, w, h, pitch)
        assert m.sum() == w * h * 3 // 2 and (buf[~m] == 0xFF).all()
    y[0, 0], y[0, 1], u[0, 0], v[0, 0] = 15, 272, -1, 256
    buf = ref.planes_to_frame(y, u, v, ref.I420, w, h)
    yy, uu, vv = ref.frame_to_planes(buf, ref.I420, w, h)
    assert (yy[0, 0], yy[0, 1], uu[0, 0], vv[0, 0]) == (16, 271, 0, 255)


def test_reference_rgb_rule_equals_oracle(orc):
    """frame_to_planes on RGB24 / BGR24 frames restates the codec's RGB -> YUV
    rule: random bytes, and the pure colours whose chroma terms reach 256 and 1,
    must give the oracle's convert, tight or pitched."""
    rng = np.random.default_rng(11)
    w, h = 70, 34
    rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    rgb[0:2, 0:2], rgb[0:2, 2:4], rgb[2:4, 0:2], rgb[2:4, 2:4] = (0, 0, 255), (255, 0, 0), (0, 255, 0), (255, 255, 255)
    want = ref.oracle_input_planes(orc, rgb)
    assert want[1].max() == 256 and want[2].max() == 256
    for fmt, pitch in ((ref.RGB24, 0), (ref.RGB24, 3 * w + 1), (ref.BGR24, 0)):
        got = ref.frame_to_planes(ref.rgb_to_frame(rgb, fmt, pitch, fill=0xFF), fmt, w, h, pitch)
        for a, b, name in zip(got, want, "yuv"):
            assert a.dtype == np.int16
            np.testing.assert_array_equal(a, b[:a.shape[0], :a.shape[1]], err_msg=f"{ref.FMT_NAMES[fmt]} {name}")


def test_gpu_inputs_fit_8_bits(orc):
    """Every frame the GPU tests submit as I420 / NV12: the oracle's planes(0)
    must come back unchanged from planes -> frame -> planes inside w x h (the
    padding of the planes is zero and is never written by a convert)."""
    n = 0
    for kind, w, h, t in ref.gpu_inputs():
        y, u, v = ref.oracle_input_planes(orc, ref.make_frame(kind, w, h, t))
        for fmt in (ref.I420, ref.NV12):
            buf = ref.planes_to_frame(y, u, v, fmt, w, h)
            for a, b, name in zip(ref.frame_to_planes(buf, fmt, w, h), (y, u, v), "yuv"):
                ph, pw = (h, w) if name == "y" else (h // 2, w // 2)
                np.testing.assert_array_equal(a, b[:ph, :pw], err_msg=f"{kind} {w}x{h} frame {t} {name}")
        assert not y[h:].any() and not y[:, w:].any() and not u[h // 2:].any() and not u[:, w // 2:].any()
        n += 1
    assert n >= len(ref.ENC_SIZES) * len(ref.ENC_KINDS) * ref.ENC_FRAMES


def test_content_ranges(orc):
    """band4 and all of tests/content.py stay inside luma 16..271 and chroma
    7..250 at every size of interest (frames 0..5).  Random RGB *pixels* would
    not do for a KAT of the YUV input (pure blue gives U = 256 before the 2x2
    mean): the noise content passes only because its chroma is averaged."""
    from tests import content

    for w, h in ((16, 16), (64, 48), (70, 34), (72, 40), (200, 120), (352, 288), (1280, 720)):
        for kind in ("band4",) + content.KINDS:
            for t in range(6 if w < 1280 else 2):
                y, u, v = ref.oracle_input_planes(orc, ref.make_frame(kind, w, h, t))
                yy, uu, vv = y[:h, :w], u[:h // 2, :w // 2], v[:h // 2, :w // 2]
                assert 16 <= yy.min() and yy.max() <= 271, (kind, w, h, t)
                assert 7 <= min(uu.min(), vv.min()) and max(uu.max(), vv.max()) <= 250, (kind, w, h, t)
    blue = np.zeros((2, 2, 3), np.uint8)
    blue[..., 2] = 255
    assert ref.oracle_input_planes(orc, blue)[1][0, 0] == 256
