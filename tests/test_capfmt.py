"""Capture and 10-bit frames without a GPU: the layouts of YUY2, UYVY and P010,
their constants, cairo_frame_fold against the numpy restatement of the header's
text (tests/capfmt_ref.py), and the binding's checks before any native call."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import capfmt_ref as cap
from tests import pixfmt_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_id = lambda f: cap.FMT_NAMES[f]  # noqa: E731


# ---------------------------------------------------------------------------
# Layout and constants
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(2, 2), (70, 34), (3840, 2160)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_frame_layout(cairo, fmt, size):
    w, h = size
    rows = h + h // 2 if fmt == cap.P010 else h
    assert cairo.frame_layout(fmt, w, h) == (2 * w * rows, 2 * w)
    assert cairo.frame_layout(fmt, w, h, 2 * w) == (2 * w * rows, 2 * w)
    pitch = cap.pitched(fmt, w)
    assert cairo.frame_layout(fmt, w, h, pitch) == (pitch * rows, 2 * w)
    assert cairo.frame_layout(fmt, w, h, pitch)[0] == cap.layout(fmt, w, h, pitch)[0]
    if size == (3840, 2160) and fmt == cap.P010:
        assert cairo.frame_layout(fmt, w, h)[0] == 3 * w * h  # exactly the staging slot's size
    assert cap.image_mask(fmt, w, h, pitch).sum() == 2 * w * rows


def test_frame_layout_refusals(cairo):
    w, h = 70, 34
    cases = [(cap.P010, w, h, 2 * w + 1), (cap.P010, w, h, 2 * w + 3)]  # an odd P010 pitch
    cases += [(f, w, h, 2 * w - 1) for f in cap.CAP_FMTS]               # a pitch below tight
    cases += [(f, w + 1, h, 0) for f in cap.CAP_FMTS] + [(f, w, h + 1, 0) for f in cap.CAP_FMTS]
    cases += [(f, 0, h, 0) for f in cap.CAP_FMTS]
    cases += [(f, w, h, 0) for f in (5, 6, 7, 11)]
    for fmt, ww, hh, pitch in cases:
        with pytest.raises(ValueError):
            cairo.frame_layout(fmt, ww, hh, pitch)
        nb = ctypes.c_uint64()
        assert cairo.lib().cairo_frame_layout(fmt, ww, hh, pitch, ctypes.byref(nb), None) == cairo.EVX_ERROR_INVALID_ARGS
    assert cairo.frame_layout(cap.YUY2, w, h, 2 * w + 1) == ((2 * w + 1) * h, 2 * w)  # an odd pitch is fine for 8-bit samples
    assert cairo.frame_layout(cap.UYVY, w, h, 2 * w + 1) == ((2 * w + 1) * h, 2 * w)


@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_scale_check_refuses(cairo, fmt):
    """The scaled submit does not take the new layouts; the same geometry is
    fine for NV12."""
    assert cairo.scale_check(cairo.FMT_NV12, (128, 96), 64, 48)
    assert not cairo.scale_check(fmt, (128, 96), 64, 48)
    assert not cairo.scale_check(fmt, (64, 48), 64, 48)  # not even as a copy
    s = (ctypes.c_uint32 * 8)(128, 96, 0, 0, 0, 0, 0, 0)
    assert cairo.lib().cairo_scale_check(fmt, 0, s, 64, 48) == cairo.EVX_ERROR_INVALID_ARGS


def test_constants_match_header(cairo):
    text = open(os.path.join(ROOT, "include", "cairo_amd.h")).read()
    body = re.search(r"enum \{([^}]*CAIRO_FMT_YUY2[^}]*)\}", text).group(1)
    got = {k: int(v) for k, v in re.findall(r"CAIRO_FMT_(\w+)\s*=\s*(\d+)", body)}
    assert got == {"YUY2": cairo.FMT_YUY2, "UYVY": cairo.FMT_UYVY, "P010": cairo.FMT_P010}
    assert (cairo.FMT_YUY2, cairo.FMT_UYVY, cairo.FMT_P010) == (cap.YUY2, cap.UYVY, cap.P010) == (8, 9, 10)
    assert int(re.search(r"#define CAIRO_AMD_API_VERSION (\d+)", text).group(1)) == cairo.API_VERSION == 4
    assert cairo.lib().cairo_api_version() == 4


# ---------------------------------------------------------------------------
# cairo_frame_fold against the restatement
# ---------------------------------------------------------------------------

def _fold_both_ways(cairo, frame, fmt, w, h, pitch=0, npitch=0):
    """dir 0 of `frame`, then dir 1 of the result, each against the restatement
    and each into a buffer pre-filled with 0xA5 where pitched."""
    L = cairo.lib()
    tag = f"{cap.FMT_NAMES[fmt]} {w}x{h} pitch {pitch}/{npitch}"
    want = cap.fold(frame, fmt, w, h, pitch, npitch, fill=0xA5)
    nv12 = np.full(want.size, 0xA5, np.uint8)
    before = frame.copy()
    assert L.cairo_frame_fold(0, fmt, w, h, pitch, frame.ctypes.data, npitch, nv12.ctypes.data) == 0
    np.testing.assert_array_equal(nv12, want, err_msg=f"{tag}: fold (image and padding)")
    np.testing.assert_array_equal(frame, before, err_msg=f"{tag}: fold wrote its source")
    want2 = cap.unfold(nv12, fmt, w, h, pitch, npitch, fill=0xA5)
    back = np.full(want2.size, 0xA5, np.uint8)
    assert L.cairo_frame_fold(1, fmt, w, h, pitch, back.ctypes.data, npitch, nv12.ctypes.data) == 0
    np.testing.assert_array_equal(back, want2, err_msg=f"{tag}: unfold (image and padding)")
    if pitch or npitch:
        m = cap.image_mask(fmt, w, h, pitch)
        assert (back[~m] == 0xA5).all() and (nv12[~ref.image_mask(ref.NV12, w, h, npitch)] == 0xA5).all()
    if not pitch and not npitch:  # the binding gives the same
        np.testing.assert_array_equal(cairo.frame_fold(0, fmt, frame, w, h), want)
        np.testing.assert_array_equal(cairo.frame_fold(1, fmt, nv12, w, h), want2)
    return nv12


@pytest.mark.parametrize("fmt", (cap.YUY2, cap.UYVY), ids=_id)
def test_fold_422_exhaustive(cairo, fmt):
    """Every (row 0, row 1) pair of chroma bytes, in U and in V."""
    frame, w, h = cap.exhaustive_422(fmt, np.random.default_rng(fmt))
    _, u, v = cap.views(frame, fmt, w, h)
    for plane in (u, v):
        pairs = plane[0::2].astype(np.int64) * 256 + plane[1::2]
        assert np.unique(pairs).size == 65536
    nv12 = _fold_both_ways(cairo, frame, fmt, w, h)
    uv = ref.views(nv12, ref.NV12, w, h)[1]
    assert uv[..., 0].min() == 0 and uv[..., 0].max() == 255


def test_fold_p010_exhaustive(cairo):
    """Every ten-bit value with random low bits, at both half-word positions."""
    frame, w, h = cap.exhaustive_p010(np.random.default_rng(10))
    y, uv = cap.views(frame, cap.P010, w, h)
    for words in (y[:, 0::2], y[:, 1::2], uv[:, :, 0], uv[:, :, 1]):
        vals = (words[..., 0].astype(np.int32) | (words[..., 1].astype(np.int32) << 8))
        assert np.unique(vals >> 6).size == 1024 and np.unique(vals & 63).size == 64
    nv12 = _fold_both_ways(cairo, frame, cap.P010, w, h)
    # the limited-range code points land on their 8-bit ones; the top clamps
    for v10, s8 in ((64, 16), (940, 235), (960, 240), (0, 0), (1, 0), (2, 1), (1021, 255), (1023, 255)):
        one = np.zeros(cap.layout(cap.P010, 2, 2)[0], np.uint8)
        one[0], one[1] = ((v10 << 6) | 63) & 255, ((v10 << 6) | 63) >> 8
        assert cap.fold(one, cap.P010, 2, 2)[0] == s8
        assert cairo.frame_fold(0, cap.P010, one, 2, 2)[0] == s8
    assert nv12.max() == 255 and nv12.min() == 0


@pytest.mark.parametrize("size", [(2, 2), (70, 34)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_fold_pitched_keeps_padding(cairo, fmt, size):
    w, h = size
    rng = np.random.default_rng(100 * fmt + w)
    for pitch, npitch in ((cap.pitched(fmt, w), 0), (0, w + 3), (cap.pitched(fmt, w), w + 5)):
        frame = rng.integers(0, 256, cap.layout(fmt, w, h, pitch)[0], dtype=np.uint8)
        _fold_both_ways(cairo, frame, fmt, w, h, pitch, npitch)


@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_fold_of_unfold_is_identity(cairo, fmt):
    w, h = 70, 34
    rng = np.random.default_rng(7 + fmt)
    for _ in range(4):
        f = rng.integers(0, 256, ref.layout(ref.NV12, w, h)[0], dtype=np.uint8)
        np.testing.assert_array_equal(cap.fold(cap.unfold(f, fmt, w, h), fmt, w, h), f)  # the restatement itself
        np.testing.assert_array_equal(cairo.frame_fold(0, fmt, cairo.frame_fold(1, fmt, f, w, h), w, h), f)


def test_fold_refusals(cairo):
    L = cairo.lib()
    w, h = 4, 2
    a, b = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    for fmt in (cairo.FMT_RGB24, cairo.FMT_I420, cairo.FMT_NV12, 4, 7, 11, -1):
        assert L.cairo_frame_fold(0, fmt, w, h, 0, a.ctypes.data, 0, b.ctypes.data) == cairo.EVX_ERROR_INVALID_ARGS
    for args in ((2, cap.YUY2, w, h, 0, 0), (0, cap.P010, w, h, 2 * w + 1, 0), (0, cap.YUY2, w, h, 2 * w - 1, 0),
                 (0, cap.UYVY, w + 1, h, 0, 0), (0, cap.YUY2, w, h, 0, w - 1)):
        d, fmt, ww, hh, p, np_ = args
        assert L.cairo_frame_fold(d, fmt, ww, hh, p, a.ctypes.data, np_, b.ctypes.data) == cairo.EVX_ERROR_INVALID_ARGS
    assert L.cairo_frame_fold(0, cap.YUY2, w, h, 0, None, 0, b.ctypes.data) == cairo.EVX_ERROR_INVALID_ARGS
    assert not a.any() and not b.any()


# ---------------------------------------------------------------------------
# The binding
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_binding_checks_frame_before_native_call(cairo, fmt):
    """After set_input_format, encode() refuses a buffer of the wrong size,
    dtype or contiguity before the native call (no device is touched); so does
    frame_fold."""
    w, h = 64, 48
    nb = cairo.frame_layout(fmt, w, h)[0]
    e = cairo.Encoder()
    try:
        e.set_input_format(fmt, 0)
        for bad in (np.zeros(nb - 1, np.uint8), np.zeros(nb + 1, np.uint8), np.zeros(nb, np.int8),
                    np.zeros(nb // 2, np.uint16), np.zeros(2 * nb, np.uint8)[::2], np.zeros((h, w, 4), np.uint8)):
            with pytest.raises(ValueError):
                e.encode(bad, None, w, h)
        e.set_input_format(fmt, 2 * w + 2)
        with pytest.raises(ValueError):
            e.encode(np.zeros(nb, np.uint8), None, w, h)  # tight bytes for a pitched format
        e.set_input_format(fmt, 2 * w - 1)  # (before the first frame the pitch waits for the size)
        with pytest.raises(ValueError):
            e.encode(np.zeros(nb, np.uint8), None, w, h)  # no layout with a pitch below tight
    finally:
        e.close()
    d = cairo.Decoder()
    try:
        d.set_output_format(fmt, 0)
        for f in (5, 6, 11):
            with pytest.raises(cairo.CairoError):
                d.set_output_format(f, 0)
    finally:
        d.close()
    for bad in (np.zeros(nb - 1, np.uint8), np.zeros(nb, np.int8), np.zeros(2 * nb, np.uint8)[::2], [0] * nb):
        with pytest.raises(ValueError):
            cairo.frame_fold(0, fmt, bad, w, h)
    with pytest.raises(ValueError):
        cairo.frame_fold(1, fmt, np.zeros(nb, np.uint8), w, h)  # direction 1 takes the NV12 frame
    with pytest.raises(ValueError):
        cairo.frame_fold(0, cairo.FMT_NV12, np.zeros(w * h * 3 // 2, np.uint8), w, h)


@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_split_frame(cairo, fmt):
    w, h = 6, 4
    for pitch in (0, cap.pitched(fmt, w)):
        buf = np.random.default_rng(fmt).integers(0, 256, cairo.frame_layout(fmt, w, h, pitch)[0], dtype=np.uint8)
        got, want = cairo.split_frame(buf, fmt, w, h, pitch), cap.views(buf, fmt, w, h, pitch)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            if fmt == cap.P010:
                assert a.dtype == np.uint16
                b = b[..., 0].astype(np.uint16) | (b[..., 1].astype(np.uint16) << 8)
            np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError):
        cairo.split_frame(np.zeros(10, np.uint8), fmt, w, h)
