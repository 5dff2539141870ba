"""The scaled tensor submit without a GPU: cairo_tensor_scale_check against
the restated constraints (tests/tensor_scale_ref.py), the binding's keywords,
the new symbols, and the order of the rule -- rounding first, then averaging --
pinned on the KAT's own inputs."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import tensor_ref as tr
from tests import tensor_scale_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cairo_tensor_scale_check", "cairo_ctx_submit_tensor_scaled", "cairo_stream_submit_tensor_scaled",
           "cairo_kat_tensor_scale")
BASE = 1 << 20
ONES, ZEROS = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)


def chw(w, h):
    return (w * h, w, 1)


def hwc(w, h):
    return (1, 3 * w, 3)


# (dtype, strides, source size, crop, output size, accepted?, what)
CHECK_CASES = [
    (tr.F16, chw(3840, 2160), (3840, 2160), None, (1920, 1080), True, "4K to 1080p"),
    (tr.F32, hwc(3840, 2160), (3840, 2160), None, (1280, 720), True, "4K to 720p, channels last"),
    (tr.U8, hwc(64, 48), (64, 48), None, (64, 48), True, "the copy case S == D"),
    (tr.BF16, (1, 4 * 160, 4), (160, 80), (6, 4, 140, 68), (70, 34), True, "a crop of an RGBA tensor"),
    (tr.F16, chw(160, 80), (160, 80), (20, 12, 140, 68), (70, 34), True, "a crop flush with the far corner"),
    (tr.F16, chw(272, 144), (272, 144), None, (34, 18), True, "8:1"),
    (tr.F16, chw(160, 80), (160, 80), (5, 4, 140, 68), (70, 34), False, "an odd crop origin"),
    (tr.F16, chw(160, 80), (160, 80), (6, 4, 140, 67), (70, 34), False, "an odd crop height"),
    (tr.F16, chw(141, 68), (141, 68), None, (70, 34), False, "an odd source width"),
    (tr.F16, chw(140, 68), (140, 68), None, (70, 33), False, "an odd output height"),
    (tr.F16, chw(160, 80), (160, 80), (22, 4, 140, 68), (70, 34), False, "a crop outside the source"),
    (tr.F16, chw(160, 80), (160, 80), (6, 14, 140, 68), (70, 34), False, "a crop below the source"),
    (tr.F16, chw(352, 288), (352, 288), (0, 0, 174, 144), (176, 144), False, "the upscale 174 -> 176"),
    (tr.F16, chw(70, 34), (70, 34), None, (70, 36), False, "an upscale in y"),
    (tr.F16, chw(306, 144), (306, 144), None, (34, 18), False, "9:1"),
    (tr.F16, chw(272, 146), (272, 146), None, (34, 18), False, "8:1 and two rows"),
    (tr.U8, chw(8192, 8192), (8192, 8192), None, (4098, 4098), False, "255 Lx Ly >= 2^31"),
    (tr.U8, chw(32770, 16), (32770, 16), None, (16386, 8), False, "a side above 32768"),
    (tr.F16, (140 * 68, 139, 1), (140, 68), None, (70, 34), False, "overlapping rows"),
    (tr.F16, (1, 3 * 140, 2), (140, 68), None, (70, 34), False, "overlapping pixels"),
    (tr.F16, chw(70, 34), (140, 68), None, (70, 34), False, "strides of the output's size, not the source's"),
    (7, chw(140, 68), (140, 68), None, (70, 34), False, "an unknown dtype"),
    (tr.F16, chw(140, 68), (0, 68), None, (70, 34), False, "an empty source"),
]


def _check(cairo, dtype, strides, src_size, crop, dw, dh, mul=ONES, add=ZEROS, reserved=(0, 0, 0), base=BASE):
    """The library's verdict (a span or None) after comparing it with the
    restatement's."""
    d = cairo.tensor_desc((base, dtype, strides), mul=mul, add=add)
    d.c.reserved0, d.c.reserved[0], d.c.reserved[1] = reserved
    got = cairo.tensor_scale_check(d, src_size, dw, dh, crop=crop)
    want = ref.valid(dtype, strides, mul, add, reserved, base, src_size, crop, dw, dh)
    assert (got is not None) == want, "the library and the restatement disagree"
    if want:  # the span is the source tensor's
        assert got == tr.check(dtype, strides, mul, add, reserved, base, *src_size)
    return got


@pytest.mark.parametrize("case", CHECK_CASES, ids=lambda c: c[6].replace(" ", "_"))
def test_tensor_scale_check(cairo, case):
    dtype, strides, size, crop, (dw, dh), want, what = case
    assert (_check(cairo, dtype, strides, size, crop, dw, dh) is not None) == want, what


def test_tensor_scale_check_descriptor_rules(cairo):
    """Each rule of cairo_tensor_check, violated alone, on a source that scales."""
    size, st, out = (140, 68), chw(140, 68), (70, 34)
    assert _check(cairo, tr.F16, st, size, None, *out) == 3 * 140 * 68 * 2
    for res in ((1, 0, 0), (0, 1, 0), (0, 0, 7)):
        assert _check(cairo, tr.F16, st, size, None, *out, reserved=res) is None
    for bad in (np.nan, np.inf, -np.inf):
        assert _check(cairo, tr.F32, st, size, None, *out, mul=(1.0, bad, 1.0)) is None
        assert _check(cairo, tr.F32, st, size, None, *out, add=(bad, 0.0, 0.0)) is None
    for dtype, base, good in ((tr.U8, BASE + 1, True), (tr.F16, BASE + 1, False), (tr.F16, BASE + 2, True),
                              (tr.BF16, BASE + 3, False), (tr.F32, BASE + 2, False), (tr.F32, BASE + 4, True)):
        assert (_check(cairo, dtype, st, size, None, *out, base=base) is not None) == good


def test_tensor_scale_check_every_4k_rendition(cairo):
    """The ladder of tests/test_scale.py from a float16 CHW 4K tensor."""
    st = chw(3840, 2160)
    for dw, dh in ((480, 270), (482, 272), (1918, 1078), (1280, 720), (1920, 1080), (3838, 2158), (3840, 2160)):
        assert _check(cairo, tr.F16, st, (3840, 2160), None, dw, dh) == 3 * 3840 * 2160 * 2, (dw, dh)


def test_tensor_scale_check_source_words_and_null(cairo):
    L = cairo.lib()
    d = cairo.tensor_desc((BASE, tr.F16, chw(140, 68)), mul=ONES, add=ZEROS)
    s = cairo._Source(140, 68, 0, 0, 0, 0)
    span = ctypes.c_uint64()
    assert L.cairo_tensor_scale_check(ctypes.byref(d.c), BASE, ctypes.byref(s), 70, 34, ctypes.byref(span)) == 0
    assert span.value == 3 * 140 * 68 * 2
    assert L.cairo_tensor_scale_check(ctypes.byref(d.c), BASE, ctypes.byref(s), 70, 34, None) == 0
    for k in (0, 1):
        s.reserved[k] = 1
        assert L.cairo_tensor_scale_check(ctypes.byref(d.c), BASE, ctypes.byref(s), 70, 34, None) == \
            cairo.EVX_ERROR_INVALID_ARGS
        s.reserved[k] = 0
    assert L.cairo_tensor_scale_check(ctypes.byref(d.c), BASE, None, 70, 34, None) == cairo.EVX_ERROR_INVALID_ARGS
    assert L.cairo_tensor_scale_check(None, BASE, ctypes.byref(s), 70, 34, None) == cairo.EVX_ERROR_INVALID_ARGS


def test_symbols_exported(cairo):
    """The header declares the entry points, the library exports them and the
    API version stays 4 (entry points only)."""
    text = open(os.path.join(ROOT, "include", "cairo_amd.h")).read()
    declared = set(re.findall(r"CAIRO_API\s+[\w\s\*]+?\b((?:cairo|evx)_\w+)\s*\(", text))
    L = cairo.lib()
    for n in SYMBOLS:
        assert n in declared, n
        assert hasattr(L, n), n
    assert L.cairo_api_version() == 4
    assert "#define CAIRO_AMD_API_VERSION 4" in text


def test_kat_refuses_invalid_arguments_without_a_device(cairo):
    """Arguments that fail cairo_tensor_scale_check never reach the device: the
    known-answer entry point refuses them first (a device call would report a
    hardware failure here, or run)."""
    t = np.zeros(3 * 140 * 68, np.float16)
    rgb = np.zeros(3 * 70 * 34 + cairo.KAT_TENSOR_GUARD, np.uint8)
    d = cairo.tensor_desc((t.ctypes.data, tr.F16, chw(140, 68)), mul=ONES, add=ZEROS)
    L = cairo.lib()

    def kat(src, nbytes=t.nbytes, dw=70, dh=34, desc=d, out=rgb):
        return L.cairo_kat_tensor_scale(ctypes.byref(desc.c), ctypes.byref(src) if src is not None else None,
                                        t.ctypes.data, nbytes, dw, dh, out.ctypes.data, 0)

    bad = cairo.EVX_ERROR_INVALID_ARGS
    assert kat(cairo._Source(140, 68, 0, 0, 68, 34)) == bad           # the upscale 68 -> 70
    assert kat(cairo._Source(140, 68, 1, 0, 138, 68)) == bad          # an odd crop
    assert kat(cairo._Source(140, 68, 0, 0, 0, 0), dw=16, dh=34) == bad   # 140 > 8 * 16
    assert kat(cairo._Source(140, 70, 0, 0, 0, 0)) == bad             # a span beyond tensor_bytes
    assert kat(cairo._Source(140, 68, 0, 0, 0, 0), nbytes=t.nbytes - 2) == bad
    assert kat(None) == bad
    wrong = cairo.tensor_desc((t.ctypes.data, tr.F16, chw(70, 34)), mul=ONES, add=ZEROS)
    assert kat(cairo._Source(140, 68, 0, 0, 0, 0), desc=wrong) == bad  # strides of the output's size
    with pytest.raises(ValueError):
        cairo.kat_tensor_scale(d, (140, 68), t.nbytes, 70, 34, rgb[:-1])
    assert (rgb == 0).all()


def _context(cairo, w, h):
    """A Context object with no device behind it: the keyword errors below are
    raised before anything is handed to the library."""
    ctx = object.__new__(cairo.Context)
    ctx.h, ctx.width, ctx.height, ctx._keep = None, w, h, {}
    return ctx


def test_submit_tensor_keywords(cairo):
    ctx = _context(cairo, 176, 144)
    shapeless = (BASE, "float16", chw(352, 288))
    held = cairo.tensor_desc(shapeless)
    assert held.width is None
    arr = np.zeros((3, 288, 352), np.float16)
    for t in (shapeless, held):
        with pytest.raises(ValueError, match="src_size"):  # a crop, no shape, no src_size
            ctx.submit_tensor(t, 0, False, 16, crop=(0, 0, 352, 288))
        with pytest.raises(ValueError, match="src_size"):
            ctx.submit_tensor(t, 0, False, 16, scaled=True)
    with pytest.raises(ValueError, match="contradicts"):
        ctx.submit_tensor(arr, 0, False, 16, scaled=True, src_size=(352, 290))
    with pytest.raises(ValueError, match="contradicts"):
        ctx.submit_tensor(arr, 0, False, 16, crop=(0, 0, 176, 144), src_size=(176, 144))
    with pytest.raises(ValueError):  # a malformed crop
        ctx.submit_tensor(arr, 0, False, 16, crop=(0, 0, 352))
    # without the new keywords: today's errors
    with pytest.raises(ValueError, match="the context's are 176x144"):
        ctx.submit_tensor(arr, 0, False, 16)
    with pytest.raises(ValueError, match="scaled=True"):
        ctx.submit_tensor(arr, 0, False, 16, src_size=(352, 288))
    assert ctx._keep == {}
    # tensor_scale_check takes the size from the shape, and refuses a contradiction
    d = cairo.tensor_desc(arr)
    assert cairo.tensor_scale_check(d, None, 176, 144) == arr.nbytes
    assert cairo.tensor_scale_check(d, (352, 288), 176, 144, crop=(2, 2, 350, 286)) == arr.nbytes
    assert cairo.tensor_scale_check(d, (352, 290), 176, 144) is None
    assert cairo.tensor_scale_check(held, None, 176, 144) is None
    assert cairo.tensor_scale_check(held, (352, 288), 176, 144) == arr.nbytes


# ---------------------------------------------------------------------------
# The restatement, and the order of the rule
# ---------------------------------------------------------------------------

def test_copy_is_pack(cairo):
    """S == D: the frame is pack(tensor), which cairo_tensor_host computes."""
    case = ref.kat_case(tr.F16, "chw_padded", (64, 48), 0, 1)
    want = ref.case_expected(case, None, 64, 48)
    np.testing.assert_array_equal(want, tr.expected(case)[1])
    d = cairo.tensor_desc((case["buf"].ctypes.data, tr.F16, case["strides"]), mul=case["mul"], add=case["add"])
    rgb = np.zeros(3 * 64 * 48, np.uint8)
    cairo.tensor_host(0, d, 64, 48, rgb)
    np.testing.assert_array_equal(rgb.reshape(48, 64, 3), want)


def test_crop_equals_scaling_the_cropped_tensor():
    case = ref.kat_case(tr.BF16, "rgba", (160, 80), 2, 2)
    crop = (6, 4, 140, 68)
    whole = tr.expected(case)[1]
    want = ref.scale_rgb(whole[4:72, 6:146], 70, 34)
    np.testing.assert_array_equal(ref.case_expected(case, crop, 70, 34), want)


@pytest.mark.parametrize("dtype", (tr.U8, tr.F16, tr.BF16, tr.F32), ids=lambda d: tr.NAMES[d])
def test_the_kat_inputs_tell_the_two_orders_apart(dtype):
    """The rule rounds every element to its sample first and averages the
    samples.  Averaging the mapped values first and rounding once gives another
    frame for each of the KAT's downscaling inputs: a kernel that averaged
    floats would fail the KAT."""
    for layout in ("chw", "hwc"):
        for size, crop, (dw, dh), lead, seed in ref.kat_jobs(dtype, layout):
            cw, ch = ref.region(size, crop)[2:]
            case = ref.kat_case(dtype, layout, size, lead, seed)
            args = (case["buf"], lead, dtype, case["strides"], case["mul"], case["add"], size, crop, dw, dh)
            if (cw, ch) == (dw, dh):  # a copy averages nothing
                continue
            want, other = ref.expected(*args), ref.averaged_first(*args)
            assert (want != other).any(), f"{case['name']} {crop} -> {dw}x{dh}: the orders agree"
