"""Tensor frames without a GPU (tensor.hip's host side, tensor_pixel.h).

cairo_tensor_host -- the per-sample code the kernels compile, as host loops --
against the exact-rational restatement tests/tensor_ref.py, byte for byte in
both directions; the round trip through each float dtype; cairo_tensor_check
against its restatement over a grid of descriptors; the bytes an unpack must
leave alone; and the same code as a stand-alone program under AddressSanitizer
and UBSan on exact-size heap buffers.
"""
import itertools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import tensor_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (ref.U8, ref.F16, ref.BF16, ref.F32)
LAYOUTS = ("chw", "hwc", "rgba", "chw_padded")
_dt = lambda d: ref.NAMES[d]  # noqa: E731


def _desc(cairo, case, ptr=None):
    d = cairo.tensor_desc((case["buf"].ctypes.data + case["lead"] if ptr is None else ptr, case["dtype"],
                           case["strides"]), mul=case["mul"], add=case["add"])
    return d


def _run_host(cairo, case):
    """cairo_tensor_host on copies of the case's buffers -> (buf, rgb)."""
    c = dict(case, buf=case["buf"].copy())
    rgb = case["rgb"].copy().reshape(-1)
    cairo.tensor_host(case["dir"], _desc(cairo, c), case["w"], case["h"], rgb)
    return c["buf"], rgb.reshape(case["h"], case["w"], 3)


def _check(cairo, case):
    got_buf, got_rgb = _run_host(cairo, case)
    want_buf, want_rgb = case["want"]
    np.testing.assert_array_equal(got_rgb, want_rgb, err_msg=f"{case['name']}: RGB24 frame")
    # the whole buffer: the covered elements and every byte no element covers
    np.testing.assert_array_equal(got_buf, want_buf, err_msg=f"{case['name']}: tensor bytes")


def _grid_cases():
    """Every dtype, layout, size and direction, seeded values with the specials."""
    for n, (d, lay, (w, h), direction) in enumerate(itertools.product(DTYPES, LAYOUTS, ref.SIZES, (0, 1))):
        yield ref.make_case(direction, d, lay, w, h, 1000 + n, lead=16, tail=32)


def _tie_bits(dtype, w, h):
    """k + 0.5 for k = -1 .. w - 2 in every row and channel (w <= 257)."""
    v = (np.arange(w, dtype=np.float32) - 0.5)
    if dtype == ref.F32:
        b = v.view(np.uint32)
    elif dtype == ref.F16:
        b = v.astype(np.float16).view(np.uint16).astype(np.uint32)
    else:
        b = v.view(np.uint32) >> 16
    assert dtype != ref.BF16 or w <= 130  # 8 significand bits hold k + 0.5 up to 127.5 (128.5 is cut to 128)
    return np.broadcast_to(b.astype(np.uint32)[None, :, None], (h, w, 3)).copy()


def _special_cases():
    # exact ties: mul = 1, add = 0, inputs k + 0.5 for every k
    for d, w in ((ref.F32, 258), (ref.F16, 258), (ref.BF16, 130)):
        yield ref.make_case(0, d, "chw", w, 2, 1, mul=(1, 1, 1), add=(0, 0, 0), bits=_tie_bits(d, w, 2))
    # every binary16 subnormal, scaled up to the sample range and to its half
    sub = np.arange(1024, dtype=np.uint32).reshape(2, 512, 1).repeat(3, axis=2)
    yield ref.make_case(0, ref.F16, "hwc", 512, 2, 2, mul=(2.0 ** 24, 2.0 ** 22, 2.0 ** 21), add=(0, 0, 0.5), bits=sub)
    # outputs that overflow binary16 (255 * 300 > 65504), land in its subnormals, or overflow float32
    yield ref.make_case(1, ref.F16, "chw", 16, 16, 3, mul=(300.0, 2.0 ** -24, -300.0), add=(0, 0, 0))
    yield ref.make_case(1, ref.F16, "hwc", 18, 10, 4, mul=(2.0 ** -26, 3e-8, 1e-7), add=(0, 1e-8, -6e-6))
    yield ref.make_case(1, ref.F32, "chw", 16, 16, 5, mul=(3e38, 1e-40, -3e38), add=(0, 0, -1e38))
    yield ref.make_case(1, ref.BF16, "chw", 16, 16, 6, mul=(3e38, 1e-40, 1.00390625), add=(3e38, 0, 0))
    # a zero product and a negative zero
    yield ref.make_case(1, ref.F32, "hwc", 16, 16, 7, mul=(-1.0, 0.0, -0.0), add=(0.0, -0.0, -0.0))


@pytest.fixture(scope="module")
def cases():
    """Every case with the reference's result, computed once and left unchanged."""
    out = list(_grid_cases()) + list(_special_cases())
    for c in out:
        c["want"] = ref.expected(c)
    return out


def test_host_matches_the_reference(cairo, cases):
    for case in cases:
        _check(cairo, case)


def test_ties_round_to_even(cairo):
    case = ref.make_case(0, ref.F32, "chw", 258, 2, 1, mul=(1, 1, 1), add=(0, 0, 0), bits=_tie_bits(ref.F32, 258, 2))
    _, rgb = _run_host(cairo, case)
    row = rgb[0, :, 0].astype(int)
    # column j holds j - 0.5: -0.5 -> 0, 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, ... 255.5 -> 255, 256.5 -> 255
    assert list(row[:6]) == [0, 0, 2, 2, 4, 4]
    want = [min(max(2 * ((j + 0) // 2), 0), 255) for j in range(258)]
    assert list(row) == want


@pytest.mark.parametrize("dtype", (ref.F16, ref.BF16, ref.F32), ids=_dt)
@pytest.mark.parametrize("vr", ((0.0, 1.0), (-1.0, 1.0)), ids=("0..1", "-1..1"))
def test_round_trip(cairo, dtype, vr):
    """pack(unpack(s)) == s for all 256 samples under value_range's maps."""
    w, h = 256, 2
    s = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (h, w, 3)).copy()
    buf = np.zeros(3 * w * h * ref.SIZE[dtype], np.uint8)
    t = (buf.ctypes.data, dtype, (w * h, w, 1))
    out_d = cairo.tensor_desc(t, value_range=vr, output=True)
    in_d = cairo.tensor_desc(t, value_range=vr)
    mo, ao = ref.range_map(*vr, output=True)
    mi, ai = ref.range_map(*vr, output=False)
    assert tuple(out_d.c.mul) == (mo,) * 3 and tuple(out_d.c.add) == (ao,) * 3
    assert tuple(in_d.c.mul) == (mi,) * 3 and tuple(in_d.c.add) == (ai,) * 3
    cairo.tensor_host(1, out_d, w, h, s.reshape(-1))
    back = np.zeros(3 * w * h, np.uint8)
    cairo.tensor_host(0, in_d, w, h, back)
    np.testing.assert_array_equal(back.reshape(h, w, 3), s)


def test_untouched_bytes(cairo):
    """After a host unpack, the stride gaps, the alpha channel and the bytes
    before and behind the span keep their values."""
    for d in DTYPES:
        for lay in ("rgba", "chw_padded"):
            case = ref.make_case(1, d, lay, 18, 10, 7, lead=16, tail=64)
            buf, _ = _run_host(cairo, case)
            covered = np.zeros(buf.size, bool)
            off = ref.offsets(d, case["strides"], 18, 10) + case["lead"]
            for k in range(ref.SIZE[d]):
                covered[off + k] = True
            assert covered.sum() == 3 * 18 * 10 * ref.SIZE[d] and not covered[:16].any() and not covered[-64:].any()
            assert (buf[~covered] == ref.FILL).all(), f"{case['name']}: a byte outside the elements was written"


# ---------------------------------------------------------------------------
# cairo_tensor_check
# ---------------------------------------------------------------------------

def _check_both(cairo, dtype, strides, w, h, mul=(1, 1, 1), add=(0, 0, 0), reserved=(0, 0, 0), base=4096):
    d = cairo.tensor_desc((base, dtype, strides), mul=mul, add=add)
    d.c.reserved0, d.c.reserved[0], d.c.reserved[1] = reserved
    got = cairo.tensor_check(d, w, h)
    want = ref.check(dtype, strides, mul, add, reserved, base, w, h)
    assert got == want, f"dtype {dtype} strides {strides} {w}x{h} mul {mul} add {add} reserved {reserved} base {base}"
    return got


def test_check_grid(cairo):
    w, h = 18, 10
    ok = bad = 0
    # every order of (channel, row, column) strides, each bound met and missed by one
    # (perm lists the dimensions from the innermost out; a stride is its bound -- 1, then the
    # previous stride times its extent -- plus delta)
    ext = (3, h, w)
    for perm in itertools.permutations(range(3)):
        for deltas in itertools.product((-1, 0, 3), repeat=3):
            strides, bound = [0, 0, 0], 1
            for k, dim in enumerate(perm):
                strides[dim] = bound + deltas[k]
                bound = max(strides[dim], 1) * ext[dim]
            for d in DTYPES:
                r = _check_both(cairo, d, tuple(strides), w, h)
                assert (r is not None) == (min(deltas) >= 0), (perm, deltas)
                ok, bad = ok + (r is not None), bad + (r is None)
    assert (ok, bad) == (6 * 8 * 4, 6 * 19 * 4)
    for lay, (strides, _, elems) in ref.layouts(w, h).items():
        for d in DTYPES:
            span = _check_both(cairo, d, strides, w, h)
            assert span is not None and span <= elems * ref.SIZE[d], lay
    assert _check_both(cairo, ref.F16, (1, 4 * w, 4), w, h) == (1 + 2 + 9 * 72 + 17 * 4) * 2
    # a frame of an NCHW batch, a channels_last frame, a crop of a wider frame
    assert _check_both(cairo, ref.F32, (w * h, w, 1), w, h) == 3 * w * h * 4
    assert _check_both(cairo, ref.F32, (1, 3 * 40, 3), w, h) is not None
    # zero and negative strides
    for strides in ((0, w, 1), (w * h, 0, 1), (w * h, w, 0), (-w * h, w, 1), (w * h, -w, 1), (w * h, w, -1),
                    (-1, -3 * w, -3)):
        assert _check_both(cairo, ref.U8, strides, w, h) is None
    # overlapping: two channels on one address, rows shorter than their pixels
    assert _check_both(cairo, ref.U8, (1, 3 * w, 2), w, h) is None
    assert _check_both(cairo, ref.U8, (1, 3 * w - 1, 3), w, h) is None
    assert _check_both(cairo, ref.U8, (w * h - 1, w, 1), w, h) is None
    # dtype, reserved words, mul and add, alignment, height, span
    for d in (4, 5, 255, 2 ** 31):
        assert _check_both(cairo, d, (w * h, w, 1), w, h) is None
    for res in ((1, 0, 0), (0, 1, 0), (0, 0, 7)):
        assert _check_both(cairo, ref.F16, (w * h, w, 1), w, h, reserved=res) is None
    for bad_v in (np.nan, np.inf, -np.inf):
        for k in range(3):
            v = [1.0, 1.0, 1.0]
            v[k] = bad_v
            assert _check_both(cairo, ref.F32, (w * h, w, 1), w, h, mul=tuple(v)) is None
            assert _check_both(cairo, ref.F32, (w * h, w, 1), w, h, add=tuple(v)) is None
    for d, base, good in ((ref.U8, 4097, True), (ref.F16, 4097, False), (ref.F16, 4098, True), (ref.BF16, 4099, False),
                          (ref.F32, 4098, False), (ref.F32, 4100, True)):
        assert (_check_both(cairo, d, (w * h, w, 1), w, h, base=base) is not None) == good
    assert _check_both(cairo, ref.U8, (w * 65535, w, 1), w, 65535) is not None
    assert _check_both(cairo, ref.U8, (w * 65536, w, 1), w, 65536) is None
    assert _check_both(cairo, ref.U8, (w * h, w, 1), w, 0) is None
    big = 2 ** 39
    assert _check_both(cairo, ref.U8, (big, w, 1), w, h) is None           # 1 + 2 * 2^39 > 2^40
    assert _check_both(cairo, ref.U8, (big - w * h, w, 1), w, h) is not None
    assert _check_both(cairo, ref.F32, (2 ** 62, 2 ** 60, 1), w, h) is None  # no wrap-around
    assert cairo.lib().cairo_tensor_size() == 64


def test_tensor_desc_shapes(cairo):
    a = np.zeros((4, 3, 10, 18), np.float32)
    d = cairo.tensor_desc(a[2])
    assert (d.c.dtype, tuple(d.c.stride), d.width, d.height) == (cairo.DT_F32, (180, 18, 1), 18, 10)
    assert d.ptr == a[2].ctypes.data
    rgba = np.zeros((10, 18, 4), np.uint8)
    d = cairo.tensor_desc(rgba)
    assert (d.c.dtype, tuple(d.c.stride), d.width, d.height) == (cairo.DT_U8, (1, 72, 4), 18, 10)
    crop = np.zeros((3, 20, 40), np.float16)[:, 4:14, 6:24]
    d = cairo.tensor_desc(crop, value_range=(-1.0, 1.0))
    assert (d.c.dtype, tuple(d.c.stride), d.width, d.height) == (cairo.DT_F16, (800, 40, 1), 18, 10)
    assert tuple(d.c.mul) == (127.5,) * 3 and tuple(d.c.add) == (127.5,) * 3
    d = cairo.tensor_desc((64, "torch.bfloat16", (1, 54, 3)), mul=2.0, add=(0, 1, 2))
    assert (d.c.dtype, tuple(d.c.mul), tuple(d.c.add)) == (cairo.DT_BF16, (2.0,) * 3, (0.0, 1.0, 2.0))
    with pytest.raises(ValueError):
        cairo.tensor_desc(np.zeros((10, 18, 3), np.int16))
    with pytest.raises(ValueError):
        cairo.tensor_desc(np.zeros((10, 18), np.uint8))


# ---------------------------------------------------------------------------
# The per-sample header as a stand-alone program under ASan and UBSan
# ---------------------------------------------------------------------------

# The runtimes are linked into the program, so nothing is preloaded.
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
       "-fno-omit-frame-pointer", "-g", "-O1"]


def test_host_loops_sanitized(tmp_path, cases):
    """Every case above on heap buffers of exactly the span and exactly
    3 * w * h bytes: no access outside them, no undefined behaviour, and the
    reference's bytes."""
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build tensor_host_main")
    exe = str(tmp_path / "tensor_host_main")
    subprocess.run(["g++", "-std=c++17", *SAN, "-o", exe, os.path.join(ROOT, "tests/sanitize/tensor_host_main.cpp")],
                   check=True, capture_output=True, text=True)
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<I", len(cases)))
        for c in cases:
            tensor = c["buf"][c["lead"]:c["lead"] + c["span"]]
            f.write(struct.pack("<iIII3q3f3fQ", c["dir"], c["dtype"], c["w"], c["h"], *c["strides"],
                                *(float(x) for x in c["mul"]), *(float(x) for x in c["add"]), tensor.size))
            f.write(tensor.tobytes())
            f.write(c["rgb"].tobytes())
    run = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-4000:]
    assert run.stdout.split() == ["cases", str(len(cases))]
    got = np.fromfile(dst, np.uint8)
    pos = 0
    for c in cases:
        want_buf, want_rgb = c["want"]
        want_t = want_buf[c["lead"]:c["lead"] + c["span"]]
        np.testing.assert_array_equal(got[pos:pos + want_t.size], want_t, err_msg=f"{c['name']}: tensor bytes")
        pos += want_t.size
        np.testing.assert_array_equal(got[pos:pos + want_rgb.size], want_rgb.reshape(-1), err_msg=f"{c['name']}: RGB24")
        pos += want_rgb.size
    assert pos == got.size
