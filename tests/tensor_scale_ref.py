"""Restatement of the scaled tensor submit's rule (include/cairo_amd.h, the
scaled tensor submit) for the tests, composed of the two
restatements it is defined by:

    frame = scale(pack(tensor))

tests/tensor_ref.py maps every element of the crop to its 8-bit sample on
exact rationals, tests/scale_ref.py averages each channel's samples in exact
integers.  Nothing else is computed here.
"""
from __future__ import annotations

import numpy as np

from tests import scale_ref as sr
from tests import tensor_ref as tr


def region(src_size, crop):
    sw, sh = src_size
    return tuple(crop) if crop else (0, 0, sw, sh)


def packed_crop(buf: np.ndarray, base: int, dtype: int, strides, mul, add, src_size, crop) -> np.ndarray:
    """pack() of the crop's elements, (ch, cw, 3) uint8.  base: byte of element
    (0, 0, 0) of the whole source tensor in the uint8 buffer."""
    cx, cy, cw, ch = region(src_size, crop)
    at = base + (cy * strides[1] + cx * strides[2]) * tr.SIZE[dtype]
    return tr.pack(dtype, tr.gather(buf, at, dtype, strides, cw, ch), mul, add)


def scale_rgb(rgb: np.ndarray, dw: int, dh: int) -> np.ndarray:
    """scale_ref.scale_plane per channel of an (h, w, 3) image -> (dh, dw, 3)."""
    return np.stack([sr.scale_plane(rgb[..., c], dw, dh) for c in range(3)], axis=-1)


def expected(buf, base, dtype, strides, mul, add, src_size, crop, dw: int, dh: int) -> np.ndarray:
    """The frame a scaled tensor submit encodes, (dh, dw, 3) uint8."""
    return scale_rgb(packed_crop(buf, base, dtype, strides, mul, add, src_size, crop), dw, dh)


def valid(dtype, strides, mul, add, reserved, base: int, src_size, crop, dw: int, dh: int) -> bool:
    """cairo_tensor_scale_check restated: cairo_tensor_check on the source size
    and every rule of cairo_scale_check for (RGB24, pitch 0)."""
    sw, sh = src_size
    return tr.check(dtype, strides, mul, add, reserved, base, sw, sh) is not None and \
        sr.valid(sr.RGB24, 0, (sw, sh), crop, dw, dh)


def _elem_f64(dtype: int, bits: np.ndarray) -> np.ndarray:
    if dtype == tr.U8:
        return bits.astype(np.float64)
    if dtype == tr.F16:
        return bits.astype(np.uint16).view(np.float16).astype(np.float64)
    if dtype == tr.BF16:
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
    return bits.astype(np.uint32).view(np.float32).astype(np.float64)


def averaged_first(buf, base, dtype, strides, mul, add, src_size, crop, dw: int, dh: int) -> np.ndarray:
    """The OTHER order, which the rule rejects: the mapped values x * mul + add
    are area-averaged as floats and the average is rounded and clamped once.
    Only used to show that the KAT's inputs tell the two orders apart."""
    cx, cy, cw, ch = region(src_size, crop)
    at = base + (cy * strides[1] + cx * strides[2]) * tr.SIZE[dtype]
    x = _elem_f64(dtype, tr.gather(buf, at, dtype, strides, cw, ch))
    wx, wy = sr.weights(cw, dw).astype(np.float64), sr.weights(ch, dh).astype(np.float64)
    n = float(sr.axis(cw, dw)[0] * sr.axis(ch, dh)[0])
    out = np.empty((dh, dw, 3), np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(3):
            t = x[..., c] * float(mul[c]) + float(add[c])
            avg = (wy @ t @ wx.T) / n
            r = np.clip(np.rint(avg), 0.0, 255.0)
            out[..., c] = np.where(np.isnan(r), 0.0, r).astype(np.uint8)
    return out


# The KAT's cases (tests/test_gpu_tensor_scale.py).  Whole sources: scale_ref's
# sizes; the 3840-wide one is run for two configurations only.
KAT_SIZES = sr.KAT_SIZES[:6]
KAT_WIDE = sr.KAT_SIZES[6]
KAT_WIDE_CONFIGS = ((tr.U8, "chw"), (tr.F16, "hwc"))
# Crops (source size, crop, output size): origins that are no multiple of 4
# pixels, so that a strip's first column group starts mid-access.
KAT_CROPS = (
    ((160, 80), (6, 4, 140, 68), (70, 34)),    # 2:1
    ((150, 76), (2, 6, 140, 68), (70, 34)),    # 2:1, flush with the right edge
    ((104, 80), (6, 2, 96, 72), (64, 48)),     # 3:2
)
GUARD = 64


def kat_leads(dtype: int):
    """Bytes in front of element (0, 0, 0) in a 16-byte aligned buffer: with 0
    the wide loads run, with one element they cannot (but for uint8 columns
    that start a dword), with 16 + one element the same a line further."""
    es = tr.SIZE[dtype]
    return (0, es, 16 + es)


def kat_case(dtype: int, layout: str, src_size, lead: int, seed: int):
    """A source tensor of src_size for the KAT: tensor_ref.make_case's buffer
    (specials in the first and last strips, MAP_IN's per-channel map, FILL
    elsewhere) with GUARD bytes behind the span."""
    return tr.make_case(0, dtype, layout, src_size[0], src_size[1], seed, lead=lead, tail=GUARD)


def kat_jobs(dtype: int, layout: str):
    """The KAT's runs of one dtype and layout: (source size, crop, output size,
    lead, seed).  The leads take turns over the sizes and crops; the 2:1 size
    and the first crop are run with all three."""
    leads = kat_leads(dtype)
    runs = [(s, None, d) for s, d in KAT_SIZES] + list(KAT_CROPS)
    if (dtype, layout) in KAT_WIDE_CONFIGS:
        runs.append((KAT_WIDE[0], None, KAT_WIDE[1]))
    jobs = [(s, crop, d, leads[i % 3], 900 + 16 * i + dtype) for i, (s, crop, d) in enumerate(runs)]
    for i in (1, 6):
        s, crop, d = runs[i]
        jobs += [(s, crop, d, lead, 900 + 16 * i + dtype) for lead in leads if lead != leads[i % 3]]
    return jobs


def case_expected(case, crop, dw: int, dh: int) -> np.ndarray:
    return expected(case["buf"], case["lead"], case["dtype"], case["strides"], case["mul"], case["add"],
                    (case["w"], case["h"]), crop, dw, dh)


def tensor_of(rgb: np.ndarray, dtype: int, layout: str, vr, lead: int = 0):
    """A tensor frame made from an RGB image, as a tensor_ref.make_case dict
    for direction 0: uint8 holds the image; the float dtypes hold its values
    spread over value_range vr with a small position-dependent offset, so that
    the rounding decides samples."""
    h, w = rgb.shape[:2]
    if dtype == tr.U8:
        bits = rgb.astype(np.uint32)
        mul, add = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    else:
        y, x = np.mgrid[0:h, 0:w]
        jit = np.array([-0.45, -0.2, 0.3, 0.49], np.float32)[(x + 2 * y) % 4][..., None]
        m, a = tr.range_map(*vr, output=True)
        f = ((rgb.astype(np.float32) + jit) * m + a).astype(np.float32)
        if dtype == tr.F32:
            bits = f.view(np.uint32)
        elif dtype == tr.BF16:
            bits = f.view(np.uint32) >> 16
        else:
            bits = f.astype(np.float16).view(np.uint16).astype(np.uint32)
        mi, ai = tr.range_map(*vr, output=False)
        mul, add = (mi,) * 3, (ai,) * 3
    return tr.make_case(0, dtype, layout, w, h, 0, mul=mul, add=add, lead=lead, bits=np.ascontiguousarray(bits))
