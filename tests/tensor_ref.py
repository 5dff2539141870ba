"""Exact restatement of the tensor frame map (include/cairo_amd.h, cairo_tensor;
DESIGN.md §4.15) for the tests.

Every floating-point step is done on exact rationals and rounded once, by
comparing the exact value with its two neighbours in the target format and
breaking ties to even; nothing passes through float64 arithmetic (a double
rounding).  The strided gather and scatter are plain numpy on byte buffers.
"""
from fractions import Fraction
import math

import numpy as np

U8, F16, BF16, F32 = range(4)
NAMES = {U8: "u8", F16: "f16", BF16: "bf16", F32: "f32"}
SIZE = {U8: 1, F16: 2, BF16: 2, F32: 4}
NP_BITS = {U8: np.uint8, F16: np.uint16, BF16: np.uint16, F32: np.uint32}
INF = "inf"

# (significand bits with the hidden one, exponent of the smallest normal, exponent at which a value overflows)
_FORMATS = {F16: (11, -14, 16), BF16: (8, -126, 128), F32: (24, -126, 128)}


def round_to(v: Fraction, fmt: int):
    """|v| rounded to nearest even in the format -> a Fraction, or INF."""
    a = abs(v)
    if a == 0:
        return Fraction(0)
    p, emin, eover = _FORMATS[fmt]
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    quantum = Fraction(2) ** (max(e, emin) - (p - 1))
    q = a / quantum
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    r = n * quantum
    return INF if r >= Fraction(2) ** eover else r


def elem_value(dtype: int, bits: int):
    """Element bits -> ('nan' | 'inf' | 'num', negative, Fraction)."""
    if dtype == U8:
        return "num", False, Fraction(bits)
    if dtype == F16:
        f = float(np.array([bits], np.uint16).view(np.float16)[0])
    elif dtype == BF16:
        f = float(np.array([bits << 16], np.uint32).view(np.float32)[0])
    else:
        f = float(np.array([bits], np.uint32).view(np.float32)[0])
    if math.isnan(f):
        return "nan", False, None
    neg = math.copysign(1.0, f) < 0
    if math.isinf(f):
        return "inf", neg, None
    return "num", neg, Fraction(f)  # a float64 holds every value of the three formats exactly


def _f32_parts(x):
    f = float(np.float32(x))
    assert math.isfinite(f)
    return math.copysign(1.0, f) < 0, Fraction(f)


def fma32(kind, neg, val, mul, add):
    """fmaf(x, mul, add) for finite float32 mul and add -> ('nan' | 'inf' |
    'num', negative, Fraction): the exact x * mul + add rounded once."""
    mneg, m = _f32_parts(mul)
    aneg, a = _f32_parts(add)
    if kind == "nan":
        return "nan", False, None
    if kind == "inf":
        if m == 0:
            return "nan", False, None  # inf * 0
        return "inf", neg != mneg, None
    exact = val * m + a
    if exact == 0:
        # an exact zero sum is +0 under round to nearest, unless both terms are -0
        prod_zero = val * m == 0
        return "num", (prod_zero and a == 0 and (neg != mneg) and aneg), Fraction(0)
    r = round_to(exact, F32)
    if r == INF:
        return "inf", exact < 0, None
    return "num", exact < 0, r if exact > 0 else -r


def sat8(kind, neg, val) -> int:
    """isnan(t) ? 0 : (int)min(max(rintf(t), 0), 255), rintf to nearest even."""
    if kind == "nan":
        return 0
    if kind == "inf":
        return 0 if neg else 255
    n = val.numerator // val.denominator  # floor
    rem = val - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (n & 1)):
        n += 1
    return min(max(n, 0), 255)


def store_bits(dtype: int, kind, neg, val) -> int:
    """A float32 t (never NaN on this path) -> element bits of the dtype."""
    if dtype == U8:
        return sat8(kind, neg, val)
    assert kind != "nan"
    if dtype == F32:
        f = (-math.inf if neg else math.inf) if kind == "inf" else float(val)
        if kind == "num" and val == 0 and neg:
            f = -0.0
        return int(np.array([f], np.float32).view(np.uint32)[0])
    sign = 0x8000 if neg else 0
    r = INF if kind == "inf" else round_to(val, dtype)
    if r == INF:
        return sign | (0x7C00 if dtype == F16 else 0x7F80)
    if dtype == F16:
        return sign | int(np.array([float(r)], np.float16).view(np.uint16)[0])  # exact: r is a binary16 value
    return sign | int(np.array([float(r)], np.float32).view(np.uint32)[0] >> 16)


def pack(dtype: int, bits: np.ndarray, mul, add) -> np.ndarray:
    """dir 0: element bits (h, w, 3) -> samples (h, w, 3) uint8."""
    out = np.empty(bits.shape, np.uint8)
    for c in range(3):
        uniq, inv = np.unique(bits[..., c], return_inverse=True)
        lut = np.array([sat8(*fma32(*elem_value(dtype, int(b)), mul[c], add[c])) for b in uniq], np.uint8)
        out[..., c] = lut[inv.reshape(bits.shape[:2])]
    return out


def unpack(dtype: int, rgb: np.ndarray, mul, add) -> np.ndarray:
    """dir 1: samples (h, w, 3) uint8 -> element bits (h, w, 3) uint32."""
    out = np.empty(rgb.shape, np.uint32)
    for c in range(3):
        lut = np.array([store_bits(dtype, *fma32("num", False, Fraction(s), mul[c], add[c])) for s in range(256)],
                       np.uint32)
        out[..., c] = lut[rgb[..., c]]
    return out


def offsets(dtype: int, strides, w: int, h: int) -> np.ndarray:
    """Byte offset of element (c, y, x) from element (0, 0, 0), shape (h, w, 3)."""
    y, x, c = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), np.arange(3, dtype=np.int64),
                          indexing="ij")
    return (c * strides[0] + y * strides[1] + x * strides[2]) * SIZE[dtype]


def gather(buf: np.ndarray, base: int, dtype: int, strides, w: int, h: int) -> np.ndarray:
    """The element bits (h, w, 3) uint32 of a tensor whose element (0, 0, 0) is
    at byte `base` of the uint8 buffer (little endian)."""
    off = offsets(dtype, strides, w, h) + base
    bits = np.zeros(off.shape, np.uint32)
    for k in range(SIZE[dtype]):
        bits |= buf[off + k].astype(np.uint32) << np.uint32(8 * k)
    return bits


def scatter(buf: np.ndarray, base: int, dtype: int, strides, w: int, h: int, bits: np.ndarray) -> None:
    """Write element bits into the buffer; every other byte keeps its value."""
    off = offsets(dtype, strides, w, h) + base
    for k in range(SIZE[dtype]):
        buf[off + k] = ((bits >> np.uint32(8 * k)) & np.uint32(255)).astype(np.uint8)


def check(dtype, strides, mul, add, reserved, base: int, w: int, h: int):
    """cairo_tensor_check restated -> the span in bytes, or None.  reserved:
    (reserved0, reserved[0], reserved[1])."""
    if w < 1 or h < 1 or h > 65535:
        return None
    if dtype not in SIZE or any(reserved):
        return None
    if not all(math.isfinite(float(v)) for v in list(mul) + list(add)):
        return None
    if base % SIZE[dtype]:
        return None
    pairs = sorted(zip(strides, (3, h, w)))  # ascending by stride, ties by extent
    if pairs[0][0] < 1:
        return None
    for (s1, e1), (s2, _) in zip(pairs, pairs[1:]):
        if s2 < s1 * e1:
            return None
    span = 1 + sum((e - 1) * s for s, e in pairs)
    if span > 2 ** 40:
        return None
    return span * SIZE[dtype]


def range_map(lo: float, hi: float, output: bool):
    """value_range -> (mul, add) as float32, computed in double, rounded once."""
    if output:
        mul, add = (hi - lo) / 255.0, lo
    else:
        mul = 255.0 / (hi - lo)
        add = -lo * mul
    return np.float32(mul), np.float32(add)


# Layouts of a w x h frame: name -> (strides (channel, row, column) in elements,
# elements from the buffer's start to element (0, 0, 0), elements of the buffer).
def layouts(w: int, h: int):
    return {
        "chw": ((w * h, w, 1), 0, 3 * w * h),
        "hwc": ((1, 3 * w, 3), 0, 3 * w * h),
        "chw_padded": ((h * (w + 5) + 7, w + 5, 1), 0, 3 * (h * (w + 5) + 7)),
        "rgba": ((1, 4 * w, 4), 0, 4 * w * h),
    }


SIZES = ((16, 16), (18, 10), (64, 48))  # the host tests' frame sizes
# Maps with a different factor and offset per channel.
MAP_IN = {False: ((255.0, 254.5, 127.5), (0.0, 0.25, 127.5)), True: ((1.0, 0.5, 2.0), (0.0, 0.25, -100.0))}
MAP_OUT = {False: ((1.0 / 255.0, 2.0 / 255.0, 0.5), (0.0, -1.0, 0.125)), True: ((1.0, 0.5, 2.0), (0.0, 0.5, -100.0))}
FILL = 0xA5


def f32s(v):
    return tuple(np.float32(x) for x in v)


def make_case(direction: int, dtype: int, layout: str, w: int, h: int, seed: int, mul=None, add=None, lead: int = 0,
              tail: int = 0, bits=None):
    """One case of the map on host buffers: a uint8 buffer `buf` of lead + span
    + tail bytes whose element (0, 0, 0) is at byte `lead`, FILL everywhere
    but, for direction 0, the covered elements (tensor_ref.values, or `bits`
    (h, w, 3)); and `rgb` (h, w, 3), seeded noise for direction 1."""
    rng = np.random.default_rng(seed)
    strides, _, _ = layouts(w, h)[layout]
    m, a = (MAP_OUT if direction else MAP_IN)[dtype == U8]
    mul, add = f32s(m if mul is None else mul), f32s(a if add is None else add)
    span = check(dtype, strides, mul, add, (0, 0, 0), 0, w, h)
    assert span is not None
    buf = np.full(lead + span + tail, FILL, np.uint8)
    if direction == 0:
        if bits is None:
            bits = values(dtype, 3 * w * h, rng).reshape(3, h, w).transpose(1, 2, 0)
        scatter(buf, lead, dtype, strides, w, h, np.ascontiguousarray(bits))
        rgb = np.full((h, w, 3), FILL, np.uint8)
    else:
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        rgb[0, 0], rgb[-1, -1] = (0, 255, 128), (255, 0, 1)
    return dict(dir=direction, dtype=dtype, layout=layout, w=w, h=h, strides=strides, mul=mul, add=add, buf=buf,
                lead=lead, span=span, rgb=rgb, name=f"dir{direction} {NAMES[dtype]} {layout} {w}x{h}")


def expected(case):
    """-> (buf, rgb) after the map ran on the case."""
    buf, rgb = case["buf"].copy(), case["rgb"].copy()
    d, st, w, h = case["dtype"], case["strides"], case["w"], case["h"]
    if case["dir"] == 0:
        rgb = pack(d, gather(buf, case["lead"], d, st, w, h), case["mul"], case["add"])
    else:
        scatter(buf, case["lead"], d, st, w, h, unpack(d, rgb, case["mul"], case["add"]))
    return buf, rgb


SPECIAL_F32 = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e30, -1e30, 3.4e38, -3.4e38, 1e-40, 254.5, 255.5, 0.5, 1.5, 2.5,
               -0.5, 65504.0, 6e-8, 5.96e-8, 3e-8]


def values(dtype: int, n: int, rng, lo=-0.25, hi=1.25) -> np.ndarray:
    """n seeded element bit patterns: mostly values in [lo, hi], then the
    specials (NaN, +-inf, -0.0, far out of range, f16 subnormals) at the front
    and the back -- the first and the last strip of a row."""
    if dtype == U8:
        return rng.integers(0, 256, n, dtype=np.uint32)
    # (drawn from 509 seeded values, so that the exact reference maps each once)
    f = rng.uniform(lo, hi, 509).astype(np.float32)[rng.integers(0, 509, n)]
    sp = np.array(SPECIAL_F32, np.float32)
    k = min(len(sp), n // 2)
    f[:k] = sp[:k]
    f[n - k:] = sp[:k][::-1]
    if dtype == F32:
        return f.view(np.uint32).copy()
    if dtype == BF16:
        return (f.view(np.uint32) >> 16).astype(np.uint32)
    with np.errstate(over="ignore"):
        b = f.astype(np.float16).view(np.uint16).astype(np.uint32)
    b[k:k + 4] = [0x0001, 0x03FF, 0x8001, 0x0200]  # binary16 subnormals
    return b
