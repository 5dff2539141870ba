"""Crafted macroblocks for the encode side of the transform chain
(cairo_kat_transform: fdct_lane, vaq_mb, quant_elem, dequant_elem, idct_lane).

A pure, seeded numpy generator in the manner of tests/tables.py.  cases()
returns a list of (src, pred, type, quality, class_name): src and pred are
(6, 8, 8) int16 (Y TL, TR, BL, BR, U, V), type is 0..3, quality 1..31.  The
classes (the part of class_name before the slash is the group the GPU test is
parametrized by):

  ladder/...    every (type, quality, idx) with idx = the VAQ's variance class
                log2(variance2) >> 1 in 1..15: noise of amplitude 1..4096 on the
                residual (idx 3..15), one to three single-sample perturbations
                of an otherwise zero residual (idx 1 and 2), a zero residual
  vaq/...       count 0 and 1, a sum whose square wraps int32, a sum of
                squares beyond 2^32, a negative variance2, variance2 within
                +-1 of 4^k (POW4: found by search_pow4, a search of seeds)
  narrow/...    all-equal 32767 and -32768, +-32767 checkerboards, residuals
                that wrap int16, row-pass and column-pass values beyond int16
  single/...    one non-zero quantized coefficient at each of the 64
                positions, luma and chroma, intra path (with its DC) and inter
  content/...   as test_kat_transform_chain draws them (src 16..271, pred
                -200..600)

The generator places its cases with a numpy restatement of the forward
transform and the VAQ (fdct, variance2, vaq_idx, vaq_qp below; the quantizer
is tests/quant_ref.py).  It proves nothing by that: tests/test_mb_cases.py
pins these restatements to the oracle and asserts every class from the
oracle's own results.

The second half names the frame-level schedule of
tests/test_gpu_mb_chain.py (a quality per frame), whose coverage the same
CPU test asserts.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import quant_ref
from tests.quant_ref import i16, rdiv, tdiv

TYPES = (0, 1, 2, 3)
QUALITIES = tuple(range(1, 32))
IDX = tuple(range(1, 16))  # log2_u32 is at most 31
SEED = 20240

# EVX_TRANSFORM_8x8_TRIG_128_LUT (xftables.h:57-67): row j = frequency, column i = sample
_J, _I = np.mgrid[0:8, 0:8]
LUT8 = np.rint(128.0 * np.cos((2 * _I + 1) * _J * np.pi / 16.0)).astype(np.int64)


# ---------------------------------------------------------------------------
# numpy restatements (wide integers; every narrowing explicit)
# ---------------------------------------------------------------------------

def _fline_wide(x):
    """transform_8x8_line_fast (transform.cpp:264-284) along the last axis,
    before its (int16_t) cast."""
    t = np.asarray(x, np.int64) @ LUT8.T
    t = np.concatenate([tdiv(t[..., :1] * 45, 128), tdiv(t[..., 1:], 2)], -1)
    return rdiv(t, 128)


def row_pass_wide(blocks):
    """The row pass of transform_8x8 on (..., 8, 8) blocks, before the cast."""
    return _fline_wide(blocks)


def col_pass_wide(blocks):
    """The column pass (on the narrowed row pass), before the final cast."""
    s = i16(row_pass_wide(blocks))
    return np.swapaxes(_fline_wide(np.swapaxes(s, -1, -2)), -1, -2)


def fdct(blocks):
    """transform_8x8 (transform.cpp:286-301) -> int64 values in int16 range."""
    return i16(col_pass_wide(blocks))


def residual(src, pred, typ):
    """What the transform sees: src for type 1, (int16)(src - pred) otherwise."""
    s = np.asarray(src, np.int64)
    return s if typ == 1 else i16(s - np.asarray(pred, np.int64))


def _wrap32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def luma_counted(coef):
    """(n, 6, 8, 8) coefficients -> (n, 255) luma coefficients the variance
    reads: all but the first of quadrant 0."""
    return np.asarray(coef, np.int64)[:, :4].reshape(-1, 256)[:, 1:]


def variance2(coef):
    """compute_block_variance2 (analysis.h:176-198) with its int32 wrap-around
    on (n, 6, 8, 8) coefficients -> (variance2 as int32, count)."""
    t = luma_counted(coef)
    count = (t != 0).sum(1)
    s = _wrap32(t.sum(1))
    sumsq = (t * t).sum(1) & 0xFFFFFFFF
    sq = _wrap32((s * s) & 0xFFFFFFFF)
    d = np.maximum(count, 1)
    r = np.where(sq < 0, tdiv(_wrap32(sq - d // 2), d), tdiv(_wrap32(sq + d // 2), d))
    return np.where(count > 0, _wrap32(sumsq - (r & 0xFFFFFFFF)), 0), count


def vaq_idx(v2):
    """The variance class of query_block_quantization_parameter (quantize.cpp:60-77)."""
    u = np.asarray(v2, np.int64) & 0xFFFFFFFF
    lg = np.zeros_like(u)
    for s in (16, 8, 4, 2, 1):
        m = (u >> s) > 0
        lg += s * m
        u = np.where(m, u >> s, u)
    return np.clip(lg >> 1, 1, 31)


def vaq_qp(quality, idx):
    q, idx = np.asarray(quality, np.int64), np.asarray(idx, np.int64)
    return np.clip(np.where(idx > q, q + ((idx - q) >> 1), q - ((q - idx) >> 1)), 1, 31)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------

def _compose(r, typ, rng):
    """(src, pred) whose residual for this type is r (any int16 values)."""
    r = np.asarray(r, np.int64)
    pred = rng.integers(-200, 600, r.shape)
    if typ == 1:
        return r.astype(np.int16), pred.astype(np.int16)
    return i16(pred + r).astype(np.int16), pred.astype(np.int16)


def _ladder_pool(rng):
    """Residuals by variance class."""
    pool = {k: [] for k in IDX}
    res = [np.zeros((1, 6, 8, 8), np.int64)]
    for a in (1, 2, 3, 4, 6, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        res.append(rng.integers(-a, a + 1, (16, 6, 8, 8)))
    n = 1500
    sparse = np.zeros((n, 384), np.int64)
    pos = rng.integers(0, 256, (n, 3))
    val = rng.integers(1, 13, (n, 3)) * rng.choice((-1, 1), (n, 3))
    cnt = rng.integers(1, 4, n)
    for j in range(3):
        rows = np.flatnonzero(cnt > j)
        sparse[rows, pos[rows, j]] = val[rows, j]
    res.append(sparse.reshape(n, 6, 8, 8))
    res = np.concatenate(res)
    idx = vaq_idx(variance2(fdct(res))[0])
    for r, k in zip(res, idx):
        if len(pool[int(k)]) < 24:
            pool[int(k)].append(r)
    missing = [k for k in IDX if not pool[k]]
    if missing:
        raise RuntimeError(f"mb_cases: no residual of variance class {missing}")
    return pool


# variance2 within +-1 of 4^k: k -> (seed, index in _pow4_batch(k, seed)), from
# search_pow4 (python -m tests.mb_cases pow4).  For k = 14 and 15 a hit is one
# draw in some 10^8: there the batch's nearest macroblock was moved onto the
# value by a few single-sample steps (flat index, delta), found by trying 8192
# random steps at a time and keeping the closest.
POW4 = {1: (10, 926), 2: (0, 712), 3: (0, 97), 4: (0, 1394), 5: (0, 55), 6: (5, 3721), 7: (0, 1031), 8: (0, 1751),
        9: (2, 3553), 10: (23, 1699), 11: (21, 3756), 12: (220, 2293), 13: (397, 3266), 14: (0, 3818), 15: (0, 3553)}
POW4_STEPS = {14: ((125, 2), (119, 3), (130, 12), (100, 3), (156, 4)), 15: ((29, 6), (21, 24))}
POW4_BATCH = 4096


def _pow4_batch(k, seed):
    rng = np.random.default_rng([SEED, 4, k, seed])
    n = POW4_BATCH
    out = np.zeros((n, 6, 8, 8), np.int64)
    if k <= 4:
        flat = out.reshape(n, 384)
        pos = rng.integers(0, 256, (n, 3))
        val = rng.integers(1, 25, (n, 3)) * rng.choice((-1, 1), (n, 3))
        for j in range(3):
            flat[np.arange(n), pos[:, j]] = val[:, j]
        return out
    a = max(1, int(round(0.108 * 2 ** k)))
    out[:, :4] = rng.integers(-a, a + 1, (n, 4, 8, 8))
    return out


def _pow4_case(k):
    seed, index = POW4[k]
    r = _pow4_batch(k, seed)[index].copy()
    for pos, d in POW4_STEPS.get(k, ()):
        r.reshape(-1)[pos] += d
    return r


def search_pow4(kmax=13, seeds=400):
    """-> {k: (seed, index)} for the k a search of `seeds` batches finds."""
    found = {}
    for k in range(1, kmax + 1):
        for seed in range(seeds):
            v, _ = variance2(fdct(_pow4_batch(k, seed)))
            hit = np.flatnonzero(np.abs(v - 4 ** k) <= 1)
            if hit.size:
                found[k] = (seed, int(hit[0]))
                break
    return found


def _single_block(pos, a):
    v, u = divmod(pos, 8)
    y, x = np.mgrid[0:8, 0:8]
    return np.rint(a * np.cos((2 * x + 1) * u * np.pi / 16) * np.cos((2 * y + 1) * v * np.pi / 16)).astype(np.int64)


SINGLE_GRID = tuple((q, a) for a in (80, 60, 100, 40, 120, 50, 70, 90, 110) for q in (8, 4, 12))
SINGLE_PATHS = (("intra", 1), ("inter", 0))
SINGLE_DC_OFFSET = 64  # on the intra path the block's DC is non-zero as well


def single_block_index(plane, pos):
    """Which of the six blocks holds the pattern."""
    return pos % 4 if plane == "luma" else 4 + pos % 2


def _quantized(res, typ, quality):
    """(n, 6, 8, 8) residuals, one type, per-macroblock quality -> quantized (n, 6, 8, 8)."""
    coef = fdct(res)
    qp = vaq_qp(quality, vaq_idx(variance2(coef)[0]))
    out = np.zeros_like(coef)
    for p in np.unique(qp):
        m = qp == p
        out[m] = quant_ref.quantize(coef[m].reshape(-1, 384), typ, int(p)).reshape(-1, 6, 8, 8)
    return out


def _singles():
    """[(path, plane, pos, type, quality, residual)]: the first (quality, A) of
    SINGLE_GRID whose quantized block holds the position alone (and the DC on
    the intra path)."""
    out = []
    for path, typ in SINGLE_PATHS:
        specs = [(plane, pos, q, a) for plane in ("luma", "chroma") for pos in range(64) for q, a in SINGLE_GRID]
        res = np.zeros((len(specs), 6, 8, 8), np.int64)
        for n, (plane, pos, q, a) in enumerate(specs):
            res[n, single_block_index(plane, pos)] = _single_block(pos, a) + (SINGLE_DC_OFFSET if typ == 1 else 0)
        quant = _quantized(res, typ, np.array([s[2] for s in specs]))
        done = set()
        for n, (plane, pos, q, a) in enumerate(specs):
            if (plane, pos) in done:
                continue
            want = np.zeros((6, 64), bool)
            want[single_block_index(plane, pos), pos] = True
            if typ == 1:
                want[single_block_index(plane, pos), 0] = True
            if np.array_equal(quant[n].reshape(6, 64) != 0, want):
                done.add((plane, pos))
                out.append((path, plane, pos, typ, q, res[n]))
        if len(done) != 128:
            raise RuntimeError(f"mb_cases: no single-coefficient pattern for {path} at some position")
    return out


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(SEED)
    out = []

    def add(name, r, typ, quality, srcpred=None):
        src, pred = srcpred if srcpred is not None else _compose(r, typ, rng)
        out.append((np.ascontiguousarray(src, dtype=np.int16), np.ascontiguousarray(pred, dtype=np.int16), int(typ),
                    int(quality), name))

    # -- variance ladder
    pool = _ladder_pool(rng)
    for t in TYPES:
        for q in QUALITIES:
            for k in IDX:
                add(f"ladder/idx{k}", pool[k][(t * 31 + q) % len(pool[k])], t, q)

    # -- VAQ edges, in every type
    const = lambda *vals: np.stack([np.full((8, 8), v, np.int64) for v in vals])  # noqa: E731
    neg = rng.integers(-16000, 16001, (64, 6, 8, 8))
    neg = neg[variance2(fdct(neg))[0] < 0]
    pow4 = {k: _pow4_case(k) for k in POW4}
    for n, t in enumerate(TYPES):
        q = (5, 12, 19, 27)[n]
        r = const(37, 0, 0, 0, 0, 0)
        r[4:] = rng.integers(-20, 21, (2, 8, 8))
        add("vaq/count0", r, t, q)
        add("vaq/count0", np.zeros((6, 8, 8), np.int64), t, q + 1)
        add("vaq/one", const(37, 0, -53, 0, 9, -9), t, q)
        add("vaq/sum_wrap", const(0, 3000, 3000, 3000, 0, 0), t, q)
        add("vaq/sum_wrap", const(-100, -4000, -4000, -2500, 0, 0), t, q + 2)
        add("vaq/sumsq_wrap", rng.integers(-16000, 16001, (6, 8, 8)), t, q)
        add("vaq/negative", neg[n], t, q)
        add("vaq/negative", neg[4 + n], t, 31 - q)
        for k in sorted(POW4):
            add(f"vaq/pow4_{k}", pow4[k], t, (q + k) % 31 + 1)

    # -- narrowing
    checker = np.where(np.indices((6, 8, 8)).sum(0) % 2 == 0, 32767, -32767)
    zero = np.zeros((6, 8, 8), np.int64)
    for n, t in enumerate(TYPES):
        q = (3, 9, 16, 31)[n]
        add("narrow/max", None, t, q, (zero + 32767, zero))
        add("narrow/min", None, t, q, (zero - 32768, zero))
        add("narrow/checker", None, t, q, (checker, zero))
        add("narrow/checker", None, t, q, (-checker, zero))
        rows = rng.integers(12000, 32768, (6, 8, 1)) * rng.choice((-1, 1), (6, 8, 1)) + zero
        add("narrow/rowpass", None, t, q, (rows, zero))
        flat = rng.integers(4200, 11000, (6, 1, 1)) * rng.choice((-1, 1), (6, 1, 1)) + zero
        add("narrow/colpass", None, t, q, (flat, zero))
        if t != 1:  # (type 1 has no residual)
            add("narrow/residual_wrap", None, t, q, (zero + 30000, zero - 30000))
            add("narrow/residual_wrap", None, t, q, (zero - 32768, zero + 1))
            add("narrow/residual_wrap", None, t, q,
                (rng.integers(-32768, 32768, (6, 8, 8)), rng.integers(-32768, 32768, (6, 8, 8))))

    # -- single coefficient
    for path, plane, pos, typ, q, r in _singles():
        add(f"single/{path}_{plane}", r, typ, q)

    # -- content range
    n = 320
    src = rng.integers(16, 272, (n, 6, 8, 8))
    pred = rng.integers(-200, 600, (n, 6, 8, 8))
    src[0], src[1], pred[2] = 16, 271, -32000
    src[3] = np.where(np.indices((6, 8, 8)).sum(0) % 2 == 0, 16, 271)
    for m in range(n):
        add("content/random", None, (1, 0, 2, 3)[m % 4], int(rng.integers(1, 32)), (src[m], pred[m]))
    return tuple(out)


GROUPS = ("content", "ladder", "narrow", "single", "vaq")  # (tests/test_mb_cases.py checks the list)


def stacked(group=None):
    """-> (src (n, 6, 8, 8), pred, types (n,), qualities (n,), names) of one group or all."""
    sel = [c for c in cases() if group is None or c[4].split("/")[0] == group]
    return (np.stack([c[0] for c in sel]), np.stack([c[1] for c in sel]), np.array([c[2] for c in sel], np.uint8),
            np.array([c[3] for c in sel], np.uint8), [c[4] for c in sel])


# ---------------------------------------------------------------------------
# The frame-level schedule: a quality per frame, as a rate-controlled context
# gives the engine.
# ---------------------------------------------------------------------------

ENGINE_SIZES = ((64, 48), (72, 40))
ENGINE_RING = 4
INTRA_QUALITIES = tuple(t + 1 for t in range(31))
IP_QUALITIES = (16,) + tuple(((7 * i) % 31) + 1 for i in range(31))
ENGINE_RUNS = (("intra", INTRA_QUALITIES), ("ip", IP_QUALITIES))


def engine_kinds():
    from tests import content

    return ("band4",) + content.KINDS


def engine_frame(orc, kind, w, h, t):
    from tests import content

    return orc.make_frame(w, h, t) if kind == "band4" else content.make(kind, w, h, t)


# The quantizer's near-exhaustive values (tests/test_gpu_mb_chain.py): every
# |c| <= 4096, +-(4096 + 61 j) out to the ends, and the two extremes.
def quant_values():
    far = 4096 + 61 * np.arange(1, (32767 - 4096) // 61 + 1)
    return np.unique(np.concatenate([np.arange(-4096, 4097), far, -far, [-32768, 32767]])).astype(np.int16)


if __name__ == "__main__":
    import sys

    if sys.argv[1:2] == ["pow4"]:
        print(search_pow4())
    else:
        from collections import Counter

        for name, n in sorted(Counter(c[4] for c in cases()).items()):
            print(f"{name:28s} {n}")
