"""Synthetic inputs of the entropy precode (cairo_amd/csrc/precode.hip, the
host's entropy.cpp): block tables and coefficient planes the encoder never
picks, each case aimed at one mechanism of the GPU scan or packer (DESIGN.md
§2.1).  Pure numpy and seeded.  The tables need not be decode-legal: they hold
anything the 16-byte descriptor can carry and the serializer reads.

cases() yields (name, wmb, hmb, ring, table, (y, u, v)).  The coefficient
planes are built from the *coded* values of each 8x8 block (zig-zag order, the
DC as the delta the stream carries), so a case states exactly which codes it
holds; coded_blocks() recovers them from the planes independently, and
tests/test_feed_tables.py checks with it and with the oracle's counts that
every class below really occurs.  No coded value is -32768 (its own cases,
rule_cases(), hold that one: DESIGN.md §4.0).

`python -m tests.feed_tables` prints the cases and their feed sizes.
"""
from __future__ import annotations

import functools

import numpy as np

# evx_block_desc (common.h:78-95, pack(2), 16 bytes)
BLOCK_DESC = np.dtype(
    [("block_type", "<u4"), ("prediction_target", "u1"), ("pad", "u1"), ("motion_x", "<i2"),
     ("motion_y", "<i2"), ("sp_pred", "u1"), ("sp_amount", "u1"), ("sp_index", "u1"),
     ("q_index", "u1"), ("variance", "<i2")]
)
INTRA, MOTION, COPY = 1, 2, 4
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
CHUNK, WAVE, TILE = 256, 64, 64   # precode.h kFeedChunk; a wavefront; k_feed_carry's chunks per tile
CAPACITY = 32 * 1024 * 1024       # bits of one feed section (common.cpp:147)
FULL_BLOCK = 13 + 64 * 31         # ue(64) and 64 codes of 31 bits: 1997, precode.hip kBlockWords
MAX_BATCH, MAX_RING = 48, 4
LISTS = ("types", "targets", "motion_x", "motion_y", "sp_pred", "sp_amount", "sp_index", "quality", "y", "u", "v")


# ---------------------------------------------------------------------------
# The code lengths, restated plainly (golomb.cpp:8-91), and the coded values.
# ---------------------------------------------------------------------------

def wrap16(v):
    return ((np.asarray(v, np.int64) + 32768) % 65536 - 32768)


def ue_len(v):
    """Bits of ue(v), v >= 0: the exp-Golomb code of v + 1."""
    n = np.asarray(v, np.int64) + 1
    return 2 * np.floor(np.log2(n)).astype(np.int64) + 1


def se_len(v):
    """Bits of se(v) for an int16 v other than -32768: 0 -> 1, v -> 2|v| + (v < 0)."""
    v = np.asarray(v, np.int64)
    assert not (v == -32768).any()
    m = np.where(v == 0, 1, 2 * np.abs(v) + (v < 0))
    return 2 * np.floor(np.log2(m)).astype(np.int64) + 1


def _blocks_of(planes, wmb, hmb):
    """(mbs, 6, 64) raster values of the six blocks of each macroblock (Y TL, TR, BL, BR, U, V)."""
    y, u, v = (np.asarray(p, np.int16) for p in planes)
    b = np.zeros((hmb * wmb, 6, 64), np.int16)
    b[:, :4] = y.reshape(hmb, 2, 8, wmb, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(hmb * wmb, 4, 64)
    b[:, 4] = u.reshape(hmb, 8, wmb, 8).transpose(0, 2, 1, 3).reshape(hmb * wmb, 64)
    b[:, 5] = v.reshape(hmb, 8, wmb, 8).transpose(0, 2, 1, 3).reshape(hmb * wmb, 64)
    return b


def _planes_of(b, wmb, hmb):
    y = b[:, :4].reshape(hmb, wmb, 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(hmb * 16, wmb * 16)
    u, v = (b[:, k].reshape(hmb, wmb, 8, 8).transpose(0, 2, 1, 3).reshape(hmb * 8, wmb * 8) for k in (4, 5))
    return tuple(np.ascontiguousarray(p, dtype=np.int16) for p in (y, u, v))


def coded_blocks(planes, wmb, hmb):
    """The values the stream codes for each block, (mbs, 6, 64) in zig-zag
    order: the block's coefficients with the DC replaced by its delta
    (serialize.cpp:35-123).  Luma TL takes the block 8 samples to the left of
    the macroblock (the left neighbour's TR), in the first column the one 8
    rows above (the upper neighbour's BL), 0 at the origin; TR and BL take TL,
    BR takes BL.  Chroma takes the left neighbour's block, in the first column
    the upper one's.  Neighbours' values count as stored, copy macroblocks'
    included.  (What is coded of a copy macroblock is nothing: mask by type.)"""
    b = _blocks_of(planes, wmb, hmb).astype(np.int64)
    dc = b[:, :, 0].reshape(hmb, wmb, 6)
    pred = np.zeros_like(dc)
    pred[:, 1:, 0] = dc[:, :-1, 1]
    pred[1:, 0, 0] = dc[:-1, 0, 2]
    pred[:, :, 1] = dc[:, :, 0]
    pred[:, :, 2] = dc[:, :, 0]
    pred[:, :, 3] = dc[:, :, 2]
    for k in (4, 5):
        pred[:, 1:, k] = dc[:, :-1, k]
        pred[1:, 0, k] = dc[:-1, 0, k]
    out = b[:, :, ZIGZAG]
    out[:, :, 0] = wrap16(dc - pred).reshape(-1, 6)
    return out


def place(table, wmb, hmb, coded, stale=None):
    """Planes whose non-copy macroblocks code exactly `coded` ((mbs, 6, 64),
    zig-zag order, position 0 the DC delta); copy macroblocks hold `stale`
    (raster values, (mbs, 6, 64); zeros if None), which their right and lower
    neighbours' deltas are taken against."""
    mbs = wmb * hmb
    copy = (table["block_type"] & COPY) != 0
    b = np.zeros((mbs, 6, 64), np.int64)
    b[:, :, ZIGZAG] = coded
    if stale is not None:
        b[copy] = stale[copy]
    else:
        b[copy] = 0
    dc = b[:, :, 0].reshape(hmb, wmb, 6)  # a view: deltas are replaced by values in coding order
    for my in range(hmb):
        for mx in range(wmb):
            if copy[my * wmb + mx]:
                continue
            d = dc[my, mx]
            for k, (near, above) in ((0, (1, 2)), (4, (4, 4)), (5, (5, 5))):
                p = dc[my, mx - 1, near] if mx > 0 else (dc[my - 1, 0, above] if my > 0 else 0)
                d[k] = wrap16(p + d[k])
            d[1] = wrap16(d[0] + d[1])
            d[2] = wrap16(d[0] + d[2])
            d[3] = wrap16(d[2] + d[3])
    return _planes_of(b.astype(np.int16), wmb, hmb)


def block_bits(coded):
    """Bits of each block, (..., 64) zig-zag coded values -> (...)."""
    nz = coded != 0
    run = np.where(nz.any(-1), 64 - np.argmax(nz[..., ::-1], -1), 0)
    inside = np.arange(64) < run[..., None]
    return ue_len(run) + np.where(inside, se_len(coded), 0).sum(-1)


def delta_items(table, field):
    """The present values of a delta list and their macroblock indices, and the coded deltas."""
    t = table["block_type"]
    sel = (t & COPY) == 0 if field == "q_index" else (t & MOTION) != 0
    idx = np.flatnonzero(sel)
    val = table[field][idx].astype(np.int64)
    return idx, val, wrap16(np.diff(val, prepend=0))


# ---------------------------------------------------------------------------
# Building blocks
# ---------------------------------------------------------------------------

def _table(mbs, types=COPY, q=8, target=1):
    t = np.zeros(mbs, BLOCK_DESC)
    t["block_type"], t["q_index"], t["prediction_target"] = types, q, target
    return t


def _no_excluded_delta(values, rng):
    """Redraw values whose int16 delta to the one before is -32768."""
    v = np.asarray(values, np.int64).copy()
    for _ in range(100):
        bad = np.flatnonzero(wrap16(np.diff(v, prepend=0)) == -32768)
        if not bad.size:
            return v
        v[bad] = rng.integers(-32768, 32768, bad.size)
    raise AssertionError("could not avoid -32768")


def _refix(table, rng):
    """After the motion set changed: no delta of -32768 between its members."""
    motion = np.flatnonzero((table["block_type"] & MOTION) != 0)
    for f in ("motion_x", "motion_y"):
        table[f][motion] = _no_excluded_delta(table[f][motion], rng)


def _wide_fields(table, rng):
    """Motion values over the whole int16 range, every other field random over its byte."""
    n = table.size
    for f in ("motion_x", "motion_y"):
        table[f] = rng.integers(-32768, 32768, n)
    _refix(table, rng)
    table["prediction_target"] = rng.integers(0, 256, n)
    table["sp_pred"] = rng.choice([0, 1, 1, 2, 255], n)
    table["sp_amount"] = rng.integers(0, 256, n)
    table["sp_index"] = rng.integers(0, 256, n)
    table["q_index"] = rng.integers(0, 256, n)
    table["variance"] = rng.integers(-32768, 32768, n)
    table["pad"] = rng.integers(0, 256, n)


def _full31(rng, shape):
    """Values whose codes have 31 bits: 16384 <= |v| <= 32767."""
    return rng.integers(16384, 32768, shape) * rng.choice([-1, 1], shape)


def _mixed_coded(rng, mbs, peak=32767, zero=0.5):
    """Coded values of every size: per block a random run, per value a random bit width."""
    width = rng.integers(0, 16, (mbs, 6, 64))
    mag = rng.integers(0, 1 << 15, (mbs, 6, 64)) >> (15 - width)
    c = np.minimum(mag, peak) * rng.choice([-1, 1], (mbs, 6, 64))
    c[rng.random((mbs, 6, 64)) < zero] = 0
    run = rng.choice([0, 0, 1, 2, 5, 17, 40, 63, 64], (mbs, 6))
    c[np.arange(64) >= run[..., None]] = 0
    return c


def _stale(rng, mbs):
    return rng.integers(-32768, 32768, (mbs, 6, 64))


def _dense(name, wmb, hmb, ring, seed, types=(0, 1, 2, 3, 4, 5, 6, 7)):
    """Every field random over its whole range, every type, coefficients of every size."""
    rng = np.random.default_rng(seed)
    mbs = wmb * hmb
    t = _table(mbs, rng.choice(types, mbs))
    _wide_fields(t, rng)
    return name, wmb, hmb, ring, t, place(t, wmb, hmb, _mixed_coded(rng, mbs), _stale(rng, mbs))


def _sparse(name, wmb, hmb, ring, seed, present, types=(MOTION,), fill=COPY):
    """Copy macroblocks (stale planes) except `present`, which cycle through `types`."""
    rng = np.random.default_rng(seed)
    mbs = wmb * hmb
    ty = np.full(mbs, fill)
    present = np.asarray(present, dtype=np.int64)
    ty[present] = np.resize(types, present.size)
    t = _table(mbs, ty)
    _wide_fields(t, rng)
    return name, wmb, hmb, ring, t, place(t, wmb, hmb, _mixed_coded(rng, mbs), _stale(rng, mbs))


# ---------------------------------------------------------------------------
# Delta-list cases
# ---------------------------------------------------------------------------

def delta_cases():
    # one chunk: items in waves 0 and 3, waves 1 and 2 empty (both motion and quality lists)
    yield _sparse("empty_waves", 16, 16, 4, 11, np.r_[3:9, 40, 63, 192, 200:230, 255], types=(MOTION, MOTION | INTRA))
    # 4 chunks, the last one partial: chunk 0 has no item; then one item per wave, on lane 0 and on lane 63 in turn
    at = [c * CHUNK + w * WAVE + (63 if (c + w) & 1 else 0) for c in range(1, 4) for w in range(4)]
    at[-1] = 3 * CHUNK + 3 * WAVE  # (the frame ends at lane 62 of its last wave)
    yield _sparse("one_per_wave", 33, 31, 2, 12, at)
    # chunks 0 and 3 hold motion macroblocks, 1 and 2 none (but quality items)
    mid = np.r_[CHUNK:3 * CHUNK]
    name, wmb, hmb, ring, t, _ = _dense("empty_motion_chunks", 33, 31, 4, 13, types=(2, 3, 6, 7, 0, 4))
    t["block_type"][mid] = np.resize([0, 1, 4], mid.size)
    _refix(t, np.random.default_rng(13))
    yield name, wmb, hmb, ring, t, place(t, wmb, hmb, _mixed_coded(np.random.default_rng(13), t.size, zero=0.8))
    # chunks 1 and 2 are all copy: no quality item (some with motion, some without any item)
    name, wmb, hmb, ring, t, _ = _dense("empty_quality_chunks", 33, 31, 3, 14, types=(0, 1, 2, 3, 6))
    t["block_type"][mid] = np.where(np.arange(mid.size) < CHUNK, COPY | MOTION, COPY)
    _refix(t, np.random.default_rng(14))
    yield name, wmb, hmb, ring, t, place(t, wmb, hmb, _mixed_coded(np.random.default_rng(14), t.size, zero=0.8))
    # every macroblock a copy: only the type list has items (the planes are stale values)
    yield _sparse("all_copy", 15, 17, 4, 15, [])
    # no motion macroblock at all
    yield _dense("no_motion", 15, 17, 4, 16, types=(0, 1, 4, 5))
    # wide deltas: the int16 extremes, 32767 followed by -32768 (coded as +1), q_index alternating 1 and 31
    name, wmb, hmb, ring, t, planes = _dense("wide_deltas", 16, 16, 4, 17, types=(2, 3, 6, 7, 2, 0))
    motion = np.flatnonzero((t["block_type"] & MOTION) != 0)
    for f, head in (("motion_x", [32767, -32768, -32768, 32767, 0, -32767, 32767, -2, 32767]),
                    ("motion_y", [-32767, 32767, -32768, 1, 32767, 16384, -16383, 32767, -32768])):
        t[f][motion[:len(head)]] = head
        t[f][motion] = _no_excluded_delta(t[f][motion], np.random.default_rng(18))
        assert (t[f][motion[:len(head)]] == head).all()
    coded = np.flatnonzero((t["block_type"] & COPY) == 0)
    t["q_index"][coded] = np.where(np.arange(coded.size) & 1, 31, 1)  # every quality delta is +-30
    yield name, wmb, hmb, ring, t, planes
    # more than one carry tile (66 chunks): sparse items on both sides of chunk 64
    at = [5, 300, 63 * CHUNK + 255, 64 * CHUNK, 64 * CHUNK + 70, 65 * CHUNK - 1, 65 * CHUNK, 16640]
    yield _sparse("two_carry_tiles", 129, 129, 4, 19, at, types=(MOTION, MOTION | INTRA, MOTION))
    # partial last waves, workgroups and chunks
    for k, (wmb, hmb) in enumerate(((1, 1), (3, 1), (15, 17), (16, 16), (257, 1))):
        yield _dense(f"dense_{wmb}x{hmb}", wmb, hmb, 4, 20 + k, **({"types": (INTRA | MOTION,)} if wmb * hmb == 1 else {}))
    # every ring size (target bits 0, 1, 1, 2), targets with bits above the mask
    for ring in range(1, MAX_RING + 1):
        yield _dense(f"ring_{ring}", 5, 4, ring, 30 + ring)
    # odd descriptor values: sp_pred 2 (flag bit 0, amount and index present), high bits in
    # sp_amount / sp_index, type 5, block_type bits above 7
    name, wmb, hmb, ring, t, planes = _dense("odd_descriptors", 16, 16, 4, 40)
    t["sp_pred"] = np.resize([2, 0, 1, 2, 254, 3], t.size)
    t["sp_amount"] = np.resize([0xFE, 0xFF, 2, 1, 0x80], t.size)
    t["sp_index"] = np.resize([0xF8, 0xFF, 8, 7, 0x85], t.size)
    t["block_type"][::3] = 5
    t["block_type"][1::4] |= np.resize(np.array([0x8, 0x100, 0xFFFFFFF8, 0x80000000], np.uint32), t.size // 4)
    _refix(t, np.random.default_rng(41))
    yield name, wmb, hmb, ring, t, place(t, wmb, hmb, coded_blocks(planes, wmb, hmb), _blocks_of(planes, wmb, hmb))


# ---------------------------------------------------------------------------
# Coefficient cases
# ---------------------------------------------------------------------------

def coef_cases():
    rng = np.random.default_rng(50)
    # extreme blocks: 1997-bit blocks beside all-zero ones, run 1, only position 63, +-32767
    wmb, hmb = 5, 4
    mbs = wmb * hmb
    c = np.zeros((mbs, 6, 64), np.int64)
    kinds = rng.permutation(np.resize(np.arange(6), mbs * 6)).reshape(mbs, 6)
    kinds[0] = [0, 1, 0, 1, 0, 1]
    kinds[1] = [1, 0, 1, 0, 1, 0]
    c[kinds == 0] = _full31(rng, ((kinds == 0).sum(), 64))
    # (kind 1: all zero)
    c[kinds == 2, 0] = rng.choice([1, -1, 32767, -32767, 255], (kinds == 2).sum())  # run 1
    c[kinds == 3, 63] = rng.choice([1, -32767, 300], (kinds == 3).sum())           # only position 63
    c[kinds == 4] = rng.choice([32767, -32767], ((kinds == 4).sum(), 64))
    k5 = kinds == 5
    c[k5] = _mixed_coded(rng, mbs)[k5]
    t = _table(mbs, np.resize([1, 0, 3, 2, 1, 7], mbs))
    t["block_type"][7] = COPY
    yield "extreme_blocks", wmb, hmb, 4, t, place(t, wmb, hmb, c, _stale(rng, mbs))
    # the DC chain: first column from above, others from the left, a copy macroblock on the left with stale
    # values, deltas and values that wrap in int16, the TL -> TR / BL -> BR chain inside a macroblock
    wmb, hmb = 4, 4
    mbs = wmb * hmb
    c = np.zeros((mbs, 6, 64), np.int64)
    c[:, :, 0] = rng.choice([32767, -32767, 30000, -30000, 1, -1, 0, 12345], (mbs, 6))
    c[0, :, 0] = [32767, 1, 1, 32767, 32767, -32767]  # TL 32767; TR and BL wrap to -32768; BR wraps back
    c[1, :, 0] = [1, 0, -1, 5, 1, -2]                 # chroma: 32767 + 1 wraps
    c[:, :, 1] = rng.integers(-3, 4, (mbs, 6))
    t = _table(mbs, 1)
    # macroblock 4 (first column) takes macroblock 0's BL; 8 is a copy, so 12 below it takes its stale BL;
    # 3, 6, 9 and 12 have a copy on their left and take its stale TR
    t["block_type"][[2, 5, 8, 11]] = COPY
    yield "dc_chain", wmb, hmb, 4, t, place(t, wmb, hmb, c, _stale(rng, mbs))


# ---------------------------------------------------------------------------
# Capacity cases: a section at, one bit over and well over 32 Mbit
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _block_plan(n):
    """(run, a, b): a block of n bits as ue(run), a codes of 31 bits, b of 3 bits and run - a - b zeros."""
    for run in range(64, -1, -1):
        rest = n - int(ue_len(run)) - run  # every value inside the run takes at least one bit
        if run == 0:
            if rest == 0:
                return 0, 0, 0
            continue
        for a in range(min(run, rest // 30), -1, -1):
            r2 = rest - 30 * a
            if r2 >= 0 and r2 % 2 == 0 and a + r2 // 2 <= run and a + r2 // 2 >= 1:
                return run, a, r2 // 2
    return None


def _block_of_bits(n, rng):
    run, a, b = _block_plan(n)
    c = np.zeros(64, np.int64)
    if run:
        vals = np.r_[_full31(rng, a), rng.choice([-1, 1], b)]
        body = np.r_[vals[:-1], np.zeros(run - a - b, np.int64)]
        c[:run - 1] = rng.permutation(body)
        c[run - 1] = vals[-1]  # the run ends on a nonzero value
    assert int(block_bits(c)) == n
    return c


def _split_bits(n, k):
    """n bits as k block sizes, each one a block can have, the first ones as large as possible."""
    if k == 1:
        return [n] if 1 <= n <= FULL_BLOCK and _block_plan(n) else None
    for take in range(min(FULL_BLOCK, n - (k - 1)), 0, -1):
        if _block_plan(take):
            rest = _split_bits(n - take, k - 1)
            if rest:
                return [take] + rest
    return None


def _capacity_frame(name, wmb, hmb, seed, extra_bits, tail=None):
    """Luma: full macroblocks (4 x 1997 bits), then one macroblock that brings
    the Y section to CAPACITY + extra_bits, then `tail` macroblocks (coded
    values (k, 4, 64)); every other macroblock is a copy."""
    rng = np.random.default_rng(seed)
    mbs = wmb * hmb
    full = CAPACITY // (4 * FULL_BLOCK) - 1
    rem = CAPACITY + extra_bits - full * 4 * FULL_BLOCK
    t = _table(mbs, COPY)
    c = np.zeros((mbs, 6, 64), np.int64)
    # spread over the frame, so that copy macroblocks lie between coded ones
    n_coded = full + 2 + (0 if tail is None else len(tail))
    at = np.sort(rng.choice(mbs, n_coded, replace=False))
    t["block_type"][at] = np.resize([1, 0, 3], n_coded)
    c[at[:full], :4] = _full31(rng, (full, 4, 64))
    for mb, bits in zip(at[full:full + 2], (4 * FULL_BLOCK, rem - 4 * FULL_BLOCK)):
        for b, n in enumerate(_split_bits(bits, 4)):
            c[mb, b] = _block_of_bits(n, rng)
    if tail is not None:
        c[at[full + 2:], :4] = tail
    c[at, 4:, 0] = rng.integers(-5, 6, (n_coded, 2))  # a little chroma
    return name, wmb, hmb, 4, t, place(t, wmb, hmb, c, None)


def capacity_cases(u_section=True):
    wmb = hmb = 66
    yield _capacity_frame("y_at_capacity", wmb, hmb, 60, 0)
    yield _capacity_frame("y_one_bit_over", wmb, hmb, 61, 1)
    # 17 bits below the capacity, then a block of run 8: ue(8) takes 7 bits; a 31-bit code is dropped; three
    # 3-bit codes fit (one bit left); a 31-bit code is dropped; a zero's single bit fits (none left); the rest
    # and the next macroblock's codes (all kinds) are dropped
    rng = np.random.default_rng(62)
    tail = _mixed_coded(rng, 8, zero=0.2)[:, :4]
    tail[0] = 0
    tail[0, 0, :8] = [20000, 1, -1, 1, -20000, 0, 1, -1]
    tail[1:, :, 0] = 77
    yield _capacity_frame("y_over_with_fits", wmb, hmb, 62, -17, tail)
    if u_section:
        # only the U section overflows: every U block full, luma and V all zero
        wmb = hmb = 130
        mbs = wmb * hmb
        rng = np.random.default_rng(63)
        t = _table(mbs, np.resize([1, 0, 3, 1, 2], mbs))
        c = np.zeros((mbs, 6, 64), np.int64)
        c[:, 4] = _full31(rng, (mbs, 64))
        yield "u_over", wmb, hmb, 4, t, place(t, wmb, hmb, c, None)


OVER_CAPACITY = ("y_one_bit_over", "y_over_with_fits", "u_over")
# what cases() yields, in order (for parametrised tests; tests/test_feed_tables.py checks it)
NAMES = ("empty_waves", "one_per_wave", "empty_motion_chunks", "empty_quality_chunks", "all_copy", "no_motion",
         "wide_deltas", "two_carry_tiles", "dense_1x1", "dense_3x1", "dense_15x17", "dense_16x16", "dense_257x1",
         "ring_1", "ring_2", "ring_3", "ring_4", "odd_descriptors", "extreme_blocks", "dc_chain", "y_at_capacity"
         ) + OVER_CAPACITY


# ---------------------------------------------------------------------------
# The -32768 rule's cases: the one value cases() never holds
# ---------------------------------------------------------------------------

def rule_cases():
    """A coded value of -32768 as a coefficient, as a DC delta and as a motion
    delta of each list (a quality delta cannot reach it: q_index is a byte),
    and beside each the same frame with the value the rule maps it to."""
    wmb, hmb = 3, 2
    mbs = wmb * hmb
    rng = np.random.default_rng(70)
    t = _table(mbs, np.resize([3, 2, 1, 6, 3, 2], mbs))  # macroblock 2 has no motion, 3 is a copy with motion
    t["motion_x"] = [100, -32668, 5, 5, -32763, 0]    # deltas 100, -32768, 32673, -32768, 32763
    t["motion_y"] = [-32768, 0, 32767, -1, 7, 7]      # deltas -32768 (from the start value 0), -32768 (wrapped), -1, 8, 0
    c = _mixed_coded(rng, mbs, zero=0.6)
    c[0, 0, 5] = c[2, 3, 63] = c[4, 3, 1] = c[5, 5, 17] = -32768   # coefficients
    c[1, 1, 0] = c[2, 0, 0] = c[4, 4, 0] = c[5, 2, 0] = -32768    # DC deltas
    yield "minus_32768", wmb, hmb, 4, t, place(t, wmb, hmb, c, _stale(rng, mbs))


def rule_applied(table, planes, wmb, hmb):
    """The frame that codes -32767 wherever (table, planes) codes -32768, and nothing else differently."""
    t = table.copy()
    for f in ("motion_x", "motion_y"):
        idx, val, delta = delta_items(t, f)
        # one more at each such delta and at every value after it: the later deltas stay as they are
        t[f][idx] = wrap16(val + np.cumsum(delta == -32768))
    c = coded_blocks(planes, wmb, hmb)
    c[c == -32768] = -32767
    return t, place(t, wmb, hmb, c, _blocks_of(planes, wmb, hmb))


# ---------------------------------------------------------------------------

def cases(capacity=True):
    yield from delta_cases()
    yield from coef_cases()
    if capacity:
        yield from capacity_cases()


def batch_frames(n, wmb=17, hmb=16, seed=100):
    """n different dense frames of one geometry (two chunks, the second partial) for one launch."""
    return [_dense(f"batch_{k}", wmb, hmb, 4, seed + k)[4:] for k in range(n)]


def assert_value_range(table, planes, wmb, hmb):
    """No coded value of a case is -32768."""
    c = coded_blocks(planes, wmb, hmb)[(table["block_type"] & COPY) == 0]
    assert not (c == -32768).any()
    for f in ("motion_x", "motion_y", "q_index"):
        assert not (delta_items(table, f)[2] == -32768).any()


if __name__ == "__main__":
    from oracle import oracle

    for name, wmb, hmb, ring, table, planes in cases():
        assert_value_range(table, planes, wmb, hmb)
        _, bits, lists, dropped = oracle.precode_slice(table, wmb, hmb, ring, *planes)
        print(f"{name:22s} {wmb:3d}x{hmb:<3d} ring {ring}  {bits:9d} bits  dropped {dropped:6d}  "
              + " ".join(f"{k}={v}" for k, v in zip(LISTS, lists)))
