"""Synthetic block tables and coefficient planes for the decode-mode engine.

Everything here is something a stream can legally carry (cairo_table_check,
include/cairo_amd.h), built in plain numpy from a seed, far denser in corner
cases than what the encoder's own search picks.  A frame's table has two
parts:

  directed  descs that hit named classes (desc_classes below), placed at
            macroblocks where they are legal.  They come in rounds of twelve
            descs with a fixed type pattern; q_index and the motion specs are
            taken from counters that run on over the rounds and frames of a
            sequence, so that a six-frame sequence of twelve macroblocks or
            more meets every class (tests/test_tables.py asserts it).  Frames
            of 64 macroblocks and more carry five rounds each.
  random    every other macroblock: a desc drawn at random, kept if the
            predicate accepts it alone, redrawn otherwise.  Fields its type
            does not carry (the vector of a non-motion type, the target of an
            intra type, q_index of a copy type) hold arbitrary values: they
            must be ignored.

Frame 0 holds intra types only, as a stream's first frame does.  Its intra
vectors read the never-written ring slot, zero on both sides (zero_state in
backend.hip clears ring_buf at create and reset; the oracle's planes_alloc
uses calloc, as the reference's image::allocate zeroes, image.cpp:70-94).  Later frames may predict from any target 1..ring-1, so a
target beyond the frames decoded so far reads a zero slot too; the directed
descs use targets 1..min(index, ring-1).

A frame of a single macroblock can hold only types 0, 1, 2, 4 and 6, and a
motion type only the zero vector without sub-pel (SINGLE_MB_CLASSES).
"""
from __future__ import annotations

import numpy as np

import cairo_amd
from cairo_amd import BLOCK_DESC

TYPES = (0, 1, 2, 3, 4, 6, 7)
INTRA, MOTION, COPY = 1, 2, 4
Q_MIN, Q_MAX = 1, 31  # the predicate's range for a block with coefficients
# frac_index -> direction (motion.cpp:61-109)
SP_DIR = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))

ROUND = 12
FRAME0_ROUND = (1, 1, 1, 1, 1, 1, 1, 3, 3, 3, 3, 7)
COPY_CYCLE = (6, 7, 4, 6, 6)

# Intra-motion specs: (vector, (sp_amount, sp_index)); the named extreme is
# reached by the base point or, for the second six, by the sub-pel neighbour.
INTRA_SPECS = (
    ((-32, -16), (0, 2)),  # x = px-32, base
    ((32, -16), (0, 0)),   # x = px+32, base
    ((0, -48), (0, 5)),    # y = py-48, base
    ((-24, 16), (0, 1)),   # y = py+16, base
    ((-16, 16), (0, 3)),   # corner (px-16, py+16), base
    ((16, -16), (0, 4)),   # corner (px+16, py-16), base
    ((-31, -15), (1, 0)),  # x = px-32, neighbour
    ((31, -17), (0, 7)),   # x = px+32, neighbour
    ((0, -47), (1, 1)),    # y = py-48, neighbour
    ((-24, 15), (0, 6)),   # y = py+16, neighbour
    ((-17, 15), (1, 7)),   # corner (px-16, py+16), neighbour
    ((17, -16), (1, 3)),   # corner (px+16, py-16), neighbour
    ((-8, -20), (1, 2)),
    ((5, -33), (1, 4)),
    ((-20, -3), (1, 5)),
    ((12, -17), (1, 6)),
)
# Inter-motion specs: (where the block lies, (sp_amount, sp_index)).  l r t b:
# on that frame edge, mid-way along it; tl tr bl br: in that corner; far: an
# inner block more than 31 px away.  The sub-pel neighbour of the first eight
# lies on a frame edge too.
INTER_SPECS = (
    ("l", (0, 1)), ("r", (0, 6)), ("t", (0, 3)), ("b", (0, 4)),
    ("tl", (1, 4)), ("tr", (1, 6)), ("bl", (1, 1)), ("br", (1, 3)),
    ("far", (0, 0)), ("far", (0, 2)), ("in", (0, 5)), ("in", (0, 7)),
    ("in", (1, 0)), ("in", (1, 2)), ("far", (1, 5)), ("in", (1, 7)),
)

SINGLE_MB_TYPES = (1, 0, 2, 4, 6, 2)


def rounds_of(nmb: int) -> int:
    return 5 if nmb >= 64 else 1


def _round_types(index: int, g: int):
    """Types of one round: frame 0's, or inter round g (counted over the sequence)."""
    if index == 0:
        return FRAME0_ROUND
    return (1, 1, 1, 1, 1, 3, 3, 3, 0 if g % 5 == 2 else 2, 2, 2, COPY_CYCLE[g % 5])


def _frame_rounds(nmb: int, index: int):
    s = rounds_of(nmb)
    return [_round_types(index, (index - 1) * s + j) for j in range(s)]


def _counts_before(nmb: int, index: int):
    """How many directed descs of each counter's kind the frames before
    `index` hold: (type 1, other types with coefficients, intra motion, inter
    motion, inter types)."""
    c = [0, 0, 0, 0, 0]
    for f in range(index):
        for r in _frame_rounds(nmb, f):
            for t in r:
                _count(c, t)
    return c


def _count(c, t):
    if t == 1:
        c[0] += 1
    elif not t & COPY:
        c[1] += 1
    if t & MOTION:
        c[2 if t & INTRA else 3] += 1
    if not t & INTRA:
        c[4] += 1


def _alone(desc, bx, by, wmb, hmb, ring) -> bool:
    """Does the predicate accept desc at (bx, by)?"""
    return bool(cairo_amd.desc_check(desc, by * wmb + bx, wmb, hmb, ring)[0])


def _inter_point(kind, wmb, hmb, rng):
    xmax, ymax = wmb * 16 - 16, hmb * 16 - 16
    mx, my = int(rng.integers(1, max(xmax, 2))), int(rng.integers(1, max(ymax, 2)))
    if kind == "far":  # near a corner, so that a macroblock on the other side is far from it
        mx = int(rng.choice((1, 2, xmax - 2, xmax - 1)))
        my = int(rng.choice((1, 2, ymax - 2, ymax - 1)))
    return {"l": (0, my), "r": (xmax, my), "t": (mx, 0), "b": (mx, ymax), "tl": (0, 0), "tr": (xmax, 0),
            "bl": (0, ymax), "br": (xmax, ymax)}.get(kind, (mx, my))


def make_table(wmb: int, hmb: int, ring: int, index: int, seed: int) -> np.ndarray:
    nmb = wmb * hmb
    rng = np.random.default_rng([seed, index, wmb, hmb, ring])
    table = np.zeros(nmb, BLOCK_DESC)
    tmax = max(1, min(index, ring - 1))

    def desc(t, q=0, target=0, mv=(0, 0), sp=None):
        d = np.zeros((), BLOCK_DESC)
        d["block_type"], d["q_index"], d["prediction_target"] = t, q, target
        d["motion_x"], d["motion_y"] = mv
        if sp is not None:
            d["sp_pred"], d["sp_amount"], d["sp_index"] = 1, sp[0], sp[1]
        return d

    if nmb == 1:  # what one macroblock can hold
        t = SINGLE_MB_TYPES[index % 6] if index else 1
        table[0] = desc(t, 1 + (seed * 5 + index * 7) % 31, 0 if t & INTRA else 1 + index % tmax)
        assert cairo_amd.table_check(table, wmb, hmb, ring)
        return table
    assert nmb >= ROUND * rounds_of(nmb), "a frame holds one macroblock or at least a round of directed descs"

    free = [int(i) for i in rng.permutation(nmb)]
    c = _counts_before(nmb, index)
    c = [c[0] + seed * 11, c[1] + seed * 13, c[2] + seed * 3, c[3] + seed * 5, c[4] + seed]

    def place(make):
        """Put make(bx, by) at the first free macroblock where it is legal."""
        for k, i in enumerate(free):
            d = make(i % wmb, i // wmb)
            if d is not None and _alone(d, i % wmb, i // wmb, wmb, hmb, ring):
                table[i] = d
                del free[k]
                return
        raise AssertionError("no macroblock takes a directed desc")

    todo = []  # (priority, make): the descs tied to few macroblocks are placed first
    for types in _frame_rounds(nmb, index):
        for t in types:
            if t == 1:
                q = Q_MIN + c[0] % 31
            elif not t & COPY:
                q = Q_MIN + c[1] % 31
            else:
                q = int(rng.integers(0, 256))  # not carried, never read
            target = int(rng.integers(0, 256)) if t & INTRA else 1 + c[4] % tmax
            if t & MOTION and t & INTRA:
                mv, sp = INTRA_SPECS[c[2] % 16]
                todo.append((0, lambda bx, by, a=(t, q, target, mv, sp): desc(*a)))
            elif t & MOTION:
                kind, sp = INTER_SPECS[c[3] % 16]
                x, y = _inter_point(kind, wmb, hmb, rng)

                def make(bx, by, a=(t, q, target), kind=kind, sp=sp, x=x, y=y):
                    v = (x - bx * 16, y - by * 16)
                    if kind in ("far", "tl", "tr", "bl", "br") and max(abs(v[0]), abs(v[1])) <= 31:
                        return None
                    return desc(*a, v, sp)

                todo.append((1, make))
            else:
                todo.append((2, lambda bx, by, a=(t, q, target): desc(*a)))
            _count(c, t)
    for _, make in sorted(todo, key=lambda e: e[0]):
        place(make)

    allowed = (1, 3, 7) if index == 0 else TYPES
    for i in free:
        bx, by = i % wmb, i // wmb
        while True:
            t = int(rng.choice(allowed))
            d = desc(t, int(rng.integers(0, 256)) if t & COPY else int(rng.integers(Q_MIN, Q_MAX + 1)),
                     int(rng.integers(0, 256)) if t & INTRA else int(rng.integers(1, ring)))
            if t & MOTION and t & INTRA:
                d["motion_x"], d["motion_y"] = int(rng.integers(-33, 34)), int(rng.integers(-49, 18))
            elif t & MOTION:
                d["motion_x"] = int(rng.integers(-2, wmb * 16 - 13)) - bx * 16
                d["motion_y"] = int(rng.integers(-2, hmb * 16 - 13)) - by * 16
            else:
                d["motion_x"], d["motion_y"] = int(rng.integers(-999, 1000)), int(rng.integers(-999, 1000))
            d["sp_pred"] = int(rng.integers(0, 2)) if t & MOTION else int(rng.integers(0, 256))
            d["sp_amount"] = int(rng.integers(0, 2)) if t & MOTION and d["sp_pred"] else int(rng.integers(0, 256))
            d["sp_index"] = int(rng.integers(0, 8)) if t & MOTION and d["sp_pred"] else int(rng.integers(0, 256))
            d["variance"] = int(rng.integers(-999, 1000))
            if _alone(d, bx, by, wmb, hmb, ring):
                table[i] = d
                break
    assert cairo_amd.table_check(table, wmb, hmb, ring)
    return table


# The largest coefficient magnitude.  -32768 is left out: a payload holding it
# does not decode (unserialize_slice reports a corrupt stream), so no stream
# carries it.  +-32767 passes the oracle's dequantize and inverse transform
# clean under UBSan (test_oracle_decoder_sanitized): the sums stay in int32 and
# the results are narrowed to int16 as the reference's are.
COEF_PEAK = 32767


def make_coef(wmb: int, hmb: int, index: int, seed: int):
    """Coefficient planes (y, u, v) of a frame: per macroblock sparse small
    values (most zero, |c| <= 64), dense +-2047, or a single +-COEF_PEAK per
    8x8 block (DC or one AC).  Copy macroblocks get them too."""
    rng = np.random.default_rng([seed, index, wmb, hmb, 99])
    y = np.zeros((hmb * 16, wmb * 16), np.int16)
    u = np.zeros((hmb * 8, wmb * 8), np.int16)
    v = np.zeros((hmb * 8, wmb * 8), np.int16)
    for by in range(hmb):
        for bx in range(wmb):
            kind = rng.choice(3, p=(0.6, 0.3, 0.1))
            blocks = [y[by * 16 + j:by * 16 + j + 8, bx * 16 + i:bx * 16 + i + 8] for j in (0, 8) for i in (0, 8)]
            blocks += [u[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8], v[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]]
            for b in blocks:
                if kind == 0:
                    b[...] = rng.integers(-64, 65, (8, 8)) * (rng.random((8, 8)) < 0.1)
                elif kind == 1:
                    b[...] = rng.integers(-2047, 2048, (8, 8))
                else:
                    k = 0 if rng.random() < 0.5 else int(rng.integers(1, 64))
                    b[k // 8, k % 8] = COEF_PEAK if rng.random() < 0.5 else -COEF_PEAK
    return y, u, v


def make_sequence(width: int, height: int, ring: int, frames: int, seed: int):
    """[(table, (y, u, v))] for frames 0..frames-1 of a width x height stream."""
    wmb, hmb = (width + 15) // 16, (height + 15) // 16
    return [(make_table(wmb, hmb, ring, t, seed), make_coef(wmb, hmb, t, seed)) for t in range(frames)]


# ---------------------------------------------------------------------------
# Sequences for the deblock: tables and coefficients whose planes before the
# deblock are flat 8x8 blocks a small step apart, so that the alpha/beta test
# passes on a large share of the edges and filtered lines read what earlier
# lines wrote (tests/deblock_ref.py classifies them, tests/test_deblock.py
# asserts the shares).
# ---------------------------------------------------------------------------

DEBLOCK_Q = (8, 31)  # alpha and beta are 0 below q_index 7 and 8
DEBLOCK_TYPES, DEBLOCK_TYPE_P = (1, 0, 4, 6), (0.3, 0.3, 0.3, 0.1)
# A chain: a type-1 macroblock with a flat DC and CHAIN-1 type-3 macroblocks to
# its right, each predicting from its left neighbour (vector (-16, 0)) and
# adding the same flat step, all at q_index CHAIN_Q.  A flat block from one DC
# reaches +-4048 at most (two passes of 45/128 over a dequantized 32767), so
# the fifth macroblock holds +-20240.  Two chains of opposite sign in
# adjacent rows put a step of 40480 across the H edge between their last
# macroblocks: |p0 - q0| narrowed to int16 is negative, below alpha, and the
# filter fires across it, which it would not without the narrowing.
CHAIN, CHAIN_Q = 5, 16
CHAIN_DC_INTRA = 32767 // 24  # luma DC scale q + 8 at q = 16 (quantize.cpp:37-55); the chroma scale is smaller
CHAIN_DC_INTER = 32767 // (2 * CHAIN_Q)  # 2 v qm q / 16 with qm = 16 (quantize.cpp:232-243)


def make_deblock_frame(wmb: int, hmb: int, ring: int, index: int, seed: int):
    """(table, (y, u, v)) of frame `index`."""
    rng = np.random.default_rng([seed, index, wmb, hmb, ring, 7])
    nmb = wmb * hmb
    table = np.zeros(nmb, BLOCK_DESC)
    y = np.zeros((hmb * 16, wmb * 16), np.int16)
    u = np.zeros((hmb * 8, wmb * 8), np.int16)
    v = np.zeros((hmb * 8, wmb * 8), np.int16)

    def blocks(bx, by):
        out = [y[by * 16 + j:by * 16 + j + 8, bx * 16 + i:bx * 16 + i + 8] for j in (0, 8) for i in (0, 8)]
        return out + [u[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8], v[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]]

    chained = set()
    # every fourth frame, the last of a four-frame sequence: the frames after a chain inherit its +-20240 levels,
    # whose edges no longer fire, which costs a frame of 39 macroblocks a quarter of its lines
    if index % 4 == 3 and wmb >= CHAIN and hmb >= 2:
        bx0, by0 = int(rng.integers(0, wmb - CHAIN + 1)), int(rng.integers(0, hmb - 1))
        for row, sign in ((by0, 1), (by0 + 1, -1)):
            for k in range(CHAIN):
                d = table[row * wmb + bx0 + k]
                d["block_type"], d["q_index"] = (1, CHAIN_Q) if k == 0 else (3, CHAIN_Q)
                d["motion_x"] = 0 if k == 0 else -16
                for b in blocks(bx0 + k, row):
                    b[0, 0] = sign * (CHAIN_DC_INTRA if k == 0 else CHAIN_DC_INTER)
                chained.add(row * wmb + bx0 + k)

    for i in range(nmb):
        if i in chained:
            continue
        bx, by = i % wmb, i // wmb
        t = 1 if index == 0 else int(rng.choice(DEBLOCK_TYPES, p=DEBLOCK_TYPE_P))
        d = table[i]
        d["block_type"], d["prediction_target"] = t, 1
        d["q_index"] = int(rng.integers(DEBLOCK_Q[0], DEBLOCK_Q[1] + 1))
        while t & MOTION:  # a short vector that stays in the frame, with or without a sub-pel neighbour
            d["motion_x"], d["motion_y"] = int(rng.integers(-4, 5)), int(rng.integers(-4, 5))
            d["sp_pred"], d["sp_amount"] = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            d["sp_index"] = int(rng.integers(0, 8))
            if _alone(d, bx, by, wmb, hmb, ring):
                break
        for b in blocks(bx, by):  # copies get coefficients too: they must be ignored
            b[0, 0] = (30 if t == 1 else 0) + int(rng.integers(-1, 2))
            if rng.random() < 0.3:
                b[0, 1], b[1, 0] = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
    assert cairo_amd.table_check(table, wmb, hmb, ring)
    return table, (y, u, v)


def make_deblock_sequence(width: int, height: int, ring: int, frames: int, seed: int):
    """[(table, (y, u, v))] for frames 0..frames-1: frame 0 is type 1
    throughout, later frames mix types 1, 0, 4 and 6 on target 1; q_index is
    uniform in DEBLOCK_Q; every 8x8 block holds a DC a step of -1, 0 or 1 from
    its type's level and now and then the two lowest AC terms; frames 3, 7, ...
    carry a pair of chains (above) where the frame has room."""
    wmb, hmb = (width + 15) // 16, (height + 15) // 16
    return [make_deblock_frame(wmb, hmb, ring, t, seed) for t in range(frames)]


# ---------------------------------------------------------------------------
# Which directed classes a desc meets, read off the desc alone (whoever placed it).
# ---------------------------------------------------------------------------

def desc_classes(d, bx: int, by: int, wmb: int, hmb: int):
    t = int(d["block_type"])
    out = {f"type:{t}"}
    if not t & COPY:
        out.add(("q_intra:" if t == 1 else "q_inter:") + str(int(d["q_index"])))
    if not t & INTRA:
        out.add(f"target:{int(d['prediction_target'])}")
    if not t & MOTION:
        return out
    px, py, xmax, ymax = bx * 16, by * 16, wmb * 16 - 16, hmb * 16 - 16
    pts = [("base", px + int(d["motion_x"]), py + int(d["motion_y"]))]
    if d["sp_pred"]:
        dx, dy = SP_DIR[int(d["sp_index"])]
        pts.append(("nb", pts[0][1] + dx, pts[0][2] + dy))
        out.add(f"sp_{'intra' if t & INTRA else 'inter'}:{int(d['sp_amount'])}:{int(d['sp_index'])}")
    if t & INTRA:
        for who, x, y in pts:
            if x == px - 32 and y <= py - 16:
                out.add(f"intra_xmin:{who}")
            if x == px + 32 and y <= py - 16:
                out.add(f"intra_xmax:{who}")
            if y == py - 48:
                out.add(f"intra_ymin:{who}")
            if y == py + 16 and x <= px - 16:
                out.add(f"intra_ymax:{who}")
            if (x, y) == (px - 16, py + 16):
                out.add(f"intra_corner_below:{who}")
            if (x, y) == (px + 16, py - 16):
                out.add(f"intra_corner_right:{who}")
        return out

    def edges(x, y):
        return {e for e, on in (("l", x == 0), ("r", x == xmax), ("t", y == 0), ("b", y == ymax)) if on}

    e0 = edges(pts[0][1], pts[0][2])
    e1 = edges(pts[1][1], pts[1][2]) if len(pts) > 1 else set()
    for e in e0:
        out.add(f"inter_edge:{e}")
        if e in e1:
            out.add(f"inter_edge_sp:{e}")
    for cn in ("tl", "tr", "bl", "br"):
        if set(cn) <= e0:
            out.add(f"inter_corner:{cn}")
            if e1:  # the neighbour, clamped by both edges, is itself on one
                out.add(f"inter_corner_sp:{cn}")
    if max(abs(int(d["motion_x"])), abs(int(d["motion_y"]))) > 31:
        out.add("inter_far")
    return out


def required_classes(ring: int, frames: int):
    """What a sequence of `frames` frames of twelve macroblocks or more must meet."""
    req = {f"type:{t}" for t in TYPES}
    req |= {f"q_{p}:{q}" for p in ("intra", "inter") for q in range(Q_MIN, Q_MAX + 1)}
    req |= {f"sp_{p}:{a}:{i}" for p in ("intra", "inter") for a in (0, 1) for i in range(8)}
    req |= {f"target:{k}" for k in range(1, min(frames - 1, ring - 1) + 1)}
    req |= {f"intra_{n}:{who}" for n in ("xmin", "xmax", "ymin", "ymax", "corner_below", "corner_right")
            for who in ("base", "nb")}
    req |= {f"inter_edge{s}:{e}" for s in ("", "_sp") for e in "lrtb"}
    req |= {f"inter_corner{s}:{cn}" for s in ("", "_sp") for cn in ("tl", "tr", "bl", "br")}
    req.add("inter_far")
    return req


# One macroblock: no intra motion (its own position is not yet coded), so no
# types 3 and 7; the only in-frame vector is zero and it has no in-frame
# neighbour, so no sub-pel, no far vector and no intra extreme; six frames
# hold six q_index values, not all of them.
SINGLE_MB_CLASSES = ({f"type:{t}" for t in (0, 1, 2, 4, 6)} | {"target:1"} | {f"inter_edge:{e}" for e in "lrtb"}
                     | {f"inter_corner:{cn}" for cn in ("tl", "tr", "bl", "br")})


def sequence_classes(seq, wmb: int, hmb: int):
    """class -> count over a sequence's tables."""
    from collections import Counter

    n = Counter()
    for table, _ in seq:
        for i, d in enumerate(table):
            n.update(desc_classes(d, i % wmb, i // wmb, wmb, hmb))
    return n


if __name__ == "__main__":  # the coverage table of DESIGN.md: the least count among a group's classes, per sequence
    from tests.test_tables import CONFIGS, FRAMES, SEEDS

    keys = [(w, h, r, s) for w, h, r in CONFIGS for s in SEEDS]
    rows = {}
    for w, h, r, s in keys:
        wmb, hmb = (w + 15) // 16, (h + 15) // 16
        n = sequence_classes(make_sequence(w, h, r, FRAMES, s), wmb, hmb)
        req = SINGLE_MB_CLASSES if wmb * hmb == 1 else required_classes(r, FRAMES)
        for c in required_classes(r, FRAMES):
            g = c.split(":")[0]
            rows.setdefault(g, {}).setdefault((w, h, r, s), []).append(n.get(c, 0))
    print("| class group (classes) | " + " | ".join(f"{w}x{h} R{r} s{s}" for w, h, r, s in keys) + " |")
    print("|---" * (len(keys) + 1) + "|")
    for g in sorted(rows):
        k = max(len(v) for v in rows[g].values())
        print(f"| {g} ({k}) | " + " | ".join(str(min(rows[g][key])) for key in keys) + " |")
