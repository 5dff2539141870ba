"""The reference's in-loop deblock, restated in plain Python from its rules
(deblock.cpp:13-254), line by line, with a record of what each line did.

It does not call the oracle: tests/test_deblock.py compares the two, plane for
plane.  A *line* is one call of the filter: the eight samples p3 p2 p1 p0 | q0
q1 q2 q3 through an edge, along a row for a V (vertical) edge and down a
column for an H (horizontal) edge.  Only edges of strength 1 or 2 are examined.
While deblock() walks a frame in the reference's order it records, per line
(LINE below):

  plane      0 Y, 1 U, 2 V
  vert       1 for a V edge (step 1), 0 for an H edge (step = the row pitch)
  strength   1 (one side is a copy macroblock) or 2
  mb_edge    1 on a macroblock edge, 0 on a luma macroblock's inner 8x8 edge
  x, y       the position of q0
  fired      the line passed the alpha/beta test, so it stored its samples
  changed    a stored sample differs from what was there
  dependent  one of its eight inputs had been changed by an earlier line
  seam       V edge with x % chunk == 0: the first column of a deblock chunk
  preseam    V edge with (x + 8) % chunk == 0: the band-B lag at a chunk's end
  rowseam    H edge on a macroblock-row boundary: rows of two workgroups
  narrow     the int16 narrowing decided the line: without it (differences
             and results kept in full width) the line gives other samples

`chunk` is the width in luma columns of the chunks the row helpers filter in
(16, 32 or 64); the caller passes it, halved here for the chroma planes.
"""
from __future__ import annotations

import numpy as np

# alpha_table / beta_table, deblock.cpp:13-27, indexed by the edge's qp
ALPHA = (0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 16, 18, 20, 22, 24, 26, 29, 32, 35)
BETA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 10, 11)
COPY = 4

LINE = np.dtype([("plane", "u1"), ("vert", "u1"), ("strength", "u1"), ("mb_edge", "u1"), ("x", "<i4"), ("y", "<i4"),
                 ("fired", "u1"), ("changed", "u1"), ("dependent", "u1"), ("seam", "u1"), ("preseam", "u1"),
                 ("rowseam", "u1"), ("narrow", "u1")])


def chunk_of(wmb: int) -> int:
    """Luma columns per deblock chunk for a frame `wmb` macroblocks wide, as
    DESIGN.md states the rule (restated, not read from the library)."""
    return 64 if wmb >= 200 else 32 if wmb >= 100 else 16


def i16(v: int) -> int:
    """C's narrowing of an int to int16_t."""
    return ((v + 32768) & 0xFFFF) - 32768


def rounded_div(n: int, d: int) -> int:
    """math.h:224-232: half away from zero, the quotient truncated as C does (d > 0)."""
    n = n - d // 2 if n < 0 else n + d // 2
    return -(-n // d) if n < 0 else n // d


def edge_params(ta, qa, tb, qb):
    """compute_average_qp / compute_deblock_strength, deblock.cpp:49-79:
    (qp, strength) of the edge between macroblocks a and b.  A copy block's
    q_index is not read; two copies give strength 0."""
    ca, cb = bool(ta & COPY), bool(tb & COPY)
    if not ca and not cb:
        return ((qa + qb) >> 1) & 0xFF, 2
    if not ca:
        return qa, 1
    if not cb:
        return qb, 1
    return 0, 0


def filter_line(s, qp, strength, luma, narrowed=True):
    """deblock_filter_values, deblock.cpp:81-129, on the eight samples s ->
    the eight samples after it, or None if the alpha/beta test stops it."""
    cut = i16 if narrowed else int
    p3, p2, p1, p0, q0, q1, q2, q3 = s
    if cut(abs(p0 - q0)) >= ALPHA[qp] or cut(abs(p1 - p0)) >= BETA[qp] or cut(abs(q1 - q0)) >= BETA[qp]:
        return None
    out = list(s)
    if strength == 2:
        out[3] = cut(rounded_div(p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1, 8))
        out[2] = cut(rounded_div(p2 + p1 + p0 + q0, 4))
        out[4] = cut(rounded_div(p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2, 8))
        out[5] = cut(rounded_div(p0 + q0 + q1 + q2, 4))
        if luma:
            out[1] = cut(rounded_div(2 * p3 + 3 * p2 + p1 + p0 + q0, 8))
            out[6] = cut(rounded_div(2 * q3 + 3 * q2 + q1 + q0 + p0, 8))
    else:
        out[3] = cut(rounded_div((q0 + p0) * 4 + p1 - q1, 8))
        out[4] = cut(rounded_div((q0 + p0) * 4 + q1 - p1, 8))
        if luma:
            out[2] = cut(rounded_div(p2 * 4 + p0 * 2 + q0 * 2, 8))
            out[5] = cut(rounded_div(q2 * 4 + q0 * 2 + p0 * 2, 8))
    return out


def deblock_plane(img, types, qs, mbsz, plane, chunk, lines):
    """deblock_image, deblock.cpp:201-254, on a copy of the height x width
    plane img (returned): the first band's V edges, then
    per band of eight rows and per 8 columns the H edge above and the V edge
    to the left.  Appends one LINE tuple per filter call to `lines`."""
    height, width = img.shape
    luma = plane == 0
    a = img.ravel().tolist()
    touched = bytearray(len(a))
    wib = i16(width // mbsz)
    offs_v = tuple(range(-4, 4))
    offs_h = tuple(k * width for k in range(-4, 4))

    def mb(i, j):  # deblock_macroblock_index, deblock.cpp:44-47: a uint16
        return ((i // mbsz) + (j // mbsz) * wib) & 0xFFFF

    def edge(i, j, ia, ib, vert):
        qp, st = edge_params(types[ia], qs[ia], types[ib], qs[ib])
        if not st:
            return
        offs = offs_v if vert else offs_h
        on_mb = int((i if vert else j) % mbsz == 0)
        seam = int(vert and i % chunk == 0)
        pre = int(vert and (i + 8) % chunk == 0)
        rowseam = int(not vert and on_mb)
        for k in range(8):
            x, y = (i, j + k) if vert else (i + k, j)
            base = y * width + x
            idx = [base + o for o in offs]
            s = [a[n] for n in idx]
            dep = int(any(touched[n] for n in idx))
            out = filter_line(s, qp, st, luma)
            wide = filter_line(s, qp, st, luma, narrowed=False)
            changed = 0
            if out is not None and out != s:
                changed = 1
                for n, old, new in zip(idx, s, out):
                    if old != new:
                        a[n] = new
                        touched[n] = 1
            lines.append((plane, int(vert), st, on_mb, x, y, int(out is not None), changed, dep, seam, pre, rowseam,
                          int(out != wide)))

    for i in range(8, width, 8):
        edge(i, 0, mb(i - 1, 0), mb(i, 0), True)
    for j in range(8, height, 8):
        edge(0, j, mb(0, j - 1), mb(0, j), False)
        for i in range(8, width, 8):
            edge(i, j, mb(i, j - 1), mb(i, j), False)
            edge(i, j, mb(i - 1, j), mb(i, j), True)
    return np.array(a, np.int16).reshape(height, width)


def deblock(table, planes, chunk):
    """The three planes of a frame before the deblock -> (the planes after it,
    the LINE records in the order the reference filters).  table: the frame's
    block descs; chunk: the luma chunk width (chunk_of)."""
    types = [int(t) for t in table["block_type"]]
    qs = [int(q) for q in table["q_index"]]
    lines, out = [], []
    for k, p in enumerate(planes):
        out.append(deblock_plane(np.asarray(p, np.int16), types, qs, 16 if k == 0 else 8, k,
                                 chunk if k == 0 else chunk // 2, lines))
    return tuple(out), np.array(lines, LINE)


# ---------------------------------------------------------------------------
# Shares of the lines examined, per plane group: what tests/test_deblock.py
# asserts and DESIGN.md tabulates.
# ---------------------------------------------------------------------------

# every legal combination of H/V x strength x macroblock edge / inner edge; inner edges (luma only) are strength 2
LUMA_CLASSES = tuple((v, s, m) for v in (0, 1) for s, m in ((1, 1), (2, 1), (2, 0)))
CHROMA_CLASSES = tuple((v, s, 1) for v in (0, 1) for s in (1, 2))


def class_name(vert, strength, mb_edge):
    return f"{'V' if vert else 'H'} s{strength} {'mb' if mb_edge else 'inner'}"


def shares(lines, luma: bool):
    """name -> share of the examined lines of the luma plane, or of both
    chroma planes; 'narrow' is a count."""
    sel = lines[(lines["plane"] == 0) == luma]
    n = max(sel.size, 1)
    ch = sel["changed"] != 0
    dep = sel["dependent"] != 0
    # 'dependent': lines that change a sample and read one an earlier line changed, the ones whose result
    # turns on the order; 'reads earlier' also counts the lines that read such a sample and change nothing
    out = {"lines": int(sel.size), "changed": ch.sum() / n, "dependent": (ch & dep).sum() / n,
           "reads earlier": dep.sum() / n, "narrow": int((sel["narrow"] != 0).sum())}
    for c in LUMA_CLASSES if luma else CHROMA_CLASSES:
        m = (sel["vert"] == c[0]) & (sel["strength"] == c[1]) & (sel["mb_edge"] == c[2])
        out[class_name(*c)] = m.sum() / n
    if luma:
        out["chunk seam"] = (ch & (sel["seam"] != 0)).sum() / n
        out["chunk end"] = (ch & (sel["preseam"] != 0)).sum() / n
        out["row seam"] = (ch & (sel["rowseam"] != 0) & dep).sum() / n
    return out


def writers(lines, plane, x, y):
    """The fired lines whose stored samples include (x, y) of `plane`, in the
    order they ran.  Luma stores p2..q2 (strength 2) or p1..q1; chroma p1..q1
    or p0, q0."""
    reach = np.where(lines["strength"] == 2, 3, 2) - (0 if plane == 0 else 1)
    along = np.where(lines["vert"] != 0, x - lines["x"], y - lines["y"])
    across = np.where(lines["vert"] != 0, y - lines["y"], x - lines["x"])
    m = (lines["plane"] == plane) & (lines["fired"] != 0) & (across == 0) & (along >= -reach) & (along < reach)
    return lines[m]


def describe(line) -> str:
    flags = [n for n in ("changed", "dependent", "seam", "preseam", "rowseam", "narrow") if line[n]]
    return (f"{class_name(line['vert'], line['strength'], line['mb_edge'])} at ({line['x']}, {line['y']})"
            + (" [" + " ".join(flags) + "]" if flags else ""))


def locate(lines, plane, x, y, chunk):
    """Where sample (x, y) of `plane` lies for the row helpers, and which
    lines wrote it: the text a GPU mismatch is reported with."""
    sub, ch = (16, chunk) if plane == 0 else (8, chunk // 2)
    # Row r's helper filters band A (the H edge on the row's top boundary, which reaches 4 rows up into row r-1,
    # and the V edges of the 8 rows below it), then for luma band B (the inner H edge and the V edges of rows 8-15).
    band = "A" if plane or y % 16 < 8 else "B"
    if y % sub >= sub - (3 if plane == 0 else 2):  # the rows an H line stores above its edge: p2..p0, chroma p1, p0
        band += f" of row {y // sub}, then band A's H edge of the row below, if there is one"
    w = [describe(l) for l in writers(lines, plane, x, y)]
    return (f"plane {'YUV'[plane]} sample ({x}, {y}), macroblock ({x // sub}, {y // sub}), chunk {x // ch}, "
            f"{ch - x % ch} columns before the chunk's end, band {band}; written by: " + ("; ".join(w) or "no line"))


if __name__ == "__main__":  # the deblock coverage table of DESIGN.md
    from oracle import oracle as orc
    from tests import tables
    from tests.test_deblock import DECODE_CONFIGS, FRAMES, SEEDS, oracle_decode

    keys = [(w, h, r, s) for w, h, r in DECODE_CONFIGS for s in SEEDS]
    cols = {}
    for w, h, r, s in keys:
        recs = np.concatenate([deblock(t, pre, chunk_of((w + 15) // 16))[1]
                               for t, _, pre, _ in oracle_decode(orc, w, h, r, s)])
        cols[(w, h, r, s)] = shares(recs, True), shares(recs, False)
    print("| share of the lines examined | " + " | ".join(f"{w}x{h} R{r} s{s}" for w, h, r, s in keys) + " |")
    print("|---" * (len(keys) + 1) + "|")
    for k, name in ((0, "luma"), (1, "chroma")):
        for row in cols[keys[0]][k]:
            vals = [cols[key][k][row] for key in keys]
            fmt = (lambda v: str(v)) if row in ("lines", "narrow") else (lambda v: f"{100 * v:.1f} %")
            print(f"| {name}: {row} | " + " | ".join(fmt(v) for v in vals) + " |")
