"""GPU parity of the row helper's group start.

A helper's wait for a reference frame also reports whether the group's whole
search window is final, an inter task takes that flag instead of polling, an
older-reference task none of whose macroblocks needs a search issues no load
at all, and reference 1 issues its carry load, its zero-MV loads and its
fallback poll in one batch.  A wrong "full" stages a window that is not final
yet, a wrong "need" skips or adds a search, and a carry that lost its place
shows in the coefficient planes, so every case runs its stream two ways and
compares with the oracle:

* pipelined Context with feed outputs, as bench.py runs: every frame's block
  table, coefficient planes and payload bits, and the ring slots at the end;
* the debug path (set_debug(1), encode_frame, read_inter): additionally every
  reference's inter records and SADs of every inter frame.

Each case classes the oracle's (row, group, reference) tasks by how many of
the group's macroblocks need a search (a macroblock needs none when its record
is copy, zero vector, no sub-pel): none / all / mixed.  The cases that are
there for a class assert a floor on it, so content that stopped exercising a
path fails loudly.  The oracle's stream is computed once per case and shared.

Whether the wait's flag was set when a task read it depends on timing and
cannot be forced from here; the accounting counters (tools/acct.py,
"group_start") report it.
"""
import numpy as np
import pytest

from tests import content
from tests.test_gpu_parity import _payload_bits, _table_equal

pytestmark = pytest.mark.gpu

K_COPY = 4  # evx_defs.h kCopy


def _gen(orc, kind):
    if kind == "band4":
        return lambda w, h, t: orc.make_frame(w, h, t)
    if kind == "smooth":  # one smooth frame repeated: copy macroblocks with non-zero carried coefficients
        return lambda w, h, t: content.make("gradient", w, h, 0)
    return lambda w, h, t: content.make(kind, w, h, t)


_CACHE = {}


def _reference(orc, kind, w, h, ring, q, frames):
    """The oracle's stream, once: the source frames, per frame (block table,
    coefficient planes, payload bits, inter records, inter SADs), and the
    final ring slots."""
    key = (kind, w, h, ring, q, frames)
    if key not in _CACHE:
        gen = _gen(orc, kind)
        e = orc.OracleEncoder(ring)
        e.set_quality(q)
        src, ref = [], []
        for t in range(frames):
            rgb = gen(w, h, t)
            src.append(rgb)
            data, nbits = e.encode(rgb)
            head = (14 * 8 if t == 0 else 0) + 10 * 8  # header + frame descriptor precede the payload
            bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")[head:nbits]
            recs, sads = e.inter_records() if t > 0 else (None, None)
            ref.append((e.block_table().copy(), tuple(np.array(p, copy=True) for p in e.planes(1)), bits, recs, sads))
        slots = [tuple(np.array(p, copy=True) for p in e.planes(2 + k)) for k in range(ring)]
        _CACHE[key] = (src, ref, slots)
    return _CACHE[key]


def _classes(ref, w, h, ring):
    """(tasks, none, all, mixed) over the oracle's (row, group, reference)
    tasks of every inter frame."""
    wmb, hmb = (w + 15) // 16, (h + 15) // 16
    ng = (wmb + 3) // 4
    tasks = none = full = 0
    for r in ref[1:]:
        d = r[3].reshape(ring - 1, hmb, wmb)
        idle = ((d["block_type"] & K_COPY) != 0) & (d["motion_x"] == 0) & (d["motion_y"] == 0) & (d["sp_pred"] == 0)
        for g in range(ng):
            grp = idle[:, :, 4 * g:min(4 * g + 4, wmb)]
            searching = (~grp).sum(axis=2)
            tasks += searching.size
            none += int((searching == 0).sum())
            full += int((searching == grp.shape[2]).sum())
    return tasks, none, full, tasks - none - full


def _pipelined(orc, cairo, kind, w, h, ring, q, frames, batch, compare=True):
    """The stream through the pipelined Context with feed outputs; returns
    what the GPU produced: per frame (table, coefficient planes, payload
    bits), then the ring slots."""
    src, ref, slots = _reference(orc, kind, w, h, ring, q, frames)
    ctx = cairo.Context(w, h, ring)
    got_frames = []
    try:
        ctx.set_outputs(cairo.OUT_FEED)
        ctx.set_batch(batch)
        depth = ctx.stages
        pending = []

        def check(t, tk):
            out = ctx.wait(tk)
            tag = f"{kind} {w}x{h} R={ring} q={q} batch={batch} frame {t}"
            coef = ctx.fetch_coef(tk)
            assert out.feed_status == cairo.FEED_VALID, f"{tag}: feed status {out.feed_status}"
            bits = _payload_bits(cairo, out, ctx, ring, tk)
            got_frames.append((out.table.copy(), coef, bits))
            if compare:
                _table_equal(out.table, ref[t][0], f"{tag}: block table")
                for p, name in enumerate("YUV"):
                    bad = np.argwhere(coef[p] != ref[t][1][p])
                    assert bad.size == 0, (f"{tag}: coef {name} differs at {len(bad)} elements, first (row, col) "
                                           f"{bad[:4].tolist()}")
                assert bits.size == ref[t][2].size, f"{tag}: payload {bits.size} vs {ref[t][2].size} bits"
                assert np.array_equal(bits, ref[t][2]), f"{tag}: payload bits differ"
            ctx.release(tk)

        for t in range(frames):  # at most `depth` frames in flight (submitted, not released)
            if len(pending) == depth:
                check(*pending.pop(0))
            pending.append((t, ctx.submit(src[t], t, t > 0, q)))
        for p in pending:
            check(*p)
        ctx.sync()
        got_slots = [ctx.read_planes(2 + k) for k in range(ring)]
        if compare:
            for k in range(ring):
                for p, name in enumerate("YUV"):
                    np.testing.assert_array_equal(got_slots[k][p], slots[k][p], err_msg=f"ring slot {k} {name}")
    finally:
        ctx.close()
    return got_frames, got_slots


def _debug(orc, cairo, kind, w, h, ring, q, frames):
    """The stream frame by frame on the debug path: every reference's inter
    records and SADs, the block table and the coefficient planes."""
    src, ref, slots = _reference(orc, kind, w, h, ring, q, frames)
    ctx = cairo.Context(w, h, ring)
    try:
        ctx.set_debug(1)
        for t in range(frames):
            out = ctx.encode_frame(src[t], t, t > 0, q)
            tag = f"{kind} {w}x{h} R={ring} q={q} debug frame {t}"
            if t > 0:
                gd, gs = ctx.read_inter()
                _table_equal(gd, ref[t][3], f"{tag}: inter records")
                np.testing.assert_array_equal(gs, ref[t][4], err_msg=f"{tag}: inter SAD")
            _table_equal(out.table, ref[t][0], f"{tag}: block table")
            for p, (name, got) in enumerate(zip("YUV", (out.coef_y, out.coef_u, out.coef_v))):
                np.testing.assert_array_equal(got, ref[t][1][p], err_msg=f"{tag}: coef {name}")
        for k in range(ring):
            got = ctx.read_planes(2 + k)
            for p, name in enumerate("YUV"):
                np.testing.assert_array_equal(got[p], slots[k][p], err_msg=f"ring slot {k} {name}")
    finally:
        ctx.close()


def _run(orc, cairo, path, kind, w, h, ring, q, frames, floors=None):
    """path: "debug", or the frames per launch of the pipelined run."""
    if path == "debug":
        _debug(orc, cairo, kind, w, h, ring, q, frames)
    else:
        _pipelined(orc, cairo, kind, w, h, ring, q, frames, path)
    tasks, none, full, mixed = _classes(_reference(orc, kind, w, h, ring, q, frames)[1], w, h, ring)
    print(f"{kind} {w}x{h} R={ring}: tasks {tasks}: none {none}, all {full}, mixed {mixed}")
    for name, have in (("none", none), ("all", full), ("mixed", mixed)):
        floor = (floors or {}).get(name, 0)
        assert have >= floor, f"only {have} of {tasks} tasks are in class '{name}' (floor {floor})"


# CIF band4, R = 4 (the oracle: 1 620 tasks; none 288, all 1 126, mixed 206):
# one launch of 6, 2 per launch (the flags then come from a previous launch's
# progress words), and the debug path.
@pytest.mark.parametrize("path", [6, 2, "debug"], ids=["one_launch", "2_per_launch", "debug"])
def test_group_start_cif_band4(orc, cairo, path):
    _run(orc, cairo, path, "band4", 352, 288, 4, 16, 6, {"none": 200, "all": 800, "mixed": 150})


# No older reference (R = 2: only the wait's flag and reference 1's batch
# apply; the oracle: 540 tasks; none 120, all 320, mixed 100), and one (R = 3).
@pytest.mark.parametrize("path", [6, "debug"], ids=["one_launch", "debug"])
@pytest.mark.parametrize("ring", [2, 3])
def test_group_start_fewer_references(orc, cairo, ring, path):
    _run(orc, cairo, path, "band4", 352, 288, ring, 16, 6)


# The smooth frame repeated: the no-load path with non-zero carried
# coefficients behind it (the oracle: none 787, all 456, mixed 377).
@pytest.mark.parametrize("path", [6, "debug"], ids=["one_launch", "debug"])
def test_group_start_cif_smooth(orc, cairo, path):
    _run(orc, cairo, path, "smooth", 352, 288, 4, 16, 6, {"none": 600, "mixed": 300})


# Noise: all 972 tasks search, so the check is the exact comparison alone.
@pytest.mark.parametrize("path", [4, "debug"], ids=["one_launch", "debug"])
def test_group_start_cif_noise(orc, cairo, path):
    _run(orc, cairo, path, "noise", 352, 288, 4, 16, 4)


# Ragged sizes.  200x120: the last group holds one macroblock (none 36, all
# 442); 64x48 with one reference; 16x16: one macroblock, one group.
@pytest.mark.parametrize("path", [6, "debug"], ids=["one_launch", "debug"])
@pytest.mark.parametrize("w,h,ring", [(200, 120, 4), (64, 48, 2), (16, 16, 4)])
def test_group_start_ragged(orc, cairo, w, h, ring, path):
    _run(orc, cairo, path, "band4", w, h, ring, 16, 6)


# pan: its searches reach the window's far rows and columns, so the level-2
# decisions run (the oracle: all 1 584, none 36).
@pytest.mark.parametrize("path", [6, "debug"], ids=["one_launch", "debug"])
def test_group_start_pan(orc, cairo, path):
    _run(orc, cairo, path, "pan", 352, 288, 4, 16, 6)


# One sequence twice: whatever the flags were in each run, the outputs are equal.
def test_group_start_deterministic(orc, cairo):
    a, sa = _pipelined(orc, cairo, "band4", 352, 288, 4, 16, 6, 2, compare=False)
    b, sb = _pipelined(orc, cairo, "band4", 352, 288, 4, 16, 6, 2, compare=False)
    for t, (fa, fb) in enumerate(zip(a, b)):
        _table_equal(fa[0], fb[0], f"frame {t}: block table, run 1 vs run 2")
        for p, name in enumerate("YUV"):
            np.testing.assert_array_equal(fa[1][p], fb[1][p], err_msg=f"frame {t}: coef {name}, run 1 vs run 2")
        assert np.array_equal(fa[2], fb[2]), f"frame {t}: payload bits, run 1 vs run 2"
    for k, (pa, pb) in enumerate(zip(sa, sb)):
        for p, name in enumerate("YUV"):
            np.testing.assert_array_equal(pa[p], pb[p], err_msg=f"ring slot {k} {name}, run 1 vs run 2")
