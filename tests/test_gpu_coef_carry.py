"""GPU parity of the output_cache carry done by the row helpers.

On an inter frame the helper of row r copies each group's macroblocks from the
previous frame's coefficient planes to this frame's before it stores the
group's records; the row coder then stores only the macroblocks it codes, over
the carried values.  A carry that ran too early or too late, missed a lane of
a ragged group, or landed after the coder's store shows in a frame's
coefficient planes, so every test runs a stream through the pipelined Context
with feed outputs, as bench.py does, and compares every frame's coefficient
planes (fetched from its staging slot), block table and payload bits, and the
ring slots at the end, with the oracle.

Each test also counts copy and coded macroblocks in the oracle's tables and
asserts a minimum, so that content which stopped exercising the path fails
loudly.  The oracle's streams are computed once per stream and shared.
"""
import numpy as np
import pytest

from tests import content
from tests.test_gpu_parity import _payload_bits, _table_equal

pytestmark = pytest.mark.gpu

K_COPY = 4  # evx_defs.h kCopy


def _band4(orc):
    return lambda w, h, t: orc.make_frame(w, h, t)


def _static(w, h, t):
    return content.make("static", w, h, t)


def _smooth(w, h, t):
    """One smooth frame repeated (the gradient content's frame 0): under the
    oracle 95 % of CIF's P-frame macroblocks are copy at q=16, and nearly all
    of them carry non-zero coefficients from the intra frame."""
    return content.make("gradient", w, h, 0)


def _aabb(orc):
    """A, A, B, B, A, A, B, B: A a band4 frame, B an unrelated noise frame."""
    def gen(w, h, t):
        return orc.make_frame(w, h, 0) if (t // 2) % 2 == 0 else content.make("noise", w, h, 0)
    return gen


def _ggnn(orc):
    """The same pattern with A the smooth frame: its repeats carry non-zero
    coefficients, which the band4 frame's copy macroblocks (flat areas) rarely have."""
    def gen(w, h, t):
        return _smooth(w, h, 0) if (t // 2) % 2 == 0 else content.make("noise", w, h, 0)
    return gen


GENS = {"band4": _band4, "static": lambda orc: _static, "smooth": lambda orc: _smooth, "aabb": _aabb, "ggnn": _ggnn}
_CACHE = {}


def _reference(orc, kind, w, h, ring, q, frames):
    """The oracle's stream, once: per frame (block table, coefficient planes,
    payload bits), the final ring slots, and the source frames."""
    key = (kind, w, h, ring, q, frames)
    if key not in _CACHE:
        gen = GENS[kind](orc)
        e = orc.OracleEncoder(ring)
        e.set_quality(q)
        src, ref = [], []
        for t in range(frames):
            rgb = gen(w, h, t)
            src.append(rgb)
            data, nbits = e.encode(rgb)
            head = (14 * 8 if t == 0 else 0) + 10 * 8  # header + frame descriptor precede the payload
            bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")[head:nbits]
            ref.append((e.block_table().copy(), tuple(np.array(p, copy=True) for p in e.planes(1)), bits))
        slots = [tuple(np.array(p, copy=True) for p in e.planes(2 + k)) for k in range(ring)]
        _CACHE[key] = (src, ref, slots)
    return _CACHE[key]


def _copy_masks(ref):
    """Per P-frame (frames 1..): which macroblocks are copy types."""
    return [(r[0]["block_type"] & K_COPY) != 0 for r in ref[1:]]


def _run(orc, cairo, kind, w, h, ring, q, frames, batch, stages=0):
    src, ref, slots = _reference(orc, kind, w, h, ring, q, frames)
    ctx = cairo.Context(w, h, ring, stages=stages) if stages else cairo.Context(w, h, ring)
    try:
        ctx.set_outputs(cairo.OUT_FEED)
        ctx.set_batch(batch)
        depth = ctx.stages
        pending = []

        def check(t, tk):
            out = ctx.wait(tk)
            tag = f"{kind} {w}x{h} R={ring} q={q} batch={batch} stages={depth} frame {t}"
            _table_equal(out.table, ref[t][0], f"{tag}: block table")
            coef = ctx.fetch_coef(tk)
            for p, name in enumerate("YUV"):
                bad = np.argwhere(coef[p] != ref[t][1][p])
                assert bad.size == 0, (f"{tag}: coef {name} differs at {len(bad)} elements, first (row, col) "
                                       f"{bad[:4].tolist()}: gpu {coef[p][tuple(bad[0])]} ref {ref[t][1][p][tuple(bad[0])]}")
            assert out.feed_status == cairo.FEED_VALID, f"{tag}: feed status {out.feed_status}"
            got = _payload_bits(cairo, out, ctx, ring, tk)
            assert got.size == ref[t][2].size, f"{tag}: payload {got.size} vs {ref[t][2].size} bits"
            assert np.array_equal(got, ref[t][2]), f"{tag}: payload bits differ"
            ctx.release(tk)

        for t in range(frames):  # at most `depth` frames in flight (submitted, not released)
            if len(pending) == depth:
                check(*pending.pop(0))
            pending.append((t, ctx.submit(src[t], t, t > 0, q)))
        for p in pending:
            check(*p)
        ctx.sync()
        for k in range(ring):
            got = ctx.read_planes(2 + k)
            for p, name in enumerate("YUV"):
                np.testing.assert_array_equal(got[p], slots[k][p], err_msg=f"ring slot {k} {name}")
    finally:
        ctx.close()
    return ref


def _assert_shares(ref, min_copy, min_coded):
    masks = _copy_masks(ref)
    total = sum(m.size for m in masks)
    copy = sum(int(m.sum()) for m in masks)
    print(f"P-frame macroblocks {total}: copy {copy}, coded {total - copy}")
    assert copy >= min_copy * total, f"only {copy} of {total} P-frame macroblocks are copy"
    assert total - copy >= min_coded * total, f"only {total - copy} of {total} P-frame macroblocks are coded"


# 1, 2: CIF band4 (the oracle: 691 of the 1 980 P-frame macroblocks copy, 1 289
# coded), all 6 frames in one launch, and 2 per launch: a frame's helper then
# reads a coef_prev written by the previous launch.
@pytest.mark.parametrize("batch", [6, 2], ids=["one_launch", "2_per_launch"])
def test_carry_cif_band4(orc, cairo, batch):
    ref = _run(orc, cairo, "band4", 352, 288, 4, 16, 6, batch)
    _assert_shares(ref, 0.25, 0.25)


# 3: one reference: the group's only search is the one after the wait.
def test_carry_one_reference(orc, cairo):
    ref = _run(orc, cairo, "band4", 352, 288, 2, 16, 6, 6)
    _assert_shares(ref, 0.25, 0.25)


# 4: ragged groups.  200x120: 13 macroblocks per row, the last group has one
# (the oracle: 66 of 520 P-frame macroblocks copy); 16x16: one macroblock.
def test_carry_ragged_200x120(orc, cairo):
    ref = _run(orc, cairo, "band4", 200, 120, 4, 16, 6, 6)
    _assert_shares(ref, 0.05, 0.25)


def test_carry_single_macroblock(orc, cairo):
    _run(orc, cairo, "band4", 16, 16, 4, 16, 6, 6)


# ... and the ragged width with the smooth frame repeated, whose copy
# macroblocks carry non-zero coefficients (the oracle: 382 of 520 copy).
def test_carry_ragged_smooth(orc, cairo):
    ref = _run(orc, cairo, "smooth", 200, 120, 4, 16, 6, 6)
    _assert_shares(ref, 0.50, 0.05)


# 5: transitions.  The repeat frames are copy nearly everywhere (a carry after
# a coded frame), the switches are coded (the coder overwrites a carried value).
# The oracle alone: band4 / noise 159 and 159 of 396 positions, smooth / noise
# 389 and 389 (band4 by itself: 18 and 3).
@pytest.mark.parametrize("batch", [8, 3], ids=["one_launch", "3_per_launch"])
@pytest.mark.parametrize("kind", ["aabb", "ggnn"], ids=["band4_noise", "smooth_noise"])
def test_carry_transitions(orc, cairo, kind, batch):
    ref = _run(orc, cairo, kind, 352, 288, 4, 16, 8, batch)
    masks = _copy_masks(ref)
    after_coded = np.zeros(masks[0].size, bool)  # positions that are copy right after being coded
    after_copy = np.zeros(masks[0].size, bool)   # ... and coded right after being copy
    for prev, cur in zip(masks, masks[1:]):
        after_coded |= cur & ~prev
        after_copy |= ~cur & prev
    n = after_coded.size
    print(f"positions {n}: copy after coded {int(after_coded.sum())}, coded after copy {int(after_copy.sum())}")
    assert after_coded.sum() >= 0.25 * n, f"only {int(after_coded.sum())} of {n} positions are copy after coded"
    assert after_copy.sum() >= 0.25 * n, f"only {int(after_copy.sum())} of {n} positions are coded after copy"


# 6: static content: nearly every macroblock of every P-frame is carried.  The
# default staging slots, and 2 (the synchronous encoder's configuration: a
# slot's previous contents are two frames old; one frame per launch, the most
# two slots allow).  The API accepts no single
# slot (cairo_ctx_create_ex: stages >= 2), so coef never aliases coef_prev.
# The frame is the smooth one: band4's frame 0 repeated (tests/content.py
# "static") is only 40 % copy at CIF under the oracle (783 of 1 980 at q=16, at
# most 45 % at any quality: its quantisation error reaches the copy threshold),
# and all but one of those copy macroblocks have all-zero coefficients; the
# smooth frame gives 1 883 of 1 980 (95 %), 333 or more per frame with non-zero
# coefficients.
@pytest.mark.parametrize("stages", [0, 2], ids=["default_slots", "2_slots"])
def test_carry_static(orc, cairo, stages):
    ref = _run(orc, cairo, "smooth", 352, 288, 4, 16, 6, 1 if stages == 2 else 6, stages=stages)
    _assert_shares(ref, 0.90, 0.0)


# ... and the project's "static" kind, at the share band4 itself is held to.
def test_carry_static_band4(orc, cairo):
    ref = _run(orc, cairo, "static", 352, 288, 4, 16, 6, 1, stages=2)
    _assert_shares(ref, 0.25, 0.25)
