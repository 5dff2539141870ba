"""The GPU entropy precode (precode.hip) against the oracle's serialize_slice
walk on synthetic tables (tests/feed_tables.py), through the
known-answer entry point cairo_kat_precode: the launch a context makes for a
batch, on tables and planes the encoder never picks.  Exact: the header's bit
count, list starts and flags, every feed word, and the words after the feed's
end, with the slots holding zeros and holding ones before the launch (the
writer ORs into what the slot held: missed zeroing shows only under ones).
tests/test_feed_tables.py checks that the cases hold what they are aimed at
and the host precode against the same oracle."""
import numpy as np
import pytest

from tests import feed_tables as ft
from tests.test_feed_tables import reference

pytestmark = pytest.mark.gpu

GUARD = 64
ONES = 0xFFFFFFFF


def _check_frame(hdr, feed, guard, want_words, want_bits, want_lists, prefill, over, what):
    """One frame of a launch against the oracle's feed (over: only the flag
    and that nothing was zeroed or copied)."""
    assert hdr[3] == 0, (what, "dropped writes", int(hdr[3]))
    if over:
        assert hdr[2] == 1, (what, "overflow flag")
        assert (feed == prefill).all(), (what, "words copied on overflow")
        assert (guard == prefill).all(), (what, "words zeroed on overflow")
        return
    assert hdr[2] == 0, (what, "overflow flag")
    bits = int(hdr[0]) | (int(hdr[1]) << 32)
    assert bits == want_bits, (what, bits, want_bits)
    starts = np.concatenate([[0], np.cumsum(want_lists)[:-1]])
    np.testing.assert_array_equal(hdr[4:15], starts, err_msg=f"{what}: list starts")
    nw = (want_bits + 31) // 32
    bad = np.flatnonzero(feed[:nw] != want_words)
    assert bad.size == 0, (what, f"{bad.size} feed words differ, first at word {bad[0]} (bit {32 * bad[0]}) of {nw}: "
                                 f"{feed[bad[0]]:#010x} != {want_words[bad[0]]:#010x}; list starts {starts.tolist()}")
    assert (feed[nw:] == prefill).all(), (what, "words copied past the feed's end")
    assert guard[0] == 0, (what, "the word after the feed is zeroed")
    assert (guard[1:] == prefill).all(), (what, "words past the zeroed range were written")


def _run_case(cairo, c, prefill, slot=0, nslots=1):
    nw = (c["bits"] + 31) // 32
    return cairo.kat_precode([(c["table"], c["planes"])], c["wmb"], c["hmb"], c["ring"], slots=[slot], nslots=nslots,
                             prefill=prefill, feed_words=nw + 8, guard_words=GUARD)


@pytest.mark.parametrize("prefill", (0, ONES), ids=("zeros", "ones"))
@pytest.mark.parametrize("name", ft.NAMES)
def test_feed_case(orc, cairo, name, prefill):
    """Every case alone, on slot 2 of 3: header words 0-1 the oracle's bit
    count, 4-14 the exclusive prefix of its per-list counts, word 2 set exactly
    for the frames over the capacity (the one at the capacity exactly is
    valid), word 3 zero, the feed words the oracle's, the guard words
    untouched."""
    c = reference()[name]
    hdr, feed, guard = _run_case(cairo, c, prefill, slot=2, nslots=3)
    _check_frame(hdr[0], feed[0], guard[0], c["words"], c["bits"], c["lists"], prefill, name in ft.OVER_CAPACITY,
                 f"{name} prefill {prefill:#x}")


@pytest.fixture(scope="module")
def batch(orc):
    frames = ft.batch_frames(ft.MAX_BATCH)
    want = [orc.precode_slice(t, 17, 16, 4, *p) for t, p in frames]
    assert len({w[1] for w in want}) > ft.MAX_BATCH // 2  # different frames
    return frames, want


@pytest.mark.parametrize("count", (1, 5, ft.MAX_BATCH))
def test_feed_batch(cairo, batch, count):
    """Several different frames of one geometry in one launch, on staging
    slots that are no identity (and fewer frames than slots): each frame's
    result is the oracle's and its single-frame launch's, and a second run of
    the same launch gives the same words."""
    frames, want = batch
    nslots = {1: 4, 5: 7}.get(count, count)
    slots = np.roll(np.arange(nslots)[::-1], 3)[:count] if count > 1 else np.array([3])
    assert (slots != np.arange(count)).any() and len(set(slots.tolist())) == count
    nw = max((w[1] + 31) // 32 for w in want[:count]) + 8
    runs = [cairo.kat_precode(frames[:count], 17, 16, 4, slots=slots, nslots=nslots, prefill=ONES, feed_words=nw,
                              guard_words=GUARD) for _ in range(2)]
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b, err_msg="two runs of one launch differ")
    hdr, feed, guard = runs[0]
    for j in range(count):
        words, bits, lists, dropped = want[j]
        assert dropped == 0
        k = (bits + 31) // 32
        _check_frame(hdr[j], feed[j, :k + 8], guard[j], words, bits, lists, ONES, False, f"frame {j} of {count}, slot {slots[j]}")
        if j < 5:
            h1, f1, g1 = cairo.kat_precode(frames[j:j + 1], 17, 16, 4, prefill=ONES, feed_words=nw, guard_words=GUARD)
            np.testing.assert_array_equal(h1[0], hdr[j])
            np.testing.assert_array_equal(f1[0], feed[j])
            np.testing.assert_array_equal(g1[0], guard[j])


def test_minus_32768_rule_gpu(orc, cairo):
    """DESIGN §4.0 on the GPU: a coded -32768 (coefficient, DC delta, motion
    delta) gives the feed of the frame that holds -32767 in those places."""
    for name, wmb, hmb, ring, table, planes in ft.rule_cases():
        t2, p2 = ft.rule_applied(table, planes, wmb, hmb)
        words, bits, lists, dropped = orc.precode_slice(t2, wmb, hmb, ring, *p2)
        for prefill in (0, ONES):
            hdr, feed, guard = cairo.kat_precode([(table, planes)], wmb, hmb, ring, prefill=prefill,
                                                 feed_words=(bits + 31) // 32 + 8, guard_words=GUARD)
            _check_frame(hdr[0], feed[0], guard[0], words, bits, lists, prefill, False, name)


def test_kat_precode_refuses_bad_arguments(cairo):
    """Slots out of range or used twice, too many frames, a ring or a frame
    size the library does not accept: refused before any launch."""
    t, p = ft.batch_frames(1, 2, 2)[0]
    for kw, frames, ring in ((dict(slots=[1], nslots=1), 1, 4), (dict(slots=[0, 0], nslots=2), 2, 4),
                             (dict(slots=[0], nslots=ft.MAX_BATCH + 1), 1, 4), (dict(), 1, 0), (dict(), 1, 5)):
        with pytest.raises(cairo.CairoError):
            cairo.kat_precode([(t, p)] * frames, 2, 2, ring, **kw)
