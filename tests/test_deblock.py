"""CPU side of the deblock parity (tests/test_gpu_deblock.py): the line-by-line
restatement of the reference deblock (tests/deblock_ref.py) against the
oracle's, and what the sequences the GPU tests run put through the filter:
the share of lines that change a sample, that read what an earlier line wrote,
and that lie on the seams between the row helpers' chunks and rows.  Content
that stops firing the filter fails here, without a GPU."""
import numpy as np
import pytest

from tests import deblock_ref as ref
from tests import tables
from tests.test_tables import CONFIGS

# (width, height, ring): what tests/test_gpu_deblock.py decodes, four frames, seeds 1 and 2
DECODE_CONFIGS = ((208, 48, 2), (1600, 48, 2), (1616, 64, 4), (3200, 48, 2), (3248, 48, 4), (3216, 32, 2))
FRAMES, SEEDS = 4, (1, 2)
# (width, height, ring, quality, frames): the band4 streams it encodes
ENCODE_CONFIGS = ((1600, 48, 4, 31, 3), (3200, 48, 4, 31, 3))

# Least shares of the lines examined in a plane group, per decode sequence.
LUMA_MIN = {"changed": 0.20, "dependent": 0.05, "chunk seam": 0.005, "row seam": 0.004,
            **{ref.class_name(*c): 0.005 for c in ref.LUMA_CLASSES}}
CHROMA_MIN = {"changed": 0.15, "dependent": 0.015, **{ref.class_name(*c): 0.02 for c in ref.CHROMA_CLASSES}}
NARROW_MIN = 16  # lines the int16 narrowing decides, in a sequence of 12 macroblocks or more

_oracle_runs = {}


def _mbs(w, h):
    return (w + 15) // 16, (h + 15) // 16


def oracle_decode(orc, w, h, ring, seed, make=tables.make_deblock_sequence, frames=FRAMES):
    """A sequence and the oracle's decode of it, computed once and not
    changed: [(table, coef, pre-deblock planes, slot planes)]."""
    key = (w, h, ring, seed, make.__name__, frames)
    if key not in _oracle_runs:
        d = orc.OracleDecoder(w, h, ring)
        run = []
        for t, (table, coef) in enumerate(make(w, h, ring, frames, seed)):
            d.decode(table, coef)
            run.append((table, coef, d.predeblock(), d.planes(2 + t % ring)))
        _oracle_runs[key] = run
    return _oracle_runs[key]


def oracle_encode(orc, w, h, ring, q, frames):
    """band4 through the oracle encoder, once: [(table, pre-deblock planes, slot planes)]."""
    key = (w, h, ring, q, frames)
    if key not in _oracle_runs:
        e = orc.OracleEncoder(ring)
        e.set_quality(q)
        run = []
        for t in range(frames):
            e.encode(orc.make_frame(w, h, t))
            run.append((e.block_table(), e.predeblock(), e.planes(2 + t % ring)))
        _oracle_runs[key] = run
    return _oracle_runs[key]


def _check(frames, chunk, what):
    """deblock_ref on each (table, pre-deblock, slot) equals the slot -> all LINE records."""
    recs = []
    for t, (table, pre, slot) in enumerate(frames):
        got, lines = ref.deblock(table, pre, chunk)
        for k in range(3):
            if not np.array_equal(got[k], slot[k]):
                ys, xs = np.nonzero(got[k] != slot[k])
                pytest.fail(f"{what} frame {t}: the restatement and the oracle differ, first at "
                            + ref.locate(lines, k, int(xs[0]), int(ys[0]), chunk)
                            + f": {got[k][ys[0], xs[0]]} vs {slot[k][ys[0], xs[0]]}, {ys.size} samples")
        recs.append(lines)
    return np.concatenate(recs)


def _at_least(got, least, what):
    short = {k: f"{100 * got[k]:.2f} % < {100 * v:.2f} %" for k, v in least.items() if got[k] < v}
    assert not short, (what, short)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("w,h,ring", DECODE_CONFIGS)
def test_deblock_sequences(orc, cairo, w, h, ring, seed):
    """Every sequence the GPU tests decode: the restatement equals the oracle
    on it, its tables are legal, and it meets the coverage conditions.
    `python -m tests.deblock_ref` prints the shares (decoder section)."""
    wmb, hmb = _mbs(w, h)
    run = oracle_decode(orc, w, h, ring, seed)
    for t, (table, _, _, _) in enumerate(run):
        assert cairo.table_check(table, wmb, hmb, ring)
        assert t > 0 or np.all(table["block_type"] & 1)
    lines = _check([(t, pre, slot) for t, _, pre, slot in run], ref.chunk_of(wmb), f"{w}x{h} R={ring} seed {seed}")
    luma, chroma = ref.shares(lines, True), ref.shares(lines, False)
    _at_least(luma, LUMA_MIN, "luma")
    _at_least(chroma, CHROMA_MIN, "chroma")
    assert luma["narrow"] + chroma["narrow"] >= NARROW_MIN


@pytest.mark.parametrize("w,h,ring", CONFIGS)
def test_restatement_on_decode_tables(orc, w, h, ring):
    """The tables of tests/test_tables.py, whose planes hold int16 extremes:
    here the narrowing of the differences and results decides lines."""
    run = oracle_decode(orc, w, h, ring, 1, make=tables.make_sequence, frames=6)
    lines = _check([(t, pre, slot) for t, _, pre, slot in run], ref.chunk_of(_mbs(w, h)[0]), f"tables {w}x{h} R={ring}")
    if _mbs(w, h)[0] * _mbs(w, h)[1] >= 12:
        assert lines["narrow"].sum() >= 1


@pytest.mark.parametrize("q", (16, 31))
def test_restatement_on_cif_stream(orc, q):
    lines = _check(oracle_encode(orc, 352, 288, 4, q, 3), 16, f"CIF band4 q={q}")
    assert lines["changed"].sum() > 0


@pytest.mark.parametrize("w,h,ring,q,frames", ENCODE_CONFIGS)
def test_encode_streams(orc, w, h, ring, q, frames):
    """The band4 streams the GPU tests encode at the wide chunk widths."""
    lines = _check(oracle_encode(orc, w, h, ring, q, frames), ref.chunk_of(_mbs(w, h)[0]), f"band4 {w}x{h} q={q}")
    _at_least(ref.shares(lines, True), {"changed": 0.15, "dependent": 0.02}, "luma")


def test_restatement_rules():
    """The pieces the planes above cannot tell apart when they agree."""
    assert [ref.rounded_div(n, 8) for n in (-13, -12, -11, -4, -3, 3, 4, 11, 12)] == [-2, -2, -1, -1, 0, 0, 1, 1, 2]
    assert ref.i16(32768) == -32768 and ref.i16(-32769) == 32767 and ref.i16(40480) == -25056
    assert ref.edge_params(1, 9, 0, 12) == (10, 2) and ref.edge_params(4, 200, 2, 12) == (12, 1)
    assert ref.edge_params(1, 9, 6, 77) == (9, 1) and ref.edge_params(4, 9, 6, 12) == (0, 0)
    assert [ref.chunk_of(n) for n in (1, 99, 100, 199, 200, 240)] == [16, 16, 32, 32, 64, 64]
    # a full-scale step: fires only because |p0 - q0| = 40480 narrows to a negative number
    s = [20240] * 4 + [-20240] * 4
    assert ref.filter_line(s, 16, 2, True, narrowed=False) is None
    assert ref.filter_line(s, 16, 2, True) == [20240, 15180, 10120, 5060, -5060, -10120, -15180, -20240]
    assert ref.filter_line([0, 0, 0, 0, 6, 6, 6, 6], 16, 2, True) is None  # alpha(16) = 6
    assert ref.filter_line([0, 0, 0, 0, 5, 5, 5, 5], 16, 1, False) == [0, 0, 0, 2, 3, 5, 5, 5]
