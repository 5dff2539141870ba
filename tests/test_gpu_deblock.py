"""GPU parity of the in-loop deblock (deblock_chunk, db_line, dfilter_reg)
where the filter fires: sequences whose planes are flat 8x8 blocks a small
step apart (tests/tables.py make_deblock_sequence), at the smallest frames
that reach each chunk width (16, 32 and 64 luma columns), each ragged last
chunk and the tile's wrap at column 128, through the decode-mode engine
against the oracle decoder, exact; and band4 at q = 31 at the wide chunk
widths through the encoder.  tests/test_deblock.py asserts, without a GPU,
how many lines of these sequences change a sample, read what an earlier line
wrote and lie on a chunk or row seam.  A mismatch is reported as the first
differing sample with its place in the row helper's chunks and bands and the
classes of the lines that wrote it (tests/deblock_ref.py)."""
import numpy as np
import pytest

from tests import deblock_ref as ref
from tests.test_deblock import DECODE_CONFIGS, ENCODE_CONFIGS, SEEDS, oracle_decode
from tests.test_gpu_decode_tables import _decode
from tests.test_gpu_parity import _run_batched, _run_frames

pytestmark = pytest.mark.gpu


def _first_difference(got, want, k, table, pre, chunk):
    """The first sample (raster order) where plane k of a deblocked frame
    differs from the oracle's, and what the restatement says about it."""
    ys, xs = np.nonzero(got != want)
    x, y = int(xs[0]), int(ys[0])
    _, lines = ref.deblock(table, pre, chunk)
    return f"{ys.size} samples differ, first {got[y, x]} vs {want[y, x]} at " + ref.locate(lines, k, x, y, chunk)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("w,h,ring", DECODE_CONFIGS)
def test_deblock_sequences_match_oracle(orc, cairo, w, h, ring, seed):
    run = oracle_decode(orc, w, h, ring, seed)
    wmb = (w + 15) // 16
    chunk = ref.chunk_of(wmb)
    for t, ((table, _, pre, slot), (gpre, gslot, grgb)) in enumerate(zip(run, _decode(cairo, w, h, ring, run))):
        tag = f"{w}x{h} R={ring} seed {seed} frame {t}"
        for k, n in enumerate("YUV"):
            if not np.array_equal(gpre[k], pre[k]):
                ys, xs = np.nonzero(gpre[k] != pre[k])
                sub = 16 if k == 0 else 8
                mb = int(ys[0] // sub * wmb + xs[0] // sub)
                pytest.fail(f"{tag} pre-deblock {n}: {ys.size} samples differ, first at ({xs[0]}, {ys[0]}), "
                            f"macroblock {mb} = ({mb % wmb}, {mb // wmb}), desc {table[mb]}")
        for k, n in enumerate("YUV"):
            if not np.array_equal(gslot[k], slot[k]):
                pytest.fail(f"{tag} slot {n}: " + _first_difference(gslot[k], slot[k], k, table, pre, chunk))
        want = cairo.yuv_to_rgb(*slot, w, h)
        assert np.array_equal(grgb, want), f"{tag} RGB: {int((grgb != want).any(axis=-1).sum())} pixels differ"


def test_deblock_sequences_deterministic(orc, cairo):
    """Two fresh contexts give the same planes at the widest, ragged
    configuration: no read of a cell another workgroup may still be writing
    decides a firing filter's result."""
    w, h, ring = 3248, 48, 4
    run = oracle_decode(orc, w, h, ring, SEEDS[0])
    a, b = _decode(cairo, w, h, ring, run), _decode(cairo, w, h, ring, run)
    for t, ((apre, aslot, argb), (bpre, bslot, brgb)) in enumerate(zip(a, b)):
        for n, x, y in zip(("pre Y", "pre U", "pre V", "slot Y", "slot U", "slot V", "RGB"), apre + aslot + (argb,),
                           bpre + bslot + (brgb,)):
            assert np.array_equal(x, y), f"frame {t} {n}: {int((x != y).sum())} values differ between two runs"


@pytest.mark.parametrize("w,h,ring,q,frames", ENCODE_CONFIGS)
def test_frames_wide_chunks_strong_filter(orc, cairo, w, h, ring, q, frames):
    """band4 at q = 31 on 32- and 64-column chunks: every intermediate exact."""
    _run_frames(orc, cairo, w, h, ring, q, frames)


def test_batched_wide_chunks_strong_filter(orc, cairo):
    """A frame's helpers wait on the previous frame's deblock progress while
    the filter fires at the 32-column seams."""
    _run_batched(orc, cairo, 1600, 48, 4, 31, 6, 3, outputs=cairo.OUT_FEED)
