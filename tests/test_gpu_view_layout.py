"""GPU parity over every field of the regrouped frame view.

The kernels read the per-frame view (kernels.h FrameArgs) in blocks: the row
coder's macroblock start, the window prefetch and group start, the stores and
publish.  A field at the wrong offset, or a block read that misses one, shows
as a wrong address or a wrong count somewhere in a frame, so every test is
bit-exact against the oracle, at the smallest shapes at which each field
matters:

  16x16     one macroblock: no row above, no group neighbour, no prefetch
  64x48     one group per row; rows 0..2 take the `by < 3` window paths
  200x120   13 macroblocks per row (a last group of one), padded height
  CIF       R = 2 and R = 4 (one and three references), I + 3 P, so that the
            stale rows and every reference are live; two launches of two
            frames (the previous launch's views are shared); kept
            reconstructions (the deblock's mirror, npush = 1); a decode round
            trip (the decode kernel's reads)

Each run compares every frame's block table, coefficient planes and payload
bits and the final ring slots (tests/test_gpu_coef_carry.py `_run`; the
oracle's stream is computed once per shape and shared).
"""
import pytest

from tests.test_gpu_coef_carry import _run
from tests.test_gpu_metrics import _check_ticket, _oracle_run
from tests.test_gpu_parity import _decode_round_trip

pytestmark = pytest.mark.gpu

Q = 16
FRAMES = 4  # I + 3 P: at R = 4 the last frame reads all three references


@pytest.mark.parametrize("size", [(16, 16), (64, 48), (200, 120)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_small_shapes(orc, cairo, size):
    _run(orc, cairo, "band4", size[0], size[1], 4, Q, FRAMES, FRAMES)


@pytest.mark.parametrize("ring", [2, 4], ids=["R2", "R4"])
def test_cif_references(orc, cairo, ring):
    _run(orc, cairo, "band4", 352, 288, ring, Q, FRAMES, FRAMES)


def test_cif_two_launches(orc, cairo):
    """Two frames per launch: the second launch's workers take the first
    launch's remaining tasks through its views too."""
    _run(orc, cairo, "band4", 352, 288, 4, Q, FRAMES, 2)


def test_cif_kept_reconstruction(orc, cairo):
    """keep_recon: the deblock stores every word to one mirror as well
    (npush = 1); the mirrors and the metrics are the oracle's."""
    w, h, ring = 352, 288, 4
    recs = _oracle_run(orc, "band4", w, h, ring, Q, FRAMES)
    ctx = cairo.Context(w, h, ring, stages=2 * FRAMES)
    try:
        ctx.set_metrics()
        ctx.set_batch(FRAMES)
        tks = [ctx.submit(r["rgb"], t, t > 0, Q) for t, r in enumerate(recs)]
        for t, tk in enumerate(tks):
            ctx.wait(tk)
            _check_ticket(ctx, tk, recs[t], w, h, f"CIF R={ring} frame {t}")
        for tk in tks:
            ctx.release(tk)
    finally:
        ctx.close()


def test_cif_decode_round_trip(orc, cairo):
    _decode_round_trip(orc, cairo, 352, 288, 4, Q, FRAMES)
