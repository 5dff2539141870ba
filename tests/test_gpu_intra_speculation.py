"""GPU parity of the intra search's speculated stages.

The row coder evaluates a stage's 8 non-centre candidates in lane groups 0..7
and, in groups 8..15, the next stage's candidates as they are if the stage
keeps its centre; the replay reuses them when it did and drops them when it
did not.  A wrong reuse, a wrong discard or a centre that should have been
kept as a candidate changes a macroblock's motion vector, type or SAD, so the
block tables and the inter records are compared field by field with the
oracle, as tests/test_gpu_parity.py does.

Sizes: 64x48 (4x3 macroblocks) and 72x40 (padded to 5x3) put most macroblocks
on a frame edge, where speculated candidates are out of frame or not yet coded
while the stage's own are valid, and the reverse; CIF has every stay/move
pattern of stages 1-4 on band4.  Content: every kind of tests/content.py plus
band4 ("ties" for the SSD and index tie-breaks without the centre; "black",
"white" and "static" for copy mode and the MAD gate), q = 1, 16, 31, R = 4,
I + 3 P.
"""
import numpy as np
import pytest

from tests import content

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (72, 40), (352, 288)]
KINDS = ("band4",) + content.KINDS
QUALITIES = (1, 16, 31)
RING, FRAMES = 4, 4


def _table_equal(a, b, what):
    for f in a.dtype.names:
        if f == "pad":
            continue
        bad = np.nonzero(a[f] != b[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at MBs {bad[:10]} gpu={a[f][bad[:5]]} ref={b[f][bad[:5]]}"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_tables_match_oracle(orc, cairo, w, h, kind):
    gen = orc.make_frame if kind == "band4" else (lambda w_, h_, t: content.make(kind, w_, h_, t))
    frames = [gen(w, h, t) for t in range(FRAMES)]
    for q in QUALITIES:
        e = orc.OracleEncoder(RING)
        e.set_quality(q)
        ctx = cairo.Context(w, h, RING)
        ctx.set_debug(1)
        for t, rgb in enumerate(frames):
            e.encode(rgb)
            out = ctx.encode_frame(rgb, t, t > 0, q)
            tag = f"{kind} {w}x{h} q={q} frame {t}"
            if t > 0:
                gd, gs = ctx.read_inter()
                od, os_ = e.inter_records()
                _table_equal(gd, od, f"{tag}: inter records")
                np.testing.assert_array_equal(gs, os_, err_msg=f"{tag}: inter SAD")
            _table_equal(out.table, e.block_table(), f"{tag}: block table")
        ctx.close()
