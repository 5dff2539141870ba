"""GPU parity of the intra search with per-lane candidate geometry.

The row coder takes a group's candidate from per-lane unit offsets scaled by
the pass's step, the replay reads the coordinates the group stored beside its
(sad, mad), the source's own SAD is a packed sum against the bias, and the
sub-pel lerp takes half or quarter as data.  A wrong slot, step, stored
coordinate or lerp changes a macroblock's motion vector, type, sub-pel fields
or SAD, so the block tables and the inter records are compared field by field
with the oracle, as tests/test_gpu_intra_speculation.py does.

Sizes: 64x48 (4x3 macroblocks) and 72x40 (padded to 5x3, ragged) put nearly
every macroblock on a frame edge, where candidates are out of frame or not yet
coded; 160x64 is 10x4 macroblocks, so the coder's 128-column circular window
wraps (cx & 127) and row 3 takes the by >= 3 prefetch path.  Content: band4
plus every kind of tests/content.py ("ties" for the SSD and index rules,
"gradient" for the sub-pel, "black" / "white" / "static" for copy mode and the
MAD gate, "pan" and "noise" for out-of-reach candidates), q = 1, 16, 31,
R = 4, I + 3 P.
"""
import numpy as np
import pytest

from tests import content

pytestmark = pytest.mark.gpu

SIZES = [(64, 48), (72, 40), (160, 64)]
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
