"""GPU parity of the decode-mode engine (code_row<kDecode>, pred_global, the
window read, dequantize, inverse transform, deblock) on synthetic block tables
(tests/tables.py) against the oracle decoder (orc_decode_frame): the planes
before the deblock, the ring slot after it and the RGB frame, exact, frame by
frame.  The tables hold what a stream can legally carry and the encoder's own
search hardly ever picks; tests/test_tables.py asserts what they cover."""
import numpy as np
import pytest

from tests import tables
from tests.test_tables import CONFIGS, FRAMES, SEEDS

pytestmark = pytest.mark.gpu

_oracle_runs = {}


def _oracle(orc, cairo, w, h, ring, seed):
    """The sequence and the oracle's decode of it, computed once and not changed:
    [(table, coef, pre-deblock planes, slot planes, rgb)]."""
    key = (w, h, ring, seed)
    if key not in _oracle_runs:
        d = orc.OracleDecoder(w, h, ring)
        run = []
        for t, (table, coef) in enumerate(tables.make_sequence(w, h, ring, FRAMES, seed)):
            d.decode(table, coef)
            slot = d.planes(2 + t % ring)
            run.append((table, coef, d.predeblock(), slot, cairo.yuv_to_rgb(*slot, w, h)))
        _oracle_runs[key] = run
    return _oracle_runs[key]


def _decode(cairo, w, h, ring, run):
    """The sequence through a fresh context -> [(pre-deblock planes, slot planes, rgb)]."""
    ctx = cairo.Context(w, h, ring=ring, stages=2)
    out = []
    try:
        ctx.set_debug(1)
        for t, (table, coef, *_) in enumerate(run):
            assert cairo.table_check(table, ctx.wmb, ctx.hmb, ring)  # (decode_frame refuses it otherwise)
            rgb = ctx.decode_frame(table, coef, t)
            out.append((ctx.read_predeblock(), ctx.read_planes(2 + t % ring), rgb))
    finally:
        ctx.close()
    return out


def _first_difference(got, want, table, wmb, sub):
    """The first macroblock (raster order) where two planes differ, and its desc."""
    ys, xs = np.nonzero(got != want)
    k = int(np.argmin((ys // sub) * wmb + xs // sub))
    mb = int((ys[k] // sub) * wmb + xs[k] // sub)
    return f"macroblock {mb} = ({mb % wmb}, {mb // wmb}), desc {table[mb]}, {ys.size} samples differ"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("w,h,ring", CONFIGS)
def test_decode_tables_match_oracle(orc, cairo, w, h, ring, seed):
    run = _oracle(orc, cairo, w, h, ring, seed)
    wmb = (w + 15) // 16
    for t, ((table, _, pre, slot, rgb), (gpre, gslot, grgb)) in enumerate(zip(run, _decode(cairo, w, h, ring, run))):
        for stage, got, want in (("pre-deblock", gpre, pre), ("slot", gslot, slot)):
            for k, n in enumerate("YUV"):
                if not np.array_equal(got[k], want[k]):
                    pytest.fail(f"{w}x{h} R={ring} seed {seed} frame {t} {stage} {n}: "
                                + _first_difference(got[k], want[k], table, wmb, 16 if k == 0 else 8))
        np.testing.assert_array_equal(grgb, rgb, err_msg=f"{w}x{h} R={ring} seed {seed} frame {t} RGB")


def test_decode_tables_deterministic(orc, cairo):
    """Two fresh contexts give the same planes: no read of a cell another
    workgroup may still be writing decides a legal table's reconstruction."""
    run = _oracle(orc, cairo, 352, 288, 4, SEEDS[0])
    a, b = _decode(cairo, 352, 288, 4, run), _decode(cairo, 352, 288, 4, run)
    for t, ((apre, aslot, argb), (bpre, bslot, brgb)) in enumerate(zip(a, b)):
        for x, y in zip(apre + aslot + (argb,), bpre + bslot + (brgb,)):
            np.testing.assert_array_equal(x, y, err_msg=f"frame {t}")
