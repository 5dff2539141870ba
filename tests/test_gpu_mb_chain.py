"""GPU parity of the encode side of the transform chain (fdct_lane, vaq_mb,
quant_elem, dequant_elem, idct_lane) at every quality, variance class and
coefficient.  Exact integer parity throughout.

  chain      every macroblock of tests/mb_cases.py through cairo_kat_transform
             against the oracle: qp, variance2, quantized coefficients and the
             reconstruction (tests/test_mb_cases.py asserts what the cases cover)
  quantizer  cairo_kat_quant, the engine's quant_elem / dequant_elem alone, at
             every qp 1..31 over some 9 100 coefficient values against the plain
             reference tests/quant_ref.py
  engine     the engine itself with a quality per frame, as a rate-controlled
             context runs it, against the oracle: its all-zero shortcuts around
             the transforms and the block table's narrowed variance, which the
             KAT kernels do not share
"""
import numpy as np
import pytest

from tests import mb_cases, quant_ref
from tests.test_mb_cases import oracle_results

pytestmark = pytest.mark.gpu
P = lambda a: a.ctypes.data  # noqa: E731


# ---------------------------------------------------------------------------
# The chain
# ---------------------------------------------------------------------------

def _first_difference(got, want):
    m, b, k = (int(x) for x in np.argwhere(got.reshape(len(got), 6, 64) != want.reshape(len(want), 6, 64))[0])
    return m, b, k


@pytest.mark.parametrize("group", mb_cases.GROUPS)
def test_chain(orc, cairo, group):
    src, pred, types, quals, names = mb_cases.stacked(group)
    want = oracle_results(group)
    n = len(names)
    qtype = np.ascontiguousarray(np.stack([types, quals], 1).astype(np.uint8))
    coef, rec = np.zeros((n, 6, 8, 8), np.int16), np.zeros((n, 6, 8, 8), np.int16)
    qv = np.zeros((n, 2), np.int32)
    assert cairo.lib().cairo_kat_transform(P(src), P(pred), P(qtype), n, P(coef), P(rec), P(qv), 0) == 0
    tag = lambda m: f"{names[m]} (macroblock {m} of group {group}): type {types[m]}, quality {quals[m]}"  # noqa: E731
    for what, got, ref in (("qp", qv[:, 0], want["qp"]), ("variance2", qv[:, 1], want["var"])):
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, f"{what} of {tag(bad[0])}: gpu {got[bad[0]]}, oracle {ref[bad[0]]} ({bad.size} differ)"
    for what, got, ref in (("quantized coefficient", coef, want["quant"]), ("reconstruction", rec, want["rec"])):
        if not np.array_equal(got, ref):
            m, b, k = _first_difference(got, ref)
            bad = int((got != ref).reshape(n, -1).any(1).sum())
            raise AssertionError(f"{what} of {tag(m)}, qp {want['qp'][m]}: first difference at macroblock {m}, block {b}, "
                                 f"position {k}: gpu {got[m].reshape(6, 64)[b, k]}, oracle {ref[m].reshape(6, 64)[b, k]} "
                                 f"({bad} macroblocks differ)")


# ---------------------------------------------------------------------------
# The quantizer, near-exhaustive
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def quant_input():
    """Macroblock m holds one value at all 384 elements: every value as type 1
    and as type 0, |c| <= 512 as types 2 and 3 (which path each type takes)."""
    v = mb_cases.quant_values()
    small = v[np.abs(v.astype(np.int32)) <= 512]
    vals = np.concatenate([v, v, small, small])
    types = np.concatenate([np.full(v.size, 1), np.full(v.size, 0), np.full(small.size, 2), np.full(small.size, 3)])
    coef = np.ascontiguousarray(np.repeat(vals[:, None], 384, 1))
    coef.setflags(write=False)
    return coef, types.astype(np.uint8)


@pytest.mark.parametrize("qp", range(1, 32))
def test_quantizer(cairo, quant_input, qp):
    coef, types = quant_input
    quant, dequant = cairo.kat_quant(coef, types, qp)
    for typ in mb_cases.TYPES:
        m = types == typ
        want_q = quant_ref.quantize(coef[m], typ, qp)
        want_d = quant_ref.dequantize(want_q, typ, qp)
        for what, got, ref in (("quant", quant[m], want_q), ("dequant", dequant[m], want_d)):
            if not np.array_equal(got, ref):
                r, e = (int(x) for x in np.argwhere(got != ref)[0])
                raise AssertionError(f"{what} type {typ} qp {qp}: c = {coef[m][r, e]} at block {e >> 6} position {e & 63}: "
                                     f"gpu {got[r, e]}, reference {ref[r, e]} ({int((got != ref).sum())} elements differ)")


def test_kat_quant_refuses_bad_arguments(cairo):
    L = cairo.lib()
    c, q, d = np.zeros((2, 384), np.int16), np.zeros((2, 384), np.int16), np.zeros((2, 384), np.int16)
    bad = cairo.EVX_ERROR_INVALID_ARGS

    def call(tq, coef=c, count=2, quant=q, dequant=d):
        tq = np.array(tq, np.uint8)
        return L.cairo_kat_quant(P(coef) if coef is not None else None, P(tq), count,
                                 P(quant) if quant is not None else None, P(dequant) if dequant is not None else None, 0)

    ok = [[1, 1], [0, 31]]
    assert call(ok) == 0
    assert call(ok, coef=None) == bad and call(ok, quant=None) == bad and call(ok, dequant=None) == bad
    assert L.cairo_kat_quant(P(c), None, 2, P(q), P(d), 0) == bad
    assert call(ok, count=0) == bad and call(ok, count=-1) == bad
    assert call([[1, 1], [0, 0]]) == bad and call([[1, 32], [0, 1]]) == bad and call([[1, 1], [0, 255]]) == bad  # qp
    for typ in (4, 5, 6, 7):  # the copy bit
        assert call([[1, 1], [typ, 8]]) == bad


# ---------------------------------------------------------------------------
# The engine at every quality
# ---------------------------------------------------------------------------

def _table_equal(a, b, what):
    for f in a.dtype.names:
        if f == "pad":
            continue
        bad = np.nonzero(a[f] != b[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at MBs {bad[:10]} gpu={a[f][bad[:5]]} ref={b[f][bad[:5]]}"


def _planes_equal(got, want, what):
    for g, o, n in zip(got, want, "YUV"):
        np.testing.assert_array_equal(g, o, err_msg=f"{what} {n}")


@pytest.mark.parametrize("size", mb_cases.ENGINE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", mb_cases.engine_kinds())
def test_engine_quality_per_frame(orc, cairo, kind, size):
    """An intra-only run at qualities 1..31 and an I + 31 P run whose quality
    changes every frame (mb_cases.ENGINE_RUNS), compared per frame as
    tests/test_gpu_parity.py::_run_frames compares."""
    w, h = size
    ring = mb_cases.ENGINE_RING
    for run, quals in mb_cases.ENGINE_RUNS:
        e = orc.OracleEncoder(ring)
        ctx = cairo.Context(w, h, ring)
        try:
            ctx.set_debug(1)
            for t, q in enumerate(quals):
                rgb = mb_cases.engine_frame(orc, kind, w, h, t)
                inter = run == "ip" and t > 0
                if run == "intra":
                    e.insert_intra()
                e.set_quality(q)
                e.encode(rgb)
                out = ctx.encode_frame(rgb, t, inter, q)
                tag = f"{kind} {w}x{h} {run} run, frame {t}, quality {q}"
                if inter:
                    gd, gs = ctx.read_inter()
                    od, os_ = e.inter_records()
                    _table_equal(gd, od, f"{tag}: inter records")
                    np.testing.assert_array_equal(gs, os_, err_msg=f"{tag}: inter SAD")
                _table_equal(out.table, e.block_table(), f"{tag}: block table")
                _planes_equal((out.coef_y, out.coef_u, out.coef_v), e.planes(1), f"{tag}: coefficients")
                _planes_equal(ctx.read_predeblock(), e.predeblock(), f"{tag}: reconstruction before the deblock")
                slot = 2 + t % ring
                _planes_equal(ctx.read_planes(slot), e.planes(slot), f"{tag}: deblocked reconstruction")
        finally:
            ctx.close()
