"""CPU side of the encode-side transform chain parity (tests/mb_cases.py,
tests/quant_ref.py, tests/test_gpu_mb_chain.py): the plain quantizer reference
against the oracle, the generator's numpy restatements against the oracle, and
the coverage of the crafted macroblocks and of the per-frame quality schedule,
each asserted from the oracle's own results.  `pytest -s` prints the counts
DESIGN.md §2.3 records."""
import functools
from collections import Counter

import numpy as np

from tests import mb_cases, quant_ref

P = lambda a: a.ctypes.data  # noqa: E731


def _luma16(blocks):
    y = np.empty((16, 16), np.int16)
    for b in range(4):
        y[(b >> 1) * 8:(b >> 1) * 8 + 8, (b & 1) * 8:(b & 1) * 8 + 8] = blocks[b]
    return y


def _blocks(y16, u, v):
    out = np.empty((6, 8, 8), np.int16)
    for b in range(4):
        out[b] = y16[(b >> 1) * 8:(b >> 1) * 8 + 8, (b & 1) * 8:(b & 1) * 8 + 8]
    out[4], out[5] = u, v
    return out


def oracle_chain(orc, src, pred, typ, quality):
    """One macroblock through the oracle: transform, VAQ, quantize, dequantize,
    inverse transform (+ prediction), as tests/test_gpu_parity.py::_oracle_chain
    -> (coefficients, quantized, reconstruction, qp, variance2)."""
    L = orc.lib()
    coef = np.zeros((6, 8, 8), np.int16)
    for b in range(6):
        s = np.ascontiguousarray(src[b])
        if typ == 1:
            L.orc_transform_8x8(P(s), 8, P(coef[b]), 8)
        else:
            p = np.ascontiguousarray(pred[b])
            L.orc_sub_transform_8x8(P(s), 8, P(p), 8, P(coef[b]), 8)
    y16 = _luma16(coef)
    qp = L.orc_vaq(quality, P(y16), 16)
    var = L.orc_variance2(P(y16), 16)
    quant, deq = _oracle_quant(orc, coef, typ, qp)
    rec = np.zeros((6, 8, 8), np.int16)
    for b in range(6):
        d = np.ascontiguousarray(deq[b])
        if typ == 1:
            L.orc_inverse_transform_8x8(P(d), 8, P(rec[b]), 8)
        else:
            p = np.ascontiguousarray(pred[b])
            L.orc_inverse_transform_add_8x8(P(d), 8, P(p), 8, P(rec[b]), 8)
    return coef, quant, rec, qp, var


def _oracle_quant(orc, coef, typ, qp):
    """orc_quantize_mb / orc_dequantize_mb on one (6, 8, 8) macroblock."""
    L = orc.lib()
    y16, u, v = _luma16(coef), np.ascontiguousarray(coef[4]), np.ascontiguousarray(coef[5])
    qy, qu, qv = np.zeros((16, 16), np.int16), np.zeros((8, 8), np.int16), np.zeros((8, 8), np.int16)
    L.orc_quantize_mb(qp, typ, P(y16), P(u), P(v), P(qy), P(qu), P(qv))
    dy, du, dv = np.zeros_like(qy), np.zeros_like(qu), np.zeros_like(qv)
    L.orc_dequantize_mb(qp, typ, P(qy), P(qu), P(qv), P(dy), P(du), P(dv))
    return _blocks(qy, qu, qv), _blocks(dy, du, dv)


@functools.lru_cache(maxsize=None)
def _oracle_results_cached():
    from oracle import oracle as orc

    src, pred, types, quals, names = mb_cases.stacked()
    n = len(names)
    out = {"coef": np.zeros((n, 6, 8, 8), np.int16), "quant": np.zeros((n, 6, 8, 8), np.int16),
           "rec": np.zeros((n, 6, 8, 8), np.int16), "qp": np.zeros(n, np.int32), "var": np.zeros(n, np.int32)}
    for m in range(n):
        c, q, r, qp, var = oracle_chain(orc, src[m], pred[m], int(types[m]), int(quals[m]))
        out["coef"][m], out["quant"][m], out["rec"][m], out["qp"][m], out["var"][m] = c, q, r, qp, var
    for a in out.values():
        a.setflags(write=False)
    return out


def oracle_results(group=None):
    """The oracle chain over mb_cases.cases(), computed once and left unchanged
    -> dict of arrays, of one group's macroblocks or of all."""
    res = _oracle_results_cached()
    if group is None:
        return res
    names = mb_cases.stacked()[4]
    sel = np.array([n.split("/")[0] == group for n in names])
    return {k: v[sel] for k, v in res.items()}


def _by_name(prefix):
    names = mb_cases.stacked()[4]
    return np.array([n.startswith(prefix) for n in names])


# ---------------------------------------------------------------------------
# quant_ref against the oracle
# ---------------------------------------------------------------------------

def test_quant_ref_matches_oracle(orc):
    """tests/quant_ref.py equals orc_quantize_mb / orc_dequantize_mb on 4 x 31 x
    32 macroblocks: all four types, every qp 1..31, and per (type, qp) the
    extreme values, small values around the dead zone, and noise of several
    amplitudes."""
    rng = np.random.default_rng(31)
    per = 32
    n = 0
    for typ in mb_cases.TYPES:
        for qp in range(1, 32):
            c = np.zeros((per, 6, 8, 8), np.int16)
            c[0], c[1], c[2], c[3] = 32767, -32768, 32766, -32767
            c[4] = rng.choice(np.array([-32768, 32767], np.int16), (6, 8, 8))
            for k in range(5, 12):  # around the inter dead zone qm * qp / 16 * (1 .. 3) and the rounding points
                c[k] = rng.integers(-4 * qp - 4, 4 * qp + 5, (6, 8, 8))
            for k in range(12, per):
                a = (1, 2, 4, 8, 16, 64, 256, 1024, 2200, 4096, 16384, 32767)[(k - 12) % 12]
                c[k] = rng.integers(-a, a + 1, (6, 8, 8))
            want = [_oracle_quant(orc, c[m], typ, qp) for m in range(per)]
            got_q = quant_ref.quantize(c.reshape(per, 384), typ, qp).reshape(per, 6, 8, 8)
            np.testing.assert_array_equal(got_q, np.stack([w[0] for w in want]), err_msg=f"quantize type {typ} qp {qp}")
            got_d = quant_ref.dequantize(got_q.reshape(per, 384), typ, qp).reshape(per, 6, 8, 8)
            np.testing.assert_array_equal(got_d, np.stack([w[1] for w in want]), err_msg=f"dequantize type {typ} qp {qp}")
            n += per
    assert n == 4 * 31 * per


def test_reciprocal_division_is_exact():
    """What quant_elem's comment claims, by brute force: mulhi(u, ceil(2^32 / d))
    == u / d for every u < 2^21 and every divisor 2..62."""
    u = np.arange(1 << 21, dtype=np.uint64)
    for d in range(2, 63):
        m = np.uint64(0xFFFFFFFF // d + 1)
        assert np.array_equal((u * m) >> np.uint64(32), u // np.uint64(d)), d


# ---------------------------------------------------------------------------
# the generator's restatements and its coverage, from the oracle's results
# ---------------------------------------------------------------------------

def test_restatements_match_oracle(orc):
    """mb_cases' numpy transform, variance and VAQ (which place the cases and
    define the narrowing classes below) equal the oracle on every case."""
    src, pred, types, quals, names = mb_cases.stacked()
    res = oracle_results()
    for t in mb_cases.TYPES:
        m = types == t
        coef = mb_cases.fdct(mb_cases.residual(src[m], pred[m], t))
        np.testing.assert_array_equal(coef, res["coef"][m], err_msg=f"fdct type {t}")
    v2, _ = mb_cases.variance2(res["coef"])
    np.testing.assert_array_equal(v2, res["var"])
    np.testing.assert_array_equal(mb_cases.vaq_qp(quals, mb_cases.vaq_idx(v2)), res["qp"])


def test_ladder_coverage(orc):
    """Every (type, quality, idx) triple occurs in the ladder, hence every
    (type, qp) for qp 1..23, and no other qp is reachable."""
    src, pred, types, quals, names = mb_cases.stacked()
    res = oracle_results()
    sel = _by_name("ladder/")
    idx = mb_cases.vaq_idx(res["var"])
    triples = Counter(zip(types[sel].tolist(), quals[sel].tolist(), idx[sel].tolist()))
    want = {(t, q, k) for t in mb_cases.TYPES for q in mb_cases.QUALITIES for k in mb_cases.IDX}
    assert set(triples) == want, sorted(want - set(triples))[:10]
    pairs = Counter(zip(types[sel].tolist(), res["qp"][sel].tolist()))
    assert set(pairs) == {(t, qp) for t in mb_cases.TYPES for qp in range(1, 24)}
    # the whole reachable set: the same from the formula over every quality and class
    reach = {int(mb_cases.vaq_qp(q, k)) for q in mb_cases.QUALITIES for k in mb_cases.IDX}
    assert reach == set(range(1, 24))
    print(f"\nladder: {int(sel.sum())} macroblocks, {len(triples)} (type, quality, idx) triples, "
          f"{len(pairs)} (type, qp) pairs; per pair {min(pairs.values())}..{max(pairs.values())} macroblocks")
    allp = Counter(zip(types.tolist(), res["qp"].tolist()))
    print(f"all cases: {len(types)} macroblocks, qp {min(q for _, q in allp)}..{max(q for _, q in allp)}")


def test_vaq_edges(orc):
    """Each VAQ edge occurs in every type, computed from the oracle's
    coefficients in wide integers."""
    src, pred, types, quals, names = mb_cases.stacked()
    res = oracle_results()
    t = mb_cases.luma_counted(res["coef"])
    count, total, sumsq = (t != 0).sum(1), t.sum(1), (t * t).sum(1)
    first = res["coef"][:, 0, 0, 0]
    var = res["var"].astype(np.int64)
    props = {
        "vaq/count0": (count == 0),
        "vaq/count0 with the skipped coefficient set": (count == 0) & (first != 0),
        "vaq/one": (count == 1),
        "vaq/sum_wrap": (np.abs(total) >= 46341),
        "vaq/sumsq_wrap": (sumsq >= 1 << 32),
        "vaq/negative": (var < 0),
    }
    print()
    for name, prop in props.items():
        sel = _by_name(name.split(" ")[0])
        for typ in mb_cases.TYPES:
            assert (sel & prop & (types == typ)).any(), (name, typ)
        print(f"{name}: {int((sel & prop).sum())} macroblocks ({int(prop.sum())} among all cases)")
    assert (res["var"][_by_name("vaq/count0") | _by_name("vaq/one")] == 0).all()
    # variance2 within +-1 of 4^k
    found = {}
    for k in range(1, 16):
        near = np.abs(var - 4 ** k) <= 1
        sel = np.array([n == f"vaq/pow4_{k}" for n in names])
        if sel.any():
            assert (near[sel]).all(), k
            for typ in mb_cases.TYPES:
                assert (sel & (types == typ)).any(), (k, typ)
        if near.any():
            found[k] = sorted({int(v) - 4 ** k for v in var[near]})
    assert set(mb_cases.POW4) <= set(found)
    print("variance2 within +-1 of 4^k, k: offsets =", found)


def test_narrowing_classes(orc):
    """Each narrowing class holds what its name says, from the wide-integer
    row and column passes (whose narrowed result the oracle pins above)."""
    src, pred, types, quals, names = mb_cases.stacked()
    n = len(names)
    r = np.stack([mb_cases.residual(src[m], pred[m], int(types[m])) for m in range(n)])
    row = mb_cases.row_pass_wide(r)
    col = mb_cases.col_pass_wide(r)
    out16 = lambda a: ((a < -32768) | (a > 32767)).reshape(n, -1).any(1)  # noqa: E731
    wide_res = src.astype(np.int64) - pred.astype(np.int64)
    sign = np.where(np.indices((6, 8, 8)).sum(0) % 2 == 0, 1, -1)
    props = {
        "narrow/max": (r == 32767).reshape(n, -1).all(1),
        "narrow/min": (r == -32768).reshape(n, -1).all(1),
        "narrow/checker": ((r == 32767 * sign) | (r == -32767 * sign)).reshape(n, -1).all(1),
        "narrow/residual_wrap": (types != 1) & out16(wide_res),
        "narrow/rowpass": out16(row),
        "narrow/colpass": ~out16(row) & out16(col),
    }
    print()
    for name, prop in props.items():
        sel = _by_name(name)
        assert sel.any() and prop[sel].all(), name
        for typ in mb_cases.TYPES:
            if not (name == "narrow/residual_wrap" and typ == 1):
                assert (sel & (types == typ)).any(), (name, typ)
        print(f"{name}: {int(sel.sum())} macroblocks ({int(prop.sum())} among all cases)")
    # both signs of the row-pass overflow, and an overflow of the row pass's DC and of another frequency
    sel = _by_name("narrow/rowpass")
    assert (row[sel] > 32767).any() and (row[sel] < -32768).any()
    assert (np.abs(row[..., 0]) > 32768).any() and (np.abs(row[..., 1:]) > 32768).any()


def test_single_coefficient_coverage(orc):
    """All 2 paths x 64 positions x {luma, chroma}: the oracle's quantized
    macroblock holds that position alone, and the DC beside it on the intra path."""
    src, pred, types, quals, names = mb_cases.stacked()
    res = oracle_results()
    seen = set()
    for m in np.flatnonzero(_by_name("single/")):
        path, plane = names[m].split("/")[1].split("_")
        nz = res["quant"][m].reshape(6, 64) != 0
        blocks = np.flatnonzero(nz.any(1))
        assert blocks.size == 1, names[m]
        b = int(blocks[0])
        assert (b < 4) == (plane == "luma")
        pos = np.flatnonzero(nz[b])
        assert int(types[m]) == dict(mb_cases.SINGLE_PATHS)[path]
        if path == "intra":
            assert pos[0] == 0 and pos.size <= 2, (names[m], pos)
        else:
            assert pos.size == 1, (names[m], pos)
        seen.add((path, plane, int(pos[-1])))
    assert seen == {(p, pl, k) for p, _ in mb_cases.SINGLE_PATHS for pl in ("luma", "chroma") for k in range(64)}
    print(f"\nsingle coefficient: {len(seen)} (path, plane, position) cases; qualities "
          f"{sorted(set(quals[_by_name('single/')].tolist()))}, qp {sorted(set(res['qp'][_by_name('single/')].tolist()))}")


def test_content_range(orc):
    """The old KAT's draw is contained: a few hundred macroblocks of src
    16..271 and pred -200..600 over all four types."""
    src, pred, types, quals, names = mb_cases.stacked()
    assert sorted({n.split("/")[0] for n in names}) == sorted(mb_cases.GROUPS)
    sel = _by_name("content/")
    assert sel.sum() >= 300 and set(types[sel].tolist()) == set(mb_cases.TYPES)
    body = np.flatnonzero(sel)[4:]
    assert src[body].min() >= 16 and src[body].max() <= 271 and pred[body].min() >= -200 and pred[body].max() < 600
    res = oracle_results()
    print(f"\ncontent: {int(sel.sum())} macroblocks, {len(set(zip(types[sel].tolist(), res['qp'][sel].tolist())))} (type, qp) pairs")


def test_quant_values():
    """The quantizer test's values: every |c| <= 4096, steps of 61 beyond, both ends."""
    v = mb_cases.quant_values().astype(np.int64)
    assert v[0] == -32768 and v[-1] == 32767 and np.all(np.diff(v) > 0) and np.diff(v).max() <= 61
    assert set(range(-4096, 4097)) <= set(v.tolist()) and 9000 < v.size < 9200
    print(f"\nquantizer values: {v.size}")


# ---------------------------------------------------------------------------
# the per-frame quality schedule of the engine test
# ---------------------------------------------------------------------------

def _mb_block_flags(y, u, v):
    """(hmb * wmb, 6) bool: has the block a non-zero coefficient."""
    hmb, wmb = y.shape[0] // 16, y.shape[1] // 16
    fy = (y.reshape(hmb, 2, 8, wmb, 2, 8) != 0).any((2, 5)).transpose(0, 2, 1, 3).reshape(hmb * wmb, 4)
    fu = (u.reshape(hmb, 8, wmb, 8) != 0).any((1, 3)).reshape(hmb * wmb, 1)
    fv = (v.reshape(hmb, 8, wmb, 8) != 0).any((1, 3)).reshape(hmb * wmb, 1)
    return np.concatenate([fy, fu, fv], 1)


def test_engine_schedule_coverage(orc):
    """What tests/test_gpu_mb_chain.py's per-frame quality runs reach, from the
    oracle's block tables and coefficient planes: types 0..3 at every qp 1..20
    (21 too for types 1 and 3), coded macroblocks with some but not all
    quantized blocks zero in every type, all-zero coded macroblocks in types
    0, 2 and 3."""
    pairs, partial, allzero, coded = Counter(), Counter(), Counter(), Counter()
    peak = 0
    for kind in mb_cases.engine_kinds():
        for w, h in mb_cases.ENGINE_SIZES:
            for run, quals in mb_cases.ENGINE_RUNS:
                e = orc.OracleEncoder(mb_cases.ENGINE_RING)
                for t, q in enumerate(quals):
                    if run == "intra":
                        e.insert_intra()
                    e.set_quality(q)
                    e.encode(mb_cases.engine_frame(orc, kind, w, h, t))
                    table = e.block_table()
                    flags = _mb_block_flags(*e.planes(1))
                    y = e.planes(0)[0]
                    peak = max(peak, int(np.abs(mb_cases.fdct(
                        y.reshape(y.shape[0] // 8, 8, y.shape[1] // 8, 8).transpose(0, 2, 1, 3))).max()))
                    for d, f in zip(table, flags):
                        typ = int(d["block_type"])
                        if typ & 4:
                            continue
                        coded[typ] += 1
                        pairs[(typ, int(d["q_index"]))] += 1
                        if not f.any():
                            allzero[typ] += 1
                        elif not f.all():
                            partial[typ] += 1
    print(f"\nengine schedule: coded {dict(sorted(coded.items()))}\n  partly zero {dict(sorted(partial.items()))}"
          f"\n  all zero {dict(sorted(allzero.items()))}\n  largest |coefficient| of the intra transform of an input frame: {peak}")
    for typ in mb_cases.TYPES:
        got = sorted(q for t, q in pairs if t == typ)
        print(f"  type {typ}: qp {got}")
        top = 21 if typ in (1, 3) else 20
        assert got == list(range(1, top + 1)), (typ, got)
        assert partial[typ] >= 180, (typ, partial[typ])
        if typ != 1:  # (an intra block's DC carries its mean: never all zero on 8-bit content)
            assert allzero[typ] >= 290, (typ, allzero[typ])
