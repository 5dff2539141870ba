"""CPU side of the decode-mode parity on synthetic block tables
(tests/tables.py, tests/test_gpu_decode_tables.py): the legality predicate
against a plain restatement, the generator's coverage, the oracle decoder in
closed loop with the oracle encoder, the host entropy round trip on synthetic
tables, rejection of illegal tables, and the host decode path and the oracle
decoder as stand-alone programs under AddressSanitizer / UBSan."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import content, tables

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (width, height, ring): what tests/test_gpu_decode_tables.py decodes, six frames, seeds 1 and 2
CONFIGS = ((16, 16, 2), (48, 64, 3), (208, 128, 4), (352, 288, 2), (352, 288, 4))
FRAMES, SEEDS = 6, (1, 2)


def _mbs(w, h):
    return (w + 15) // 16, (h + 15) // 16


# ---------------------------------------------------------------------------
# The predicate (cairo_table_check / cairo_desc_check) against the rules as
# the reference states them.
# ---------------------------------------------------------------------------

def _legal(t, q, target, mx, my, sp, amount, index, bx, by, wmb, hmb, ring):
    """The legal set, restated (arrays broadcast).  decode.cpp:14-142: seven
    types.  quantize.cpp:65-68: q_index 1..31 where there are coefficients.
    encode.cpp:17-67: inter targets 1..R-1.  motion.cpp:225-275, 277-352:
    candidates in frame; for intra ones :238-241 and :303-306 skip y > py-16
    && x > px-16, and the search reaches 32 px sideways, 48 up, 16 down."""
    t, q, target, mx, my, sp, amount, index, bx, by = np.broadcast_arrays(t, q, target, mx, my, sp, amount, index, bx, by)
    intra, motion, copy = (t & 1) != 0, (t & 2) != 0, (t & 4) != 0
    ok = (t <= 7) & (t != 5)
    ok &= copy | ((q >= 1) & (q <= 31))
    ok &= intra | ((target >= 1) & (target <= ring - 1))
    ok &= ~motion | (sp == 0) | ((sp == 1) & (amount <= 1) & (index <= 7))
    dirs = np.array(tables.SP_DIR)
    px, py = bx * 16, by * 16

    def point_ok(x, y):
        inside = (x >= 0) & (x + 16 <= wmb * 16) & (y >= 0) & (y + 16 <= hmb * 16)
        reach = (abs(x - px) <= 32) & (y >= py - 48) & (y <= py + 16)
        coded = ~((y > py - 16) & (x > px - 16))
        return inside & (~intra | (reach & coded))

    x0, y0 = px + mx, py + my
    d = dirs[np.minimum(index, 7)]
    pts = point_ok(x0, y0) & ((sp != 1) | point_ok(x0 + d[..., 0], y0 + d[..., 1]))
    return ok & (~motion | pts)


def _descs(t, q, target, mx, my, sp, amount, index):
    arrs = np.broadcast_arrays(t, q, target, mx, my, sp, amount, index)
    d = np.zeros(arrs[0].shape, tables.BLOCK_DESC)
    for name, a in zip(("block_type", "q_index", "prediction_target", "motion_x", "motion_y", "sp_pred", "sp_amount",
                        "sp_index"), arrs):
        d[name] = a
    return d


VEC = np.arange(-80, 81)
# every value at which a rule changes, for a 5x4 frame (x to +-64, y to +-48) and the window, and one beyond
EDGE_VEC = np.array(sorted({s * v for s in (-1, 1) for v in (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80)}))


def test_predicate_matches_restatement(cairo):
    """Exhaustive on a 5x4-macroblock frame, at every macroblock.  The full
    product of the ranges is 4e9 descs; it is taken in two slices.
    (a) every type x every vector in [-80, 80]^2 x sp off and the 16 settings,
    with ring 4, target 1, q 1: the geometry, which depends on nothing else.
    (b) every type x rings 2-4 x targets 0-4 x q in {0, 1, 31, 32} x sp off
    and the 16 settings x the vectors whose components are rule boundaries."""
    wmb, hmb = 5, 4
    mb = np.arange(wmb * hmb, dtype=np.uint32)
    sps = [(0, 0, 0)] + [(1, a, i) for a in (0, 1) for i in range(8)]
    n = accepted = 0

    def compare(ring, t, q, target, mx, my, sp, a, i):
        """Fields broadcast against each other behind a leading macroblock axis."""
        nonlocal n, accepted
        f = [np.asarray(v, np.int64) for v in (t, q, target, mx, my, sp, a, i)]
        nd = max(v.ndim for v in f)
        shape = (mb.size,) + np.broadcast_shapes(*[v.shape for v in f])
        f = [np.broadcast_to(v.reshape((1,) * (nd - v.ndim) + v.shape), shape[1:])[None] for v in f]
        idx = mb.reshape((-1,) + (1,) * nd)
        want = np.broadcast_to(_legal(*f, (idx % wmb).astype(np.int64), (idx // wmb).astype(np.int64), wmb, hmb, ring), shape)
        d = np.broadcast_to(_descs(*f), shape)
        got = cairo.desc_check(np.ascontiguousarray(d).reshape(-1), np.ascontiguousarray(np.broadcast_to(idx, shape)).reshape(-1),
                               wmb, hmb, ring).reshape(shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (d[tuple(bad[0])], int(bad[0][0]), ring, bool(want[tuple(bad[0])]))
        n += got.size
        accepted += int(got.sum())

    for t in range(8):
        for sp, a, i in sps:  # (a)
            compare(4, t, 1, 1, VEC[:, None], VEC[None, :], sp, a, i)
    tg = np.arange(5).reshape(5, 1, 1, 1)
    qs = np.array([0, 1, 31, 32]).reshape(1, 4, 1, 1)
    for t in range(8):
        for ring in (2, 3, 4):
            for sp, a, i in sps:  # (b)
                compare(ring, t, qs, tg, EDGE_VEC.reshape(1, 1, -1, 1), EDGE_VEC.reshape(1, 1, 1, -1), sp, a, i)
    assert n > 90_000_000 and 0 < accepted < n // 4
    # a table is legal exactly when each desc is, at its own macroblock
    rng = np.random.default_rng(5)
    for _ in range(300):
        t = tables.make_table(wmb, hmb, 4, 1, int(rng.integers(1 << 30)))
        assert cairo.table_check(t, wmb, hmb, 4)
        k = int(rng.integers(t.size))
        t[k]["block_type"] = 5
        assert not cairo.table_check(t, wmb, hmb, 4) and cairo.desc_check(t, mb, wmb, hmb, 4).sum() == t.size - 1
    # sp_pred, sp_amount and sp_index beyond their ranges on a motion type
    base = tables.make_table(wmb, hmb, 4, 1, 3)
    k = int(np.flatnonzero((base["block_type"] & 2) != 0)[0])
    for f, v in (("sp_pred", 2), ("sp_amount", 2), ("sp_index", 8)):
        t = base.copy()
        t[k]["sp_pred"] = 1
        t[k]["sp_index"] = 0 if f != "sp_index" else 8
        t[k][f] = v
        assert not cairo.table_check(t, wmb, hmb, 4), f


# ---------------------------------------------------------------------------
# Coverage of the sequences the GPU tests decode.
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sequences():
    return {(w, h, r, s): tables.make_sequence(w, h, r, FRAMES, s) for w, h, r in CONFIGS for s in SEEDS}


def test_generator_coverage(cairo, sequences):
    """Every directed class occurs in every sequence (frame 0 is intra only, so
    the inter and target classes come from frames 1-5), every table passes
    the predicate, frame 0 holds intra types only, and the coefficient planes
    hold all three kinds.  The single-macroblock frame must meet what one
    macroblock can hold (tables.SINGLE_MB_CLASSES says what that leaves out).
    `python -m tests.tables` prints the counts (decoder section)."""
    for (w, h, r, s), seq in sequences.items():
        wmb, hmb = _mbs(w, h)
        for t, (table, coef) in enumerate(seq):
            assert cairo.table_check(table, wmb, hmb, r), (w, h, r, s, t)
            assert t > 0 or np.all(table["block_type"] & 1)
            assert all(np.abs(p.astype(np.int32)).max() <= tables.COEF_PEAK for p in coef)
        n = tables.sequence_classes(seq, wmb, hmb)
        req = tables.SINGLE_MB_CLASSES if wmb * hmb == 1 else tables.required_classes(r, FRAMES)
        assert not req - set(n), (w, h, r, s, sorted(req - set(n)))
        if wmb * hmb > 1:
            y = np.concatenate([c[0].ravel() for _, c in seq]).astype(np.int32)
            assert (np.abs(y) == tables.COEF_PEAK).any() and (np.abs(y) > 1024).sum() > 1000 and (y == 0).mean() > 0.3


# ---------------------------------------------------------------------------
# The oracle decoder against the oracle encoder's own reconstruction.
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("band4",) + content.KINDS)
@pytest.mark.parametrize("ring", (2, 4))
def test_oracle_decoder_closed_loop(orc, kind, ring):
    """The reference is closed-loop: decode_slice over the encoder's block
    table and output_cache rebuilds the encoder's reconstruction (encode.cpp:196
    calls the same decode_block), before and after the deblock, bit for bit."""
    w, h = 176, 144
    e = orc.OracleEncoder(ring)
    e.set_quality(12)
    d = orc.OracleDecoder(w, h, ring)
    for t in range(5):
        e.encode(orc.make_frame(w, h, t) if kind == "band4" else content.make(kind, w, h, t))
        d.decode(e.block_table(), e.planes(1))
        for a, b, n in zip(d.predeblock(), e.predeblock(), "YUV"):
            np.testing.assert_array_equal(a, b, err_msg=f"{kind} R={ring} frame {t} pre-deblock {n}")
        for a, b, n in zip(d.planes(2 + t % ring), e.planes(2 + t % ring), "YUV"):
            np.testing.assert_array_equal(a, b, err_msg=f"{kind} R={ring} frame {t} slot {n}")
        assert d.dims()[3] == t + 1


# ---------------------------------------------------------------------------
# Host entropy round trip on the generator's tables.
# ---------------------------------------------------------------------------

def check_stream_fields(got, want, ring):
    """Every block-table field the stream carries for a block (unserialize.cpp:150-287)."""
    bt = want["block_type"]
    np.testing.assert_array_equal(got["block_type"], bt)
    inter, motion, copy = (bt & 1) == 0, (bt & 2) != 0, (bt & 4) != 0
    mask = (1 << (int(ring).bit_length() - 1)) - 1  # log2((uint8)R) target bits, serialize.cpp:179
    np.testing.assert_array_equal(got["prediction_target"][inter] & mask, want["prediction_target"][inter] & mask)
    for f in ("motion_x", "motion_y", "sp_pred"):
        np.testing.assert_array_equal(got[f][motion], want[f][motion], err_msg=f)
    sp = motion & (want["sp_pred"] != 0)
    for f in ("sp_amount", "sp_index"):
        np.testing.assert_array_equal(got[f][sp], want[f][sp], err_msg=f)
    np.testing.assert_array_equal(got["q_index"][~copy], want["q_index"][~copy])


def mb_mask(table, wmb, hmb, sel, sub):
    """Per-sample mask (luma sub = 16, chroma 8) of the macroblocks where sel holds."""
    return np.kron(sel.reshape(hmb, wmb), np.ones((sub, sub), bool))


def carried(table, coef, prev, wmb, hmb):
    """The coefficient planes as an encoder holds them: a copy macroblock keeps
    the previous frame's (zero before the first).  The DC of a block is coded
    against its neighbour's as stored (serialize.cpp:34-130), so only such
    planes make a stream the decoder's persistent planes can follow."""
    copy = (table["block_type"] & 4) != 0
    out = []
    for k, p in enumerate(coef):
        m = mb_mask(table, wmb, hmb, copy, 16 if k == 0 else 8)
        out.append(np.where(m, prev[k] if prev else 0, p).astype(np.int16))
    return out


def test_entropy_round_trip_synthetic(cairo, sequences):
    """unserialize_slice(serialize_slice(table, coef)) on the generator's
    sequences, into a persistent state as the decoder keeps it: every field the
    stream carries and every coefficient, a copy macroblock's being the ones it
    had before."""
    for (w, h, r, s), seq in sequences.items():
        wmb, hmb = _mbs(w, h)
        state = planes = want = None
        for t, (table, coef) in enumerate(seq):
            want = carried(table, coef, want, wmb, hmb)
            pay, nb = cairo.serialize_slice(table, wmb, hmb, r, *want)
            state, planes, used = cairo.unserialize_slice(pay, nb, wmb, hmb, r, state, planes)
            assert used == nb, (w, h, r, t)
            check_stream_fields(state, table, r)
            for k, (a, b) in enumerate(zip(planes, want)):
                np.testing.assert_array_equal(a, b, err_msg=f"{w}x{h} R{r} seed {s} frame {t} plane {k}")
            if r != 3:  # (one target bit for R = 3: a target 2 arrives as 0 and is refused)
                assert cairo.table_check(state, wmb, hmb, r)


# ---------------------------------------------------------------------------
# Rejection: a stream that breaks one rule is refused before any GPU call.
# ---------------------------------------------------------------------------

def test_illegal_streams_are_refused(cairo):
    """Tables that break one rule each, through serialize and unserialize as a
    stream would bring them: the predicate refuses each.  (sp_index 8 does not
    fit the stream's three bits.)  No such table goes to a GPU call."""
    wmb, hmb, ring = 5, 4, 4
    base = tables.make_table(wmb, hmb, ring, 2, 9)
    coef = tables.make_coef(wmb, hmb, 2, 9)
    mid, last = 2 * wmb + 2, 3 * wmb + 4  # macroblocks (2, 2) at (32, 32) and (4, 3) at (64, 48), the last one

    def d(t, q=5, target=1, mx=0, my=0, sp=None):
        r = np.zeros((), tables.BLOCK_DESC)
        r["block_type"], r["q_index"], r["prediction_target"], r["motion_x"], r["motion_y"] = t, q, target, mx, my
        if sp:
            r["sp_pred"], r["sp_amount"], r["sp_index"] = 1, sp[0], sp[1]
        return r

    cases = {
        "type 5": (mid, d(5)), "q_index 32": (mid, d(1, q=32)), "q_index 32 inter": (mid, d(2, q=32)),
        "q_index 0": (mid, d(1, q=0)),
        "left of the frame": (mid, d(2, mx=-33)), "right of the frame": (mid, d(2, mx=33)),
        "above the frame": (mid, d(2, my=-33)), "below the frame": (mid, d(2, my=17)),
        "neighbour left of the frame": (mid, d(2, mx=-32, sp=(0, 3))),
        "neighbour below the frame": (mid, d(2, my=16, sp=(1, 6))),
        "intra left of the frame": (mid, d(3, mx=-33, my=-16)),
        "intra beyond the window": (last, d(3, mx=-33, my=-16)),
        "intra neighbour beyond the window": (last, d(3, mx=-32, my=-16, sp=(0, 3))),
        "intra not yet coded: itself": (mid, d(3)),
        "intra not yet coded: one step inside, beside": (mid, d(3, mx=-15, my=-15)),
        "intra not yet coded: one step inside, below": (mid, d(3, mx=-15, my=16)),
        "intra neighbour not yet coded": (mid, d(3, mx=-16, my=-15, sp=(0, 4))),
        "intra neighbour not yet coded, from above": (mid, d(3, mx=16, my=-16, sp=(0, 6))),
        "inter target 0": (mid, d(2, target=0)), "inter target 0, no motion": (mid, d(0, target=0)),
        "copy target 0": (mid, d(4, target=0)),
    }
    assert cairo.table_check(base, wmb, hmb, ring)
    for name, (k, desc) in cases.items():
        t = base.copy()
        t[k] = desc
        pay, nb = cairo.serialize_slice(t, wmb, hmb, ring, *coef)
        got, _, used = cairo.unserialize_slice(pay, nb, wmb, hmb, ring)
        assert used == nb and got[k]["block_type"] == desc["block_type"], name
        assert not cairo.table_check(got, wmb, hmb, ring), name
        got[k] = base[k]  # and nothing else in it is wrong
        ok = cairo.desc_check(got, np.arange(got.size), wmb, hmb, ring)
        assert ok[(base["block_type"] & 4) == 0].all(), name
    k = mid
    # a stream of ring 3 that used target 2 arrives with target 0
    t = base.copy()
    t["prediction_target"] = np.minimum(t["prediction_target"], 2)
    t[k] = d(2, target=2)
    assert cairo.table_check(t, wmb, hmb, 3)
    got, _, _ = cairo.unserialize_slice(*cairo.serialize_slice(t, wmb, hmb, 3, *coef), wmb, hmb, 3)
    assert got[k]["prediction_target"] == 0 and not cairo.table_check(got, wmb, hmb, 3)


# ---------------------------------------------------------------------------
# Stand-alone programs under AddressSanitizer and UBSan.
# ---------------------------------------------------------------------------

# The runtimes are linked into the program: it then starts whatever else the
# environment preloads, where a shared runtime insists on being loaded first.
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
       "-fno-omit-frame-pointer", "-g", "-O1"]


def _build(tmp_path, compiler, std, sources, name, extra=()):
    if not shutil.which(compiler):
        pytest.fail(f"{compiler} is needed to build {name}")
    exe = str(tmp_path / name)
    subprocess.run([compiler, std, *SAN, "-o", exe, *[os.path.join(ROOT, s) for s in sources], *extra],
                   check=True, capture_output=True, text=True)
    return exe


def test_unserialize_driver_sanitized(tmp_path):
    """Arbitrary streams through unserialize.cpp and the predicate: no
    out-of-bounds access, no undefined behaviour, read_index <= write_index."""
    exe = _build(tmp_path, "g++", "-std=c++17",
                 ["tests/sanitize/unserialize_driver.cpp", "cairo_amd/csrc/unserialize.cpp",
                  "cairo_amd/csrc/table_check.cpp"], "unserialize_driver")
    r = subprocess.run([exe, "1500"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    decoded = int(r.stdout.split()[1])
    assert decoded > 100, r.stdout  # (the streams are not all refused at once)


def test_oracle_decoder_sanitized(orc, tmp_path, sequences):
    """The oracle decoder over the generator's sequences as a C program under
    the sanitizers: clean, and the same planes as the shared library gives."""
    exe = _build(tmp_path, "gcc", "-std=c11", ["tests/sanitize/oracle_decode_main.c", "oracle/evx_oracle.c"],
                 "oracle_decode", extra=["-lm"])
    for (w, h, r, s), seq in sequences.items():
        if s != SEEDS[0] or (w, h, r) == (352, 288, 2):
            continue
        path = tmp_path / f"seq_{w}x{h}_{r}.bin"
        with open(path, "wb") as f:
            f.write(struct.pack("<4i", w, h, r, len(seq)))
            for table, coef in seq:
                f.write(table.tobytes())
                for p in coef:
                    f.write(np.ascontiguousarray(p).tobytes())
        run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-4000:]
        d = orc.OracleDecoder(w, h, r)
        want = orc.FNV_OFFSET
        for t, (table, coef) in enumerate(seq):
            d.decode(table, coef)
            for p in d.predeblock() + d.planes(2 + t % r):
                want = orc.fnv1a64(p.tobytes(), want)
        assert int(run.stdout.strip(), 16) == want, (w, h, r)
