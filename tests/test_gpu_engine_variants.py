"""The engine's two instantiations on the GPU.

A launch without stamps, trace or inject flag, none of whose frames belongs
to a group across devices or processes, runs the plain engine (no diagnostics
compiled in, agent-scope hand-offs only); every other launch the general one.
cairo_ctx_engine_variant says which ran (0 plain, 1 general).  Both compute
the same stream bit for bit, which is the oracle's:

* CIF I + 3 P in one launch, debug flags 0 against 2|4 (stamps and trace):
  every frame's block table and feed, the last frame's inter records of every
  reference (one launch keeps only its last frame's) and the ring slots;
* the inject flag (16): the general engine and CAIRO_WAIT_INJECTED, then,
  after a reset with the flag cleared, the plain engine and a bit-exact stream;
* QCIF with one, two and three ring slots (0, 1, 2 inter records per
  macroblock; 11 macroblocks wide: a ragged last group of three) at q 1 and 16;
* two processes as the members of one group on one device (system-scope
  hand-offs): tests/engine_variant_worker.py, 2 * 2 + ring frames.

The oracle's stream is computed once per geometry and shared.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_parity import _payload_bits, _table_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "engine_variant_worker.py")

CIF = (352, 288, 4, 16, 4)  # w, h, ring, q, frames: I + 3 P

_CACHE = {}


def _reference(orc, w, h, ring, q, frames):
    """The oracle's band4 stream, once: the source frames, per frame (block
    table, coefficient planes, payload bits, inter records, inter SADs; the
    last two None without a reference), and the final ring slots."""
    key = (w, h, ring, q, frames)
    if key not in _CACHE:
        e = orc.OracleEncoder(ring)
        e.set_quality(q)
        src, ref = [], []
        for t in range(frames):
            rgb = orc.make_frame(w, h, t)
            src.append(rgb)
            data, nbits = e.encode(rgb)
            head = (14 * 8 if t == 0 else 0) + 10 * 8  # header + frame descriptor precede the payload
            bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")[head:nbits]
            recs, sads = e.inter_records() if t > 0 and ring > 1 else (None, None)
            ref.append((e.block_table().copy(), tuple(np.array(p, copy=True) for p in e.planes(1)), bits, recs, sads))
        slots = [tuple(np.array(p, copy=True) for p in e.planes(2 + k)) for k in range(ring)]
        _CACHE[key] = (src, ref, slots)
    return _CACHE[key]


def _one_launch(orc, cairo, w, h, ring, q, frames, flags):
    """The stream as one launch with feed outputs under debug `flags`; checks
    it against the oracle and returns what the GPU produced: per frame (table,
    payload bits), the last frame's (records, SADs), the ring slots, the
    engine variant and the context's stamps (None without flag 2)."""
    src, ref, slots = _reference(orc, w, h, ring, q, frames)
    ctx = cairo.Context(w, h, ring)
    try:
        ctx.set_outputs(cairo.OUT_FEED)
        ctx.set_batch(frames)
        assert ctx.stages >= frames
        if flags:
            ctx.set_debug(flags)
        tks = [ctx.submit(src[t], t, t > 0, q) for t in range(frames)]
        ctx.flush()
        variant = ctx.engine_variant()
        got = []
        for t, tk in enumerate(tks):
            out = ctx.wait(tk)
            tag = f"{w}x{h} R={ring} q={q} flags={flags} frame {t}"
            assert out.feed_status == cairo.FEED_VALID, f"{tag}: feed status {out.feed_status}"
            bits = _payload_bits(cairo, out, ctx, ring, tk)
            _table_equal(out.table, ref[t][0], f"{tag}: block table")
            assert bits.size == ref[t][2].size, f"{tag}: payload {bits.size} vs {ref[t][2].size} bits"
            assert np.array_equal(bits, ref[t][2]), f"{tag}: payload bits differ"
            got.append((out.table.copy(), bits))
            ctx.release(tk)
        ctx.sync()
        recs = ctx.read_inter() if ring > 1 and frames > 1 else None
        if recs is not None:
            tag = f"{w}x{h} R={ring} q={q} flags={flags} frame {frames - 1}"
            _table_equal(recs[0], ref[-1][3], f"{tag}: inter records")
            np.testing.assert_array_equal(recs[1], ref[-1][4], err_msg=f"{tag}: inter SAD")
        got_slots = [ctx.read_planes(2 + k) for k in range(ring)]
        for k in range(ring):
            for p, name in enumerate("YUV"):
                np.testing.assert_array_equal(got_slots[k][p], slots[k][p],
                                              err_msg=f"flags={flags}: ring slot {k} {name}")
        stamps = ctx.read_stamps() if flags & 2 else None
    finally:
        ctx.close()
    return got, recs, got_slots, variant, stamps


def test_plain_and_general_engine_agree(orc, cairo):
    w, h, ring, q, frames = CIF
    plain = _one_launch(orc, cairo, w, h, ring, q, frames, 0)
    general = _one_launch(orc, cairo, w, h, ring, q, frames, 2 | 4)
    assert plain[3] == 0, "a launch without diagnostics runs the plain engine"
    assert general[3] == 1, "stamps and trace need the general engine"
    for t, (a, b) in enumerate(zip(plain[0], general[0])):
        _table_equal(a[0], b[0], f"frame {t}: block table, plain vs general")
        assert np.array_equal(a[1], b[1]), f"frame {t}: feed, plain vs general"
    _table_equal(plain[1][0], general[1][0], "inter records, plain vs general")
    np.testing.assert_array_equal(plain[1][1], general[1][1], err_msg="inter SAD, plain vs general")
    for k in range(ring):
        for p, name in enumerate("YUV"):
            np.testing.assert_array_equal(plain[2][k][p], general[2][k][p], err_msg=f"ring slot {k} {name}")
    mb, db, span, inter = general[4]
    assert mb[:frames, :, :, 0].all() and mb[:frames, :, :, 9].all(), "a macroblock without its first or last stamp"
    assert span[0] != np.uint64(0xFFFFFFFFFFFFFFFF) and span[1] >= span[0] > 0, "no engine entry / exit stamps"
    assert inter[:frames, :, :, 0].all(), "a helper group without its start stamp"


def test_inject_takes_general_engine_then_recovers(orc, cairo):
    w, h, ring, q, frames = CIF
    src, ref, _ = _reference(orc, w, h, ring, q, frames)
    ctx = cairo.Context(w, h, ring)
    try:
        ctx.encode_frame(src[0], 0, False, q)
        assert ctx.engine_variant() == 0
        ctx.set_debug(16)
        with pytest.raises(cairo.CairoError) as ei:
            ctx.encode_frame(src[1], 1, True, q)
        assert ctx.engine_variant() == 1, "the inject hook is in the general engine only"
        assert ei.value.status == cairo.EVX_ERROR_HARDWAREFAIL
        assert ei.value.timeout["kind"] == "injected"
        ctx.set_debug(0)
        ctx.reset()
        assert ctx.timeout_info() is None
        for t in range(frames):
            out = ctx.encode_frame(src[t], t, t > 0, q)
            assert ctx.engine_variant() == 0, f"frame {t} after the reset"
            _table_equal(out.table, ref[t][0], f"after reset, frame {t}: block table")
            for p, (name, got) in enumerate(zip("YUV", (out.coef_y, out.coef_u, out.coef_v))):
                np.testing.assert_array_equal(got, ref[t][1][p], err_msg=f"after reset, frame {t}: coef {name}")
            data, n = cairo.serialize_slice(out.table, ctx.wmb, ctx.hmb, ring, out.coef_y, out.coef_u, out.coef_v)
            bits = np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")[:n]
            assert np.array_equal(bits, ref[t][2]), f"after reset, frame {t}: payload bits"
    finally:
        ctx.close()


@pytest.mark.parametrize("q", [1, 16])
@pytest.mark.parametrize("ring", [1, 2, 3])
def test_inter_records_at_every_nref(orc, cairo, ring, q):
    got = _one_launch(orc, cairo, 176, 144, ring, q, 3, 0)
    assert got[3] == 0


def test_two_process_group_takes_general_engine(tmp_path):
    ring, members = 4, 2
    frames = 2 * members + ring
    store = tmp_path / "store"
    procs = [subprocess.Popen([sys.executable, WORKER, "--members", str(members), "--rank", str(k), "--store",
                               str(store), "--ring", str(ring), "--frames", str(frames), "--batch", "2"], cwd=ROOT,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k in range(members)]
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=240)
        except subprocess.TimeoutExpired:
            for x in procs:
                x.kill()
            raise
        outs.append((p.returncode, o, e))
    for rc, o, e in outs:
        assert rc == 0, o[-2000:] + e[-3000:]
        res = json.loads(o.strip().splitlines()[-1])
        assert res["mismatched"] == []
        assert res["launches"] >= 2 and res["variants"] == [1] * res["launches"], res
