"""Target bitrate on the GPU (rate.hip, cairo_ctx_set_rate).

KAT: k_rate_observe / k_rate_finish on their own (cairo_kat_rate_observe)
against numpy's popcount.  Then the controller in a context: for one sequence
of calls every frame's quality, feed size, set bits, aim and debt equal the CPU
simulation (tools/rate_sim.py: oracle encoder + host precode + the law on the
host), and every frame's payload equals the oracle's frame coded at that
quality -- through Context and through Stream, with metrics on and mixed
formats, across reset() and set_rate(None), and the refusals.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import pixfmt_ref as ref
from tools import rate_sim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING = 4
LAUNCHES = [3, 3, 2, 3, 3]  # set_batch(3), 14 frames, flush() after frame 7
INFO = ("quality", "feed_bits", "ones", "est_bits", "aim", "debt")


# ---- KAT --------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1, 3])
def test_kat_rate_observe(cairo, base):
    """Feeds of every length around a word and a 16-byte load, several frames a
    call, at word offsets (base, and an odd stride) where a frame's first
    16-byte boundary comes after 0, 1, 2 or 3 words; every bit beyond a feed's
    N set, in its last word and in all the words up to the next frame."""
    rng = np.random.default_rng(5 + base)
    nbits = [0, 1, 31, 32, 33, 127, 128, 129, 100003, 95, 97, 160]
    stride = (100003 + 31) // 32 + 3  # 3129 words: odd
    words = rng.integers(0, 1 << 32, base + stride * len(nbits) + 5, dtype=np.uint64).astype(np.uint32)
    words[:base] = 0xFFFFFFFF
    want = []
    for j, n in enumerate(nbits):
        f = words[base + j * stride: base + (j + 1) * stride]
        bits = np.unpackbits(f.view(np.uint8), bitorder="little")
        bits[n:] = 1
        f[:] = np.packbits(bits, bitorder="little").view(np.uint32)
        want.append(int(bits[:n].sum()))
    got = cairo.kat_rate_observe(words, nbits, base=base, stride=stride)
    for j, n in enumerate(nbits):
        g = got[j]
        assert (g["feed_bits"], g["ones"], g["overflow"]) == (n, want[j], 0), f"frame {j} ({n} bits): {g}, want {want[j]}"
        assert g["est_bits"] == cairo.rate_estimate(n, n - want[j]) + 80


# ---- the controller in a context ----------------------------------------------
def _target(frames, launches):
    """Between the fixed q = 8 and q = 16 means of the same frames (payload + 80)."""
    m = [rate_sim.summary(rate_sim.simulate(frames, launches, RING, fixed_q=q))[2] for q in (8, 16)]
    assert m[1] < m[0]
    return int(sum(m) / 2)


@pytest.fixture(scope="module")
def sims():
    """size -> (frames, rate keywords, the simulation's records of LAUNCHES), computed once."""
    out = {}
    for w, h in ((64, 48), (352, 288)):
        frames = rate_sim.make_frames("band4", w, h, sum(LAUNCHES))
        rate = dict(target_bits=_target(frames, LAUNCHES), q0=8, qmin=1, qmax=31, window=16)
        out[w, h] = (frames, rate, rate_sim.simulate(frames, LAUNCHES, RING, rate=rate))
    return out


def _same_bits(got, want, what):
    """(bytes, nbits) pairs: the same bits (bits of the last byte beyond nbits are not compared)."""
    assert got[1] == want[1], f"{what}: {got[1]} vs {want[1]} payload bits"
    a = np.unpackbits(np.frombuffer(got[0], np.uint8), bitorder="little")[:got[1]]
    b = np.unpackbits(np.frombuffer(want[0], np.uint8), bitorder="little")[:want[1]]
    np.testing.assert_array_equal(a, b, err_msg=f"{what}: payload differs")


def _check(cairo, info, out_quality, payload, rec, what):
    assert {k: info[k] for k in INFO} == {k: rec[k] for k in INFO}, f"{what}: {info} vs the simulation's {rec['quality']}"
    assert info["overflow"] == 0 and out_quality == rec["quality"], what
    _same_bits(payload, (rec["payload"], rec["payload_bits"]), what)


def _submit_all(ctx, via, frames, launches, q=5, first=0, make=None):
    """Submit the frames in the given launches: set_batch(max), and an explicit
    flush() wherever a launch ends short.  q: the submitted quality, which the
    controller ignores."""
    batch = max(launches)
    ctx.set_batch(batch)
    tks, t = [], first
    for n in launches:
        for _ in range(n):
            frame, kw = make(t) if make else (frames[t], {})
            tks.append(via.submit(frame, t, t > 0, q, **kw))
            t += 1
        if n < batch:
            ctx.flush()
    return tks


def _wait_and_check(cairo, ctx, tks, recs, tag, first=0):
    for k, tk in enumerate(tks):
        out = ctx.wait(tk)
        assert out.feed_status == cairo.FEED_VALID
        _check(cairo, ctx.frame_rate(tk), out.quality, cairo.serialize_feed(out.feed, out.feed_bits), recs[first + k],
               f"{tag} frame {first + k}")
        ctx.release(tk)


@pytest.mark.parametrize("size", [(64, 48), (352, 288)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_context(cairo, sims, size):
    frames, rate, recs = sims[size]
    assert len({r["quality"] for r in recs}) > 1, "the simulation never left q0: the case checks nothing"
    ctx = cairo.Context(*size, RING, stages=16)
    try:
        ctx.set_outputs(cairo.OUT_FEED)
        ctx.set_rate(**rate)
        tks = _submit_all(ctx, ctx, frames, LAUNCHES)
        _wait_and_check(cairo, ctx, tks, recs, f"context {size}")
        assert ctx.engine_variant() == 0, "a launch with rate control on takes the plain engine"
    finally:
        ctx.close()


@pytest.mark.parametrize("size", [(64, 48), (352, 288)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_parity_stream(cairo, sims, size):
    frames, rate, recs = sims[size]
    ctx = cairo.Context(*size, RING, stages=16)
    st = cairo.Stream(ctx, threads=2)
    try:
        ctx.set_rate(**rate)
        tks = _submit_all(ctx, st, frames, LAUNCHES)
        for k, tk in enumerate(tks):
            payload = st.collect(tk)
            info = st.frame_rate(tk)
            _check(cairo, info, info["quality"], payload, recs[k], f"stream {size} frame {k}")
    finally:
        st.close()
        ctx.close()


def test_metrics_on_mixed_launch(orc, cairo, sims):
    """Launches that mix RGB24 and NV12 frames (the general convert kernel
    writes the views the controller then edits), per-frame metrics on."""
    w, h = 64, 48
    frames, rate, recs = sims[w, h]
    e = orc.OracleEncoder(RING)
    nv12 = []
    for f in frames:  # the NV12 frame of the same input planes (they do not depend on the quality)
        e.encode(f)
        nv12.append(ref.planes_to_frame(*e.planes(0), ref.NV12, w, h))
    ctx = cairo.Context(w, h, RING, stages=16)
    try:
        ctx.set_outputs(cairo.OUT_FEED)
        ctx.set_metrics(sse=True, ssim=True)
        ctx.set_rate(**rate)
        make = lambda t: (nv12[t], dict(fmt=cairo.FMT_NV12)) if t % 2 else (frames[t], {})  # noqa: E731
        tks = _submit_all(ctx, ctx, frames, LAUNCHES, make=make)
        for k, tk in enumerate(tks):
            out = ctx.wait(tk)
            _check(cairo, ctx.frame_rate(tk), out.quality, cairo.serialize_feed(out.feed, out.feed_bits), recs[k],
                   f"mixed launch frame {k}")
            m = ctx.frame_metrics(tk)
            assert m["flags"] and m["samples"][0] == w * h
            ctx.release(tk)
    finally:
        ctx.close()


def test_lifecycle_reset_and_off(orc, cairo, sims):
    """reset() mid-stream restarts the controller at q0 (the run repeats bit for
    bit); set_rate(None) returns to the submitted qualities, the stream going
    on: the next frames equal the oracle's continuation at a fixed quality."""
    w, h = 64, 48
    frames, rate, recs = sims[w, h]
    ctx = cairo.Context(w, h, RING, stages=16)
    try:
        ctx.set_outputs(cairo.OUT_FEED)
        ctx.set_rate(**rate)
        _wait_and_check(cairo, ctx, _submit_all(ctx, ctx, frames, LAUNCHES), recs, "first run")
        ctx.reset()
        part = LAUNCHES[:3]  # 8 frames: the same qualities again, from q0
        _wait_and_check(cairo, ctx, _submit_all(ctx, ctx, frames, part), recs, "after reset")
        ctx.set_rate(None)
        fixed = 11
        enc = orc.OracleEncoder(RING)
        want = []
        for t in range(sum(part) + 3):
            enc.set_quality(recs[t]["quality"] if t < sum(part) else fixed)
            data, nbits = enc.encode(frames[t])
            head = 80 + (112 if t == 0 else 0)
            want.append((data[head // 8:], nbits - head))
        tks = _submit_all(ctx, ctx, frames, [3], q=fixed, first=sum(part))
        for k, tk in enumerate(tks):
            out = ctx.wait(tk)
            assert out.quality == fixed
            with pytest.raises(cairo.CairoError):
                ctx.frame_rate(tk)
            _same_bits(cairo.serialize_feed(out.feed, out.feed_bits), want[sum(part) + k], f"rate off, frame {sum(part) + k}")
            ctx.release(tk)
    finally:
        ctx.close()


GROUP_MEMBER = """
import sys
sys.path.insert(0, {root!r})
import cairo_amd as ca
g = ca.Group(64, 48, 4, [0, 0], stages=8)
m = g.members[0]
m.set_outputs(ca.OUT_FEED)
try:
    m.set_rate(20000)
    print("accepted")
except ca.CairoError as e:
    print("refused", e.status)
g.close()
"""


def test_refusals(cairo, sims):
    w, h = 64, 48
    frames, rate, recs = sims[w, h]
    ctx = cairo.Context(w, h, RING, stages=16)
    other = cairo.Context(w, h, RING, stages=16)
    try:
        with pytest.raises(cairo.CairoError) as e:  # the outputs are the coefficient planes only
            ctx.set_rate(**rate)
        assert e.value.status == cairo.EVX_ERROR_INVALID_ARGS
        ctx.set_outputs(cairo.OUT_FEED)
        with pytest.raises(cairo.CairoError) as e:
            ctx.set_rate(**dict(rate, qmin=9, qmax=8))
        assert e.value.status == cairo.EVX_ERROR_INVALID_ARGS
        # a frame in flight (pending, not launched): refused, and nothing changes -- it stays pending,
        # and is coded at its submitted quality
        ctx.set_batch(3)
        tk = ctx.submit(frames[0], 0, False, recs[0]["quality"])
        with pytest.raises(cairo.CairoError) as e:
            ctx.set_rate(**rate)
        assert e.value.status == 8  # EVX_ERROR_INVALID_RESOURCE
        out = ctx.wait(tk)
        assert out.quality == recs[0]["quality"]
        with pytest.raises(cairo.CairoError):
            ctx.frame_rate(tk)
        _same_bits(cairo.serialize_feed(out.feed, out.feed_bits), (recs[0]["payload"], recs[0]["payload_bits"]), "refused set_rate")
        with pytest.raises(cairo.CairoError) as e:  # waited but not released: still in flight
            ctx.set_rate(**rate)
        assert e.value.status == 8
        ctx.release(tk)
        # on: no group, no decode, no outputs without the feed; each refusal leaves the controller on
        ctx.reset()
        ctx.set_rate(**rate)
        with pytest.raises(cairo.CairoError) as e:
            ctx.join_group(0, [ctx.peer_info(), other.peer_info()])
        assert e.value.status == cairo.EVX_ERROR_INVALID_ARGS
        table = np.zeros(ctx.wmb * ctx.hmb, cairo.BLOCK_DESC)
        coef = np.zeros(ctx.wa * ctx.ha * 3 // 2, np.int16)
        rgb = np.zeros((h, w, 3), np.uint8)
        # (the entry point itself: Context.decode_frame checks the table before it calls)
        assert cairo.lib().cairo_ctx_decode_frame(ctx.h, table.ctypes.data, coef.ctypes.data, 0, rgb.ctypes.data) == 8
        with pytest.raises(cairo.CairoError) as e:
            ctx.set_outputs(cairo.OUT_COEF)
        assert e.value.status == cairo.EVX_ERROR_INVALID_ARGS
        part = LAUNCHES[:2]
        _wait_and_check(cairo, ctx, _submit_all(ctx, ctx, frames, part), recs, "after the refusals")
    finally:
        ctx.close()
        other.close()


def test_refused_on_a_group_member():
    """Two members on one device need eight hardware queues, which the HIP
    runtime reads when it starts: a process of its own."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    r = subprocess.run([sys.executable, "-c", GROUP_MEMBER.format(root=ROOT)], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["refused", "1"], r.stdout + r.stderr[-2000:]
