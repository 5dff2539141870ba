"""Per-frame metrics and kept reconstructions on the GPU (metrics.hip,
cairo_ctx_set_metrics and friends).

KAT: the kernels on their own (cairo_kat_metrics) against the numpy restatement
(tests/metrics_ref.py).  Then every frame of a pipelined launch: the kept
reconstruction against the oracle's deblocked slot taken right after it encoded
that frame, and the reported metrics against metrics_ref on the oracle's planes.

Exactness: SSE, sample and window counts are integers and must be equal.  The
window values are bit-identical by construction (integer sums, one IEEE
division), so only the order of the additions differs from numpy's: at most
1.3e4 values in [-1, 1] per plane here, which moves their mean by less than
1e-12; the bound asserted is 1e-9.
"""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import content
from tests import metrics_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KAT_SIZES = ((2, 2), (8, 8), (18, 10), (64, 48), (72, 40), (130, 66), (352, 288))
ENC_SIZES = ((64, 48), (72, 40), (352, 288))
FRAMES = 12
SSIM_TOL = 1e-9


def _check_metrics(got, want, w, h, tag, flags=3):
    assert got["flags"] == flags and (got["width"], got["height"]) == (w, h), tag
    assert got["samples"] == want["samples"], tag
    assert got["sse"] == want["sse"], f"{tag}: SSE {got['sse']} vs {want['sse']}"
    assert got["ssim_windows"] == want["ssim_windows"], tag
    for k in range(3):
        n = want["ssim_windows"][k]
        if n:
            d = abs(got["ssim_sum"][k] / n - want["ssim_sum"][k] / n)
            assert d <= SSIM_TOL, f"{tag}: plane {k} SSIM differs by {d}"
        else:
            assert got["ssim_sum"][k] == 0.0, tag


# ---------------------------------------------------------------------------
# 1. KAT
# ---------------------------------------------------------------------------

def _padded(planes, w, h, pitch, rng):
    """Planes with rows of `pitch` (chroma pitch / 2) elements; the padding holds other values."""
    out = []
    for k, p in enumerate(planes):
        pp, ph = (pitch, h) if k == 0 else (pitch // 2, h // 2)
        q = rng.integers(-300, 601, (ph, pp)).astype(np.int16)
        q[:, :p.shape[1]] = p
        out.append(q)
    return tuple(out)


def _kat_cases(rng, w, h):
    shapes = ((h, w), (h // 2, w // 2), (h // 2, w // 2))
    rnd = lambda: tuple(rng.integers(-300, 601, s).astype(np.int16) for s in shapes)  # noqa: E731
    a = rnd()
    yield "random", a, rnd()
    near = tuple(np.clip(p.astype(np.int32) + rng.integers(-6, 7, p.shape), -32768, 32767).astype(np.int16) for p in a)
    yield "near", a, near
    yield "equal", a, tuple(p.copy() for p in a)
    zero = tuple(np.full(s, 16 if k == 0 else 0, np.int16) for k, s in enumerate(shapes))
    full = tuple(np.full(s, 271 if k == 0 else 255, np.int16) for k, s in enumerate(shapes))
    yield "0-255", zero, full


@pytest.mark.parametrize("size", KAT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kat(cairo, size):
    w, h = size
    rng = np.random.default_rng(31 * w + h)
    for name, a, b in _kat_cases(rng, w, h):
        want = ref.frame_metrics(a, b, w, h)
        for pitch in (w, (w + 15) & ~15):  # tight (rows at any alignment), and the aligned pitch of a context
            pa, pb = (a, b) if pitch == w else (_padded(a, w, h, pitch, rng), _padded(b, w, h, pitch, rng))
            tag = f"{w}x{h} {name} pitch {pitch}"
            got = cairo.kat_metrics(pa, pb, w, h)
            _check_metrics(got, want, w, h, tag)
            if name == "equal":
                assert got["sse"] == [0, 0, 0], tag
                assert got["ssim_sum"] == [float(n) for n in got["ssim_windows"]], f"{tag}: a window is not exactly 1"
                assert got["psnr_all"] == float("inf")
            if name == "0-255":
                assert got["sse"] == [65025 * n for n in got["samples"]], tag
            again = cairo.kat_metrics(pa, pb, w, h)
            assert again == got, f"{tag}: two calls differ"
            assert [struct.pack("<d", x) for x in again["ssim_sum"]] == [struct.pack("<d", x) for x in got["ssim_sum"]]


def test_kat_refuses_bad_arguments(cairo):
    a = (np.zeros((4, 4), np.int16), np.zeros((2, 2), np.int16), np.zeros((2, 2), np.int16))
    m = cairo._FrameMetrics()
    import ctypes
    p = [x.ctypes.data for x in a]
    L = cairo.lib()
    assert L.cairo_kat_metrics(3, 4, 4, *p, *p, ctypes.byref(m), 0) == cairo.EVX_ERROR_INVALID_ARGS  # odd width
    assert L.cairo_kat_metrics(4, 4, 2, *p, *p, ctypes.byref(m), 0) == cairo.EVX_ERROR_INVALID_ARGS  # pitch < width
    assert L.cairo_kat_metrics(4, 4, 4, None, *p[1:], *p, ctypes.byref(m), 0) == cairo.EVX_ERROR_INVALID_ARGS


# ---------------------------------------------------------------------------
# 2. Every frame of one pipelined launch against the oracle
# ---------------------------------------------------------------------------

def _make(kind, w, h, t):
    if kind == "band4":
        from oracle import oracle
        return oracle.make_frame(w, h, t)
    return content.make(kind, w, h, t)


def _oracle_run(orc, kind, w, h, ring, q, frames):
    """Per frame: the RGB frame, planes(0) and the deblocked slot right after its encode."""
    e = orc.OracleEncoder(ring)
    e.set_quality(q)
    out = []
    for t in range(frames):
        rgb = _make(kind, w, h, t)
        e.encode(rgb)
        cp = lambda p: tuple(a.copy() for a in p)  # noqa: E731
        out.append(dict(rgb=rgb, src=cp(e.planes(0)), recon=cp(e.planes(2 + t % ring))))
    return out


def _check_ticket(ctx, tk, rec, w, h, tag):
    for got, want, n in zip(ctx.fetch_recon_planes(tk), rec["recon"], "YUV"):
        np.testing.assert_array_equal(got, want, err_msg=f"{tag}: kept reconstruction {n}")
    _check_metrics(ctx.frame_metrics(tk), ref.frame_metrics(rec["src"], rec["recon"], w, h), w, h, tag)


@pytest.mark.parametrize("kind", content.KINDS)
@pytest.mark.parametrize("q", [1, 16, 31])
@pytest.mark.parametrize("ring", [4, 2])
@pytest.mark.parametrize("size", ENC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_frame_of_a_launch(orc, cairo, size, ring, q, kind):
    w, h = size
    recs = _oracle_run(orc, kind, w, h, ring, q, FRAMES)
    ctx = cairo.Context(w, h, ring, stages=2 * FRAMES)
    try:
        ctx.set_metrics()
        ctx.set_batch(FRAMES)
        tks = [ctx.submit(r["rgb"], t, t > 0, q) for t, r in enumerate(recs)]  # one launch: all before the first wait
        for t, tk in enumerate(tks):
            ctx.wait(tk)
            _check_ticket(ctx, tk, recs[t], w, h, f"{kind} {w}x{h} R={ring} q={q} frame {t}")
        for tk in tks:
            ctx.release(tk)
    finally:
        ctx.close()


def test_slot_reuse(orc, cairo):
    """4 staging slots, 2 frames per launch, 10 frames: every keep slot is
    written two or three times, with the next launch already queued."""
    w, h, ring, q, n = 72, 40, 4, 16, 10
    recs = _oracle_run(orc, "band4", w, h, ring, q, n)
    ctx = cairo.Context(w, h, ring, stages=4)
    try:
        ctx.set_metrics()
        ctx.set_batch(2)
        held = []
        for t, r in enumerate(recs):
            if len(held) == 4:  # the two oldest: check, then hand their slots back
                for tt, tk in held[:2]:
                    ctx.wait(tk)
                    _check_ticket(ctx, tk, recs[tt], w, h, f"slot reuse frame {tt}")
                    ctx.release(tk)
                held = held[2:]
            held.append((t, ctx.submit(r["rgb"], t, t > 0, q)))
        for tt, tk in held:
            ctx.wait(tk)
            _check_ticket(ctx, tk, recs[tt], w, h, f"slot reuse frame {tt}")
            ctx.release(tk)
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# 3. Metrics on changes nothing else
# ---------------------------------------------------------------------------

def test_metrics_change_no_output(cairo):
    w, h, ring, q = 352, 288, 4, 16
    frames = [_make("band4", w, h, t) for t in range(FRAMES)]

    def run(flags):
        ctx = cairo.Context(w, h, ring, stages=2 * FRAMES)
        ctx.set_outputs(cairo.OUT_COEF | cairo.OUT_FEED)
        if flags:
            ctx.set_metrics(flags=flags)
        ctx.set_batch(FRAMES)
        tks = [ctx.submit(f, t, t > 0, q) for t, f in enumerate(frames)]
        outs = [ctx.wait(tk) for tk in tks]
        ctx.close()
        return outs

    off = run(0)
    for flags in (cairo.KEEP_RECON, cairo.METRIC_SSE | cairo.METRIC_SSIM):
        for t, (a, b) in enumerate(zip(off, run(flags))):
            tag = f"flags {flags} frame {t}"
            assert a.table.tobytes() == b.table.tobytes(), f"{tag}: block table"
            assert a.feed_bits == b.feed_bits and a.feed_status == b.feed_status == cairo.FEED_VALID, tag
            np.testing.assert_array_equal(a.feed, b.feed, err_msg=f"{tag}: feed words")
            for x, y in ((a.coef_y, b.coef_y), (a.coef_u, b.coef_u), (a.coef_v, b.coef_v)):
                np.testing.assert_array_equal(x, y, err_msg=f"{tag}: coefficients")


# ---------------------------------------------------------------------------
# 4. End to end without the oracle
# ---------------------------------------------------------------------------

def _i420(cairo, w, h, t):
    """An I420 frame from the gradient content (any 8-bit samples are a valid frame)."""
    rgb = content.make("gradient", w, h, t).astype(np.int32)
    buf = np.zeros(cairo.frame_layout(cairo.FMT_I420, w, h)[0], np.uint8)
    y, u, v = cairo.split_frame(buf, cairo.FMT_I420, w, h)
    y[...] = (rgb[..., 0] + 2 * rgb[..., 1] + rgb[..., 2]) // 4
    u[...] = 64 + rgb[::2, ::2, 2] // 2
    v[...] = 64 + rgb[::2, ::2, 0] // 2
    y[0, :8], y[1, :8] = 0, 255  # both ends of the 8-bit range
    return buf


def _sse_i420(cairo, a, b, w, h):
    return [int(((x.astype(np.int64) - y.astype(np.int64)) ** 2).sum())
            for x, y in zip(cairo.split_frame(a, cairo.FMT_I420, w, h), cairo.split_frame(b, cairo.FMT_I420, w, h))]


def test_end_to_end_i420(cairo):
    w, h, ring, q, n = 72, 40, 4, 16, 6
    frames = [_i420(cairo, w, h, t) for t in range(n)]
    # a context driven directly: the reference for the other layers
    ctx = cairo.Context(w, h, ring, stages=16)
    ctx.set_metrics()
    tks = [ctx.submit(f, t, t > 0, q, fmt=cairo.FMT_I420) for t, f in enumerate(frames)]
    direct, recon = [], []
    pitch = 3 * w + 5
    for tk in tks:
        ctx.wait(tk)
        direct.append(ctx.frame_metrics(tk))
        recon.append(ctx.fetch_recon(tk, cairo.FMT_I420))
        # a pitched BGR24 view: equal to the tight one, padding untouched
        tight = cairo.split_frame(ctx.fetch_recon(tk, cairo.FMT_BGR24), cairo.FMT_BGR24, w, h)
        buf = np.full(cairo.frame_layout(cairo.FMT_BGR24, w, h, pitch)[0], 0xA5, np.uint8)
        ctx.fetch_recon(tk, cairo.FMT_BGR24, pitch, out=buf)
        np.testing.assert_array_equal(cairo.split_frame(buf, cairo.FMT_BGR24, w, h, pitch), tight)
        assert (buf.reshape(h, pitch)[:, 3 * w:] == 0xA5).all(), "fetch_recon wrote the pitch padding"
        y, u, v = ctx.fetch_recon_planes(tk)
        np.testing.assert_array_equal(cairo.split_frame(recon[-1], cairo.FMT_I420, w, h)[0],
                                      np.clip(y[:h, :w].astype(np.int32) - 16, 0, 255))
    for tk in tks:
        ctx.release(tk)
    ctx.close()

    # the pipeline: its stream through the decoder gives the kept reconstruction
    ctx = cairo.Context(w, h, ring, stages=16)
    ctx.set_metrics()
    ctx.set_batch(3)
    st = cairo.Stream(ctx, threads=2)
    tks = [st.submit(f, t, t > 0, q, fmt=cairo.FMT_I420) for t, f in enumerate(frames)]
    dec = cairo.Decoder()
    dec.set_output_format(cairo.FMT_I420)
    bs = cairo.BitStream(w * h * 64 + 65536)
    for t, tk in enumerate(tks):
        hdr = struct.pack("<4sHBxHHH", b"EVX1", 14, ring, (2 << 8) | 47, w, h) if t == 0 else b""
        head = hdr + struct.pack("<IIH", 0 if t == 0 else 1, t, q)
        buf = np.zeros(len(head) + w * h * 8, np.uint8)
        buf[:len(head)] = np.frombuffer(head, np.uint8)
        nbits = st.collect(tk, buf, len(head) * 8)
        bs.empty()
        bs.write(buf.tobytes(), nbits)
        shown = dec.decode(bs, w, h)
        np.testing.assert_array_equal(shown, recon[t], err_msg=f"frame {t}: decoder output vs fetch_recon(I420)")
        assert _sse_i420(cairo, frames[t], shown, w, h) == direct[t]["sse"], f"frame {t}: SSE vs numpy on the I420 frames"
        assert st.frame_metrics(tk) == direct[t], f"frame {t}: Stream.frame_metrics"
    st.close()
    ctx.close()
    dec.close()

    # the drop-in encoder
    enc = cairo.Encoder(ring=ring)
    enc.set_quality(q)
    enc.set_input_format(cairo.FMT_I420)
    enc.set_metrics()
    for t, f in enumerate(frames):
        bs.empty()
        enc.encode(f, bs, w, h)
        assert enc.last_metrics() == direct[t], f"frame {t}: Encoder.last_metrics"
        if t == 2:  # between frames: off, and on again
            enc.set_metrics(sse=False, ssim=False)
            enc.set_metrics()
    enc.close()


# ---------------------------------------------------------------------------
# 5. Refusals
# ---------------------------------------------------------------------------

def _refused(cairo, fn, *a, **kw):
    with pytest.raises(cairo.CairoError) as ei:
        fn(*a, **kw)
    return ei.value.status


def test_refusals(orc, cairo):
    w, h, ring, q = 64, 48, 4, 16
    recs = _oracle_run(orc, "band4", w, h, ring, q, 4)
    ctx = cairo.Context(w, h, ring, stages=8)
    try:
        assert _refused(cairo, ctx.set_metrics, flags=8) == cairo.EVX_ERROR_INVALID_ARGS
        assert _refused(cairo, ctx.set_metrics, flags=-1) == cairo.EVX_ERROR_INVALID_ARGS
        # metrics off: nothing to fetch
        tk = ctx.submit(recs[0]["rgb"], 0, False, q)
        assert _refused(cairo, ctx.set_metrics) != 0, "set_metrics with a frame in flight"
        ctx.wait(tk)
        assert _refused(cairo, ctx.frame_metrics, tk) == cairo.EVX_ERROR_INVALID_ARGS
        assert _refused(cairo, ctx.fetch_recon, tk, cairo.FMT_I420) == cairo.EVX_ERROR_INVALID_ARGS
        assert _refused(cairo, ctx.fetch_recon_planes, tk) == cairo.EVX_ERROR_INVALID_ARGS
        assert _refused(cairo, ctx.set_metrics) != 0, "set_metrics with an unreleased frame"
        ctx.release(tk)
        # keep only: the reconstruction, but no metrics
        ctx.reset()
        ctx.set_metrics(sse=False, ssim=False, keep_recon=True)
        tk = ctx.submit(recs[0]["rgb"], 0, False, q)
        assert _refused(cairo, ctx.fetch_recon_planes, tk) == cairo.EVX_ERROR_INVALID_ARGS, "not waited yet"
        ctx.wait(tk)
        assert _refused(cairo, ctx.frame_metrics, tk) == cairo.EVX_ERROR_INVALID_ARGS
        for got, want in zip(ctx.fetch_recon_planes(tk), recs[0]["recon"]):
            np.testing.assert_array_equal(got, want)
        ctx.release(tk)
        assert _refused(cairo, ctx.fetch_recon_planes, tk) == cairo.EVX_ERROR_INVALID_ARGS, "released"
        # metrics on; the setting survives a reset
        ctx.set_metrics()
        ctx.reset()
        tk = ctx.submit(recs[0]["rgb"], 0, False, q)
        assert _refused(cairo, ctx.frame_metrics, tk) == cairo.EVX_ERROR_INVALID_ARGS, "not waited yet"
        out0 = ctx.wait(tk)
        _check_ticket(ctx, tk, recs[0], w, h, "after reset")
        ctx.release(tk)
        assert _refused(cairo, ctx.frame_metrics, tk) == cairo.EVX_ERROR_INVALID_ARGS, "released"
        assert _refused(cairo, ctx.fetch_recon, tk, cairo.FMT_I420) == cairo.EVX_ERROR_INVALID_ARGS, "released"
        assert _refused(cairo, ctx.fetch_recon, tk + 1, cairo.FMT_I420) == cairo.EVX_ERROR_INVALID_ARGS, "never submitted"
        # a decoded frame has neither (it takes the next ticket and holds no staging slot afterwards)
        mbs = ctx.wmb * ctx.hmb
        coef = np.concatenate([p.reshape(-1) for p in (out0.coef_y, out0.coef_u, out0.coef_v)])
        rgb = np.zeros((h, w, 3), np.uint8)
        ctx.reset()
        assert ctx.L.cairo_ctx_decode_frame(ctx.h, out0.table.ctypes.data, coef.ctypes.data, 0, rgb.ctypes.data) == 0
        assert mbs == out0.table.size
        np.testing.assert_array_equal(rgb, cairo.yuv_to_rgb(*recs[0]["recon"], w, h))
        assert _refused(cairo, ctx.frame_metrics, 0) == cairo.EVX_ERROR_INVALID_ARGS, "decoded frame"
        assert _refused(cairo, ctx.fetch_recon, 0, cairo.FMT_I420) == cairo.EVX_ERROR_INVALID_ARGS, "decoded frame"
        # off again: the context encodes as before
        ctx.set_metrics(flags=0)
        ctx.reset()
        for t, rec in enumerate(recs):
            tk = ctx.submit(rec["rgb"], t, t > 0, q)
            ctx.wait(tk)
            assert _refused(cairo, ctx.frame_metrics, tk) == cairo.EVX_ERROR_INVALID_ARGS
            ctx.release(tk)
            for got, want, n in zip(ctx.read_planes(2 + t % ring), rec["recon"], "YUV"):
                np.testing.assert_array_equal(got, want, err_msg=f"after set_metrics(0), frame {t}: recon {n}")
    finally:
        ctx.close()


_GROUP_SCRIPT = """
import json, sys
sys.path.insert(0, %r)
import cairo_amd as c
a, b = c.Context(64, 48, 4, stages=8), c.Context(64, 48, 4, stages=8)
out = {}
def status(fn, *args, **kw):
    try:
        fn(*args, **kw)
        return 0
    except c.CairoError as e:
        return e.status
a.set_metrics()
recs = [a.peer_info(), b.peer_info()]
out["join_with_metrics"] = status(a.join_group, 0, recs)
a.set_metrics(flags=0)
out["join"] = [status(a.join_group, 0, recs), status(b.join_group, 1, recs)]
out["set_on_member"] = status(a.set_metrics)
a.close(); b.close()
print(json.dumps(out))
"""


def test_group_members_are_refused():
    """A group member's deblock pushes to its mirrors: set_metrics is refused
    on it, and a context with metrics on cannot join.  Two members in one
    process need 8 hardware queues, so this runs in a process of its own."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="8")
    r = subprocess.run([sys.executable, "-c", _GROUP_SCRIPT % ROOT], capture_output=True, text=True, timeout=120,
                       env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out == {"join_with_metrics": 1, "join": [0, 0], "set_on_member": 1}, out
