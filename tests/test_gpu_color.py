"""Colour descriptions of I420 / NV12 frames on the GPU (include/cairo_amd.h
CAIRO_RANGE_*, CAIRO_MATRIX_*).

Every path under a description must give exactly what the existing path gives
on the *mapped* frame (tests/color_ref.py map_frame), and the existing paths
are pinned to the oracle elsewhere (tests/test_gpu_pixfmt.py): the kernels on
their own over all 2^24 sample triples and at the edge sizes, then the
encoder, a mixed launch, the scaled submit, the decoder's output, the drop-in
classes and the pipeline.  Every comparison is exact.
"""
import numpy as np
import pytest

from tests import color_ref as cr
from tests import pixfmt_ref as ref
from tests import scale_ref
from tests.test_gpu_pixfmt import KAT_SIZES, _DeviceBuffer, _pitches, _table_equal

pytestmark = pytest.mark.gpu

YUV = (ref.I420, ref.NV12)
_id = lambda f: ref.FMT_NAMES[f]  # noqa: E731
_cname = lambda c: f"{'limited' if c[0] else 'full'}-{'709' if c[1] else '601'}"  # noqa: E731
RING, Q = 4, 16


def _kat(cairo, direction, fmt, desc, w, h, pitch, frame, y, u, v):
    for a in (frame, y, u, v):
        assert a.flags["C_CONTIGUOUS"]
    assert frame.dtype == np.uint8 and y.dtype == u.dtype == v.dtype == np.int16
    assert frame.size == ref.layout(fmt, w, h, pitch)[0] and y.shape == (h, w) and u.shape == v.shape == (h // 2, w // 2)
    st = cairo.lib().cairo_kat_convert_color(direction, fmt, desc[0], desc[1], w, h, pitch, frame.ctypes.data,
                                             y.ctypes.data, u.ctypes.data, v.ctypes.data, 0)
    assert st == 0, f"cairo_kat_convert_color status {st}"


def _empty_planes(w, h):
    return np.full((h, w), -1, np.int16), np.full((h // 2, w // 2), -1, np.int16), np.full((h // 2, w // 2), -1, np.int16)


# ---------------------------------------------------------------------------
# 1. Exhaustive KAT: all 2^24 (Y8, U8, V8) triples, once each
# ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def all_triples():
    """A 4096x4096 NV12 frame: chroma sample (cx, cy) is (cx & 255, cy & 255);
    copy j = (cx >> 8) + 8 (cy >> 8) carries luma 4 j + 2 dy + dx in its quad."""
    w = h = 4096
    frame = np.empty(w * h * 3 // 2, np.uint8)
    y, uv = ref.views(frame, ref.NV12, w, h)
    c = np.arange(2048)
    uv[..., 0] = (c & 255)[None, :]
    uv[..., 1] = (c & 255)[:, None]
    j = (c >> 8)[None, :] + 8 * (c >> 8)[:, None]
    y[...] = np.repeat(np.repeat(4 * j, 2, axis=0), 2, axis=1) + np.tile(np.array([[0, 1], [2, 3]]), (2048, 2048))
    seen = np.zeros(1 << 24, bool)
    seen[(y.astype(np.int64) << 16) | (np.repeat(np.repeat(uv[..., 0], 2, 0), 2, 1).astype(np.int64) << 8)
         | np.repeat(np.repeat(uv[..., 1], 2, 0), 2, 1)] = True
    assert seen.all()
    frame.setflags(write=False)
    return frame


@pytest.mark.parametrize("desc", cr.NON_IDENTITY, ids=_cname)
def test_kat_exhaustive(cairo, all_triples, desc):
    w = h = 4096
    want = ref.frame_to_planes(cr.map_frame(all_triples, ref.NV12, w, h, 0, 0, *desc), ref.NV12, w, h)
    frame = all_triples.copy()
    got = _empty_planes(w, h)
    _kat(cairo, 0, ref.NV12, desc, w, h, 0, frame, *got)
    for g, x, n in zip(got, want, "YUV"):
        np.testing.assert_array_equal(g, x, err_msg=f"{_cname(desc)} dir 0: {n}")
    # dir 1: the same triples as 8-bit-clean internal planes
    planes = tuple(np.ascontiguousarray(p) for p in ref.frame_to_planes(all_triples, ref.NV12, w, h))
    out = np.full(all_triples.size, 0xFF, np.uint8)
    _kat(cairo, 1, ref.NV12, desc, w, h, 0, out, *planes)
    np.testing.assert_array_equal(out, cr.map_frame(all_triples, ref.NV12, w, h, 0, 1, *desc),
                                  err_msg=f"{_cname(desc)} dir 1")


# ---------------------------------------------------------------------------
# 2. Edges: odd chroma width, five workgroups per row, a strip cut by the edge
# ---------------------------------------------------------------------------

def _corner_frame(rng, fmt, w, h, pitch, variant):
    frame = rng.integers(0, 256, ref.layout(fmt, w, h, pitch)[0], dtype=np.uint8)
    frame[~ref.image_mask(fmt, w, h, pitch)] = 0xFF
    vw = ref.views(frame, fmt, w, h, pitch)
    lo, hi = (0, 255) if variant == 0 else (255, 0)
    vw[0][0, 0], vw[0][-1, -1] = lo, hi
    if fmt == ref.I420:
        vw[1][0, 0], vw[2][0, 0], vw[1][-1, -1], vw[2][-1, -1] = lo, hi, hi, lo
    else:
        vw[1][0, 0], vw[1][-1, -1] = (lo, hi), (hi, lo)
    return frame


@pytest.mark.parametrize("size", KAT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", YUV, ids=_id)
def test_kat_edges_input(cairo, fmt, size):
    w, h = size
    rng = np.random.default_rng(3000 * fmt + w)
    for pitch in _pitches(fmt, w):
        for variant in range(2):
            frame = _corner_frame(rng, fmt, w, h, pitch, variant)
            for desc in cr.NON_IDENTITY:
                want = ref.frame_to_planes(cr.map_frame(frame, fmt, w, h, pitch, 0, *desc), fmt, w, h, pitch)
                before = frame.copy()
                got = _empty_planes(w, h)
                _kat(cairo, 0, fmt, desc, w, h, pitch, frame, *got)
                tag = f"{ref.FMT_NAMES[fmt]} {w}x{h} pitch {pitch} variant {variant} {_cname(desc)}"
                for g, x, n in zip(got, want, "YUV"):
                    np.testing.assert_array_equal(g, x, err_msg=f"{tag}: {n}")
                np.testing.assert_array_equal(frame, before, err_msg=f"{tag}: the source frame")


def _wild_planes(rng, w, h, variant):
    """Planes holding values outside 8 bits (-300..600, and the int16 extremes)
    next to in-range neighbours: every second sample is 8-bit clean."""
    y = rng.integers(-300, 600, (h, w)).astype(np.int16)
    u = rng.integers(-300, 600, (h // 2, w // 2)).astype(np.int16)
    v = rng.integers(-300, 600, (h // 2, w // 2)).astype(np.int16)
    y[:, variant::2] = rng.integers(16, 272, y[:, variant::2].shape)
    u[:, variant::2] = rng.integers(0, 256, u[:, variant::2].shape)
    v[:, 1 - variant::2] = rng.integers(0, 256, v[:, 1 - variant::2].shape)
    y[0, 0], y[-1, -1] = (-32768, 32767) if variant else (32767, -32768)
    u[0, 0], v[0, 0], u[-1, -1], v[-1, -1] = (-32768, 32767, 256, -1) if variant else (32767, -32768, -1, 256)
    return y, u, v


@pytest.mark.parametrize("size", KAT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", YUV, ids=_id)
def test_kat_edges_output(cairo, fmt, size):
    w, h = size
    rng = np.random.default_rng(4000 * fmt + w)
    for pitch in _pitches(fmt, w):
        m = ref.image_mask(fmt, w, h, pitch)
        for variant in range(4):
            if variant < 2:  # 8-bit clean: random bytes with 0 and 255 at the corners
                y, u, v = (np.ascontiguousarray(p) for p in
                           ref.frame_to_planes(_corner_frame(rng, fmt, w, h, pitch, variant), fmt, w, h, pitch))
            else:
                y, u, v = _wild_planes(rng, w, h, variant - 2)
            identity = ref.planes_to_frame(y, u, v, fmt, w, h, pitch, fill=0xFF)  # the clamp comes first
            for desc in cr.NON_IDENTITY:
                want = cr.map_frame(identity, fmt, w, h, pitch, 1, *desc)
                frame = np.full(want.size, 0xFF, np.uint8)
                _kat(cairo, 1, fmt, desc, w, h, pitch, frame, y, u, v)
                tag = f"{ref.FMT_NAMES[fmt]} {w}x{h} pitch {pitch} variant {variant} {_cname(desc)}"
                np.testing.assert_array_equal(frame[m], want[m], err_msg=f"{tag}: image")
                assert (frame[~m] == 0xFF).all(), f"{tag}: pitch padding written"


def test_kat_identity_and_rgb_ignore_the_description(cairo):
    """cairo_kat_convert equals (FULL, BT601), and an RGB frame is converted the
    same under any description."""
    w, h = 70, 34
    rng = np.random.default_rng(77)
    for fmt in (ref.RGB24, ref.NV12):
        frame = rng.integers(0, 256, ref.layout(fmt, w, h)[0], dtype=np.uint8)
        a, b, c = _empty_planes(w, h), _empty_planes(w, h), _empty_planes(w, h)
        st = cairo.lib().cairo_kat_convert(0, fmt, w, h, 0, frame.ctypes.data, *(p.ctypes.data for p in a), 0)
        assert st == 0
        _kat(cairo, 0, fmt, (cr.FULL, cr.BT601), w, h, 0, frame, *b)
        _kat(cairo, 0, fmt, (cr.LIMITED, cr.BT709), w, h, 0, frame, *c)
        for k in range(3):
            assert np.array_equal(a[k], b[k])
            assert np.array_equal(a[k], c[k]) == (fmt == ref.RGB24)
    bad = cairo.lib().cairo_kat_convert_color(0, ref.NV12, 2, 0, w, h, 0, frame.ctypes.data,
                                              *(p.ctypes.data for p in a), 0)
    assert bad == cairo.EVX_ERROR_INVALID_ARGS


# ---------------------------------------------------------------------------
# 3. Encoder parity with the mapped frame
# ---------------------------------------------------------------------------

def _raw_frames(orc, kind, w, h, n, fmt, pitch=0, fill=0):
    """The content's own source planes as raw I420 / NV12 bytes, to be
    *interpreted* under a description."""
    return [ref.planes_to_frame(*ref.oracle_input_planes(orc, ref.make_frame(kind, w, h, t)), fmt, w, h, pitch, fill)
            for t in range(n)]


def _encode_all(cairo, ctx, items, metrics=False):
    """items: (frame or device address, submit kwargs, description or None) per
    frame, I then P -> per frame the table, the coefficient planes, the payload
    and, with metrics, frame_metrics.  The description is set before each
    submit, so a launch of several frames mixes them."""
    tks = []
    for t, (frame, kw, desc) in enumerate(items):
        if desc is not None:
            ctx.set_input_color(*desc)
        tks.append(ctx.submit(frame, t, t > 0, Q, **kw))
    out = []
    for tk in tks:
        o = ctx.wait(tk)
        rec = dict(table=o.table.copy(), coef=(o.coef_y.copy(), o.coef_u.copy(), o.coef_v.copy()))
        rec["payload"] = cairo.serialize_slice(rec["table"], ctx.wmb, ctx.hmb, ctx.ring, *rec["coef"])
        if metrics:
            rec["metrics"] = ctx.frame_metrics(tk)
        ctx.release(tk)
        out.append(rec)
    return out


def _same(got, want, tag):
    assert len(got) == len(want)
    for t, (g, x) in enumerate(zip(got, want)):
        _table_equal(g["table"], x["table"], f"{tag} frame {t}: block table")
        for a, b, n in zip(g["coef"], x["coef"], "YUV"):
            np.testing.assert_array_equal(a, b, err_msg=f"{tag} frame {t}: coef {n}")
        assert g["payload"] == x["payload"], f"{tag} frame {t}: payload bits"
        if "metrics" in g:
            assert g["metrics"] == x["metrics"], f"{tag} frame {t}: frame_metrics"


@pytest.mark.parametrize("kind", ("band4", "noise"))
@pytest.mark.parametrize("size", ref.ENC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encoder_parity_with_mapped_frame(orc, cairo, size, kind):
    """I + 3 P at q = 16, R = 4: a context with set_input_color(c) fed the raw
    frame gives the bits of a fresh default context fed map_frame(frame, 0, c);
    host I420 frames, and device NV12 frames with metrics on."""
    w, h = size
    n = ref.ENC_FRAMES
    raw = {fmt: _raw_frames(orc, kind, w, h, n, fmt) for fmt in YUV}
    if kind == "noise":
        assert min(f[:w * h].min() for f in raw[ref.I420]) < 16 and max(f[:w * h].max() for f in raw[ref.I420]) > 235
    dev = _DeviceBuffer(n * raw[ref.NV12][0].nbytes)
    try:
        for desc in cr.NON_IDENTITY:
            tag = f"{kind} {w}x{h} {_cname(desc)}"
            plain = cairo.Context(w, h, RING, stages=8)
            plain.set_metrics()
            mapped = [cr.map_frame(f, ref.I420, w, h, 0, 0, *desc) for f in raw[ref.I420]]
            want = _encode_all(cairo, plain, [(f, dict(fmt=ref.I420), None) for f in mapped], metrics=True)
            plain.close()
            ctx = cairo.Context(w, h, RING, stages=8)
            ctx.set_input_color(*desc)
            got = _encode_all(cairo, ctx, [(f, dict(fmt=ref.I420), None) for f in raw[ref.I420]])
            _same(got, want, f"{tag} host i420")
            ctx.reset()  # the description survives a reset
            ctx.set_metrics()
            ptrs = [dev.upload(f, offset=t * f.nbytes) for t, f in enumerate(raw[ref.NV12])]
            got = _encode_all(cairo, ctx, [(p, dict(fmt=ref.NV12, on_device=True), None) for p in ptrs], metrics=True)
            _same(got, want, f"{tag} device nv12")
            ctx.close()
    finally:
        dev.free()


# ---------------------------------------------------------------------------
# 4. A mixed launch
# ---------------------------------------------------------------------------

def test_mixed_launch(orc, cairo):
    """Six frames of one launch alternate descriptions and formats, host and
    device, tight and pitched, with an RGB24 frame submitted while a
    description is set (ignored)."""
    w, h = 70, 34
    n = 6
    rgbs = [ref.make_frame("band4", w, h, t) for t in range(n)]
    plan = [(ref.NV12, (cr.LIMITED, cr.BT709), False, 0), (ref.I420, (cr.FULL, cr.BT709), True, 1),
            (ref.RGB24, (cr.LIMITED, cr.BT601), False, 0), (ref.NV12, (cr.LIMITED, cr.BT601), True, 1),
            (ref.I420, (cr.FULL, cr.BT601), False, 0), (ref.NV12, (cr.LIMITED, cr.BT709), True, 0)]
    devs = []

    def items(mapped):
        out = []
        for t, (fmt, desc, on_dev, pk) in enumerate(plan):
            pitch = _pitches(fmt, w)[pk]
            if fmt == ref.RGB24:
                frame = ref.rgb_to_frame(rgbs[t], fmt, pitch, 0xFF)
                frame = frame.reshape(h, w, 3) if not pitch else frame
            else:
                frame = ref.planes_to_frame(*ref.oracle_input_planes(orc, rgbs[t]), fmt, w, h, pitch, 0xFF)
                if mapped:
                    frame = cr.map_frame(frame, fmt, w, h, pitch, 0, *desc)
            kw = dict(fmt=fmt, pitch=pitch)
            if on_dev:
                devs.append(_DeviceBuffer(frame.nbytes))
                frame = devs[-1].upload(frame.reshape(-1))
                kw["on_device"] = True
            out.append((frame, kw, None if mapped else desc))
        return out

    try:
        results = []
        for mapped in (True, False):
            ctx = cairo.Context(w, h, RING, stages=16)
            ctx.set_batch(n)
            results.append(_encode_all(cairo, ctx, items(mapped)))
            ctx.close()
        _same(results[1], results[0], "mixed launch")
    finally:
        for d in devs:
            d.free()


# ---------------------------------------------------------------------------
# 5. Scaled submit: scaled first, on the samples as stored, then mapped
# ---------------------------------------------------------------------------

def test_scaled_submit(orc, cairo):
    sw, sh, w, h = 704, 576, 352, 288
    desc = (cr.LIMITED, cr.BT709)
    raw = _raw_frames(orc, "band4", sw, sh, 2, ref.NV12)
    dev = _DeviceBuffer(2 * raw[0].nbytes)
    try:
        ptrs = [dev.upload(f, offset=t * f.nbytes) for t, f in enumerate(raw)]
        for crop in (None, (32, 16, 640, 544)):
            scaled = [scale_ref.scaled_frame(f, ref.NV12, 0, ((sw, sh), crop), w, h) for f in raw]
            plain = cairo.Context(w, h, RING, stages=8)
            want = _encode_all(cairo, plain, [(cr.map_frame(f, ref.NV12, w, h, 0, 0, *desc), dict(fmt=ref.NV12), None)
                                              for f in scaled])
            plain.close()
            ctx = cairo.Context(w, h, RING, stages=8)
            ctx.set_input_color(*desc)
            got = _encode_all(cairo, ctx, [(p, dict(fmt=ref.NV12, on_device=True, src_size=(sw, sh), crop=crop), None)
                                           for p in ptrs])
            ctx.close()
            _same(got, want, f"scaled submit crop {crop}")
    finally:
        dev.free()


# ---------------------------------------------------------------------------
# 6. Output side
# ---------------------------------------------------------------------------

def _decode_fmt(cairo, ctx, rec, index, fmt, pitch):
    """cairo_ctx_decode_frame_fmt into a buffer prefilled with 0xA5."""
    out = np.full(ref.layout(fmt, ctx.width, ctx.height, pitch)[0], 0xA5, np.uint8)
    t = np.ascontiguousarray(rec["table"]).view(np.uint8)
    coef = np.concatenate([np.ascontiguousarray(p, dtype=np.int16).ravel() for p in rec["coef"]])
    assert cairo.table_check(rec["table"], ctx.wmb, ctx.hmb, ctx.ring)
    st = cairo.lib().cairo_ctx_decode_frame_fmt(ctx.h, t.ctypes.data, coef.ctypes.data, index, fmt, pitch, out.ctypes.data)
    assert st == 0, f"cairo_ctx_decode_frame_fmt status {st}"
    return out


@pytest.mark.parametrize("size", ref.DEC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_output_color(cairo, size):
    """cairo_ctx_decode_frame_fmt and fetch_recon after set_output_color(c)
    equal map_frame(identity output, 1, c), the padding untouched; RGB24 output
    is what it is without a description."""
    w, h = size
    n = ref.DEC_FRAMES
    enc = cairo.Context(w, h, RING, stages=8)
    enc.set_metrics(sse=False, ssim=False, keep_recon=True)
    tks = [enc.submit(ref.make_frame("noise", w, h, t), t, t > 0, Q) for t in range(n)]
    recs = []
    for tk in tks:
        o = enc.wait(tk)
        recs.append(dict(table=o.table.copy(), coef=(o.coef_y.copy(), o.coef_u.copy(), o.coef_v.copy())))
    layouts = [(fmt, p) for fmt in YUV for p in _pitches(fmt, w)]
    try:
        # fetch_recon of the kept last frame: the description may change between fetches
        for fmt, pitch in layouts:
            enc.set_output_color(cr.FULL, cr.BT601)
            identity = enc.fetch_recon(tks[-1], fmt, pitch, out=np.full(ref.layout(fmt, w, h, pitch)[0], 0xA5, np.uint8))
            for desc in cr.NON_IDENTITY:
                enc.set_output_color(*desc)
                got = enc.fetch_recon(tks[-1], fmt, pitch, out=np.full(identity.size, 0xA5, np.uint8))
                np.testing.assert_array_equal(got, cr.map_frame(identity, fmt, w, h, pitch, 1, *desc),
                                              err_msg=f"fetch_recon {ref.FMT_NAMES[fmt]} pitch {pitch} {_cname(desc)}")
        rgb = enc.fetch_recon(tks[-1], ref.RGB24)
        enc.set_output_color(cr.FULL, cr.BT601)
        np.testing.assert_array_equal(enc.fetch_recon(tks[-1], ref.RGB24), rgb, err_msg="fetch_recon rgb24")
        for tk in tks:
            enc.release(tk)
    finally:
        enc.close()
    # a frame is decoded once per context: four contexts (the identity's never calls the setter) per layout
    for fmt, pitch in layouts + [(ref.RGB24, 0)]:
        decs = {d: cairo.Context(w, h, RING, stages=8) for d in cr.DESCRIPTIONS}
        try:
            for d in cr.NON_IDENTITY:
                decs[d].set_output_color(*d)
            m = ref.image_mask(fmt, w, h, pitch)
            for t, rec in enumerate(recs):
                identity = _decode_fmt(cairo, decs[(cr.FULL, cr.BT601)], rec, t, fmt, pitch)
                assert (identity[~m] == 0xA5).all()
                for desc in cr.NON_IDENTITY:
                    got = _decode_fmt(cairo, decs[desc], rec, t, fmt, pitch)
                    np.testing.assert_array_equal(got, cr.map_frame(identity, fmt, w, h, pitch, 1, *desc),
                                                  err_msg=f"decode frame {t} {ref.FMT_NAMES[fmt]} pitch {pitch} {_cname(desc)}")
        finally:
            for c in decs.values():
                c.close()


# ---------------------------------------------------------------------------
# 7. Drop-in classes and the pipeline
# ---------------------------------------------------------------------------

def _dropin_stream(cairo, frames, fmt, w, h, desc=None):
    enc = cairo.Encoder(ring=RING)
    enc.set_quality(Q)
    enc.set_input_format(fmt)
    if desc is not None:
        enc.set_input_color(*desc)
    bs = cairo.BitStream(w * h * 64 + 65536)
    out = []
    for t, f in enumerate(frames):
        bs.empty()
        enc.encode(f, bs, w, h)
        data = bytearray(bs.data())
        if t == 0:
            data[7] = 0  # the header's unwritten pad byte
        out.append((bytes(data), bs.bits()))
    enc.close()
    return out


def test_dropin_and_pipeline(orc, cairo):
    w, h, n = 352, 288, 4
    raw = {fmt: _raw_frames(orc, "band4", w, h, n, fmt) for fmt in YUV}
    for desc in cr.NON_IDENTITY:
        mapped = {fmt: [cr.map_frame(f, fmt, w, h, 0, 0, *desc) for f in raw[fmt]] for fmt in YUV}
        # Encoder.set_input_color, set before the first frame (I420) and between frames (NV12)
        want = _dropin_stream(cairo, mapped[ref.I420], ref.I420, w, h)
        assert _dropin_stream(cairo, raw[ref.I420], ref.I420, w, h, desc) == want, f"Encoder {_cname(desc)}"
        enc = cairo.Encoder(ring=RING)
        enc.set_quality(Q)
        enc.set_input_format(ref.NV12)
        bs = cairo.BitStream(w * h * 64 + 65536)
        for t in range(n):  # frames 0 and 1 mapped by the caller, 2 and 3 by the encoder
            if t == 2:
                enc.set_input_color(*desc)
            bs.empty()
            enc.encode((mapped if t < 2 else raw)[ref.NV12][t], bs, w, h)
            data = bytearray(bs.data())
            if t == 0:
                data[7] = 0
            assert (bytes(data), bs.bits()) == want[t], f"Encoder, description set at frame 2: frame {t} {_cname(desc)}"
        enc.close()

        # Decoder.set_output_color
        plain, col = cairo.Decoder(), cairo.Decoder()
        pitch = w + 3
        for d in (plain, col):
            d.set_output_format(ref.NV12, pitch)
        col.set_output_color(*desc)
        for t, (data, nbits) in enumerate(want):
            outs = []
            for d in (plain, col):
                bs.empty()
                bs.write(data, nbits)
                outs.append(d.decode(bs, w, h, out=np.full(ref.layout(ref.NV12, w, h, pitch)[0], 0xA5, np.uint8)))
            np.testing.assert_array_equal(outs[1], cr.map_frame(outs[0], ref.NV12, w, h, pitch, 1, *desc),
                                          err_msg=f"Decoder frame {t} {_cname(desc)}")
        plain.close()
        col.close()

        # a Stream over a context with an input description
        def pipeline(frames, d):
            ctx = cairo.Context(w, h, RING, stages=16)
            ctx.set_batch(2)
            if d is not None:
                ctx.set_input_color(*d)
            st = cairo.Stream(ctx, threads=2)
            tks = [st.submit(f, t, t > 0, Q, fmt=ref.NV12) for t, f in enumerate(frames)]
            out = [st.collect(tk) for tk in tks]
            st.close()
            ctx.close()
            return out

        assert pipeline(raw[ref.NV12], desc) == pipeline(mapped[ref.NV12], None), f"Stream {_cname(desc)}"


# ---------------------------------------------------------------------------
# 8. The default is untouched
# ---------------------------------------------------------------------------

def test_explicit_identity_equals_default(orc, cairo):
    w, h, n = 70, 34, 3
    rgbs = [ref.make_frame("band4", w, h, t) for t in range(n)]
    nv12 = _raw_frames(orc, "band4", w, h, n, ref.NV12)
    for frames, kw in ((rgbs, dict()), (nv12, dict(fmt=ref.NV12))):
        res = []
        for explicit in (False, True):
            ctx = cairo.Context(w, h, RING, stages=8)
            if explicit:
                ctx.set_input_color(cairo.RANGE_FULL, cairo.MATRIX_BT601)
            res.append(_encode_all(cairo, ctx, [(f, kw, None) for f in frames]))
            ctx.close()
        _same(res[1], res[0], f"explicit identity {kw}")
    ctx = cairo.Context(w, h, RING, stages=8)
    try:
        for bad in ((2, 0), (0, 2), (-1, 0)):
            for fn in (ctx.set_input_color, ctx.set_output_color):
                with pytest.raises(cairo.CairoError) as ei:
                    fn(*bad)
                assert ei.value.status == cairo.EVX_ERROR_INVALID_ARGS
    finally:
        ctx.close()
