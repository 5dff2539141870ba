"""Pixel formats on the GPU (pixfmt.hip, cairo_ctx_submit_fmt and friends).

KAT: k_convert_fmt_batch and k_planes_to_fmt on their own (cairo_kat_convert)
against the oracle's convert (RGB, BGR) or the numpy restatement
(tests/pixfmt_ref.py: I420, NV12), at sizes and values the encoder never makes.
Then the same bits as the RGB24 path, whatever the format a frame comes in:
every intermediate against the oracle, streams against the RGB24 run, the
decoder's output in every format, and the refusal of a frame that does not fit
its allocation.

The I420 / NV12 inputs are built from the oracle's input planes; that they fit
8 bits is checked in tests/test_pixfmt.py::test_gpu_inputs_fit_8_bits.
"""
import ctypes

import numpy as np
import pytest

from tests import pixfmt_ref as ref

pytestmark = pytest.mark.gpu

FMTS = (ref.RGB24, ref.BGR24, ref.I420, ref.NV12)
NEW_FMTS = (ref.BGR24, ref.I420, ref.NV12)
_id = lambda f: ref.FMT_NAMES[f]  # noqa: E731
# 70x34: chroma width 35 is odd, nothing is a multiple of 4.  4100x4: a row
# spans five workgroups (a workgroup of k_convert_fmt_batch covers 1024 luma
# columns) and ends in a strip cut by the right edge.
KAT_SIZES = ((2, 2), (16, 16), (70, 34), (4100, 4))


def _pitches(fmt, w):
    """Tight, and a pitch 2 (I420, which needs an even one) or 3 bytes wider."""
    tight = ref.layout(fmt, w, 2)[1]
    return (0, tight + (2 if fmt == ref.I420 else 3))


class _DeviceBuffer:
    """Device memory from the HIP runtime the library itself uses (by soname:
    the copy already loaded into this process; a second runtime, such as the
    one bundled with torch, sees no GPU once this one holds it)."""

    def __init__(self, nbytes: int, fill: int = 0xFF):
        self.hip = ctypes.CDLL("libamdhip64.so.7")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), nbytes) == 0
        self.ptr, self.nbytes = p.value, nbytes
        self.upload(np.full(nbytes, fill, np.uint8))

    def upload(self, a: np.ndarray, offset: int = 0) -> int:
        """Synchronous host-to-device copy at a byte offset -> the device address."""
        a = np.ascontiguousarray(a)
        assert a.dtype == np.uint8 and offset + a.nbytes <= self.nbytes
        assert self.hip.hipMemcpy(self.ptr + offset, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return self.ptr + offset

    def free(self) -> None:
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = None


def _kat(cairo, direction, fmt, w, h, pitch, frame, y, u, v):
    for a in (frame, y, u, v):
        assert a.flags["C_CONTIGUOUS"]
    assert frame.dtype == np.uint8 and y.dtype == u.dtype == v.dtype == np.int16
    assert frame.size == ref.layout(fmt, w, h, pitch)[0] and y.shape == (h, w) and u.shape == v.shape == (h // 2, w // 2)
    st = cairo.lib().cairo_kat_convert(direction, fmt, w, h, pitch, frame.ctypes.data, y.ctypes.data, u.ctypes.data,
                                       v.ctypes.data, 0)
    assert st == 0, f"cairo_kat_convert status {st}"


def _tight_convert(orc, rgb):
    """orc_convert_rgb into tight planes (w and w / 2 elements per row)."""
    h, w = rgb.shape[:2]
    y, u, v = np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)
    rgb = np.ascontiguousarray(rgb)
    orc.lib().orc_convert_rgb(rgb.ctypes.data, w, h, y.ctypes.data, u.ctypes.data, v.ctypes.data, w, h)
    return y, u, v


# ---------------------------------------------------------------------------
# KAT, input side
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("size", KAT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", FMTS, ids=_id)
def test_kat_input(orc, cairo, fmt, size):
    w, h = size
    rng = np.random.default_rng(1000 * fmt + w)
    for pitch in _pitches(fmt, w):
        for variant in range(2):
            if fmt in (ref.RGB24, ref.BGR24):
                rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                blue, red = (0, 0, 255), (255, 0, 0)  # U = 256 / V = 256 before the 2x2 mean; bytes 0 and 255
                rgb[0:2, 0:2] = blue if variant == 0 else red
                if w >= 4:
                    rgb[0:2, 2:4] = red if variant == 0 else blue
                    rgb[h - 2:h, w - 2:w] = blue if variant == 0 else red  # the strip cut by the right edge
                frame = ref.rgb_to_frame(rgb, fmt, pitch, fill=0xFF)
                want = _tight_convert(orc, rgb)
                assert max(want[1].max(), want[2].max()) == 256
            else:
                frame = rng.integers(0, 256, ref.layout(fmt, w, h, pitch)[0], dtype=np.uint8)
                frame[~ref.image_mask(fmt, w, h, pitch)] = 0xFF
                vw = ref.views(frame, fmt, w, h, pitch)
                lo, hi = (0, 255) if variant == 0 else (255, 0)
                vw[0][0, 0], vw[0][-1, -1] = lo, hi
                if fmt == ref.I420:
                    vw[1][0, 0], vw[2][0, 0], vw[1][-1, -1], vw[2][-1, -1] = lo, hi, hi, lo
                else:
                    vw[1][0, 0], vw[1][-1, -1] = (lo, hi), (hi, lo)
                want = ref.frame_to_planes(frame, fmt, w, h, pitch)
            y, u, v = np.full((h, w), -1, np.int16), np.full((h // 2, w // 2), -1, np.int16), \
                np.full((h // 2, w // 2), -1, np.int16)
            before = frame.copy()
            _kat(cairo, 0, fmt, w, h, pitch, frame, y, u, v)
            tag = f"{ref.FMT_NAMES[fmt]} {w}x{h} pitch {pitch} variant {variant}"
            np.testing.assert_array_equal(y, want[0], err_msg=f"{tag}: Y")
            np.testing.assert_array_equal(u, want[1], err_msg=f"{tag}: U")
            np.testing.assert_array_equal(v, want[2], err_msg=f"{tag}: V")
            np.testing.assert_array_equal(frame, before, err_msg=f"{tag}: the source frame")


def test_default_rgb24_path_equals_its_restatements(orc, cairo):
    """The default input path (tight RGB24 through Context.submit: k_convert_batch)
    on bytes the encoder tests never feed it, against both restatements of its
    rule: tests/pixfmt_ref.py (and, through it, the oracle's convert) and the
    strip kernel (cairo_kat_convert, RGB24).  70x34: chroma width 35, wa != w,
    nothing a multiple of 4.  1030x18: 515 quad columns, so a row spans three of
    k_convert_batch's 256-thread workgroups and the last holds three threads;
    wa = 1040."""
    corners = ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255))
    n = 0
    for w, h in ((70, 34), (1030, 18)):
        rng = np.random.default_rng(3000 + w)
        ctx = cairo.Context(w, h, 4, stages=8)
        try:
            for t in range(2):  # two intra frames
                rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
                rgb[0, 0] = rgb[h - 1, w - 1] = corners[n % 4]
                n += 1
                frame = ref.rgb_to_frame(rgb, ref.RGB24)
                ctx.encode_frame(rgb, t, False, 16)  # Context.submit with its defaults, wait, release
                got = [p[:ph, :pw] for p, (ph, pw) in
                       zip(ctx.read_planes(0), ((h, w), (h // 2, w // 2), (h // 2, w // 2)))]
                want = ref.frame_to_planes(frame, ref.RGB24, w, h)
                for a, b in zip(want, _tight_convert(orc, rgb)):
                    np.testing.assert_array_equal(a, b, err_msg="the numpy restatement against the oracle")
                strip = (np.full((h, w), -1, np.int16), np.full((h // 2, w // 2), -1, np.int16),
                         np.full((h // 2, w // 2), -1, np.int16))
                _kat(cairo, 0, ref.RGB24, w, h, 0, frame, *strip)
                for g, wn, s, name in zip(got, want, strip, "YUV"):
                    tag = f"{w}x{h} frame {t} {name}"
                    np.testing.assert_array_equal(g, wn, err_msg=f"{tag}: k_convert_batch against pixfmt_ref")
                    np.testing.assert_array_equal(g, s, err_msg=f"{tag}: k_convert_batch against the strip kernel")
        finally:
            ctx.close()


# ---------------------------------------------------------------------------
# KAT, output side
# ---------------------------------------------------------------------------

def _arbitrary_planes(rng, w, h, variant):
    """int16 planes well outside what an encoder stores: luma below 16 and
    above 271, chroma below 0 and above 255, and the int16 extremes."""
    y = rng.integers(-300, 700, (h, w)).astype(np.int16)
    u = rng.integers(-300, 600, (h // 2, w // 2)).astype(np.int16)
    v = rng.integers(-300, 600, (h // 2, w // 2)).astype(np.int16)
    ey = (15, 16, 271, 272, -32768, 32767, 0, 255)
    ec = (-1, 0, 255, 256, -32768, 32767, 128, 127)
    for k in range(min(len(ey), w * h)):
        y.reshape(-1)[-1 - k if variant else k] = ey[(k + 4 * variant) % len(ey)]
    for k in range(min(len(ec), u.size)):
        u.reshape(-1)[-1 - k if variant else k] = ec[(k + variant) % len(ec)]
        v.reshape(-1)[-1 - k if variant else k] = ec[(k + 3 + variant) % len(ec)]
    return y, u, v


@pytest.mark.parametrize("size", KAT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", FMTS, ids=_id)
def test_kat_output(cairo, fmt, size):
    w, h = size
    rng = np.random.default_rng(2000 * fmt + w)
    for pitch in _pitches(fmt, w):
        for variant in range(2):
            y, u, v = _arbitrary_planes(rng, w, h, variant)
            if fmt in (ref.RGB24, ref.BGR24):
                want = ref.rgb_to_frame(cairo.yuv_to_rgb(y, u, v, w, h), fmt, pitch, fill=0xA5)
            else:
                want = ref.planes_to_frame(y, u, v, fmt, w, h, pitch, fill=0xA5)
            frame = np.full(want.size, 0xA5, np.uint8)
            _kat(cairo, 1, fmt, w, h, pitch, frame, y, u, v)
            tag = f"{ref.FMT_NAMES[fmt]} {w}x{h} pitch {pitch} variant {variant}"
            m = ref.image_mask(fmt, w, h, pitch)
            np.testing.assert_array_equal(frame[m], want[m], err_msg=f"{tag}: image")
            assert (frame[~m] == 0xA5).all(), f"{tag}: pitch padding written"


def test_kat_rgb24_equals_k_yuv_to_rgb(orc, cairo):
    """RGB24 through k_planes_to_fmt equals k_yuv_to_rgb: the decoder's frame
    through cairo_ctx_decode_frame_fmt(RGB24) and through cairo_ctx_decode_frame."""
    w, h, ring, q = 70, 34, 4, 16
    enc = cairo.Encoder(ring=ring)
    enc.set_quality(q)
    old, tight, pitched = cairo.Decoder(), cairo.Decoder(), cairo.Decoder()
    tight.set_output_format(cairo.FMT_RGB24, 3 * w)  # an explicit pitch, tight or not, takes the new kernel
    pitched.set_output_format(cairo.FMT_RGB24, 3 * w + 1)
    bs, bs2 = cairo.BitStream(w * h * 64 + 65536), cairo.BitStream(w * h * 64 + 65536)
    for t in range(3):
        bs.empty()
        enc.encode(orc.make_frame(w, h, t), bs)
        data, nbits = bs.data(), bs.bits()
        a = old.decode(bs, w, h)
        for dec, pitch in ((tight, 3 * w), (pitched, 3 * w + 1)):
            bs2.empty()
            bs2.write(data, nbits)
            b = cairo.split_frame(dec.decode(bs2, w, h), cairo.FMT_RGB24, w, h, pitch)
            np.testing.assert_array_equal(a, b, err_msg=f"frame {t} pitch {pitch}")
    for x in (old, tight, pitched, enc):
        x.close()


# ---------------------------------------------------------------------------
# Encoder parity: a frame in any format gives the oracle's bits
# ---------------------------------------------------------------------------

def _table_equal(a, b, what):
    for f in a.dtype.names:
        if f == "pad":
            continue
        bad = np.nonzero(a[f] != b[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at MBs {bad[:10]} gpu={a[f][bad[:5]]} ref={b[f][bad[:5]]}"


def _oracle_run(orc, kind, w, h, ring, q, frames):
    """The oracle's intermediates of I + (frames - 1) P: per frame the RGB
    frame, planes(0), the block table, planes(1) and the deblocked slot."""
    e = orc.OracleEncoder(ring)
    e.set_quality(q)
    out = []
    for t in range(frames):
        rgb = ref.make_frame(kind, w, h, t)
        e.encode(rgb)
        cp = lambda p: tuple(a.copy() for a in p)  # noqa: E731
        out.append(dict(rgb=rgb, src=cp(e.planes(0)), table=e.block_table().copy(), coef=cp(e.planes(1)),
                        recon=cp(e.planes(2 + t % ring))))
    return out


def _frame_of(rec, fmt, w, h, pitch=0, fill=0):
    if fmt in (ref.RGB24, ref.BGR24):
        return ref.rgb_to_frame(rec["rgb"], fmt, pitch, fill)
    return ref.planes_to_frame(*rec["src"], fmt, w, h, pitch, fill)


def _check_frame(ctx, out, rec, t, ring, tag, planes=True):
    _table_equal(out.table, rec["table"], f"{tag}: block table")
    for got, want, n in zip((out.coef_y, out.coef_u, out.coef_v), rec["coef"], "YUV"):
        np.testing.assert_array_equal(got, want, err_msg=f"{tag}: coef {n}")
    if planes:
        for got, want, n in zip(ctx.read_planes(0), rec["src"], "YUV"):  # wa x ha: the padding stays zero
            np.testing.assert_array_equal(got, want, err_msg=f"{tag}: input {n}")
        for got, want, n in zip(ctx.read_planes(2 + t % ring), rec["recon"], "YUV"):
            np.testing.assert_array_equal(got, want, err_msg=f"{tag}: recon {n} (deblocked)")


def _run_format(cairo, ctx, recs, fmt, w, h, ring, q, tag, make=None):
    """I + P through Context.encode_frame(fmt=...) on a fresh encoder state;
    make(rec, t) -> (frame, kwargs) overrides how a frame is handed over."""
    ctx.reset()
    keep = []
    for t, rec in enumerate(recs):
        frame, kw = make(rec, t) if make else (_frame_of(rec, fmt, w, h), dict(fmt=fmt))
        keep.append(frame)
        out = ctx.encode_frame(frame, t, t > 0, q, **kw)
        _check_frame(ctx, out, rec, t, ring, f"{tag} {ref.FMT_NAMES[fmt]} frame {t}")


@pytest.mark.parametrize("kind", ref.ENC_KINDS)
@pytest.mark.parametrize("q", [1, 16, 31])
@pytest.mark.parametrize("size", ref.ENC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_encoder_parity(orc, cairo, size, q, kind):
    w, h = size
    ring = 4
    recs = _oracle_run(orc, kind, w, h, ring, q, ref.ENC_FRAMES)
    ctx = cairo.Context(w, h, ring, stages=8)
    try:
        for fmt in NEW_FMTS:
            _run_format(cairo, ctx, recs, fmt, w, h, ring, q, f"{kind} {w}x{h} q={q}")
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def odd_recs(orc):
    """The oracle's run of band4 70x34, q = 16, 6 frames (computed once)."""
    return _oracle_run(orc, "band4", 70, 34, 4, 16, 6)


@pytest.mark.parametrize("fmt", FMTS, ids=_id)
def test_encoder_parity_pitched_host(cairo, odd_recs, fmt):
    """A pitched host frame (packed into the staging slot on upload), the pitch
    padding filled with 0xFF."""
    w, h, ring, q = 70, 34, 4, 16
    pitch = _pitches(fmt, w)[1]
    ctx = cairo.Context(w, h, ring, stages=8)
    try:
        _run_format(cairo, ctx, odd_recs[:4], fmt, w, h, ring, q, f"pitched host, pitch {pitch}",
                    make=lambda rec, t: (_frame_of(rec, fmt, w, h, pitch, 0xFF), dict(fmt=fmt, pitch=pitch)))
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", FMTS, ids=_id)
def test_encoder_parity_device_odd_base(cairo, odd_recs, fmt):
    """An on-device frame read in place at an odd base address (byte 1 of a
    device allocation) with a pitch 3 (I420: 2) bytes wider than tight."""
    w, h, ring, q = 70, 34, 4, 16
    pitch = _pitches(fmt, w)[1]
    nb = ref.layout(fmt, w, h, pitch)[0]
    ctx = cairo.Context(w, h, ring, stages=8)
    held = []

    def make(rec, t):
        buf = _DeviceBuffer(nb + 1)
        held.append(buf)
        ptr = buf.upload(_frame_of(rec, fmt, w, h, pitch, 0xFF), offset=1)
        assert ptr % 2 == 1
        return ptr, dict(fmt=fmt, pitch=pitch, on_device=True)

    try:
        _run_format(cairo, ctx, odd_recs[:4], fmt, w, h, ring, q, f"device frame at an odd base, pitch {pitch}", make=make)
    finally:
        ctx.close()
        for b in held:
            b.free()


def test_encoder_parity_mixed_launch(cairo, odd_recs):
    """One launch of 6 frames cycling through all four formats, host and
    device, tight and pitched."""
    w, h, ring, q = 70, 34, 4, 16
    ctx = cairo.Context(w, h, ring, stages=16)
    ctx.set_batch(6)
    held, devs, tickets = [], [], []
    try:
        for t, rec in enumerate(odd_recs):
            fmt = FMTS[t % 4]
            pitch = _pitches(fmt, w)[t // 2 % 2]
            frame = _frame_of(rec, fmt, w, h, pitch, 0xFF)
            if fmt == ref.RGB24 and not pitch:
                frame = frame.reshape(h, w, 3)  # today's format keeps today's shape check
            if t % 2:  # odd frames live on the device
                dev = _DeviceBuffer(frame.nbytes)
                devs.append(dev)
                tickets.append(ctx.submit(dev.upload(frame), t, t > 0, q, on_device=True, fmt=fmt, pitch=pitch))
            else:
                held.append(frame)
                tickets.append(ctx.submit(frame, t, t > 0, q, fmt=fmt, pitch=pitch))
        for t, tk in enumerate(tickets):
            out = ctx.wait(tk)
            _check_frame(ctx, out, odd_recs[t], t, ring, f"mixed launch frame {t}", planes=False)
            ctx.release(tk)
        last = len(odd_recs) - 1
        for got, want, n in zip(ctx.read_planes(0), odd_recs[last]["src"], "YUV"):
            np.testing.assert_array_equal(got, want, err_msg=f"mixed launch: input {n} of the last frame")
        for k in range(ring):  # frames 2..5 are in the ring
            t = max(tt for tt in range(len(odd_recs)) if tt % ring == k)
            for got, want, n in zip(ctx.read_planes(2 + k), odd_recs[t]["recon"], "YUV"):
                np.testing.assert_array_equal(got, want, err_msg=f"mixed launch: recon {n} of frame {t}")
    finally:
        ctx.close()
        for b in devs:
            b.free()


def test_encoder_parity_720p_nv12(orc, cairo):
    """A row spans two workgroups of the convert inside a real context."""
    kind, w, h, frames = ref.BIG_CASE
    ring, q = 4, 16
    recs = _oracle_run(orc, kind, w, h, ring, q, frames)
    ctx = cairo.Context(w, h, ring, stages=8)
    try:
        _run_format(cairo, ctx, recs, ref.NV12, w, h, ring, q, "720p")
    finally:
        ctx.close()


# ---------------------------------------------------------------------------
# Streams: the same payload bits as the RGB24 run of the same frames
# ---------------------------------------------------------------------------

def test_streams_equal_rgb24_run(orc, cairo):
    kind, w, h, n = ref.STREAM_CASE
    ring, q = 4, 16
    rgbs = [ref.make_frame(kind, w, h, t) for t in range(n)]
    planes = [ref.oracle_input_planes(orc, f) for f in rgbs]

    def pipeline(frames, **kw):
        ctx = cairo.Context(w, h, ring, stages=16)
        ctx.set_batch(3)
        st = cairo.Stream(ctx, threads=2)
        tks = [st.submit(f, t, t > 0, q, **kw) for t, f in enumerate(frames)]
        out = [st.collect(tk) for tk in tks]
        st.close()
        ctx.close()
        return out

    want = pipeline(rgbs)
    got = pipeline([ref.planes_to_frame(*p, ref.NV12, w, h) for p in planes], fmt=cairo.FMT_NV12)
    assert got == want, "Stream.submit(fmt=FMT_NV12) payloads differ from the RGB24 run"
    assert all(nb > 0 for _, nb in want)

    def dropin(frames, fmt):
        enc = cairo.Encoder(ring=ring)
        enc.set_quality(q)
        if fmt is not None:
            enc.set_input_format(fmt)
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

    assert dropin([ref.planes_to_frame(*p, ref.I420, w, h) for p in planes], cairo.FMT_I420) == dropin(rgbs, None), \
        "Encoder.set_input_format(FMT_I420) stream differs from the RGB24 run"


# ---------------------------------------------------------------------------
# Decoder: every output format, tight and pitched
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", ref.DEC_CASES, ids=lambda c: f"{c[0]}-q{c[1]}")
@pytest.mark.parametrize("size", ref.DEC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decoder_formats(orc, cairo, size, case):
    """Decoding the encoder's stream into each format gives yuv_to_rgb (byte
    swapped for BGR) or the clamp of the oracle's deblocked slot; the pitch
    padding of the caller's buffer keeps its bytes.  black and noise drive luma
    below 16 and above 271, so both luma clamps fire; these contents never
    drive chroma out of 0..255: that clamp is covered by test_kat_output only."""
    (w, h), (kind, q) = size, case
    ring = 4
    e = orc.OracleEncoder(ring)
    e.set_quality(q)
    enc = cairo.Encoder(ring=ring)
    enc.set_quality(q)
    bs = cairo.BitStream(w * h * 64 + 65536)
    recs = []
    for t in range(ref.DEC_FRAMES):
        rgb = ref.make_frame(kind, w, h, t)
        e.encode(rgb)
        bs.empty()
        enc.encode(rgb, bs)
        recs.append((bs.data(), bs.bits(), tuple(a.copy() for a in e.planes(2 + t % ring))))
    enc.close()
    below = sum(int((r[2][0][:h, :w] < 16).sum()) for r in recs)
    above = sum(int((r[2][0][:h, :w] > 271).sum()) for r in recs)
    if kind == "black":
        assert below > 0, "black no longer drives luma below 16: the lower clamp is not exercised"
    if kind == "noise":
        assert below > 0 and above > 0, "noise no longer drives luma past both clamps"
    for fmt in FMTS:
        for pitch in _pitches(fmt, w):
            dec = cairo.Decoder()
            dec.set_output_format(fmt, pitch)
            m = ref.image_mask(fmt, w, h, pitch)
            for t, (data, nbits, (y, u, v)) in enumerate(recs):
                bs.empty()
                bs.write(data, nbits)
                buf = np.full(m.size, 0xA5, np.uint8)
                out = dec.decode(bs, w, h, out=buf)
                assert bs.bits() == 0
                tag = f"{kind} {w}x{h} q={q} {ref.FMT_NAMES[fmt]} pitch {pitch} frame {t}"
                if fmt in (ref.RGB24, ref.BGR24):
                    want = ref.rgb_to_frame(cairo.yuv_to_rgb(y, u, v, w, h), fmt, pitch, fill=0xA5)
                    if not pitch:
                        assert out.shape == (h, w, 3)
                else:
                    want = ref.planes_to_frame(y, u, v, fmt, w, h, pitch, fill=0xA5)
                    assert out.ndim == 1
                np.testing.assert_array_equal(buf[m], want[m], err_msg=f"{tag}: image")
                assert (buf[~m] == 0xA5).all(), f"{tag}: pitch padding written"
            dec.close()


# ---------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------

def test_device_frame_must_fit_its_allocation(orc, cairo):
    """An on-device NV12 frame whose pitch makes frame_layout's size exceed its
    allocation is refused with EVX_ERROR_INVALID_ARGS before any kernel reads
    it, and the context encodes the next valid frame correctly."""
    w, h, ring, q = 64, 48, 4, 16
    recs = _oracle_run(orc, "band4", w, h, ring, q, 2)
    ctx = cairo.Context(w, h, ring, stages=8)
    dev = _DeviceBuffer(ref.layout(ref.NV12, w, h)[0])
    try:
        ptr = dev.upload(_frame_of(recs[0], ref.NV12, w, h))
        pitch = 1 << 24  # 1.2 GB by the layout, in an allocation of 4608 bytes
        assert cairo.frame_layout(cairo.FMT_NV12, w, h, pitch)[0] > 1 << 30
        with pytest.raises(cairo.CairoError) as ei:
            ctx.submit(ptr, 0, False, q, on_device=True, fmt=cairo.FMT_NV12, pitch=pitch)
        assert ei.value.status == cairo.EVX_ERROR_INVALID_ARGS
        with pytest.raises(cairo.CairoError) as ei:  # an odd I420 pitch
            ctx.submit(ptr, 0, False, q, on_device=True, fmt=cairo.FMT_I420, pitch=w + 1)
        assert ei.value.status == cairo.EVX_ERROR_INVALID_ARGS
        with pytest.raises(cairo.CairoError):  # a pitch below the width
            ctx.submit(ptr, 0, False, q, on_device=True, fmt=cairo.FMT_NV12, pitch=w - 2)
        for t, rec in enumerate(recs):
            dev.upload(_frame_of(rec, ref.NV12, w, h))
            out = ctx.encode_frame(ptr, t, t > 0, q, on_device=True, fmt=cairo.FMT_NV12)
            _check_frame(ctx, out, rec, t, ring, f"after the refusals, frame {t}")
    finally:
        ctx.close()
        dev.free()
