"""Capture and 10-bit frames on the GPU: YUY2, UYVY and P010 through
pixfmt.hip, cairo_ctx_submit_fmt and friends.

A frame of one of the three layouts is, by definition, the NV12 frame it folds
to (input) or unfolds from (output); tests/capfmt_ref.py restates both maps
from the header's text.  KAT: the two kernels on their own against the
restatement.  Then the encoder: against the oracle where the frames are
unfolded oracle inputs, and against the NV12 run of the folded frame where the
4:2:2 rows differ or the words carry all 16 bits, from every kind of source.
The decoder's two outputs, the drop-in classes, and the refusals.
"""
import numpy as np
import pytest

from tests import capfmt_ref as cap
from tests import pixfmt_ref as ref
from tests import test_gpu_pixfmt as px  # its helpers: device memory, the oracle's run, the comparisons

pytestmark = pytest.mark.gpu

_id = lambda f: cap.FMT_NAMES[f]  # noqa: E731
# 70x34: the chroma width 35 is odd and the last strip is cut.  4100x4: a row
# spans five workgroups and ends in a cut strip.
KAT_SIZES = ((2, 2), (16, 16), (70, 34), (4100, 4))
LIMITED, BT601, BT709 = 1, 0, 1
DESCS = ((LIMITED, BT709), (LIMITED, BT601))
RING, Q = 4, 16


def _pitches(fmt, w):
    return (0, cap.pitched(fmt, w))


def _kat(cairo, direction, fmt, w, h, pitch, frame, y, u, v, desc=None):
    for a in (frame, y, u, v):
        assert a.flags["C_CONTIGUOUS"]
    assert frame.dtype == np.uint8 and y.dtype == u.dtype == v.dtype == np.int16
    assert frame.size == cairo.frame_layout(fmt, w, h, pitch)[0]
    assert y.shape == (h, w) and u.shape == v.shape == (h // 2, w // 2)
    if desc is None:
        st = cairo.lib().cairo_kat_convert(direction, fmt, w, h, pitch, frame.ctypes.data, y.ctypes.data,
                                           u.ctypes.data, v.ctypes.data, 0)
    else:
        st = cairo.lib().cairo_kat_convert_color(direction, fmt, desc[0], desc[1], w, h, pitch, frame.ctypes.data,
                                                 y.ctypes.data, u.ctypes.data, v.ctypes.data, 0)
    assert st == 0, f"cairo_kat_convert status {st}"


def _empty_planes(w, h):
    return np.full((h, w), -1, np.int16), np.full((h // 2, w // 2), -1, np.int16), \
        np.full((h // 2, w // 2), -1, np.int16)


def _random_frame(rng, fmt, w, h, pitch=0, fill=0xFF):
    """Random bytes in every image byte (P010: all 16 bits of every word)."""
    frame = rng.integers(0, 256, cap.layout(fmt, w, h, pitch)[0], dtype=np.uint8)
    frame[~cap.image_mask(fmt, w, h, pitch)] = fill
    return frame


def _check_input(cairo, frame, fmt, w, h, pitch, tag, desc=None):
    y, u, v = _empty_planes(w, h)
    before = frame.copy()
    _kat(cairo, 0, fmt, w, h, pitch, frame, y, u, v, desc)
    folded = cap.fold(frame, fmt, w, h, pitch)
    if desc is None:
        want = ref.frame_to_planes(folded, ref.NV12, w, h)
    else:  # the NV12 kernel's answer for the folded frame
        want = _empty_planes(w, h)
        _kat(cairo, 0, ref.NV12, w, h, 0, folded, *want, desc)
    for got, exp, n in zip((y, u, v), want, "YUV"):
        np.testing.assert_array_equal(got, exp, err_msg=f"{tag}: {n}")
    np.testing.assert_array_equal(frame, before, err_msg=f"{tag}: the source frame")


# ---------------------------------------------------------------------------
# KAT, input side
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("size", KAT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_kat_input(cairo, fmt, size):
    w, h = size
    rng = np.random.default_rng(1000 * fmt + w)
    for pitch in _pitches(fmt, w):
        for variant in range(2):
            frame = _random_frame(rng, fmt, w, h, pitch)
            vw = cap.views(frame, fmt, w, h, pitch)
            lo, hi = (0, 255) if variant == 0 else (255, 0)
            for plane in vw:  # the extreme bytes (P010: words 0x0000 and 0xFFFF) in the first and the last sample
                plane[0, 0] = lo
                plane[-1, -1] = hi
            _check_input(cairo, frame, fmt, w, h, pitch, f"{cap.FMT_NAMES[fmt]} {w}x{h} pitch {pitch} variant {variant}")


@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_kat_input_exhaustive(cairo, fmt):
    """Every pair of 4:2:2 chroma bytes; every ten-bit value at both half-word
    positions with random low bits."""
    rng = np.random.default_rng(fmt)
    frame, w, h = cap.exhaustive_p010(rng) if fmt == cap.P010 else cap.exhaustive_422(fmt, rng)
    _check_input(cairo, frame, fmt, w, h, 0, f"{cap.FMT_NAMES[fmt]} exhaustive")


# ---------------------------------------------------------------------------
# KAT, output side
# ---------------------------------------------------------------------------

def _wild_planes(rng, w, h):
    """int16 planes that also hold values outside 8 bits, so the clamps run."""
    y = rng.integers(-300, 601, (h, w)).astype(np.int16)
    u = rng.integers(-300, 601, (h // 2, w // 2)).astype(np.int16)
    v = rng.integers(-300, 601, (h // 2, w // 2)).astype(np.int16)
    return y, u, v


def _check_output(cairo, y, u, v, fmt, w, h, pitch, tag, desc=None):
    if desc is None:
        nv12 = ref.planes_to_frame(y, u, v, ref.NV12, w, h)
    else:  # the NV12 kernel's answer
        nv12 = np.zeros(ref.layout(ref.NV12, w, h)[0], np.uint8)
        _kat(cairo, 1, ref.NV12, w, h, 0, nv12, y, u, v, desc)
    want = cap.unfold(nv12, fmt, w, h, pitch, fill=0xA5)
    frame = np.full(want.size, 0xA5, np.uint8)
    _kat(cairo, 1, fmt, w, h, pitch, frame, y, u, v, desc)
    m = cap.image_mask(fmt, w, h, pitch)
    np.testing.assert_array_equal(frame[m], want[m], err_msg=f"{tag}: image")
    assert (frame[~m] == 0xA5).all(), f"{tag}: pitch padding written"
    return frame


@pytest.mark.parametrize("size", KAT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_kat_output(cairo, fmt, size):
    w, h = size
    rng = np.random.default_rng(2000 * fmt + w)
    for pitch in _pitches(fmt, w):
        y, u, v = _wild_planes(rng, w, h)
        y[0, 0], y[-1, -1], u[0, 0], v[0, 0], u[-1, -1], v[-1, -1] = -32768, 32767, 32767, -32768, -1, 256
        _check_output(cairo, y, u, v, fmt, w, h, pitch, f"{cap.FMT_NAMES[fmt]} {w}x{h} pitch {pitch}")


@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_kat_output_every_value_at_every_position(cairo, fmt):
    """Rows 0 and 1 walk all 256 sample values through the even and the odd
    luma columns and through U and V, that is through every byte of a YUY2 /
    UYVY dword and both half-words of a P010 dword, each between neighbours
    that differ; rows 2 and 3 hold values outside 8 bits."""
    w, h = 1024, 4
    rng = np.random.default_rng(3000 + fmt)
    y, u, v = _wild_planes(rng, w, h)
    x = np.arange(w)
    y[0] = 16 + (x // 2 + 5 * (x & 1)) % 256
    y[1] = 16 + (255 - x // 2 + 9 * (x & 1)) % 256
    cx = np.arange(w // 2)
    u[0], v[0] = (cx + 3) % 256, (200 - cx) % 256
    for pitch in _pitches(fmt, w):
        frame = _check_output(cairo, y, u, v, fmt, w, h, pitch, f"{cap.FMT_NAMES[fmt]} pitch {pitch}")
        p = cap.layout(fmt, w, h, pitch)[2]
        rows = [0, 1] + ([h] if fmt == cap.P010 else [])  # (P010: the first UV row as well)
        picked = np.concatenate([frame[r * p:r * p + 2 * w] for r in rows])
        assert cap.covers_all_positions(picked, fmt, w, len(rows))


# ---------------------------------------------------------------------------
# KAT under a colour description
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("desc", DESCS, ids=("limited-bt709", "limited-bt601"))
@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_kat_color(cairo, fmt, desc):
    """Both kernels under a description: the NV12 kernel's answer for the
    folded frame, and the unfold of the NV12 kernel's answer."""
    w, h = 70, 34
    rng = np.random.default_rng(4000 + 10 * fmt + desc[1])
    for pitch in _pitches(fmt, w):
        tag = f"{cap.FMT_NAMES[fmt]} {desc} pitch {pitch}"
        _check_input(cairo, _random_frame(rng, fmt, w, h, pitch), fmt, w, h, pitch, tag + " in", desc)
        _check_output(cairo, *_wild_planes(rng, w, h), fmt, w, h, pitch, tag + " out", desc)


# ---------------------------------------------------------------------------
# Encoder
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("q", [1, 16, 31])
@pytest.mark.parametrize("size", [(64, 48), (70, 34)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_encoder_parity(orc, cairo, size, q):
    """Anchored on the oracle: NV12 from the oracle's input planes (8-bit
    clean, tests/test_pixfmt.py::test_gpu_inputs_fit_8_bits), unfolded to each
    layout, gives the oracle's block tables, coefficients and ring slots."""
    w, h = size
    ctx = cairo.Context(w, h, RING, stages=8)
    try:
        for kind in ("band4", "noise"):
            recs = px._oracle_run(orc, kind, w, h, RING, q, ref.ENC_FRAMES)
            for fmt in cap.CAP_FMTS:
                ctx.reset()
                for t, rec in enumerate(recs):
                    frame = cap.unfold(ref.planes_to_frame(*rec["src"], ref.NV12, w, h), fmt, w, h)
                    out = ctx.encode_frame(frame, t, t > 0, q, fmt=fmt)
                    px._check_frame(ctx, out, rec, t, RING, f"{kind} {w}x{h} q={q} {cap.FMT_NAMES[fmt]} frame {t}")
    finally:
        ctx.close()


def _outputs(out):
    return dict(table=out.table.copy(), coef=(out.coef_y.copy(), out.coef_u.copy(), out.coef_v.copy()))


def _same(got, want, tag):
    px._table_equal(got["table"], want["table"], f"{tag}: block table")
    for a, b, n in zip(got["coef"], want["coef"], "YUV"):
        np.testing.assert_array_equal(a, b, err_msg=f"{tag}: coef {n}")


@pytest.fixture(scope="module")
def wild(cairo):
    """Per layout, 4 random 70x34 frames (4:2:2 rows that differ, full 16-bit
    words), their folds, and what the NV12 run of the folds gives (computed
    once)."""
    w, h = 70, 34
    out = {}
    ctx = cairo.Context(w, h, RING, stages=8)
    try:
        for fmt in cap.CAP_FMTS:
            rng = np.random.default_rng(5000 + fmt)
            frames = [_random_frame(rng, fmt, w, h, 0) for _ in range(4)]
            folds = [cap.fold(f, fmt, w, h) for f in frames]
            ctx.reset()
            want = [_outputs(ctx.encode_frame(f, t, t > 0, Q, fmt=ref.NV12)) for t, f in enumerate(folds)]
            out[fmt] = (frames, folds, want)
    finally:
        ctx.close()
    return out


def _repitch(frame, fmt, w, h, pitch, fill=0xFF):
    """The tight frame with row pitch `pitch`."""
    out = np.full(cap.layout(fmt, w, h, pitch)[0], fill, np.uint8)
    out[cap.image_mask(fmt, w, h, pitch)] = frame
    return out


@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_encoder_equals_nv12_of_fold(cairo, wild, fmt):
    """Tight host frames, pitched host frames, and device frames read in place
    at an odd base (P010: base + 2) with a wider pitch."""
    w, h = 70, 34
    frames, _, want = wild[fmt]
    pitch = cap.pitched(fmt, w)
    off = 2 if fmt == cap.P010 else 1
    ctx = cairo.Context(w, h, RING, stages=8)
    held = []
    try:
        for t, f in enumerate(frames):
            _same(_outputs(ctx.encode_frame(f, t, t > 0, Q, fmt=fmt)), want[t], f"tight host frame {t}")
        ctx.reset()
        for t, f in enumerate(frames):
            got = ctx.encode_frame(_repitch(f, fmt, w, h, pitch), t, t > 0, Q, fmt=fmt, pitch=pitch)
            _same(_outputs(got), want[t], f"pitched host frame {t}")
        ctx.reset()
        for t, f in enumerate(frames):
            pf = _repitch(f, fmt, w, h, pitch)
            buf = px._DeviceBuffer(pf.size + off)
            held.append(buf)
            ptr = buf.upload(pf, offset=off)
            assert ptr % 4 == off
            got = ctx.encode_frame(ptr, t, t > 0, Q, on_device=True, fmt=fmt, pitch=pitch)
            _same(_outputs(got), want[t], f"device frame {t} at base + {off}")
    finally:
        ctx.close()
        for b in held:
            b.free()


def test_mixed_launch_of_all_formats(orc, cairo, wild):
    """One launch of 7 frames, one per format, host and device alternating:
    the same tables and coefficients as the launch in which the three new
    layouts are replaced by the NV12 of their folds."""
    w, h = 70, 34
    recs = px._oracle_run(orc, "band4", w, h, RING, Q, 4)
    old = [(fmt, px._frame_of(recs[t], fmt, w, h)) for t, fmt in enumerate(px.FMTS)]
    old[0] = (old[0][0], old[0][1].reshape(h, w, 3))
    new = [(fmt, wild[fmt][0][k]) for k, fmt in enumerate(cap.CAP_FMTS)]
    folded = [(ref.NV12, wild[fmt][1][k]) for k, fmt in enumerate(cap.CAP_FMTS)]

    def launch(items):
        ctx = cairo.Context(w, h, RING, stages=16)
        ctx.set_batch(len(items))
        devs, tks = [], []
        try:
            for t, (fmt, frame) in enumerate(items):
                if t % 2:
                    devs.append(px._DeviceBuffer(frame.nbytes))
                    tks.append(ctx.submit(devs[-1].upload(frame.reshape(-1)), t, t > 0, Q, on_device=True, fmt=fmt))
                else:
                    tks.append(ctx.submit(frame, t, t > 0, Q, fmt=fmt))
            out = []
            for tk in tks:
                out.append(_outputs(ctx.wait(tk)))
                ctx.release(tk)
            return out
        finally:
            ctx.close()
            for d in devs:
                d.free()

    got, want = launch(old + new), launch(old + folded)
    for t in range(7):
        _same(got[t], want[t], f"mixed launch frame {t}")
    for t in range(4):  # and the first four are the oracle's
        px._table_equal(got[t]["table"], recs[t]["table"], f"mixed launch frame {t} against the oracle")


def _varied(nv12, fmt, w, h, rng):
    """The unfold of an NV12 frame, made to differ from a plain unfold where
    the fold must work: the second 4:2:2 chroma row of each pair moves by one,
    the low byte of every P010 word is random."""
    f = cap.unfold(nv12, fmt, w, h)
    vw = cap.views(f, fmt, w, h)
    if fmt == cap.P010:
        for plane in vw:
            plane[..., 0] = rng.integers(0, 256, plane.shape[:-1])
    else:
        for plane in vw[1:]:
            odd = plane[1::2]
            odd[...] = np.where(odd < 255, odd + 1, odd - 1)
    return f


@pytest.mark.parametrize("fmt", cap.CAP_FMTS, ids=_id)
def test_stream_equals_nv12_run(orc, cairo, fmt):
    kind, w, h, n = ref.STREAM_CASE
    rng = np.random.default_rng(6000 + fmt)
    frames = [_varied(ref.planes_to_frame(*ref.oracle_input_planes(orc, ref.make_frame(kind, w, h, t)), ref.NV12, w, h),
                      fmt, w, h, rng) for t in range(n)]
    folds = [cap.fold(f, fmt, w, h) for f in frames]
    assert all((f != cap.unfold(g, fmt, w, h)).any() for f, g in zip(frames, folds)), "the fold has nothing to do"

    def pipeline(items, f):
        ctx = cairo.Context(w, h, RING, stages=16)
        ctx.set_batch(3)
        st = cairo.Stream(ctx, threads=2)
        try:
            tks = [st.submit(x, t, t > 0, Q, fmt=f) for t, x in enumerate(items)]
            return [st.collect(tk) for tk in tks]
        finally:
            st.close()
            ctx.close()

    want = pipeline(folds, cairo.FMT_NV12)
    assert pipeline(frames, fmt) == want, f"Stream.submit(fmt={cap.FMT_NAMES[fmt]}) payloads differ from the NV12 run"
    assert all(nb > 0 for _, nb in want)


# ---------------------------------------------------------------------------
# Decoder
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", (("band4", 16), ("noise", 31)), ids=lambda c: f"{c[0]}-q{c[1]}")
@pytest.mark.parametrize("size", ref.DEC_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_decoder_formats(cairo, size, case):
    """cairo_ctx_decode_frame_fmt (through Decoder) and fetch_recon in each
    layout, tight and pitched: the unfold of their NV12 output, the padding
    untouched; once under an output colour description."""
    (w, h), (kind, q) = size, case
    assert case in ref.DEC_CASES
    enc = cairo.Encoder(ring=RING)
    enc.set_quality(q)
    bs = cairo.BitStream(w * h * 64 + 65536)
    streams = []
    for t in range(ref.DEC_FRAMES):
        bs.empty()
        enc.encode(ref.make_frame(kind, w, h, t), bs)
        streams.append((bs.data(), bs.bits()))
    enc.close()
    layouts = [(None, ref.NV12, 0)] + [(None, fmt, p) for fmt in cap.CAP_FMTS for p in _pitches(fmt, w)]
    layouts += [((LIMITED, BT709), ref.NV12, 0), ((LIMITED, BT709), cap.P010, 0), ((LIMITED, BT709), cap.YUY2, 2 * w + 3)]
    shown = {}
    for desc, fmt, pitch in layouts:
        dec = cairo.Decoder()
        dec.set_output_format(fmt, pitch)
        if desc:
            dec.set_output_color(*desc)
        for t, (data, nbits) in enumerate(streams):
            bs.empty()
            bs.write(data, nbits)
            buf = np.full(cairo.frame_layout(fmt, w, h, pitch)[0], 0xA5, np.uint8)
            out = dec.decode(bs, w, h, out=buf)
            assert out.ndim == 1 and bs.bits() == 0
            if fmt == ref.NV12:
                shown[desc, t] = buf
                continue
            want = cap.unfold(shown[desc, t], fmt, w, h, pitch, fill=0xA5)
            np.testing.assert_array_equal(buf, want, err_msg=f"decode {kind} {w}x{h} q={q} {cap.FMT_NAMES[fmt]} "
                                                             f"pitch {pitch} {desc} frame {t} (image and padding)")
        dec.close()
    assert (shown[None, 0] != shown[(LIMITED, BT709), 0]).any()

    ctx = cairo.Context(w, h, RING, stages=8)
    try:
        ctx.set_metrics(sse=False, ssim=False, keep_recon=True)
        tks = [ctx.submit(ref.make_frame(kind, w, h, t), t, t > 0, q) for t in range(2)]
        for tk in tks:
            ctx.wait(tk)
        for desc in (None, (LIMITED, BT601)):
            if desc:
                ctx.set_output_color(*desc)
            nv12 = ctx.fetch_recon(tks[-1], cairo.FMT_NV12)
            for fmt in cap.CAP_FMTS:
                for pitch in _pitches(fmt, w):
                    got = ctx.fetch_recon(tks[-1], fmt, pitch, out=np.full(cap.layout(fmt, w, h, pitch)[0], 0xA5, np.uint8))
                    np.testing.assert_array_equal(got, cap.unfold(nv12, fmt, w, h, pitch, fill=0xA5),
                                                  err_msg=f"fetch_recon {cap.FMT_NAMES[fmt]} pitch {pitch} {desc}")
        for tk in tks:
            ctx.release(tk)
    finally:
        ctx.close()


def test_dropin_round_trip(orc, cairo):
    """Encoder.set_input_format(FMT_UYVY) gives the NV12 encoder's stream for
    the folded frames; Decoder.set_output_format(FMT_P010) the unfold of the
    NV12 decoder's frames."""
    w, h, n = 64, 48, 3
    rng = np.random.default_rng(77)
    frames = [_varied(ref.planes_to_frame(*ref.oracle_input_planes(orc, ref.make_frame("band4", w, h, t)), ref.NV12, w, h),
                      cap.UYVY, w, h, rng) for t in range(n)]
    folds = [cap.fold(f, cap.UYVY, w, h) for f in frames]
    assert all((f != cap.unfold(g, cap.UYVY, w, h)).any() for f, g in zip(frames, folds)), "the fold has nothing to do"

    def encode(items, fmt):
        enc = cairo.Encoder(ring=RING)
        enc.set_quality(Q)
        enc.set_input_format(fmt)
        bs = cairo.BitStream(w * h * 64 + 65536)
        out = []
        for t, f in enumerate(items):
            bs.empty()
            enc.encode(f, bs, w, h)
            data = bytearray(bs.data())
            if t == 0:
                data[7] = 0  # the header's unwritten pad byte
            out.append((bytes(data), bs.bits()))
        enc.close()
        return out

    streams = encode(frames, cairo.FMT_UYVY)
    assert streams == encode(folds, cairo.FMT_NV12), "the UYVY encoder's stream differs from the NV12 encoder's"

    def decode(fmt):
        dec = cairo.Decoder()
        dec.set_output_format(fmt)
        bs = cairo.BitStream(w * h * 64 + 65536)
        out = []
        for data, nbits in streams:
            bs.empty()
            bs.write(data, nbits)
            out.append(dec.decode(bs, w, h).copy())
        dec.close()
        return out

    for t, (a, b) in enumerate(zip(decode(cairo.FMT_P010), decode(cairo.FMT_NV12))):
        np.testing.assert_array_equal(a, cap.unfold(b, cap.P010, w, h), err_msg=f"decoded P010 frame {t}")
        y16, uv16 = cairo.split_frame(a, cairo.FMT_P010, w, h)
        assert not (y16 & 0xFF).any() and not (uv16 & 0xFF).any()


# ---------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------

def test_refusals_take_no_ticket(cairo, wild):
    w, h = 70, 34
    ctx = cairo.Context(w, h, RING, stages=8)
    frames, _, want = wild[cap.P010]
    nb = cap.layout(cap.P010, w, h)[0]
    dev = px._DeviceBuffer(nb + 4)
    big = px._DeviceBuffer(cap.layout(cap.P010, 2 * w, 2 * h)[0])

    def refused(*a, **kw):
        with pytest.raises(cairo.CairoError) as ei:
            ctx.submit(*a, **kw)
        assert ei.value.status == cairo.EVX_ERROR_INVALID_ARGS

    try:
        ptr = dev.upload(frames[0], offset=1)
        refused(ptr, 0, False, Q, on_device=True, fmt=cap.P010)                     # an odd address
        refused(dev.ptr, 0, False, Q, on_device=True, fmt=cap.P010, pitch=2 * w + 1)  # an odd pitch
        refused(dev.ptr + 6, 0, False, Q, on_device=True, fmt=cap.P010)             # 2 bytes past the allocation's end
        refused(dev.ptr, 0, False, Q, on_device=True, fmt=cap.P010, pitch=1 << 24)  # 1.7 GB by the layout
        refused(dev.ptr, 0, False, Q, on_device=True, fmt=cap.YUY2, pitch=1 << 24)
        for fmt in cap.CAP_FMTS:                                                     # no scaled submit
            refused(big.ptr, 0, False, Q, on_device=True, fmt=fmt, src_size=(2 * w, 2 * h))
            refused(big.ptr, 0, False, Q, on_device=True, fmt=fmt, src_size=(w, h))
        for f in (4, 5, 6, 7, 11):
            refused(dev.ptr, 0, False, Q, on_device=True, fmt=f)
        for t, f in enumerate(frames[:2]):  # the next submit takes the ticket the refused ones would have taken
            tk = ctx.submit(dev.upload(f, offset=2), t, t > 0, Q, on_device=True, fmt=cap.P010)
            assert tk == t
            _same(_outputs(ctx.wait(tk)), want[t], f"after the refusals, frame {t}")
            ctx.release(tk)
    finally:
        ctx.close()
        dev.free()
        big.free()
