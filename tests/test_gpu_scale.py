"""The scaled submit on the GPU (scale.hip, cairo_ctx_submit_scaled).

KAT: k_scale_batch on its own (cairo_kat_scale) against the numpy restatement
of the rule (tests/scale_ref.py), byte for byte.  Then the defining property:
a scaled submit produces exactly the bits of submitting the scaled frame --
against the oracle for RGB, against a tight submit on a second context for the
YUV formats, mixed launches, reused staging slots, two renditions of one
resident source, the frame pipeline, and the refusals.
"""
import ctypes

import numpy as np
import pytest

from tests import pixfmt_ref as pf
from tests import scale_ref as ref

pytestmark = pytest.mark.gpu

FMTS = (ref.RGB24, ref.BGR24, ref.I420, ref.NV12)
_id = lambda f: pf.FMT_NAMES[f]  # noqa: E731
RING = 4


class _DeviceBuffer:
    """Device memory from the HIP runtime the library itself uses (by soname:
    the copy already loaded into this process)."""

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
        a = np.ascontiguousarray(a).reshape(-1)
        assert a.dtype == np.uint8 and offset + a.nbytes <= self.nbytes
        assert self.hip.hipMemcpy(self.ptr + offset, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return self.ptr + offset

    def free(self) -> None:
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = None


class _Resident:
    """Frames uploaded once, each into its own allocation; freed together."""

    def __init__(self):
        self.bufs = []

    def put(self, frame: np.ndarray, offset: int = 0) -> int:
        b = _DeviceBuffer(frame.size + offset)
        self.bufs.append(b)
        return b.upload(frame, offset)

    def free(self):
        for b in self.bufs:
            b.free()


# ---------------------------------------------------------------------------
# KAT
# ---------------------------------------------------------------------------

def _misaligned(frame: np.ndarray, offset: int) -> np.ndarray:
    """A copy of frame whose address is `offset` modulo 4 (cairo_kat_scale's
    device copy keeps that)."""
    hold = np.empty(frame.size + 8, np.uint8)
    start = (offset - hold.ctypes.data) % 4
    view = hold[start:start + frame.size]
    view[...] = frame
    assert view.ctypes.data % 4 == offset and view.flags["C_CONTIGUOUS"]
    return view


def _kat(cairo, frame, fmt, pitch, size, crop, dw, dh, tag):
    want = ref.scaled_frame(frame, fmt, pitch, (size, crop), dw, dh)
    before = frame.copy()
    out = cairo.kat_scale(frame, fmt, size, dw, dh, crop=crop, pitch=pitch)
    assert out.size == want.size + cairo.KAT_SCALE_GUARD
    np.testing.assert_array_equal(out[:want.size], want, err_msg=f"{tag}: scaled frame")
    assert (out[want.size:] == 0xA5).all(), f"{tag}: bytes beyond the tight frame written"
    np.testing.assert_array_equal(frame, before, err_msg=f"{tag}: the source frame")


@pytest.mark.parametrize("sizes", ref.KAT_SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}-{s[1][0]}x{s[1][1]}")
@pytest.mark.parametrize("fmt", FMTS, ids=_id)
def test_kat(cairo, fmt, sizes):
    (sw, sh), (dw, dh) = sizes
    rng = np.random.default_rng(100 * fmt + sw)
    nb = pf.layout(fmt, sw, sh)[0]
    tag = f"{pf.FMT_NAMES[fmt]} {sw}x{sh} -> {dw}x{dh}"
    _kat(cairo, rng.integers(0, 256, nb, dtype=np.uint8), fmt, 0, (sw, sh), None, dw, dh, f"{tag} noise")
    # the accumulator and the reciprocal at their maximum
    _kat(cairo, np.full(nb, 255, np.uint8), fmt, 0, (sw, sh), None, dw, dh, f"{tag} all 255")


def _pitch(fmt, w):
    """A pitch 2 (I420, which needs an even one) or 3 bytes wider than tight:
    rows change their alignment, so dword and byte accesses alternate."""
    return pf.layout(fmt, w, 2)[1] + (2 if fmt == ref.I420 else 3)


@pytest.mark.parametrize("fmt", FMTS, ids=_id)
def test_kat_pitched_misaligned_cropped(cairo, fmt):
    rng = np.random.default_rng(200 + fmt)
    for (sw, sh), (dw, dh) in (((140, 68), (70, 34)), ((96, 72), (64, 48))):
        pitch = _pitch(fmt, sw)
        frame = rng.integers(0, 256, pf.layout(fmt, sw, sh, pitch)[0], dtype=np.uint8)
        _kat(cairo, frame, fmt, pitch, (sw, sh), None, dw, dh, f"{pf.FMT_NAMES[fmt]} {sw}x{sh} pitch {pitch}")
    # a source at an odd byte offset inside its allocation, tight and pitched
    for pitch in (0, _pitch(fmt, 140)):
        frame = _misaligned(rng.integers(0, 256, pf.layout(fmt, 140, 68, pitch)[0], dtype=np.uint8), 1)
        _kat(cairo, frame, fmt, pitch, (140, 68), None, 70, 34, f"{pf.FMT_NAMES[fmt]} odd base, pitch {pitch}")
    # a crop of a larger frame
    for pitch, off in ((0, 0), (_pitch(fmt, 160), 3)):
        frame = _misaligned(rng.integers(0, 256, pf.layout(fmt, 160, 80, pitch)[0], dtype=np.uint8), off)
        _kat(cairo, frame, fmt, pitch, (160, 80), (6, 4, 140, 68), 70, 34, f"{pf.FMT_NAMES[fmt]} crop, pitch {pitch}")


# ---------------------------------------------------------------------------
# Encoder: a scaled submit gives the bits of submitting the scaled frame
# ---------------------------------------------------------------------------

def _table_equal(a, b, what):
    for f in a.dtype.names:
        if f == "pad":
            continue
        bad = np.nonzero(a[f] != b[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at MBs {bad[:10]} gpu={a[f][bad[:5]]} ref={b[f][bad[:5]]}"


def _oracle_run(orc, rgbs, ring, q):
    """The oracle's intermediates of I + P... over the RGB frames: per frame
    planes(0), the block table, planes(1), the deblocked slot and the payload."""
    e = orc.OracleEncoder(ring)
    e.set_quality(q)
    out = []
    for t, rgb in enumerate(rgbs):
        e.encode(np.ascontiguousarray(rgb))
        cp = lambda p: tuple(a.copy() for a in p)  # noqa: E731
        out.append(dict(rgb=rgb, src=cp(e.planes(0)), table=e.block_table().copy(), coef=cp(e.planes(1)),
                        recon=cp(e.planes(2 + t % ring))))
    return out


def _check_frame(ctx, out, rec, t, ring, tag, planes=True):
    _table_equal(out.table, rec["table"], f"{tag}: block table")
    for got, want, n in zip((out.coef_y, out.coef_u, out.coef_v), rec["coef"], "YUV"):
        np.testing.assert_array_equal(got, want, err_msg=f"{tag}: coef {n}")
    if planes:
        for got, want, n in zip(ctx.read_planes(0), rec["src"], "YUV"):  # wa x ha: the padding stays zero
            np.testing.assert_array_equal(got, want, err_msg=f"{tag}: input {n}")
        for got, want, n in zip(ctx.read_planes(2 + t % ring), rec["recon"], "YUV"):
            np.testing.assert_array_equal(got, want, err_msg=f"{tag}: recon {n} (deblocked)")


def _payload(cairo, ctx, out):
    return cairo.serialize_slice(out.table, ctx.wmb, ctx.hmb, ctx.ring, out.coef_y, out.coef_u, out.coef_v)


def _run(cairo, w, h, q, submits, batch=None, stages=16):
    """All frames submitted to a fresh w x h context, then waited in order:
    submits is a list of (frame, kwargs of Context.submit).  -> per frame
    (FrameOutputs, payload)."""
    ctx = cairo.Context(w, h, RING, stages=stages)
    try:
        if batch:
            ctx.set_batch(batch)
        tks = [ctx.submit(f, t, t > 0, q, **kw) for t, (f, kw) in enumerate(submits)]
        res = []
        for tk in tks:
            out = ctx.wait(tk)
            res.append((out, _payload(cairo, ctx, out)))
            ctx.release(tk)
        return res
    finally:
        ctx.close()


def _same(got, want, tag):
    assert len(got) == len(want)
    for t, ((a, pa), (b, pb)) in enumerate(zip(got, want)):
        _table_equal(a.table, b.table, f"{tag} frame {t}: block table")
        for x, y, n in zip((a.coef_y, a.coef_u, a.coef_v), (b.coef_y, b.coef_u, b.coef_v), "YUV"):
            np.testing.assert_array_equal(x, y, err_msg=f"{tag} frame {t}: coef {n}")
        assert pa == pb, f"{tag} frame {t}: payload bits"
        assert pa[1] > 0


def _rgb_scaled(rgb, dw, dh, crop=None):
    """scale_ref's frame of an (h, w, 3) RGB image, as (dh, dw, 3)."""
    h, w = rgb.shape[:2]
    return ref.scaled_frame(np.ascontiguousarray(rgb).reshape(-1), ref.RGB24, 0, ((w, h), crop), dw, dh).reshape(dh, dw, 3)


@pytest.fixture(scope="module")
def cif(orc):
    """band4 at 352x288, 6 frames, and scale_ref's 176x144 frames of them
    (computed once, never modified)."""
    rgbs = [orc.make_frame(352, 288, t) for t in range(6)]
    return dict(rgbs=rgbs, small=[_rgb_scaled(f, 176, 144) for f in rgbs])


@pytest.mark.parametrize("q", [1, 16])
def test_encoder_parity_with_the_oracle(orc, cairo, cif, q):
    """The oracle encodes scale_ref's 176x144 frames; the scaled submit of the
    352x288 device frames gives its input planes, block table, coefficients,
    reconstruction and payload bits, frame by frame (I + 4 P)."""
    recs = _oracle_run(orc, cif["small"][:5], RING, q)
    ctx = cairo.Context(176, 144, RING, stages=8)
    dev = _Resident()
    try:
        for t, rec in enumerate(recs):
            ptr = dev.put(cif["rgbs"][t].reshape(-1))
            out = ctx.encode_frame(ptr, t, t > 0, q, on_device=True, src_size=(352, 288))
            _check_frame(ctx, out, rec, t, RING, f"q={q} frame {t}")
            want = cairo.serialize_slice(rec["table"], ctx.wmb, ctx.hmb, RING, *rec["coef"])
            assert _payload(cairo, ctx, out) == want, f"q={q} frame {t}: payload bits"
    finally:
        ctx.close()
        dev.free()


@pytest.mark.parametrize("fmt", (ref.I420, ref.NV12), ids=_id)
def test_yuv_scale_then_submit(orc, cairo, fmt):
    """I420 / NV12 sources built from the oracle's input planes: the scaled
    submit equals a tight submit of scale_ref's frame on a second context.
    352x288 -> 176x144 (2:1) and, from a 356x288 source, the crop
    (0, 0, 354, 288) -> 118x96 (3:1)."""
    q, n = 16, 3
    for (sw, sh), crop, (dw, dh) in (((352, 288), None, (176, 144)), ((356, 288), (0, 0, 354, 288), (118, 96))):
        srcs = [pf.planes_to_frame(*pf.oracle_input_planes(orc, orc.make_frame(sw, sh, t)), fmt, sw, sh) for t in range(n)]
        dev = _Resident()
        try:
            got = _run(cairo, dw, dh, q, [(dev.put(f), dict(on_device=True, fmt=fmt, src_size=(sw, sh), crop=crop))
                                         for f in srcs])
            want = _run(cairo, dw, dh, q, [(ref.scaled_frame(f, fmt, 0, ((sw, sh), crop), dw, dh), dict(fmt=fmt))
                                          for f in srcs])
            _same(got, want, f"{pf.FMT_NAMES[fmt]} {sw}x{sh} {crop} -> {dw}x{dh}")
        finally:
            dev.free()


def test_mixed_launch(orc, cairo, cif):
    """One launch of four frames: an unscaled RGB24 frame, a scaled RGB24
    frame, a scaled NV12 frame with a crop and a pitch, and a scaled BGR24
    frame from another source size (3:1).  Twice over, so that the second
    launch follows the first on the other stream."""
    w, h, q = 176, 144, 16
    dev = _Resident()
    try:
        mixed, plain = [], []
        for t in range(8):
            k = t % 4
            if k == 0:
                mixed.append((cif["small"][t % 6], {}))
                plain.append((cif["small"][t % 6], {}))
            elif k == 1:
                mixed.append((dev.put(cif["rgbs"][t % 6].reshape(-1)), dict(on_device=True, src_size=(352, 288))))
                plain.append((cif["small"][t % 6], {}))
            elif k == 2:
                sw, sh, crop, pitch = 356, 292, (2, 4, 352, 288), 356 + 3
                f = pf.planes_to_frame(*pf.oracle_input_planes(orc, orc.make_frame(sw, sh, t)), ref.NV12, sw, sh, pitch, 0xFF)
                mixed.append((dev.put(f, offset=1), dict(on_device=True, fmt=ref.NV12, pitch=pitch, src_size=(sw, sh),
                                                         crop=crop)))
                plain.append((ref.scaled_frame(f, ref.NV12, pitch, ((sw, sh), crop), w, h), dict(fmt=ref.NV12)))
            else:
                sw, sh = 528, 432
                f = pf.rgb_to_frame(orc.make_frame(sw, sh, t), ref.BGR24)
                mixed.append((dev.put(f), dict(on_device=True, fmt=ref.BGR24, src_size=(sw, sh))))
                plain.append((ref.scaled_frame(f, ref.BGR24, 0, ((sw, sh), None), w, h), dict(fmt=ref.BGR24)))
        got = _run(cairo, w, h, q, mixed, batch=4)
        want = _run(cairo, w, h, q, plain, batch=4)
        _same(got, want, "mixed launch")
    finally:
        dev.free()


def test_slot_reuse_release_without_wait(cairo, cif):
    """4 staging slots, 2 frames per launch, 12 scaled frames, every ticket but
    the last released unwaited: a slot's next frame is scaled into it only
    after the launch that converts its previous frame (rgb_read), or the earlier
    frame is encoded from the later image.  Every frame is a P frame of the one
    before, so the last frame's outputs and payload and the final ring slots
    equal the pre-scaled run's only if every frame did."""
    w, h, q, n = 176, 144, 16, 12

    def run(scaled):
        ctx = cairo.Context(w, h, RING, stages=4)
        ctx.set_batch(2)
        dev = _Resident()
        try:
            tk = None
            for t in range(n):
                if scaled:
                    tk = ctx.submit(dev.put(cif["rgbs"][t % 6].reshape(-1)), t, t > 0, q, on_device=True,
                                    src_size=(352, 288))
                else:
                    tk = ctx.submit(cif["small"][t % 6], t, t > 0, q)
                if t < n - 1:
                    ctx.release(tk)
            out = ctx.wait(tk)
            res = (out, _payload(cairo, ctx, out))
            ctx.release(tk)
            ctx.sync()
            return res, [ctx.read_planes(2 + k) for k in range(RING)]
        finally:
            ctx.close()
            dev.free()

    (got, slots), (want, wslots) = run(True), run(False)
    _same([got], [want], "slot reuse, last")
    for k in range(RING):
        for a, b, name in zip(slots[k], wslots[k], "YUV"):
            np.testing.assert_array_equal(a, b, err_msg=f"ring slot {k} {name}")


def test_ladder(orc, cairo):
    """One resident 528x288 source sequence feeds a 264x144 (2:1) and a 176x96
    (3:1) context in the same process, frame by frame; each stream equals its
    own pre-scaled run."""
    sw, sh, q, n = 528, 288, 16, 4
    rgbs = [orc.make_frame(sw, sh, t) for t in range(n)]
    rungs = ((264, 144), (176, 96))
    dev = _Resident()
    ctxs = [cairo.Context(w, h, RING, stages=8) for w, h in rungs]
    try:
        ptrs = [dev.put(f.reshape(-1)) for f in rgbs]
        tks = [[c.submit(p, t, t > 0, q, on_device=True, src_size=(sw, sh)) for c in ctxs] for t, p in enumerate(ptrs)]
        got = [[], []]
        for t in range(n):
            for k, c in enumerate(ctxs):
                out = c.wait(tks[t][k])
                got[k].append((out, _payload(cairo, c, out)))
                c.release(tks[t][k])
    finally:
        for c in ctxs:
            c.close()
        dev.free()
    for k, (w, h) in enumerate(rungs):
        want = _run(cairo, w, h, q, [(_rgb_scaled(f, w, h), {}) for f in rgbs])
        _same(got[k], want, f"ladder {w}x{h}")


def test_pipeline(cairo, cif):
    """Stream.submit(..., src_size=...) payload bits equal those of the
    pre-scaled Stream run over 6 frames."""
    w, h, q = 176, 144, 16

    def pipeline(frames, **kw):
        ctx = cairo.Context(w, h, RING, stages=16)
        ctx.set_batch(3)
        st = cairo.Stream(ctx, threads=2)
        try:
            tks = [st.submit(f, t, t > 0, q, **kw) for t, f in enumerate(frames)]
            return [st.collect(tk) for tk in tks]
        finally:
            st.close()
            ctx.close()

    dev = _Resident()
    try:
        got = pipeline([dev.put(f.reshape(-1)) for f in cif["rgbs"]], on_device=True, src_size=(352, 288))
    finally:
        dev.free()
    want = pipeline(cif["small"])
    assert got == want, "Stream.submit(src_size=...) payloads differ from the pre-scaled run"
    assert all(nb > 0 for _, nb in want)


def test_refusals(orc, cairo, cif):
    """A host pointer, a source that does not fit its allocation, a ratio above
    8 and upscaling are refused with EVX_ERROR_INVALID_ARGS; no ticket is
    taken, and the next valid submit is frame 0 of a correct stream."""
    w, h, q = 176, 144, 16
    ctx = cairo.Context(w, h, RING, stages=8)
    dev = _Resident()
    try:
        ptr = dev.put(cif["rgbs"][0].reshape(-1))

        def refused(frame, **kw):
            with pytest.raises(cairo.CairoError) as ei:
                ctx.submit(frame, 0, False, q, **kw)
            assert ei.value.status == cairo.EVX_ERROR_INVALID_ARGS

        refused(np.ascontiguousarray(cif["rgbs"][0]).reshape(-1), src_size=(352, 288))  # a host source
        refused(ptr, on_device=True, src_size=(352, 290))  # two rows more than the allocation holds
        big = _DeviceBuffer(1410 * 1154 * 3)
        dev.bufs.append(big)
        refused(big.ptr, on_device=True, src_size=(1410, 1152))  # 1410 > 8 * 176
        refused(big.ptr, on_device=True, src_size=(1408, 1154))  # 1154 > 8 * 144
        refused(ptr, on_device=True, src_size=(352, 288), crop=(0, 0, 174, 144))  # upscaling 174 -> 176
        refused(ptr, on_device=True, src_size=(352, 288), crop=(0, 0, 176, 142))  # upscaling 142 -> 144
        recs = _oracle_run(orc, cif["small"][:2], RING, q)
        for t in range(2):
            p = dev.put(cif["rgbs"][t].reshape(-1))
            tk = ctx.submit(p, t, t > 0, q, on_device=True, src_size=(352, 288))
            assert tk == t, "a refused submit took a ticket"
            out = ctx.wait(tk)
            _check_frame(ctx, out, recs[t], t, RING, f"after the refusals, frame {t}")
            ctx.release(tk)
    finally:
        ctx.close()
        dev.free()
