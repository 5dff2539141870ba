"""Every kind of frame source after every other in the same pending index and
the same staging slot (backend.hip: one record per pending frame, written whole
at submit; flush()'s pre-passes wait for a slot's pending rgb_read).

64x48, 4 staging slots, 2 frames per launch, 15 frames, frame t of kind t % 5:
  0  tight RGB24 host frame              3  scaled submit of a 128x96 device frame
  1  pitched I420 host frame             4  float16 CHW tensor frame
  2  pitched NV12 device frame
5 is coprime to 2 and to 4, so each pending index (t % 2) and each slot (t % 4)
takes each kind after each other kind.  The reference run submits the same
pictures as plain tight host frames."""
import numpy as np
import pytest

from tests import pixfmt_ref as pf
from tests import scale_ref
from tests import tables
from tests import tensor_ref as ref
from tests.test_gpu_tensor import (Q, RING, _DeviceBuffer, _Resident, _expect_unpacked, _out_case, _out_desc, _packed,
                                   _payload, _same, _submit_case, _tensor_of)
from tests.test_tables import SEEDS

pytestmark = pytest.mark.gpu

W, H, N, STAGES = 64, 48, 15, 4
I420_PITCH, NV12_PITCH = W + 8, W + 5
# Released without a wait: their slots' next frames are the scaled frame 8 and
# the tensor frame 9, whose pre-passes then meet an rgb_read nobody waited for.
# Both are P frames' references, so the frames after them vouch for them.
UNWAITED = (4, 5)


def _sources(orc, cairo, dev):
    """Per frame (submit of its kind, submit of the same picture as a plain host frame)."""
    mixed, plain = [], []
    for t in range(N):
        k = t % 5
        rgb = orc.make_frame(W, H, t)
        if k == 0:
            mixed.append(lambda c, t, f=rgb: c.submit(f, t, t > 0, Q))
            plain.append(mixed[-1])
        elif k in (1, 2):
            fmt, pitch = (pf.I420, I420_PITCH) if k == 1 else (pf.NV12, NV12_PITCH)
            planes = pf.oracle_input_planes(orc, rgb)
            pitched = pf.planes_to_frame(*planes, fmt, W, H, pitch, 0xA5)
            if k == 1:
                mixed.append(lambda c, t, f=pitched: c.submit(f, t, t > 0, Q, fmt=pf.I420, pitch=I420_PITCH))
            else:
                mixed.append(lambda c, t, p=dev.put(pitched): c.submit(p, t, t > 0, Q, on_device=True, fmt=pf.NV12,
                                                                       pitch=NV12_PITCH))
            plain.append(lambda c, t, f=pf.planes_to_frame(*planes, fmt, W, H), fmt=fmt: c.submit(f, t, t > 0, Q, fmt=fmt))
        elif k == 3:
            big = np.ascontiguousarray(orc.make_frame(2 * W, 2 * H, t)).reshape(-1)
            small = scale_ref.scaled_frame(big, scale_ref.RGB24, 0, ((2 * W, 2 * H), None), W, H).reshape(H, W, 3)
            mixed.append(lambda c, t, p=dev.put(big): c.submit(p, t, t > 0, Q, on_device=True, src_size=(2 * W, 2 * H)))
            plain.append(lambda c, t, f=small: c.submit(f, t, t > 0, Q))
        else:
            case = _tensor_of(rgb, ref.F16, "chw", (0.0, 1.0))
            mixed.append(lambda c, t, cs=case: _submit_case(cairo, c, dev, cs, t))
            plain.append(lambda c, t, cs=case: c.submit(_packed(cs), t, t > 0, Q))
    return mixed, plain


def _drive(cairo, ctx, submits):
    """At most STAGES tickets in flight; the oldest is waited and released (the
    UNWAITED ones only released) before its slot is taken again.  -> the waited
    frames' (FrameOutputs, payload), in order."""
    tks, res = [], []
    for t in range(N + STAGES):
        old = t - STAGES
        if old >= 0:
            if old not in UNWAITED:
                out = ctx.wait(tks[old])
                res.append((out, _payload(cairo, ctx, out)))
            ctx.release(tks[old])
        if t < N:
            tks.append(submits[t](ctx, t))
    return res


def test_drop_in_format_after_clear(orc, cairo):
    """clear() forgets the frame size: a format and pitch for a smaller coming
    stream are taken as before the first frame (the pitch is checked at the
    next frame), where the same call is refused while the size is known; the
    cleared encoder and decoder then give a fresh one's bits and frame."""
    big, (w, h), pitch = orc.make_frame(352, 288, 0), (W, H), I420_PITCH
    frame = pf.planes_to_frame(*pf.oracle_input_planes(orc, orc.make_frame(w, h, 0)), pf.I420, w, h, pitch, 0xA5)

    def encode(enc):
        bs = cairo.BitStream(352 * 288 * 64)
        enc.encode(frame, bs, w, h)
        return bs

    enc, fresh, dec, fresh_dec = cairo.Encoder(), cairo.Encoder(), cairo.Decoder(), cairo.Decoder()
    try:
        bs = cairo.BitStream(352 * 288 * 64)
        enc.encode(big, bs)
        dec.decode(bs, 352, 288)
        for obj, setter in ((enc, enc.set_input_format), (dec, dec.set_output_format)):
            with pytest.raises(cairo.CairoError):
                setter(cairo.FMT_I420, pitch)  # 72 < 352
            obj.clear()
            setter(cairo.FMT_I420, pitch)
        fresh.set_input_format(cairo.FMT_I420, pitch)
        fresh_dec.set_output_format(cairo.FMT_I420, pitch)
        got, want = encode(enc), encode(fresh)
        assert got.bits() == want.bits() > 0 and bytes(got.data()) == bytes(want.data())
        np.testing.assert_array_equal(dec.decode(got, w, h), fresh_dec.decode(want, w, h))
    finally:
        for x in (enc, fresh, dec, fresh_dec):
            x.close()


def test_every_kind_after_every_other(orc, cairo):
    dev = _Resident()
    got_ctx = cairo.Context(W, H, RING, stages=STAGES)
    ref_ctx = cairo.Context(W, H, RING, stages=STAGES)
    try:
        mixed, plain = _sources(orc, cairo, dev)
        for c in (got_ctx, ref_ctx):
            c.set_batch(2)
        got, want = _drive(cairo, got_ctx, mixed), _drive(cairo, ref_ctx, plain)
        assert len(got) == N - len(UNWAITED)
        _same(got, want, "frame sources")

        # Pending index 0 last held the tensor frame 14: a decode frame written
        # into it must carry nothing of that.  decode_frame_tensor equals
        # decode_frame's RGB888 through the output map.
        table, coef = tables.make_sequence(W, H, RING, 1, SEEDS[0])[0]
        assert cairo.table_check(table, got_ctx.wmb, got_ctx.hmb, RING)
        case = _out_case(ref.F16, W, H)
        buf = _DeviceBuffer(case["buf"].size)
        dev.bufs.append(buf)
        got_ctx.reset()
        got_ctx.decode_frame_tensor(table, coef, 0, _out_desc(cairo, case, buf.ptr))
        got_ctx.reset()
        rgb = got_ctx.decode_frame(table, coef, 0)
        np.testing.assert_array_equal(buf.download(), _expect_unpacked(case, rgb), err_msg="decode_frame_tensor after reset")
    finally:
        got_ctx.close()
        ref_ctx.close()
        dev.free()
