"""The scaled tensor submit on the GPU (tensor.hip k_tensor_scale_batch;
cairo_ctx_submit_tensor_scaled).

KAT: the kernel on its own (cairo_kat_tensor_scale) against the composed
restatement tests/tensor_scale_ref.py, byte for byte, the guard behind the
frame and every byte of the tensor included.  Then the defining property: a
scaled tensor submit produces exactly the bits of submitting the RGB24 frame
scale(pack(tensor)) -- single frames, mixed launches, launches with more such
frames than one argument block holds, a ladder, the frame pipeline, and the
refusals.
"""
import torch  # noqa: F401  (first, as the tools do: the package finds it in sys.modules)

import ctypes

import numpy as np
import pytest

from tests import pixfmt_ref as pf
from tests import scale_ref as sr
from tests import tensor_ref as tr
from tests import tensor_scale_ref as ref

pytestmark = pytest.mark.gpu

RING, Q = 4, 16
DTYPES = (tr.U8, tr.F16, tr.BF16, tr.F32)
LAYOUTS = ("chw", "hwc", "chw_padded", "rgba")
CIF = (352, 288)


class _DeviceBuffer:
    """Device memory from the HIP runtime the library itself uses (by soname:
    the copy already loaded into this process)."""

    def __init__(self, nbytes: int, fill: int = tr.FILL):
        self.hip = ctypes.CDLL("libamdhip64.so.7")
        self.hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        self.hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        self.hip.hipFree.argtypes = [ctypes.c_void_p]
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), nbytes) == 0
        self.ptr, self.nbytes = p.value, nbytes
        self.upload(np.full(nbytes, fill, np.uint8))

    def upload(self, a: np.ndarray, offset: int = 0) -> int:
        a = np.ascontiguousarray(a).reshape(-1)
        assert a.dtype == np.uint8 and offset + a.nbytes <= self.nbytes
        assert self.hip.hipMemcpy(self.ptr + offset, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice
        return self.ptr + offset

    def free(self) -> None:
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = None


class _Resident:
    """Buffers uploaded once, each its own allocation; freed together."""

    def __init__(self):
        self.bufs = []

    def put(self, a: np.ndarray, offset: int = 0) -> int:
        b = _DeviceBuffer(a.size + offset)
        self.bufs.append(b)
        return b.upload(a, offset)

    def free(self):
        for b in self.bufs:
            b.free()


# ---------------------------------------------------------------------------
# KAT
# ---------------------------------------------------------------------------

def _aligned16(buf: np.ndarray) -> np.ndarray:
    """A copy of buf at a 16-byte aligned address: element (0, 0, 0), `lead`
    bytes in, then has the address lead modulo 16, which
    cairo_kat_tensor_scale's device copy keeps."""
    hold = np.empty(buf.size + 16, np.uint8)
    start = -hold.ctypes.data % 16
    view = hold[start:start + buf.size]
    view[...] = buf
    assert view.ctypes.data % 16 == 0
    return view


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: tr.NAMES[d])
def test_kat(cairo, dtype, layout):
    jobs = ref.kat_jobs(dtype, layout)
    assert {j[3] for j in jobs} == set(ref.kat_leads(dtype))
    assert sum(1 for j in jobs if j[1] and j[1][0] % 4) >= 2, "crops whose origin is no multiple of 4 pixels"
    for size, crop, (dw, dh), lead, seed in jobs:
        case = ref.kat_case(dtype, layout, size, lead, seed)
        want = ref.case_expected(case, crop, dw, dh)
        buf = _aligned16(case["buf"])
        rgb = np.full(3 * dw * dh + cairo.KAT_TENSOR_GUARD, tr.FILL, np.uint8)
        d = cairo.tensor_desc((buf.ctypes.data + lead, dtype, case["strides"]), mul=case["mul"], add=case["add"])
        cairo.kat_tensor_scale(d, size, buf.size - lead, dw, dh, rgb, crop=crop)
        tag = f"{case['name']} crop {crop} -> {dw}x{dh} lead {lead}"
        np.testing.assert_array_equal(rgb[:3 * dw * dh].reshape(dh, dw, 3), want, err_msg=f"{tag}: scaled frame")
        assert (rgb[3 * dw * dh:] == tr.FILL).all(), f"{tag}: bytes behind the tight frame written"
        np.testing.assert_array_equal(buf, case["buf"], err_msg=f"{tag}: the tensor's bytes")


# ---------------------------------------------------------------------------
# Encoder: a scaled tensor submit gives the bits of submitting scale(pack(tensor))
# ---------------------------------------------------------------------------

def _table_equal(a, b, what):
    for f in a.dtype.names:
        if f == "pad":
            continue
        bad = np.nonzero(a[f] != b[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at MBs {bad[:10]} gpu={a[f][bad[:5]]} ref={b[f][bad[:5]]}"


def _payload(cairo, ctx, out):
    return cairo.serialize_slice(out.table, ctx.wmb, ctx.hmb, ctx.ring, out.coef_y, out.coef_u, out.coef_v)


def _run(cairo, w, h, submits, batch, stages=16, outputs=0, metrics=False):
    """Frames submitted to a fresh context, then waited in order.  submits:
    callables (ctx, t) -> ticket.  -> per frame (FrameOutputs, payload, metrics)."""
    ctx = cairo.Context(w, h, RING, stages=stages)
    try:
        if outputs:
            ctx.set_outputs(outputs)
        if metrics:
            ctx.set_metrics()
        ctx.set_batch(batch)
        tks = [s(ctx, t) for t, s in enumerate(submits)]
        res = []
        for tk in tks:
            out = ctx.wait(tk)
            res.append((out, _payload(cairo, ctx, out), ctx.frame_metrics(tk) if metrics else None))
            ctx.release(tk)
        return res
    finally:
        ctx.close()


def _same(got, want, tag, feed=False):
    assert len(got) == len(want)
    for t, ((a, pa, ma), (b, pb, mb)) in enumerate(zip(got, want)):
        _table_equal(a.table, b.table, f"{tag} frame {t}: block table")
        for x, y, n in zip((a.coef_y, a.coef_u, a.coef_v), (b.coef_y, b.coef_u, b.coef_v), "YUV"):
            np.testing.assert_array_equal(x, y, err_msg=f"{tag} frame {t}: coef {n}")
        assert pa == pb and pa[1] > 0, f"{tag} frame {t}: payload bits"
        assert ma == mb, f"{tag} frame {t}: metrics"
        if feed:
            assert a.feed_bits == b.feed_bits > 0 and a.feed_status == b.feed_status, f"{tag} frame {t}: feed"
            np.testing.assert_array_equal(a.feed, b.feed, err_msg=f"{tag} frame {t}: feed words")


def _packed(case) -> np.ndarray:
    """pack(tensor) of a case, (h, w, 3), computed once per case."""
    if "packed" not in case:
        case["packed"] = tr.expected(case)[1]
    return case["packed"]


def _small(case, dw, dh, crop=None) -> np.ndarray:
    """scale(pack(tensor)) of a case on the CPU, computed once per output."""
    key = ("small", dw, dh, crop)
    if key not in case:
        p = _packed(case)
        if crop:
            p = p[crop[1]:crop[1] + crop[3], crop[0]:crop[0] + crop[2]]
        case[key] = np.ascontiguousarray(ref.scale_rgb(p, dw, dh))
    return case[key]


def _submit_case(cairo, target, dev, case, t, crop=None, scaled=True, **kw):
    """Upload the case's buffer and submit it as a (scaled) tensor frame in
    the shapeless form -> ticket."""
    ptr = dev.put(case["buf"])
    d = cairo.tensor_desc((ptr + case["lead"], case["dtype"], case["strides"]), mul=case["mul"], add=case["add"])
    if not scaled:
        return target.submit_tensor(d, t, t > 0, Q, **kw)
    return target.submit_tensor(d, t, t > 0, Q, scaled=True, crop=crop, src_size=(case["w"], case["h"]), **kw)


CONFIGS = ((tr.F16, "chw", (0.0, 1.0)), (tr.U8, "hwc", None))


@pytest.fixture(scope="module")
def cif(orc):
    """band4 at 352x288, 6 frames, as tensor cases per config (computed once,
    never modified; pack() and the scaled frames are cached in the cases)."""
    rgbs = [orc.make_frame(*CIF, t) for t in range(6)]
    return {dtype: [ref.tensor_of(f, dtype, layout, vr) for f in rgbs] for dtype, layout, vr in CONFIGS}


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{tr.NAMES[c[0]]}-{c[1]}")
def test_submit_equals_submitting_the_scaled_frame(cairo, cif, cfg):
    """352x288 -> 176x144, an intra frame and three P frames at q = 16: block
    tables, coefficients, feed words, payload bits and metrics equal those of
    submitting the CPU-scaled RGB24 frames."""
    w, h = 176, 144
    cases = cif[cfg[0]][:4]
    dev = _Resident()
    outputs = cairo.OUT_COEF | cairo.OUT_FEED
    try:
        got = _run(cairo, w, h, [lambda ctx, t, c=c: _submit_case(cairo, ctx, dev, c, t) for c in cases], 2,
                   outputs=outputs, metrics=True)
        want = _run(cairo, w, h, [lambda ctx, t, c=c: ctx.submit(_small(c, w, h), t, t > 0, Q) for c in cases], 2,
                    outputs=outputs, metrics=True)
        _same(got, want, f"{tr.NAMES[cfg[0]]} {cfg[1]}", feed=True)
        # the same frames through cairo_ctx_submit_scaled of pack(tensor)
        mid = _run(cairo, w, h, [lambda ctx, t, c=c: ctx.submit(dev.put(_packed(c).reshape(-1)), t, t > 0, Q,
                                                                   on_device=True, src_size=CIF) for c in cases], 2,
                   outputs=outputs, metrics=True)
        _same(mid, want, "scaled submit of pack(tensor)", feed=True)
    finally:
        dev.free()


def test_mixed_launch(orc, cairo, cif):
    """Launches of five 176x144 frames: a scaled tensor frame (bfloat16, RGBA
    strides, cropped from 356x292), a plain tensor frame (float32 HWC), a scaled
    NV12 frame, a device BGR24 frame and a host RGB frame.  Twice over, so that
    the second launch follows the first on the other stream.  Every frame
    equals the run in which it is submitted pre-converted."""
    w, h = 176, 144
    crop = (2, 4, 352, 288)
    dev = _Resident()
    try:
        mixed, plain = [], []
        for t in range(10):
            k = t % 5
            if k == 0:
                c = ref.tensor_of(orc.make_frame(356, 292, t), tr.BF16, "rgba", (-1.0, 1.0), lead=6)
                mixed.append(lambda ctx, t, c=c: _submit_case(cairo, ctx, dev, c, t, crop=crop))
                plain.append(lambda ctx, t, c=c: ctx.submit(_small(c, w, h, crop), t, t > 0, Q))
            elif k == 1:
                c = ref.tensor_of(orc.make_frame(w, h, t), tr.F32, "hwc", (0.0, 255.0), lead=20)
                mixed.append(lambda ctx, t, c=c: _submit_case(cairo, ctx, dev, c, t, scaled=False))
                plain.append(lambda ctx, t, c=c: ctx.submit(_packed(c), t, t > 0, Q))
            elif k == 2:
                f = pf.planes_to_frame(*pf.oracle_input_planes(orc, orc.make_frame(*CIF, t)), pf.NV12, *CIF)
                mixed.append(lambda ctx, t, f=f: ctx.submit(dev.put(f), t, t > 0, Q, on_device=True, fmt=cairo.FMT_NV12,
                                                            src_size=CIF))
                plain.append(lambda ctx, t, f=f: ctx.submit(sr.scaled_frame(f, sr.NV12, 0, (CIF, None), w, h), t, t > 0,
                                                            Q, fmt=cairo.FMT_NV12))
            elif k == 3:
                f = pf.rgb_to_frame(orc.make_frame(w, h, t), pf.BGR24)
                mixed.append(lambda ctx, t, f=f: ctx.submit(dev.put(f), t, t > 0, Q, on_device=True, fmt=cairo.FMT_BGR24))
                plain.append(lambda ctx, t, f=f: ctx.submit(f, t, t > 0, Q, fmt=cairo.FMT_BGR24))
            else:
                c = cif[tr.U8][t % 6]
                mixed.append(lambda ctx, t, c=c: ctx.submit(_small(c, w, h), t, t > 0, Q))
                plain.append(lambda ctx, t, c=c: ctx.submit(_small(c, w, h), t, t > 0, Q))
        _same(_run(cairo, w, h, mixed, 5), _run(cairo, w, h, plain, 5), "mixed launch")
    finally:
        dev.free()


@pytest.fixture(scope="module")
def many(orc):
    """40 tensor frames of 128x96 in turning dtypes, layouts and leads."""
    layouts = ("chw", "hwc", "chw_padded", "rgba")
    return [ref.tensor_of(orc.make_frame(128, 96, t), DTYPES[t % 4], layouts[(t // 4) % 4], (0.0, 1.0),
                          lead=(0, 4, 20)[t % 3]) for t in range(40)]


@pytest.mark.parametrize("frames", (32, 40))
def test_one_launch_of_many_scaled_tensor_frames(cairo, many, frames):
    """One launch of 32 scaled tensor frames (one argument block, nearly full)
    and one of 40 (more than the 36 a block holds: two kernels), 128x96 ->
    64x48, every dtype and layout; the frames equal the pre-scaled run's."""
    w, h = 64, 48
    dev = _Resident()
    try:
        cases = many[:frames]
        got = _run(cairo, w, h, [lambda ctx, t, c=c: _submit_case(cairo, ctx, dev, c, t) for c in cases], frames,
                   stages=96)
        want = _run(cairo, w, h, [lambda ctx, t, c=c: ctx.submit(_small(c, w, h), t, t > 0, Q) for c in cases], frames,
                    stages=96)
        _same(got, want, f"{frames} frames in one launch")
    finally:
        dev.free()


def test_ladder(cairo, cif):
    """One resident 352x288 float16 tensor sequence feeds contexts of 352x288
    (a copy), 176x144 and 88x72 in the same process, frame by frame; each
    stream equals its own pre-scaled run."""
    cases = cif[tr.F16][:4]
    rungs = (CIF, (176, 144), (88, 72))
    dev = _Resident()
    ctxs = [cairo.Context(w, h, RING, stages=8) for w, h in rungs]
    got = [[] for _ in rungs]
    try:
        descs = []
        for c in cases:
            ptr = dev.put(c["buf"])
            descs.append(cairo.tensor_desc((ptr + c["lead"], c["dtype"], c["strides"]), mul=c["mul"], add=c["add"]))
        tks = [[x.submit_tensor(d, t, t > 0, Q, scaled=True, src_size=CIF) for x in ctxs] for t, d in enumerate(descs)]
        for t in range(len(cases)):
            for k, x in enumerate(ctxs):
                out = x.wait(tks[t][k])
                got[k].append((out, _payload(cairo, x, out), None))
                x.release(tks[t][k])
    finally:
        for x in ctxs:
            x.close()
        dev.free()
    for k, (w, h) in enumerate(rungs):
        want = _run(cairo, w, h, [lambda ctx, t, c=c: ctx.submit(_small(c, w, h), t, t > 0, Q) for c in cases], 4)
        _same(got[k], want, f"ladder {w}x{h}")


def test_pipeline(cairo, cif):
    """Stream.submit_tensor(..., scaled=True) payload bits equal those of the
    pre-scaled Stream run over 6 frames."""
    w, h = 176, 144
    cases = cif[tr.F16]

    def pipeline(submit):
        ctx = cairo.Context(w, h, RING, stages=16)
        ctx.set_batch(3)
        st = cairo.Stream(ctx, threads=2)
        try:
            tks = [submit(st, t) for t in range(len(cases))]
            return [st.collect(tk) for tk in tks]
        finally:
            st.close()
            ctx.close()

    dev = _Resident()
    try:
        got = pipeline(lambda st, t: _submit_case(cairo, st, dev, cases[t], t))
    finally:
        dev.free()
    want = pipeline(lambda st, t: st.submit(_small(cases[t], w, h), t, t > 0, Q))
    assert got == want, "Stream.submit_tensor(scaled=True) payloads differ from the pre-scaled run"
    assert all(nb > 0 for _, nb in want)


def test_torch_batch_frames(orc, cairo):
    """submit_tensor(batch[n], scaled=True) of a (3, 3, 96, 128) float16 CUDA
    batch into a 64x48 context, and crop= alone into a 32x24 one: the source
    size is the tensor's own shape."""
    hh, ww = 96, 128
    rgbs = [orc.make_frame(ww, hh, t) for t in range(3)]
    host = np.stack([(f.astype(np.float32) / 255.0).transpose(2, 0, 1) for f in rgbs]).astype(np.float16)
    batch = torch.from_numpy(host).to("cuda")
    mul, add = tr.range_map(0.0, 1.0, output=False)
    packed = [tr.pack(tr.F16, host[n].view(np.uint16).astype(np.uint32).transpose(1, 2, 0), (mul,) * 3, (add,) * 3)
              for n in range(3)]
    crop = (2, 6, 64, 48)
    for (w, h), kw, src in (((64, 48), dict(scaled=True), packed),
                            ((32, 24), dict(crop=crop), [p[6:54, 2:66] for p in packed])):
        got = _run(cairo, w, h, [lambda ctx, t, n=n: ctx.submit_tensor(batch[n], t, t > 0, Q, **kw) for n in range(3)], 3)
        want = _run(cairo, w, h, [lambda ctx, t, f=f: ctx.submit(np.ascontiguousarray(ref.scale_rgb(f, w, h)), t, t > 0, Q)
                                  for f in src], 3)
        _same(got, want, f"batch[n] -> {w}x{h}")
    ctx = cairo.Context(64, 48, RING, stages=4)
    try:
        with pytest.raises(ValueError):  # without the keywords: not the context's size, as ever
            ctx.submit_tensor(batch[0], 0, False, Q)
        with pytest.raises(ValueError):
            ctx.submit_tensor(batch[0], 0, False, Q, scaled=True, src_size=(128, 98))
    finally:
        ctx.close()


def test_refusals(cairo, cif):
    """A host tensor, a span two rows beyond the allocation, an upscale, more
    than 8:1 and an odd crop are refused with EVX_ERROR_INVALID_ARGS; no ticket
    is taken, and the next valid submits are frames 0 and 1 of a correct
    stream."""
    w, h = 176, 144
    cases = cif[tr.U8]
    case = cases[0]
    ctx = cairo.Context(w, h, RING, stages=8)
    dev = _Resident()
    try:
        ptr = dev.put(case["buf"])
        st = case["strides"]

        def refused(base, strides=st, src_size=CIF, crop=None):
            d = cairo.tensor_desc((base, tr.U8, strides), mul=case["mul"], add=case["add"])
            with pytest.raises(cairo.CairoError) as ei:
                ctx.submit_tensor(d, 0, False, Q, scaled=True, crop=crop, src_size=src_size)
            assert ei.value.status == cairo.EVX_ERROR_INVALID_ARGS

        refused(case["buf"].ctypes.data)                         # a host tensor
        refused(ptr, src_size=(352, 290))                        # two rows more than the allocation holds
        refused(ptr, crop=(0, 0, 174, 144))                      # upscaling 174 -> 176
        refused(ptr, crop=(0, 0, 176, 142))                      # upscaling 142 -> 144
        refused(ptr, crop=(1, 0, 350, 288))                      # an odd crop
        refused(ptr, crop=(0, 2, 352, 285))
        big = _DeviceBuffer(1410 * 1154 * 3)
        dev.bufs.append(big)
        refused(big.ptr, strides=(1, 3 * 1410, 3), src_size=(1410, 1152))  # 1410 > 8 * 176
        refused(big.ptr, strides=(1, 3 * 1408, 3), src_size=(1408, 1154))  # 1154 > 8 * 144
        tks = [_submit_case(cairo, ctx, dev, cases[t], t) for t in range(2)]
        assert tks == [0, 1], "a refused submit took a ticket"
        got = []
        for tk in tks:
            out = ctx.wait(tk)
            got.append((out, _payload(cairo, ctx, out), None))
            ctx.release(tk)
        want = _run(cairo, w, h, [lambda c, t, k=k: c.submit(_small(k, w, h), t, t > 0, Q) for k in cases[:2]], 4)
        _same(got, want, "after the refusals")
    finally:
        ctx.close()
        dev.free()
