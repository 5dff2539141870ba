"""Tensor frames on the GPU (tensor.hip; cairo_ctx_submit_tensor,
cairo_ctx_decode_frame_tensor, cairo_ctx_fetch_recon_tensor).

KAT: the two kernels on their own (cairo_kat_tensor) against the exact
restatement tests/tensor_ref.py, byte for byte, guards and untouched bytes
included.  Then the defining properties: a tensor submit produces exactly the
bits of submitting pack(tensor) as RGB24 (against the oracle), and a frame
decoded or fetched into a tensor is unpack of the RGB24 frame; mixed launches,
reused staging slots, the frame pipeline, the drop-in API, torch tensors, and
the refusals.
"""
import torch  # noqa: F401  (first, as the tools do: the package finds it in sys.modules)

import ctypes

import numpy as np
import pytest

from tests import pixfmt_ref as pf
from tests import tensor_ref as ref

pytestmark = pytest.mark.gpu

RING, Q = 4, 16
DTYPES = (ref.U8, ref.F16, ref.BF16, ref.F32)
_dt = lambda d: ref.NAMES[d]  # noqa: E731


class _DeviceBuffer:
    """Device memory from the HIP runtime the library itself uses (by soname:
    the copy already loaded into this process)."""

    def __init__(self, nbytes: int, fill: int = ref.FILL):
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

    def download(self) -> np.ndarray:
        out = np.empty(self.nbytes, np.uint8)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0  # hipMemcpyDeviceToHost
        return out

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

KAT_SIZES = ((16, 16), (18, 10), (64, 48), (1030, 6))
KAT_LAYOUTS = ("chw", "hwc", "chw_padded", "rgba", "chw_misaligned")
GUARD = 64


def _at_mod16(buf: np.ndarray, lead: int, mod: int) -> np.ndarray:
    """A copy of buf whose byte `lead` (element (0, 0, 0)) has address `mod`
    modulo 16; cairo_kat_tensor's device copy keeps that."""
    hold = np.empty(buf.size + 16, np.uint8)
    start = (mod - lead - hold.ctypes.data) % 16
    view = hold[start:start + buf.size]
    view[...] = buf
    assert (view.ctypes.data + lead) % 16 == mod
    return view


def _kat(cairo, case, mod16):
    want_buf, want_rgb = ref.expected(case)
    w, h, lead = case["w"], case["h"], case["lead"]
    buf = _at_mod16(case["buf"], lead, mod16)
    rgb = np.concatenate([case["rgb"].reshape(-1), np.full(cairo.KAT_TENSOR_GUARD, ref.FILL, np.uint8)])
    d = cairo.tensor_desc((buf.ctypes.data + lead, case["dtype"], case["strides"]), mul=case["mul"], add=case["add"])
    cairo.kat_tensor(case["dir"], d, w, h, buf.size - lead, rgb)
    tag = f"{case['name']} base%16={mod16}"
    np.testing.assert_array_equal(rgb[:3 * w * h], want_rgb.reshape(-1), err_msg=f"{tag}: RGB24 frame")
    assert (rgb[3 * w * h:] == ref.FILL).all(), f"{tag}: bytes behind the tight frame written"
    # the covered elements, every byte between them, and the guard behind the span
    np.testing.assert_array_equal(buf, want_buf, err_msg=f"{tag}: tensor bytes")


# (a float32 base that is element-aligned is 4-byte aligned: no such case)
KAT_CASES = [(d, lay) for d in DTYPES for lay in KAT_LAYOUTS if not (d == ref.F32 and lay == "chw_misaligned")]


@pytest.mark.parametrize("dtype,layout", KAT_CASES, ids=lambda v: v if isinstance(v, str) else ref.NAMES[v])
def test_kat(cairo, dtype, layout):
    es = ref.SIZE[dtype]
    mod16 = 0
    if layout == "chw_misaligned":  # element-aligned, not 4-byte aligned
        layout, mod16 = "chw", es
    for n, (w, h) in enumerate(KAT_SIZES):
        for direction in (0, 1):
            case = ref.make_case(direction, dtype, layout, w, h, 500 + 10 * dtype + n, lead=16, tail=GUARD)
            _kat(cairo, case, mod16)
            if layout == "hwc" and (w, h) == (18, 10):  # a base 8 bytes into a 16-byte line: no 16-byte accesses
                _kat(cairo, case, 8)


def test_kat_specials(cairo):
    """Exact ties, binary16 subnormals and overflowing outputs on the device."""
    tie = lambda v: np.broadcast_to(v[None, :, None], (2, v.size, 3)).copy()  # noqa: E731
    v = np.arange(258, dtype=np.float32) - 0.5
    cases = [
        ref.make_case(0, ref.F32, "chw", 258, 2, 1, mul=(1, 1, 1), add=(0, 0, 0), bits=tie(v.view(np.uint32)), tail=GUARD),
        ref.make_case(0, ref.F16, "hwc", 258, 2, 1, mul=(1, 1, 1), add=(0, 0, 0),
                      bits=tie(v.astype(np.float16).view(np.uint16).astype(np.uint32)), tail=GUARD),
        ref.make_case(0, ref.F16, "hwc", 512, 2, 2, mul=(2.0 ** 24, 2.0 ** 22, 2.0 ** 21), add=(0, 0, 0.5),
                      bits=np.arange(1024, dtype=np.uint32).reshape(2, 512, 1).repeat(3, axis=2), tail=GUARD),
        ref.make_case(1, ref.F16, "chw", 16, 16, 3, mul=(300.0, 2.0 ** -24, -300.0), add=(0, 0, 0), tail=GUARD),
        ref.make_case(1, ref.F16, "hwc", 18, 10, 4, mul=(2.0 ** -26, 3e-8, 1e-7), add=(0, 1e-8, -6e-6), tail=GUARD),
        ref.make_case(1, ref.F32, "chw", 16, 16, 5, mul=(3e38, 1e-40, -3e38), add=(0, 0, -1e38), tail=GUARD),
        ref.make_case(1, ref.BF16, "chw", 16, 16, 6, mul=(3e38, 1e-40, 1.00390625), add=(3e38, 0, 0), tail=GUARD),
        ref.make_case(1, ref.F32, "hwc", 16, 16, 7, mul=(-1.0, 0.0, -0.0), add=(0.0, -0.0, -0.0), tail=GUARD),
    ]
    for case in cases:
        _kat(cairo, case, 0)


# ---------------------------------------------------------------------------
# Encoder: a tensor submit gives the bits of submitting pack(tensor)
# ---------------------------------------------------------------------------

def _table_equal(a, b, what):
    for f in a.dtype.names:
        if f == "pad":
            continue
        bad = np.nonzero(a[f] != b[f])[0]
        assert bad.size == 0, f"{what}: field {f} differs at MBs {bad[:10]} gpu={a[f][bad[:5]]} ref={b[f][bad[:5]]}"


def _oracle_run(orc, rgbs, ring, q):
    e = orc.OracleEncoder(ring)
    e.set_quality(q)
    out = []
    for t, rgb in enumerate(rgbs):
        e.encode(np.ascontiguousarray(rgb))
        cp = lambda p: tuple(a.copy() for a in p)  # noqa: E731
        out.append(dict(rgb=rgb, table=e.block_table().copy(), coef=cp(e.planes(1)), recon=cp(e.planes(2 + t % ring))))
    return out


def _check_frame(ctx, out, rec, t, tag, slot=True):
    _table_equal(out.table, rec["table"], f"{tag}: block table")
    for got, want, n in zip((out.coef_y, out.coef_u, out.coef_v), rec["coef"], "YUV"):
        np.testing.assert_array_equal(got, want, err_msg=f"{tag}: coef {n}")
    if slot:
        for got, want, n in zip(ctx.read_planes(2 + t % RING), rec["recon"], "YUV"):
            np.testing.assert_array_equal(got, want, err_msg=f"{tag}: ring slot {n} (deblocked)")


def _tensor_of(rgb: np.ndarray, dtype: int, layout: str, vr, lead: int = 0):
    """A tensor frame made from an RGB image: values spread over value_range
    with a small position-dependent offset (four values), so that the rounding
    decides samples.  -> (case dict as tensor_ref.make_case's, for direction 0)."""
    h, w = rgb.shape[:2]
    if dtype == ref.U8:
        bits = rgb.astype(np.uint32)
        mul, add = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
    else:
        y, x = np.mgrid[0:h, 0:w]
        jit = np.array([-0.45, -0.2, 0.3, 0.49], np.float32)[(x + 2 * y) % 4][..., None]
        m, a = ref.range_map(*vr, output=True)
        f = ((rgb.astype(np.float32) + jit) * m + a).astype(np.float32)
        if dtype == ref.F32:
            bits = f.view(np.uint32)
        elif dtype == ref.BF16:
            bits = f.view(np.uint32) >> 16
        else:
            bits = f.astype(np.float16).view(np.uint16).astype(np.uint32)
        mi, ai = ref.range_map(*vr, output=False)
        mul, add = (mi,) * 3, (ai,) * 3
    return ref.make_case(0, dtype, layout, w, h, 0, mul=mul, add=add, lead=lead, bits=np.ascontiguousarray(bits))


def _packed(case) -> np.ndarray:
    """pack(tensor) of a case, (h, w, 3), computed once per case."""
    if "packed" not in case:
        case["packed"] = ref.expected(case)[1]
    return case["packed"]


def _submit_case(cairo, target, dev, case, t, **kw):
    """Upload the case's buffer and submit it as a tensor frame -> ticket."""
    ptr = dev.put(case["buf"])
    d = cairo.tensor_desc((ptr + case["lead"], case["dtype"], case["strides"]), mul=case["mul"], add=case["add"])
    return target.submit_tensor(d, t, t > 0, Q, **kw)


CONFIGS = ((ref.F16, "chw", (0.0, 1.0)), (ref.F32, "hwc", (-1.0, 1.0)), (ref.U8, "hwc", None))


@pytest.fixture(scope="module")
def streams(orc):
    """Per size and config: three tensor frames (I, P, P) made from band4, their
    pack() and the oracle's encode of those RGB24 frames.  Computed once."""
    out = {}
    for w, h in ((64, 48), (352, 288)):
        rgbs = [orc.make_frame(w, h, t) for t in range(3)]
        for dtype, layout, vr in CONFIGS:
            cases = [_tensor_of(f, dtype, layout, vr) for f in rgbs]
            out[(w, h, dtype)] = dict(cases=cases, recs=_oracle_run(orc, [_packed(c) for c in cases], RING, Q))
    return out


@pytest.mark.parametrize("size", ((64, 48), (352, 288)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"{ref.NAMES[c[0]]}-{c[1]}")
def test_submit_equals_rgb24_of_pack(cairo, streams, size, cfg):
    (w, h), dtype = size, cfg[0]
    s = streams[(w, h, dtype)]
    ctx = cairo.Context(w, h, RING, stages=8)
    dev = _Resident()
    try:
        for t, (case, rec) in enumerate(zip(s["cases"], s["recs"])):
            tk = _submit_case(cairo, ctx, dev, case, t)
            out = ctx.wait(tk)
            _check_frame(ctx, out, rec, t, f"{case['name']} frame {t}")
            ctx.release(tk)
        if dtype == ref.U8:  # mul = 1, add = 0: the tensor's bytes are the RGB24 frame
            ctx.reset()
            for t, (case, rec) in enumerate(zip(s["cases"], s["recs"])):
                np.testing.assert_array_equal(case["buf"].reshape(h, w, 3), _packed(case))
                out = ctx.encode_frame(dev.put(case["buf"]), t, t > 0, Q, on_device=True, fmt=cairo.FMT_RGB24,
                                       pitch=3 * w)  # a pitch: through cairo_ctx_submit_fmt
                _check_frame(ctx, out, rec, t, f"submit_fmt frame {t}")
    finally:
        ctx.close()
        dev.free()


def _payload(cairo, ctx, out):
    return cairo.serialize_slice(out.table, ctx.wmb, ctx.hmb, ctx.ring, out.coef_y, out.coef_u, out.coef_v)


def _run(cairo, w, h, submits, batch, stages=16):
    """Frames submitted to a fresh context, then waited in order.  submits:
    callables (ctx, t) -> ticket.  -> per frame (FrameOutputs, payload)."""
    ctx = cairo.Context(w, h, RING, stages=stages)
    try:
        ctx.set_batch(batch)
        tks = [s(ctx, t) for t, s in enumerate(submits)]
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
        assert pa == pb and pa[1] > 0, f"{tag} frame {t}: payload bits"


def test_mixed_launch(orc, cairo):
    """One launch of six 64x48 frames: F16 (padded CHW), BF16 (RGBA-strided)
    and F32 (HWC, at an offset) tensor frames with different maps, an RGB24
    host frame, an NV12 device frame and a U8 CHW tensor frame.  Every frame
    equals the run in which it is submitted in its single format."""
    w, h = 64, 48
    rgbs = [orc.make_frame(w, h, t) for t in range(6)]
    tens = {0: _tensor_of(rgbs[0], ref.F16, "chw_padded", (0.0, 1.0)),
            1: _tensor_of(rgbs[1], ref.BF16, "rgba", (-1.0, 1.0), lead=6),
            2: _tensor_of(rgbs[2], ref.F32, "hwc", (0.0, 255.0), lead=20),
            5: _tensor_of(rgbs[5], ref.U8, "chw", None, lead=3)}
    nv12 = pf.planes_to_frame(*pf.oracle_input_planes(orc, rgbs[4]), pf.NV12, w, h)
    dev = _Resident()
    try:
        mixed, plain = [], []
        for t in range(6):
            if t in tens:
                mixed.append(lambda ctx, t, c=tens[t]: _submit_case(cairo, ctx, dev, c, t))
                plain.append(lambda ctx, t, c=tens[t]: ctx.submit(_packed(c), t, t > 0, Q))
            elif t == 3:
                mixed.append(lambda ctx, t: ctx.submit(rgbs[3], t, t > 0, Q))
                plain.append(lambda ctx, t: ctx.submit(rgbs[3], t, t > 0, Q))
            else:
                mixed.append(lambda ctx, t: ctx.submit(dev.put(nv12), t, t > 0, Q, on_device=True, fmt=cairo.FMT_NV12))
                plain.append(lambda ctx, t: ctx.submit(nv12, t, t > 0, Q, fmt=cairo.FMT_NV12))
        _same(_run(cairo, w, h, mixed, 6), _run(cairo, w, h, plain, 6), "mixed launch")
    finally:
        dev.free()


def test_slot_reuse(orc, cairo):
    """stages = 4, batch = 2, ten tensor frames: slots and their rgb_read
    waits are reused; every frame matches the oracle's encode of pack()."""
    w, h, n = 64, 48, 10
    cases = [_tensor_of(orc.make_frame(w, h, t), (ref.F16, ref.F32, ref.BF16)[t % 3], ("chw", "hwc")[t % 2],
                        (0.0, 1.0)) for t in range(n)]
    recs = _oracle_run(orc, [_packed(c) for c in cases], RING, Q)
    ctx = cairo.Context(w, h, RING, stages=4)
    ctx.set_batch(2)
    dev = _Resident()
    try:
        tks = []
        for t in range(n + 4):
            if t >= 4:  # four in flight: the oldest leaves before its slot is taken again
                out = ctx.wait(tks[t - 4])
                _check_frame(ctx, out, recs[t - 4], t - 4, f"slot reuse frame {t - 4}", slot=False)
                ctx.release(tks[t - 4])
            if t < n:
                tks.append(_submit_case(cairo, ctx, dev, cases[t], t))
    finally:
        ctx.close()
        dev.free()


def test_pipeline(orc, cairo):
    """Stream.submit_tensor payload bits equal the RGB24 stream's."""
    w, h = 64, 48
    cases = [_tensor_of(orc.make_frame(w, h, t), ref.F16, "chw", (0.0, 1.0)) for t in range(6)]

    def pipeline(submit):
        ctx = cairo.Context(w, h, RING, stages=16)
        ctx.set_batch(3)
        st = cairo.Stream(ctx, threads=2)
        try:
            tks = [submit(st, t) for t in range(6)]
            return [st.collect(tk) for tk in tks]
        finally:
            st.close()
            ctx.close()

    dev = _Resident()
    try:
        got = pipeline(lambda st, t: _submit_case(cairo, st, dev, cases[t], t))
    finally:
        dev.free()
    want = pipeline(lambda st, t: st.submit(_packed(cases[t]), t, t > 0, Q))
    assert got == want, "Stream.submit_tensor payloads differ from the RGB24 run"
    assert all(nb > 0 for _, nb in want)


# ---------------------------------------------------------------------------
# Decoder: a frame written into a tensor is unpack of the RGB24 frame
# ---------------------------------------------------------------------------

OUT_LAYOUT = {ref.U8: "rgba", ref.F16: "chw_padded", ref.BF16: "rgba", ref.F32: "chw_padded"}
LEAD, TAIL = 32, 96


def _out_case(dtype, w, h):
    """A strided destination inside a larger allocation, FILL everywhere."""
    mul, add = ((1.0,) * 3, (0.0,) * 3) if dtype == ref.U8 else (None, None)
    return ref.make_case(1, dtype, OUT_LAYOUT[dtype], w, h, 0, mul=mul, add=add, lead=LEAD, tail=TAIL)


def _expect_unpacked(case, rgb):
    c = dict(case, rgb=rgb)
    return ref.expected(c)[0]


def _out_desc(cairo, case, ptr):
    return cairo.tensor_desc((ptr + case["lead"], case["dtype"], case["strides"]), mul=case["mul"], add=case["add"])


@pytest.mark.parametrize("size", ((64, 48), (352, 288)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_decode_frame_tensor(cairo, streams, size):
    """cairo_ctx_decode_frame_tensor equals unpack of cairo_ctx_decode_frame's
    RGB24, per dtype, into a strided view whose other bytes keep FILL."""
    w, h = size
    recs = streams[(w, h, ref.F16)]["recs"]
    plain = cairo.Context(w, h, RING, stages=2)
    ctxs = {d: cairo.Context(w, h, RING, stages=2) for d in DTYPES}
    try:
        for t, rec in enumerate(recs):
            rgb = plain.decode_frame(rec["table"], rec["coef"], t)
            np.testing.assert_array_equal(rgb, cairo.yuv_to_rgb(*rec["recon"], w, h))
            for d in DTYPES:
                case = _out_case(d, w, h)
                buf = _DeviceBuffer(case["buf"].size)
                try:
                    ctxs[d].decode_frame_tensor(rec["table"], rec["coef"], t, _out_desc(cairo, case, buf.ptr))
                    np.testing.assert_array_equal(buf.download(), _expect_unpacked(case, rgb),
                                                  err_msg=f"{ref.NAMES[d]} frame {t}")
                finally:
                    buf.free()
    finally:
        plain.close()
        for c in ctxs.values():
            c.close()


def test_fetch_recon_tensor(cairo, streams):
    """cairo_ctx_fetch_recon_tensor equals unpack of cairo_ctx_fetch_recon's RGB24."""
    for w, h in ((64, 48), (352, 288)):
        s = streams[(w, h, ref.F16)]
        ctx = cairo.Context(w, h, RING, stages=4)
        ctx.set_metrics(sse=False, ssim=False, keep_recon=True)
        dev = _Resident()
        try:
            for t, (case, rec) in enumerate(zip(s["cases"], s["recs"])):
                tk = _submit_case(cairo, ctx, dev, case, t)
                ctx.wait(tk)
                rgb = ctx.fetch_recon(tk, cairo.FMT_RGB24).reshape(h, w, 3)
                np.testing.assert_array_equal(rgb, cairo.yuv_to_rgb(*rec["recon"], w, h))
                for d in DTYPES:
                    oc = _out_case(d, w, h)
                    buf = _DeviceBuffer(oc["buf"].size)
                    dev.bufs.append(buf)
                    ctx.fetch_recon_tensor(tk, _out_desc(cairo, oc, buf.ptr))
                    np.testing.assert_array_equal(buf.download(), _expect_unpacked(oc, rgb),
                                                  err_msg=f"{w}x{h} {ref.NAMES[d]} frame {t}")
                ctx.release(tk)
        finally:
            ctx.close()
            dev.free()


def test_drop_in_encoder_and_decoder(orc, cairo, streams):
    """Encoder.set_input_tensor writes the oracle's stream of pack(); Decoder.
    set_output_tensor decodes it into unpack of the oracle's reconstruction."""
    w, h = 64, 48
    s = streams[(w, h, ref.F16)]
    enc, dec = cairo.Encoder(ring=RING), cairo.Decoder()
    enc.set_quality(Q)
    oracle = orc.OracleEncoder(RING)
    oracle.set_quality(Q)
    first = s["cases"][0]
    enc.set_input_tensor((0, first["dtype"], first["strides"]), mul=first["mul"], add=first["add"])
    oc = _out_case(ref.BF16, w, h)
    dec.set_output_tensor((0, oc["dtype"], oc["strides"]), mul=oc["mul"], add=oc["add"])
    bs = cairo.BitStream(w * h * 64)
    dev = _Resident()
    try:
        for t, (case, rec) in enumerate(zip(s["cases"], s["recs"])):
            bs.empty()
            enc.encode(dev.put(case["buf"]), bs, w, h)
            data, nbits = oracle.encode(_packed(case))
            assert bs.bits() == nbits and orc.canonical_frame_bytes(bs.data(), bs.bits(), t == 0) == \
                orc.canonical_frame_bytes(data, nbits, t == 0), f"frame {t}: stream differs from the oracle's"
            buf = _DeviceBuffer(oc["buf"].size)
            dev.bufs.append(buf)
            dec.decode(bs, w, h, out=buf.ptr + oc["lead"])
            want = _expect_unpacked(oc, cairo.yuv_to_rgb(*rec["recon"], w, h))
            np.testing.assert_array_equal(buf.download(), want, err_msg=f"frame {t}")
        # back to the pixel formats
        enc.set_input_tensor(None)
        dec.set_output_tensor(None)
        bs.empty()
        rgb = orc.make_frame(w, h, 3)
        enc.encode(rgb, bs)
        oracle.encode(rgb)
        np.testing.assert_array_equal(dec.decode(bs, w, h), cairo.yuv_to_rgb(*oracle.planes(2 + 3 % RING), w, h))
    finally:
        enc.close()
        dec.close()
        dev.free()


# ---------------------------------------------------------------------------
# torch
# ---------------------------------------------------------------------------

def _torch_bits(t) -> np.ndarray:
    """The element bits of a torch tensor on any device, (..., ) uint32."""
    c = t.detach().cpu().contiguous()
    if c.dtype == torch.float32:
        return c.view(torch.int32).numpy().view(np.uint32)
    if c.dtype in (torch.float16, torch.bfloat16):
        return c.view(torch.int16).numpy().view(np.uint16).astype(np.uint32)
    return c.numpy().astype(np.uint32)


def test_torch_batch_and_channels_last(orc, cairo):
    """submit_tensor of the frames batch[n] of a (4, 3, 64, 48) float16 CUDA
    tensor, and of the frames of its channels_last copy: both equal the oracle's
    encode of pack(batch[n])."""
    hh, ww = 64, 48  # (N, C, H, W): frames of 48 x 64
    rgbs = [orc.make_frame(ww, hh, t) for t in range(4)]
    host = np.stack([(f.astype(np.float32) / 255.0).transpose(2, 0, 1) for f in rgbs]).astype(np.float16)
    batch = torch.from_numpy(host).to("cuda")
    assert batch.shape == (4, 3, hh, ww)
    mul, add = ref.range_map(0.0, 1.0, output=False)
    packed = [ref.pack(ref.F16, _torch_bits(batch[n]).transpose(1, 2, 0), (mul,) * 3, (add,) * 3) for n in range(4)]
    recs = _oracle_run(orc, packed, RING, Q)
    for name, src in (("batch[n]", batch), ("channels_last", batch.to(memory_format=torch.channels_last))):
        assert name == "batch[n]" or src.stride() == (3 * hh * ww, 1, 3 * ww, 3)
        ctx = cairo.Context(ww, hh, RING, stages=8)
        try:
            tks = [ctx.submit_tensor(src[n], n, n > 0, Q) for n in range(4)]
            for n, tk in enumerate(tks):
                _check_frame(ctx, ctx.wait(tk), recs[n], n, f"{name} frame {n}", slot=False)
                ctx.release(tk)
        finally:
            ctx.close()


def test_torch_decode_into_bfloat16(orc, cairo, streams):
    """Decoder.decode(..., out=t) into a bfloat16 CUDA tensor: unpack of the
    oracle's reconstruction, compared through .cpu()."""
    w, h = 64, 48
    s = streams[(w, h, ref.F16)]
    enc, dec = cairo.Encoder(ring=RING), cairo.Decoder()
    enc.set_quality(Q)
    out = torch.full((3, h, w), -7.0, dtype=torch.bfloat16, device="cuda")
    dec.set_output_tensor(out, value_range=(-1.0, 1.0))
    mul, add = ref.range_map(-1.0, 1.0, output=True)
    bs = cairo.BitStream(w * h * 64)
    try:
        for t, (case, rec) in enumerate(zip(s["cases"], s["recs"])):
            bs.empty()
            enc.encode(_packed(case), bs)
            assert dec.decode(bs, w, h, out=out) is out
            want = ref.unpack(ref.BF16, cairo.yuv_to_rgb(*rec["recon"], w, h), (mul,) * 3, (add,) * 3)
            np.testing.assert_array_equal(_torch_bits(out).transpose(1, 2, 0), want, err_msg=f"frame {t}")
    finally:
        enc.close()
        dec.close()


# ---------------------------------------------------------------------------
# Refusals
# ---------------------------------------------------------------------------

def test_refusals(orc, cairo, streams):
    """Each refusal is EVX_ERROR_INVALID_ARGS and takes no ticket; the next
    valid submit is frame 0 of a correct stream.  A tensor submit into an
    unreleased slot reports the existing status."""
    w, h = 64, 48
    s = streams[(w, h, ref.F16)]
    case = s["cases"][0]
    ctx = cairo.Context(w, h, RING, stages=2)
    dev = _Resident()
    try:
        ptr = dev.put(case["buf"])

        def refused(base, strides=case["strides"], dtype=ref.F16, mul=case["mul"], status=cairo.EVX_ERROR_INVALID_ARGS):
            d = cairo.tensor_desc((base, dtype, strides), mul=mul, add=case["add"])
            with pytest.raises(cairo.CairoError) as ei:
                ctx.submit_tensor(d, 0, False, Q)
            assert ei.value.status == status

        refused(case["buf"].ctypes.data)                      # a host pointer
        refused(ptr, strides=(w * (h + 1), w, 1))             # a view declared one row too tall for its allocation
        refused(ptr, strides=(w * h, w - 1, 1))               # rows overlap
        refused(ptr, strides=(1, 3 * w, 2))                   # pixels overlap
        refused(ptr, dtype=7)                                 # an unknown dtype
        refused(ptr, mul=(np.inf, 255.0, 255.0))              # a non-finite factor
        refused(ptr, mul=(255.0, np.nan, 255.0))
        refused(ptr + 1)                                      # a base that is not element-aligned
        for t in range(2):
            tk = _submit_case(cairo, ctx, dev, s["cases"][t], t)
            assert tk == t, "a refused submit took a ticket"
        # both slots busy: the existing status, and still no ticket
        refused(ptr, status=8)  # EVX_ERROR_INVALID_RESOURCE
        for t in range(2):
            out = ctx.wait(t)
            _check_frame(ctx, out, s["recs"][t], t, f"after the refusals, frame {t}", slot=(t == 1))
            ctx.release(t)
        tk = _submit_case(cairo, ctx, dev, s["cases"][2], 2)
        assert tk == 2
        _check_frame(ctx, ctx.wait(tk), s["recs"][2], 2, "frame 2")
        ctx.release(tk)
        # the output side: a host destination and a span beyond the allocation
        oc = _out_case(ref.F32, w, h)
        small = _DeviceBuffer(oc["buf"].size - TAIL - 4)
        dev.bufs.append(small)
        host = np.zeros(oc["buf"].size, np.uint8)
        for base in (host.ctypes.data, small.ptr):
            with pytest.raises(cairo.CairoError) as ei:
                ctx.decode_frame_tensor(s["recs"][0]["table"], s["recs"][0]["coef"], 0, _out_desc(cairo, oc, base))
            assert ei.value.status == cairo.EVX_ERROR_INVALID_ARGS
        assert (small.download() == ref.FILL).all(), "a refused decode wrote its destination"
    finally:
        ctx.close()
        dev.free()
