"""cairo_amd -- MI355X-native EVX-1 (hinike/cairo) encode path.

The product is ``_lib/libcairo_amd.so``: hand-written HIP kernels for gfx950
(convert, inter search, macroblock wavefront with in-loop deblock), the host entropy stage
and the drop-in ``evx1_encoder`` / ``bit_stream`` C++ API.  This module is a
thin ctypes view of its C ABI (``include/cairo_amd.h``) for tests, the bench
and Python callers.  There is no Python or CPU fallback for the hot path: if
the library is missing, importing the bindings raises.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libcairo_amd.so")

# evx_block_desc (reference common.h:78-95, pack(2), 16 bytes)
BLOCK_DESC = np.dtype(
    [
        ("block_type", "<u4"),
        ("prediction_target", "u1"),
        ("pad", "u1"),
        ("motion_x", "<i2"),
        ("motion_y", "<i2"),
        ("sp_pred", "u1"),
        ("sp_amount", "u1"),
        ("sp_index", "u1"),
        ("q_index", "u1"),
        ("variance", "<i2"),
    ]
)
assert BLOCK_DESC.itemsize == 16

EVX_SUCCESS = 0
API_VERSION = 4  # include/cairo_amd.h CAIRO_AMD_API_VERSION
OUT_COEF, OUT_FEED = 1, 2  # cairo_ctx_set_outputs
FEED_NONE, FEED_VALID, FEED_OVERFLOW = 0, 1, 2
MAX_COEF_CHUNKS = 16  # CAIRO_MAX_COEF_CHUNKS
PEER_SIZE = 3 * 4 + 7 * 4 + 2 * 8 + MAX_COEF_CHUNKS * 8 + 2 * 64 + MAX_COEF_CHUNKS * 64  # sizeof(cairo_peer)
# EVX_PEEK_STATE (reference evx1.h:55-64)
PEEK_SOURCE, PEEK_PREDICTION, PEEK_BLOCK_TABLE, PEEK_QUANT_TABLE, PEEK_SPMP_TABLE, PEEK_BLOCK_VARIANCE, \
    PEEK_DESTINATION = range(7)
MAX_BATCH = 48  # kMaxBatch (kernels.h CAIRO_MAX_BATCH): frames per engine launch, stamp layout
EVX_ERROR_HARDWAREFAIL = 5
EVX_ERROR_INVALID_ARGS = 1
# Pixel formats (include/cairo_amd.h CAIRO_FMT_*): a frame is one contiguous
# uint8 buffer with a row pitch in bytes (0: tight); see frame_layout.
FMT_RGB24, FMT_BGR24, FMT_I420, FMT_NV12 = range(4)
# Capture and 10-bit layouts (packed 4:2:2, 16-bit words with the sample in the
# high ten bits): taken as the NV12 frame they fold to, see frame_fold.
FMT_YUY2, FMT_UYVY, FMT_P010 = 8, 9, 10
# Colour description of an I420 / NV12 frame (include/cairo_amd.h CAIRO_RANGE_*,
# CAIRO_MATRIX_*): (RANGE_FULL, MATRIX_BT601) is the codec's own space.
RANGE_FULL, RANGE_LIMITED = 0, 1
MATRIX_BT601, MATRIX_BT709 = 0, 1
# Per-frame metrics and kept reconstructions (include/cairo_amd.h, cairo_ctx_set_metrics)
METRIC_SSE, METRIC_SSIM, KEEP_RECON = 1, 2, 4


# In-kernel wait kinds of a timeout record (include/cairo_amd.h CAIRO_WAIT_*)
WAIT_KINDS = {1: "records", 2: "granule", 3: "prev_progress", 4: "row_above", 5: "batch", 6: "injected",
              9: "host_mark"}
TIMEOUT_FIELDS = ("kind", "epoch", "index", "row", "member", "need", "on", "seen_lo", "seen_hi")


class CairoError(RuntimeError):
    def __init__(self, what: str, status: int, timeout: dict | None = None):
        msg = f"{what} failed with evx_status {status}"
        if timeout:
            msg += f" (in-kernel wait timed out: {timeout})"
        super().__init__(msg)
        self.status = status
        self.timeout = timeout  # the first timed-out wait (Context.timeout_info), if one was reported


_lib = None


def lib() -> ctypes.CDLL:
    """Load libcairo_amd.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make` or __graft_entry__.build()"
        )
    L = ctypes.CDLL(LIB_PATH)
    P, I, U, V = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, None
    sig = {
        "cairo_ctx_create": (I, [U, U, U, I, ctypes.POINTER(P)]),
        "cairo_ctx_create_ex": (I, [U, U, U, I, I, ctypes.POINTER(P)]),
        "cairo_ctx_destroy": (I, [P]),
        "cairo_ctx_reset": (I, [P]),
        "cairo_ctx_submit": (I, [P, P, I, U, U, U, ctypes.POINTER(I)]),
        "cairo_ctx_submit_fmt": (I, [P, P, I, I, U, U, U, U, ctypes.POINTER(I)]),
        "cairo_ctx_decode_frame_fmt": (I, [P, P, P, U, I, U, P]),
        "cairo_frame_layout": (I, [I, U, U, U, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(U)]),
        "cairo_frame_fold": (I, [I, I, U, U, U, P, U, P]),
        "cairo_kat_convert": (I, [I, I, U, U, U, P, P, P, P, I]),
        "cairo_kat_convert_color": (I, [I, I, I, I, U, U, U, P, P, P, P, I]),
        "cairo_color_coefs": (I, [I, I, I, P, ctypes.POINTER(ctypes.c_int32)]),
        "cairo_ctx_set_input_color": (I, [P, I, I]),
        "cairo_ctx_set_output_color": (I, [P, I, I]),
        "evx_encoder_set_input_color": (I, [P, I, I]),
        "evx_decoder_set_output_color": (I, [P, I, I]),
        "cairo_stream_submit_fmt": (I, [P, P, I, I, U, U, U, U, ctypes.POINTER(I)]),
        "evx_encoder_set_input_format": (I, [P, I, U]),
        "evx_decoder_set_output_format": (I, [P, I, U]),
        "cairo_source_size": (I, []),
        "cairo_scale_check": (I, [I, U, P, U, U]),
        "cairo_ctx_submit_scaled": (I, [P, P, I, U, P, U, U, U, ctypes.POINTER(I)]),
        "cairo_stream_submit_scaled": (I, [P, P, I, U, P, U, U, U, ctypes.POINTER(I)]),
        "cairo_kat_scale": (I, [I, U, P, P, U, U, P, I]),
        "cairo_tensor_size": (I, []),
        "cairo_tensor_check": (I, [P, P, U, U, ctypes.POINTER(ctypes.c_uint64)]),
        "cairo_tensor_host": (I, [I, P, U, U, P, P]),
        "cairo_kat_tensor": (I, [I, P, U, U, P, ctypes.c_uint64, P, I]),
        "cairo_ctx_submit_tensor": (I, [P, P, P, U, U, U, ctypes.POINTER(I)]),
        "cairo_stream_submit_tensor": (I, [P, P, P, U, U, U, ctypes.POINTER(I)]),
        "cairo_tensor_scale_check": (I, [P, P, P, U, U, ctypes.POINTER(ctypes.c_uint64)]),
        "cairo_ctx_submit_tensor_scaled": (I, [P, P, P, P, U, U, U, ctypes.POINTER(I)]),
        "cairo_stream_submit_tensor_scaled": (I, [P, P, P, P, U, U, U, ctypes.POINTER(I)]),
        "cairo_kat_tensor_scale": (I, [P, P, P, ctypes.c_uint64, U, U, P, I]),
        "cairo_ctx_decode_frame_tensor": (I, [P, P, P, U, P, P]),
        "cairo_ctx_fetch_recon_tensor": (I, [P, I, P, P]),
        "evx_encoder_set_input_tensor": (I, [P, P]),
        "evx_decoder_set_output_tensor": (I, [P, P]),
        "cairo_frame_metrics_size": (I, []),
        "cairo_ctx_set_metrics": (I, [P, I]),
        "cairo_ctx_frame_metrics": (I, [P, I, P]),
        "cairo_ctx_fetch_recon_planes": (I, [P, I, P, P, P]),
        "cairo_ctx_fetch_recon": (I, [P, I, I, U, P]),
        "cairo_stream_frame_metrics": (I, [P, I, P]),
        "cairo_kat_metrics": (I, [U, U, U, P, P, P, P, P, P, P, I]),
        "evx_encoder_set_metrics": (I, [P, I]),
        "evx_encoder_last_metrics": (I, [P, P]),
        "cairo_rate_size": (I, []),
        "cairo_rate_state_size": (I, []),
        "cairo_rate_info_size": (I, []),
        "cairo_rate_estimate": (ctypes.c_int64, [ctypes.c_uint64, ctypes.c_uint64]),
        "cairo_rate_init": (I, [P, P]),
        "cairo_rate_step": (I, [P, P, I, ctypes.c_int64, ctypes.POINTER(U)]),
        "cairo_ctx_set_rate": (I, [P, P]),
        "cairo_ctx_frame_rate": (I, [P, I, P]),
        "cairo_stream_frame_rate": (I, [P, I, P]),
        "cairo_kat_rate_observe": (I, [P, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, P, I, P, I]),
        "cairo_ctx_wait": (I, [P, I, P]),
        "cairo_ctx_release": (I, [P, I]),
        "cairo_ctx_sync": (I, [P]),
        "cairo_ctx_stages": (I, [P]),
        "cairo_ctx_read_planes": (I, [P, I, P, P, P]),
        "cairo_ctx_read_inter": (I, [P, P, P]),
        "cairo_ctx_read_table": (I, [P, P]),
        "cairo_ctx_set_debug": (I, [P, I]),
        "cairo_ctx_read_predeblock": (I, [P, P, P, P]),
        "cairo_ctx_read_stamps": (I, [P, P]),
        "cairo_ctx_engine_variant": (I, [P]),
        "cairo_ctx_set_profiling": (I, [P, I]),
        "cairo_ctx_take_timings": (I, [P, P, ctypes.POINTER(I)]),
        "cairo_ctx_busy_intervals": (I, [P, P, I, ctypes.POINTER(I)]),
        "cairo_ctx_set_workgroups": (I, [P, I]),
        "cairo_ctx_set_batch": (I, [P, I]),
        "cairo_ctx_peer_info": (I, [P, I, P]),
        "cairo_ctx_join_group": (I, [P, I, I, P]),
        "cairo_group_check_queues": (I, [I, I]),
        "cairo_ctx_timeout_info": (I, [P, P, I]),
        "cairo_ctx_read_acct": (I, [P, P, I, I]),
        "cairo_peer_size": (I, []),
        "cairo_ctx_flush": (I, [P]),
        "cairo_ctx_set_helpers": (I, [P, I]),
        "cairo_ctx_max_workgroups": (I, [P]),
        "cairo_default_batch": (I, [U, U]),
        "cairo_task_order": (I, [I, I, P, ctypes.POINTER(I)]),
        "cairo_task_queues": (I, [I, I, I, I, I, P, P, ctypes.POINTER(I)]),
        "cairo_kat_transform": (I, [P, P, P, I, P, P, P, I]),
        "cairo_kat_quant": (I, [P, P, I, P, P, I]),
        "cairo_kat_precode": (I, [U, U, U, I, I, P, P, P, P, P, U, P, P, ctypes.c_uint64, P, U, I]),
        "cairo_serialize_slice": (I, [P, U, U, U, P, P, P, P, U, ctypes.POINTER(U)]),
        "cairo_serialize_feed": (I, [P, ctypes.c_uint64, P, U, ctypes.POINTER(U)]),
        "cairo_precode_slice": (I, [P, U, U, U, P, P, P, P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        "cairo_ctx_set_outputs": (I, [P, I]),
        "cairo_ctx_fetch_coef": (I, [P, I, P]),
        "cairo_unserialize_slice": (I, [P, ctypes.POINTER(U), U, U, U, U, P, P, P, P]),
        "cairo_table_check": (I, [P, U, U, U]),
        "cairo_desc_check": (I, [P, P, U, U, U, U, P]),
        "cairo_stream_create": (I, [P, I, ctypes.POINTER(P)]),
        "cairo_stream_submit": (I, [P, P, I, U, U, U, ctypes.POINTER(I)]),
        "cairo_stream_collect": (I, [P, I, P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
        "cairo_stream_destroy": (I, [P]),
        "cairo_stream_timeline": (I, [P, I, P]),
        "cairo_stream_payload_bits": (I, [P, I, ctypes.POINTER(ctypes.c_uint64)]),
        "cairo_bits_append": (I, [P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), P, ctypes.c_uint64]),
        "evx_encoder_create": (I, [ctypes.POINTER(P)]),
        "evx_encoder_destroy": (I, [P]),
        "evx_encoder_clear": (I, [P]),
        "evx_encoder_insert_intra": (I, [P]),
        "evx_encoder_set_quality": (I, [P, ctypes.c_uint8]),
        "evx_encoder_encode": (I, [P, P, U, U, P]),
        "evx_encoder_set_ring": (I, [P, U]),
        "evx_encoder_peek": (I, [P, I, P]),
        "evx_encoder_set_device": (I, [P, I]),
        "evx_bitstream_create": (P, [U]),
        "evx_bitstream_destroy": (V, [P]),
        "evx_bitstream_data": (P, [P]),
        "evx_bitstream_occupancy": (U, [P]),
        "evx_bitstream_empty": (V, [P]),
        "evx_bitstream_write_bits": (I, [P, P, U]),
        "evx_decoder_create": (I, [ctypes.POINTER(P)]),
        "evx_decoder_destroy": (I, [P]),
        "evx_decoder_clear": (I, [P]),
        "evx_decoder_decode": (I, [P, P, P]),
        "evx_decoder_set_device": (I, [P, I]),
        "cairo_ctx_decode_frame": (I, [P, P, P, U, P]),
        "cairo_make_band4": (V, [P, U, U, U, U]),
        "cairo_version": (ctypes.c_char_p, []),
        "cairo_api_version": (I, []),
        "cairo_device_count": (I, []),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.cairo_api_version() != API_VERSION:
        raise ImportError(f"{LIB_PATH} has C ABI version {L.cairo_api_version()}, these bindings expect "
                          f"{API_VERSION} (include/cairo_amd.h CAIRO_AMD_API_VERSION): rebuild with `make`")
    _lib = L
    return L


def _ck(status: int, what: str) -> None:
    if status != EVX_SUCCESS:
        raise CairoError(what, status)


def _ptr(a: np.ndarray) -> int:
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def _host_frame(rgb, width: int, height: int) -> int:
    """Address of a host RGB888 frame, after checking that it holds a whole
    width x height frame (the native side copies width*height*3 bytes from
    it asynchronously)."""
    if not isinstance(rgb, np.ndarray):
        raise TypeError("host frames are numpy arrays (pass on_device=True for a device address)")
    if rgb.dtype != np.uint8 or rgb.shape != (height, width, 3) or not rgb.flags["C_CONTIGUOUS"]:
        raise ValueError(f"frame must be a C-contiguous uint8 array of shape ({height}, {width}, 3), "
                         f"got {rgb.dtype} {rgb.shape}")
    return rgb.ctypes.data


def frame_layout(fmt: int, w: int, h: int, pitch: int = 0):
    """-> (bytes of a w x h frame of format fmt with row pitch `pitch`, its
    tight pitch); pitch 0 means tight (cairo_frame_layout).  ValueError for an
    unknown format, an odd or zero size, a pitch below the tight one, or an
    odd I420 or P010 pitch.  No device needed."""
    nb, tight = ctypes.c_uint64(), ctypes.c_uint32()
    ok = all(isinstance(x, (int, np.integer)) and 0 <= x < 2 ** 32 for x in (w, h, pitch)) and \
        isinstance(fmt, (int, np.integer)) and -2 ** 31 <= fmt < 2 ** 31
    if not ok or lib().cairo_frame_layout(int(fmt), int(w), int(h), int(pitch), ctypes.byref(nb), ctypes.byref(tight)):
        raise ValueError(f"no frame layout for format {fmt}, {w}x{h}, pitch {pitch}")
    return nb.value, tight.value


def frame_fold(direction: int, fmt: int, frame: np.ndarray, w: int, h: int, pitch: int = 0,
               nv12_pitch: int = 0) -> np.ndarray:
    """The maps between a YUY2, UYVY or P010 frame and the NV12 frame the codec
    takes in its place (cairo_frame_fold), on flat uint8 buffers of
    frame_layout bytes.  direction 0 (fold): frame is of format fmt with row
    pitch `pitch`; -> the NV12 frame with row pitch nv12_pitch.  direction 1
    (unfold): frame is NV12 with row pitch nv12_pitch; -> the frame of format
    fmt.  Pitch padding of the result is 0.  No device needed."""
    if fmt not in (FMT_YUY2, FMT_UYVY, FMT_P010) or direction not in (0, 1):
        raise ValueError(f"frame_fold is defined for FMT_YUY2, FMT_UYVY and FMT_P010, direction 0 or 1; got "
                         f"format {fmt}, direction {direction}")
    fb, _ = frame_layout(fmt, w, h, pitch)
    nb, _ = frame_layout(FMT_NV12, w, h, nv12_pitch)
    want = nb if direction else fb
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.nbytes != want or \
            not frame.flags["C_CONTIGUOUS"]:
        raise ValueError(f"frame must be a C-contiguous uint8 array of {want} bytes")
    out = np.zeros(fb if direction else nb, np.uint8)
    f, n = (out, frame) if direction else (frame, out)
    _ck(lib().cairo_frame_fold(int(direction), int(fmt), int(w), int(h), int(pitch), f.ctypes.data, int(nv12_pitch),
                               n.ctypes.data), "cairo_frame_fold")
    return out


def color_coefs(direction: int, range: int, matrix: int):
    """-> (k, oy): the 3x3 int32 table (2^14 fixed point) and the luma offset
    the kernels use for a colour description (cairo_color_coefs); direction 0:
    described YUV to the codec's full-range BT.601, 1: the reverse.  ValueError
    for unknown values.  No device needed."""
    k, oy = np.zeros(9, np.int32), ctypes.c_int32()
    ok = all(isinstance(x, (int, np.integer)) and -2 ** 31 <= x < 2 ** 31 for x in (direction, range, matrix))
    if not ok or lib().cairo_color_coefs(int(direction), int(range), int(matrix), _ptr(k), ctypes.byref(oy)):
        raise ValueError(f"no colour description (direction {direction}, range {range}, matrix {matrix})")
    return k.reshape(3, 3), oy.value


def split_frame(buf: np.ndarray, fmt: int, w: int, h: int, pitch: int = 0):
    """Plane views of a frame buffer: (y, u, v) for I420, (y, uv) for NV12
    (uv: (h/2, w/2, 2)), the (h, w, 3) pixels for the RGB formats; (y, u, v)
    for YUY2 and UYVY (y: (h, w); u, v: (h, w/2), one sample per pixel pair and
    row); (y, uv) as uint16 words for P010.  Each view covers the image only,
    not the pitch padding."""
    nb, tight = frame_layout(fmt, w, h, pitch)
    p = pitch or tight
    b = np.asarray(buf).reshape(-1)
    if b.dtype != np.uint8 or b.size != nb:
        raise ValueError(f"a format {fmt} frame of {w}x{h}, pitch {p} is {nb} uint8, got {b.dtype} x {b.size}")
    if fmt in (FMT_RGB24, FMT_BGR24):
        return b.reshape(h, p)[:, :3 * w].reshape(h, w, 3) if p == tight else \
            np.lib.stride_tricks.as_strided(b, (h, w, 3), (p, 3, 1))
    if fmt in (FMT_YUY2, FMT_UYVY):
        o = 1 if fmt == FMT_UYVY else 0  # YUY2: Y0 U Y1 V; UYVY: U Y0 V Y1
        at = lambda first, step, count: np.lib.stride_tricks.as_strided(b[first:], (h, count), (p, step))
        return at(o, 2, w), at(1 - o, 4, w // 2), at(3 - o, 4, w // 2)
    if fmt == FMT_P010:
        words = b.view(np.uint16)  # (the pitch is even)
        y = words[:p // 2 * h].reshape(h, p // 2)[:, :w]
        uv = words[p // 2 * h:].reshape(h // 2, p // 2)[:, :w].reshape(h // 2, w // 2, 2)
        return y, uv
    y = b[:p * h].reshape(h, p)[:, :w]
    if fmt == FMT_I420:
        cp, ch = p // 2, h // 2
        u = b[p * h:p * h + cp * ch].reshape(ch, cp)[:, :w // 2]
        v = b[p * h + cp * ch:p * h + 2 * cp * ch].reshape(ch, cp)[:, :w // 2]
        return y, u, v
    uv = b[p * h:].reshape(h // 2, p)[:, :w].reshape(h // 2, w // 2, 2)
    return y, uv


def _host_frame_fmt(frame, fmt: int, width: int, height: int, pitch: int) -> int:
    """Address of a host frame of any format, after checking dtype, contiguity
    and that it holds exactly frame_layout's bytes (the native side copies
    that many from it asynchronously).  (RGB24, 0) is _host_frame."""
    if fmt == FMT_RGB24 and not pitch:
        return _host_frame(frame, width, height)
    nb, _ = frame_layout(fmt, width, height, pitch)
    if not isinstance(frame, np.ndarray):
        raise TypeError("host frames are numpy arrays (pass on_device=True for a device address)")
    if frame.dtype != np.uint8 or frame.nbytes != nb or not frame.flags["C_CONTIGUOUS"]:
        raise ValueError(f"a format {fmt} frame of {width}x{height}, pitch {pitch} must be a C-contiguous uint8 "
                         f"array of {nb} bytes, got {frame.dtype} {frame.shape}")
    return frame.ctypes.data


class _Source(ctypes.Structure):
    """cairo_source (include/cairo_amd.h): the source frame of a scaled submit."""
    _fields_ = [
        ("width", ctypes.c_uint32),
        ("height", ctypes.c_uint32),
        ("crop_x", ctypes.c_uint32),
        ("crop_y", ctypes.c_uint32),
        ("crop_w", ctypes.c_uint32),
        ("crop_h", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32 * 2),
    ]


KAT_SCALE_GUARD = 64  # CAIRO_KAT_SCALE_GUARD


def _source(src_size, crop) -> "_Source":
    vals = tuple(src_size) + (tuple(crop) if crop is not None else (0, 0, 0, 0))
    if len(vals) != 6 or not all(isinstance(x, (int, np.integer)) and 0 <= x < 2 ** 32 for x in vals):
        raise ValueError(f"src_size is (w, h) and crop (x, y, w, h) in 0..2^32-1, got {src_size} {crop}")
    return _Source(*(int(x) for x in vals))


def scale_check(fmt: int, src_size, dst_w: int, dst_h: int, crop=None, pitch: int = 0) -> bool:
    """Whether a source frame of src_size = (w, h), format fmt and row pitch
    `pitch` (0: tight), or its region crop = (x, y, w, h), can be scaled to
    dst_w x dst_h (cairo_scale_check): even sizes and crop values, the crop
    inside the source, a copy or a downscale of at most 8:1 per axis, and
    255 Lx Ly < 2^31.  No device needed."""
    ok = all(isinstance(x, (int, np.integer)) and 0 <= x < 2 ** 32 for x in (pitch, dst_w, dst_h)) and \
        isinstance(fmt, (int, np.integer)) and -2 ** 31 <= fmt < 2 ** 31
    if not ok:
        return False
    try:
        s = _source(src_size, crop)
    except (ValueError, TypeError):
        return False
    return lib().cairo_scale_check(int(fmt), int(pitch), ctypes.byref(s), int(dst_w), int(dst_h)) == EVX_SUCCESS


def kat_scale(frame: np.ndarray, fmt: int, src_size, dst_w: int, dst_h: int, crop=None, pitch: int = 0,
              out: np.ndarray | None = None, device: int = 0) -> np.ndarray:
    """The scaling kernel on a host frame, without a context (cairo_kat_scale):
    -> the tight dst_w x dst_h frame followed by KAT_SCALE_GUARD bytes the
    kernel must leave alone (0xA5 unless `out` brings its own contents).  The
    device copy keeps frame's address modulo 4."""
    sw, sh = src_size
    nb, _ = frame_layout(fmt, sw, sh, pitch)
    db, _ = frame_layout(fmt, dst_w, dst_h)
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.nbytes != nb or \
            not frame.flags["C_CONTIGUOUS"]:
        raise ValueError(f"frame must be a C-contiguous uint8 array of {nb} bytes")
    if out is None:
        out = np.full(db + KAT_SCALE_GUARD, 0xA5, np.uint8)
    elif out.dtype != np.uint8 or out.nbytes != db + KAT_SCALE_GUARD or not out.flags["C_CONTIGUOUS"]:
        raise ValueError(f"out must be a C-contiguous uint8 array of {db + KAT_SCALE_GUARD} bytes")
    s = _source(src_size, crop)
    _ck(lib().cairo_kat_scale(fmt, pitch, ctypes.byref(s), frame.ctypes.data, dst_w, dst_h, _ptr(out), device),
        "cairo_kat_scale")
    return out


def _scaled_source_ptr(frame, on_device: bool, fmt: int, src_size, pitch: int) -> int:
    """Address of the source of a scaled submit.  Only device sources are
    scaled; a host array is still checked and handed over, so that the refusal
    is the library's (EVX_ERROR_INVALID_ARGS)."""
    if on_device:
        return frame
    nb, _ = frame_layout(fmt, src_size[0], src_size[1], pitch)
    if not isinstance(frame, np.ndarray) or frame.dtype != np.uint8 or frame.nbytes != nb or \
            not frame.flags["C_CONTIGUOUS"]:
        raise ValueError(f"a format {fmt} source of {src_size[0]}x{src_size[1]}, pitch {pitch} is a C-contiguous uint8 "
                         f"array of {nb} bytes")
    return frame.ctypes.data


# Tensor frames (include/cairo_amd.h cairo_tensor, CAIRO_DT_*)
DT_U8, DT_F16, DT_BF16, DT_F32 = range(4)
DT_SIZE = {DT_U8: 1, DT_F16: 2, DT_BF16: 2, DT_F32: 4}
KAT_TENSOR_GUARD = 64  # CAIRO_KAT_TENSOR_GUARD
_DT_NAMES = {"uint8": DT_U8, "float16": DT_F16, "half": DT_F16, "bfloat16": DT_BF16, "float32": DT_F32,
             "float": DT_F32}


class _Tensor(ctypes.Structure):
    """cairo_tensor (include/cairo_amd.h)."""
    _fields_ = [
        ("dtype", ctypes.c_uint32),
        ("reserved0", ctypes.c_uint32),
        ("stride", ctypes.c_int64 * 3),
        ("mul", ctypes.c_float * 3),
        ("add", ctypes.c_float * 3),
        ("reserved", ctypes.c_uint32 * 2),
    ]


@dataclass
class TensorDesc:
    """A tensor frame: the address of element (0, 0, 0), its cairo_tensor (c,
    a ctypes structure), the frame size where the shape gave one, and the
    object that owns the memory."""
    ptr: int
    c: _Tensor
    width: int | None = None
    height: int | None = None
    owner: object = None


def _three(v, what: str):
    a = np.asarray(v, np.float64).reshape(-1)
    if a.size == 1:
        a = np.repeat(a, 3)
    if a.size != 3:
        raise ValueError(f"{what} is a number or three numbers (R, G, B)")
    return a


def tensor_desc(t, mul=None, add=None, value_range=(0.0, 1.0), output: bool = False) -> TensorDesc:
    """Describe a tensor frame.  t is any object with data_ptr(), dtype, shape,
    stride() and device (a torch tensor; this package does not import torch),
    of shape (3, H, W) or (H, W, C >= 3) with positive strides: a frame of an
    NCHW batch, a channels_last view, a crop and the RGB channels of an RGBA
    tensor all qualify.  A numpy array is taken the same way (host tensors, for
    tensor_host and kat_tensor), and so is a plain (ptr, dtype, strides) with
    dtype a DT_* value or a name and strides = (channel, row, column) in
    elements.  The dtype is read from its name: uint8, float16, bfloat16 or
    float32.

    The map (include/cairo_amd.h): input s = clamp(rint(fmaf(x, mul, add))),
    output x = fmaf(s, mul, add).  mul / add: numbers or per-channel triples;
    left out, they come from value_range = (lo, hi), the values 0 and 255 stand
    for: for an input (output=False) mul = 255 / (hi - lo), add = -lo * mul; for
    an output mul = (hi - lo) / 255, add = lo -- computed in double, rounded
    once to float32."""
    if isinstance(t, TensorDesc):
        return t
    width = height = None
    if isinstance(t, tuple):
        ptr, dt, strides = t
        owner = None
    else:
        shape = tuple(int(x) for x in t.shape)
        if isinstance(t, np.ndarray):
            ptr, st = t.ctypes.data, tuple(s // t.itemsize for s in t.strides)
        else:
            ptr, st = int(t.data_ptr()), tuple(int(s) for s in t.stride())
        dt = str(t.dtype)
        if len(shape) != 3:
            raise ValueError(f"a tensor frame has shape (3, H, W) or (H, W, C >= 3), got {shape}")
        if shape[0] == 3:
            strides, height, width = (st[0], st[1], st[2]), shape[1], shape[2]
        elif shape[2] >= 3:
            strides, height, width = (st[2], st[0], st[1]), shape[0], shape[1]
        else:
            raise ValueError(f"a tensor frame has shape (3, H, W) or (H, W, C >= 3), got {shape}")
        owner = t
    if isinstance(dt, str):
        name = dt.rsplit(".", 1)[-1]
        if name not in _DT_NAMES:
            raise ValueError(f"tensor frames are uint8, float16, bfloat16 or float32, got {dt}")
        dt = _DT_NAMES[name]
    if mul is None and add is None:
        lo, hi = float(value_range[0]), float(value_range[1])
        if not hi > lo:
            raise ValueError(f"value_range is (lo, hi) with hi > lo, got {value_range}")
        if output:
            mul, add = (hi - lo) / 255.0, lo
        else:
            mul = 255.0 / (hi - lo)
            add = -lo * mul
    c = _Tensor()
    c.dtype = int(dt)
    c.stride[:] = [int(s) for s in strides]
    c.mul[:] = [float(np.float32(x)) for x in _three(1.0 if mul is None else mul, "mul")]
    c.add[:] = [float(np.float32(x)) for x in _three(0.0 if add is None else add, "add")]
    return TensorDesc(int(ptr), c, width, height, owner)


def tensor_check(desc: TensorDesc, w: int, h: int, ptr: int | None = None):
    """-> the span in bytes of a w x h tensor frame, or None when the
    descriptor is not valid for it (cairo_tensor_check; ptr: another base
    address, of which only the alignment counts).  No device needed."""
    span = ctypes.c_uint64()
    base = desc.ptr if ptr is None else ptr
    if lib().cairo_tensor_check(ctypes.byref(desc.c), base, w, h, ctypes.byref(span)):
        return None
    return span.value


def tensor_host(direction: int, desc: TensorDesc, w: int, h: int, rgb: np.ndarray) -> None:
    """The tensor map as host loops (cairo_tensor_host) between the host
    tensor at desc.ptr and the tight RGB24 frame rgb (3 * w * h uint8):
    direction 0 writes rgb, 1 writes the tensor's covered elements."""
    if not isinstance(rgb, np.ndarray) or rgb.dtype != np.uint8 or rgb.size != 3 * w * h or \
            not rgb.flags["C_CONTIGUOUS"]:
        raise ValueError(f"rgb must be a C-contiguous uint8 array of {3 * w * h} bytes")
    _ck(lib().cairo_tensor_host(direction, ctypes.byref(desc.c), w, h, desc.ptr, _ptr(rgb)), "cairo_tensor_host")


def kat_tensor(direction: int, desc: TensorDesc, w: int, h: int, nbytes: int, rgb: np.ndarray,
               device: int = 0) -> None:
    """The tensor kernels on host buffers, without a context
    (cairo_kat_tensor): the nbytes of host memory at desc.ptr (the span and
    any guard) and rgb (3 * w * h + KAT_TENSOR_GUARD uint8) are uploaded, the
    kernel of the direction runs, and both are read back in place.  The device
    copy keeps desc.ptr modulo 16."""
    if not isinstance(rgb, np.ndarray) or rgb.dtype != np.uint8 or rgb.size != 3 * w * h + KAT_TENSOR_GUARD or \
            not rgb.flags["C_CONTIGUOUS"]:
        raise ValueError(f"rgb must be a C-contiguous uint8 array of {3 * w * h + KAT_TENSOR_GUARD} bytes")
    _ck(lib().cairo_kat_tensor(direction, ctypes.byref(desc.c), w, h, desc.ptr, nbytes, _ptr(rgb), device),
        "cairo_kat_tensor")


def _tensor_source(d: TensorDesc, src_size, crop) -> "_Source":
    """The cairo_source of a scaled tensor submit: the source size is the
    tensor's own (W, H) where its shape gave one, else src_size."""
    own = (d.width, d.height) if d.width is not None else None
    if src_size is None:
        if own is None:
            raise ValueError("a tensor given as (ptr, dtype, strides) or as a shapeless TensorDesc is scaled with "
                             "src_size = (w, h)")
        src_size = own
    s = _source(src_size, crop)
    if own is not None and (s.width, s.height) != own:
        raise ValueError(f"src_size {tuple(src_size)} contradicts the tensor's shape, a {own[0]}x{own[1]} frame")
    return s


def tensor_scale_check(desc: TensorDesc, src_size, dst_w: int, dst_h: int, crop=None, ptr: int | None = None):
    """-> the span in bytes of the source tensor of a scaled tensor submit, or
    None when it is refused (cairo_tensor_scale_check): desc must be valid for
    a frame of src_size = (w, h) (tensor_check), and that size, or its region
    crop = (x, y, w, h), must scale to dst_w x dst_h as an RGB24 frame does
    (scale_check).  src_size None: the size desc got from a shape.  ptr: another
    base address, of which only the alignment counts.  No device needed."""
    if not all(isinstance(x, (int, np.integer)) and 0 <= x < 2 ** 32 for x in (dst_w, dst_h)):
        return None
    try:
        s = _tensor_source(desc, src_size, crop)
    except (ValueError, TypeError):
        return None
    span = ctypes.c_uint64()
    base = desc.ptr if ptr is None else ptr
    if lib().cairo_tensor_scale_check(ctypes.byref(desc.c), base, ctypes.byref(s), int(dst_w), int(dst_h),
                                      ctypes.byref(span)):
        return None
    return span.value


def kat_tensor_scale(desc: TensorDesc, src_size, nbytes: int, dst_w: int, dst_h: int, rgb: np.ndarray, crop=None,
                     device: int = 0) -> None:
    """The scaled tensor submit's kernel on host buffers, without a context
    (cairo_kat_tensor_scale), with kat_tensor's conventions: the nbytes of
    host memory at desc.ptr (a tensor of src_size, and any guard) and rgb
    (3 * dst_w * dst_h + KAT_TENSOR_GUARD uint8) are uploaded, the kernel
    runs, and both are read back in place."""
    if not isinstance(rgb, np.ndarray) or rgb.dtype != np.uint8 or rgb.size != 3 * dst_w * dst_h + KAT_TENSOR_GUARD or \
            not rgb.flags["C_CONTIGUOUS"]:
        raise ValueError(f"rgb must be a C-contiguous uint8 array of {3 * dst_w * dst_h + KAT_TENSOR_GUARD} bytes")
    s = _tensor_source(desc, src_size, crop)
    _ck(lib().cairo_kat_tensor_scale(ctypes.byref(desc.c), ctypes.byref(s), desc.ptr, nbytes, dst_w, dst_h, _ptr(rgb),
                                     device), "cairo_kat_tensor_scale")


def _frame_tensor(t, width: int, height: int, output: bool, kw: dict) -> TensorDesc:
    """The descriptor of a tensor handed to a context of width x height."""
    d = tensor_desc(t, output=output, **kw)
    if d.width is not None and (d.width, d.height) != (width, height):
        raise ValueError(f"the tensor is a {d.width}x{d.height} frame, the context's are {width}x{height}")
    return d


def _sync_producer(t) -> None:
    """Order a torch tensor's producer before a submit: synchronise the
    current stream of its device.  Only when the caller already imported
    torch; the C ABI leaves the ordering to the caller."""
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and getattr(t, "is_cuda", False):
        torch.cuda.current_stream(t.device).synchronize()


def make_band4(w: int, h: int, t: int, seed: int = 1234) -> np.ndarray:
    """band4 synthetic RGB888 frame, shape (h, w, 3)."""
    out = np.empty((h, w, 3), np.uint8)
    lib().cairo_make_band4(_ptr(out), w, h, t, seed)
    return out


class _FrameResult(ctypes.Structure):
    _fields_ = [
        ("block_table", ctypes.c_void_p),
        ("coef_y", ctypes.c_void_p),
        ("coef_u", ctypes.c_void_p),
        ("coef_v", ctypes.c_void_p),
        ("wa", ctypes.c_uint32),
        ("ha", ctypes.c_uint32),
        ("wmb", ctypes.c_uint32),
        ("hmb", ctypes.c_uint32),
        ("index", ctypes.c_uint32),
        ("type", ctypes.c_uint32),
        ("quality", ctypes.c_uint32),
        ("feed", ctypes.c_void_p),
        ("feed_bits", ctypes.c_uint64),
        ("feed_status", ctypes.c_int32),
    ]


class _FrameMetrics(ctypes.Structure):
    """cairo_frame_metrics (include/cairo_amd.h)."""
    _fields_ = [
        ("flags", ctypes.c_uint32),
        ("width", ctypes.c_uint32),
        ("height", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
        ("sse", ctypes.c_uint64 * 3),
        ("ssim_sum", ctypes.c_double * 3),
        ("ssim_windows", ctypes.c_uint64 * 3),
        ("samples", ctypes.c_uint64 * 3),
    ]


def psnr(sse: int, samples: int) -> float:
    """10 log10(255^2 * samples / sse); inf at sse 0."""
    return float("inf") if sse == 0 else 10.0 * float(np.log10(255.0 ** 2 * samples / sse))


def _metrics_dict(m: "_FrameMetrics") -> dict:
    """The raw fields of a cairo_frame_metrics plus psnr_y/u/v/all and
    ssim_y/u/v (None for a metric that was not computed, or has no window)."""
    d = {"flags": int(m.flags), "width": int(m.width), "height": int(m.height), "sse": [int(x) for x in m.sse],
         "ssim_sum": [float(x) for x in m.ssim_sum], "ssim_windows": [int(x) for x in m.ssim_windows],
         "samples": [int(x) for x in m.samples]}
    has_sse, has_ssim = bool(m.flags & METRIC_SSE), bool(m.flags & METRIC_SSIM)
    for k, n in enumerate("yuv"):
        d[f"psnr_{n}"] = psnr(d["sse"][k], d["samples"][k]) if has_sse else None
        d[f"ssim_{n}"] = d["ssim_sum"][k] / d["ssim_windows"][k] if has_ssim and d["ssim_windows"][k] else None
    d["psnr_all"] = psnr(sum(d["sse"]), sum(d["samples"])) if has_sse else None
    return d


def kat_metrics(a, b, w: int, h: int, device: int = 0) -> dict:
    """The metrics kernels on host planes, without a context (cairo_kat_metrics):
    a and b are (y, u, v) int16 planes whose rows hold at least w (chroma: w / 2)
    elements; the luma row length is the pitch, the chroma planes' half of it."""
    planes = [np.ascontiguousarray(p, dtype=np.int16) for p in (*a, *b)]
    pitch = planes[0].shape[1]
    for y, u, v in (planes[:3], planes[3:]):
        if y.shape != (h, pitch) or u.shape != (h // 2, pitch // 2) or v.shape != u.shape:
            raise ValueError(f"planes must be ({h}, {pitch}) and ({h // 2}, {pitch // 2}), got {y.shape} {u.shape} {v.shape}")
    m = _FrameMetrics()
    _ck(lib().cairo_kat_metrics(w, h, pitch, *(_ptr(p) for p in planes), ctypes.byref(m), device), "cairo_kat_metrics")
    return _metrics_dict(m)


class _Rate(ctypes.Structure):
    """cairo_rate (include/cairo_amd.h)."""
    _fields_ = [("target_bits", ctypes.c_uint32), ("q0", ctypes.c_uint32), ("qmin", ctypes.c_uint32),
                ("qmax", ctypes.c_uint32), ("window", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class _RateState(ctypes.Structure):
    """cairo_rate_state."""
    _fields_ = [("debt", ctypes.c_int64), ("p_aim", ctypes.c_int64), ("o_aim", ctypes.c_int64),
                ("p_n", ctypes.c_int32), ("p_q", ctypes.c_int32), ("o_n", ctypes.c_int32), ("o_q", ctypes.c_int32),
                ("launches", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class _RateInfo(ctypes.Structure):
    """cairo_rate_info."""
    _fields_ = [("quality", ctypes.c_uint32), ("overflow", ctypes.c_uint32), ("feed_bits", ctypes.c_uint64),
                ("ones", ctypes.c_uint64), ("est_bits", ctypes.c_int64), ("aim", ctypes.c_int64),
                ("debt", ctypes.c_int64)]


RATE_FRAME_RECORD_BITS = 80  # a frame counts as its estimate plus its 10-byte frame record


def _rate_dict(r: "_RateInfo") -> dict:
    return {k: int(getattr(r, k)) for k, _ in _RateInfo._fields_}


def rate_estimate(nbits: int, zeros: int) -> int:
    """E(N, z): the integer estimate of the arithmetic coder's output, in bits,
    for a feed of nbits bits of which zeros are 0 (cairo_rate_estimate)."""
    e = lib().cairo_rate_estimate(nbits, zeros)
    if e < 0:
        raise ValueError(f"rate_estimate({nbits}, {zeros}): nbits must be below 2**32 and zeros at most nbits")
    return int(e)


class RateModel:
    """The rate controller's law on the host (cairo_rate_init / cairo_rate_step):
    what a Context with set_rate runs on the device.  step(n_new, obs_sum) ->
    the quality of the next launch's n_new frames; obs_sum is the summed bits
    (estimate + 80 each) of the frames of the launch before the last, read only
    once two launches exist.  aim and debt are the state's after the step."""

    def __init__(self, target_bits: int, q0: int = 8, qmin: int = 1, qmax: int = 31, window: int = 32):
        self.cfg = _Rate(target_bits, q0, qmin, qmax, window)
        self.state = _RateState()
        _ck(lib().cairo_rate_init(ctypes.byref(self.state), ctypes.byref(self.cfg)), "cairo_rate_init")

    def step(self, n_new: int, obs_sum: int = 0) -> int:
        q = ctypes.c_uint32()
        _ck(lib().cairo_rate_step(ctypes.byref(self.state), ctypes.byref(self.cfg), n_new, obs_sum, ctypes.byref(q)),
            "cairo_rate_step")
        return q.value

    @property
    def aim(self) -> int:
        return int(self.state.p_aim)

    @property
    def debt(self) -> int:
        return int(self.state.debt)


def kat_rate_observe(words: np.ndarray, nbits, base: int = 0, stride: int | None = None, device: int = 0):
    """The observing kernels on a host buffer, without a context
    (cairo_kat_rate_observe): words (uint32) is uploaded whole, frame j's feed is
    the nbits[j] bits from word base + j * stride on.  -> a list of dicts
    (feed_bits, ones, est_bits, ...)."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    nb = np.ascontiguousarray(nbits, dtype=np.uint64)
    if stride is None:
        stride = int((int(nb.max()) + 31) // 32) if nb.size else 0
    out = (_RateInfo * nb.size)()
    _ck(lib().cairo_kat_rate_observe(_ptr(w), w.size, base, stride, _ptr(nb), nb.size, out, device),
        "cairo_kat_rate_observe")
    return [_rate_dict(r) for r in out]


@dataclass
class FrameOutputs:
    """Host copies of one frame's outputs (block table + output_cache)."""

    table: np.ndarray  # (mbs,) BLOCK_DESC
    coef_y: np.ndarray | None  # None without OUT_COEF (Context.fetch_coef)
    coef_u: np.ndarray | None
    coef_v: np.ndarray | None
    feed: np.ndarray | None = None  # OUT_FEED: the GPU precode's feed words (uint32, LSB-first)
    feed_bits: int = 0
    feed_status: int = 0  # FEED_NONE / FEED_VALID / FEED_OVERFLOW
    quality: int = 0  # the quality the frame was coded with (with set_rate: the controller's choice)


def _view(addr: int, dtype, count: int) -> np.ndarray:
    buf = (ctypes.c_char * (count * np.dtype(dtype).itemsize)).from_address(addr)
    return np.frombuffer(buf, dtype=dtype, count=count)


def _submit(prefix: str, handle, width: int, height: int, keep: dict, rgb, index: int, inter: bool, quality: int,
            on_device: bool, fmt: int, pitch: int, src_size, crop) -> int:
    """Context.submit and Stream.submit: prefix is "cairo_ctx" or
    "cairo_stream", handle its object, width x height the context's frame size,
    keep the caller's ticket -> host frame map.  Tight RGB24 takes the plain
    call, which does not range-check a device frame."""
    L = lib()
    t = ctypes.c_int()
    if src_size is not None or crop is not None:
        if src_size is None:
            raise ValueError("crop needs src_size")
        s = _source(src_size, crop)
        ptr = _scaled_source_ptr(rgb, on_device, fmt, src_size, pitch)
        _ck(getattr(L, prefix + "_submit_scaled")(handle, ptr, fmt, pitch, ctypes.byref(s), index, int(inter), quality,
                                                  ctypes.byref(t)), prefix + "_submit_scaled")
        return t.value
    ptr = rgb if on_device else _host_frame_fmt(rgb, fmt, width, height, pitch)
    if fmt == FMT_RGB24 and not pitch:
        _ck(getattr(L, prefix + "_submit")(handle, ptr, int(on_device), index, int(inter), quality, ctypes.byref(t)),
            prefix + "_submit")
    else:
        _ck(getattr(L, prefix + "_submit_fmt")(handle, ptr, int(on_device), fmt, pitch, index, int(inter), quality,
                                               ctypes.byref(t)), prefix + "_submit_fmt")
    if not on_device:  # the H2D copy is asynchronous: keep the host frame alive
        keep[t.value] = rgb
    return t.value


def _submit_tensor(prefix: str, handle, width: int, height: int, keep: dict, t, index: int, inter: bool, quality: int,
                   sync: bool, desc: dict, scaled: bool = False, crop=None, src_size=None) -> int:
    """Context.submit_tensor and Stream.submit_tensor, as _submit.  scaled or
    a crop: the tensor is the source of a scaled tensor submit."""
    tk = ctypes.c_int()
    if scaled or crop is not None:
        d = tensor_desc(t, output=False, **desc)
        s = _tensor_source(d, src_size, crop)
        if sync:
            _sync_producer(d.owner)
        _ck(getattr(lib(), prefix + "_submit_tensor_scaled")(handle, d.ptr, ctypes.byref(d.c), ctypes.byref(s), index,
                                                             int(inter), quality, ctypes.byref(tk)),
            prefix + "_submit_tensor_scaled")
    else:
        if src_size is not None:
            raise ValueError("src_size belongs to a scaled tensor submit: pass scaled=True or a crop")
        d = _frame_tensor(t, width, height, False, desc)
        if sync:
            _sync_producer(d.owner)
        _ck(getattr(lib(), prefix + "_submit_tensor")(handle, d.ptr, ctypes.byref(d.c), index, int(inter), quality,
                                                      ctypes.byref(tk)), prefix + "_submit_tensor")
    keep[tk.value] = d
    return tk.value


class Context:
    """The encode-path backend (``cairo_ctx_*``): one encoder's device state."""

    def __init__(self, width: int, height: int, ring: int = 4, device: int = 0, stages: int = 96):
        self.L = lib()
        self.width, self.height, self.ring, self.device = width, height, ring, device
        self.wa, self.ha = (width + 15) & ~15, (height + 15) & ~15
        self.wmb, self.hmb = self.wa // 16, self.ha // 16
        p = ctypes.c_void_p()
        _ck(self.L.cairo_ctx_create_ex(width, height, ring, device, stages, ctypes.byref(p)), "cairo_ctx_create")
        self.h = p
        self._keep = {}  # ticket -> host RGB frame still being copied

    def close(self) -> None:
        if self.h:
            self.L.cairo_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stages(self) -> int:
        return int(self.L.cairo_ctx_stages(self.h))

    def submit(self, rgb, index: int, inter: bool, quality: int, on_device: bool = False,
               fmt: int = FMT_RGB24, pitch: int = 0, src_size=None, crop=None) -> int:
        """fmt / pitch: the frame's layout (FMT_*, row pitch in bytes, 0:
        tight); the defaults are today's tight RGB888 through cairo_ctx_submit.
        src_size = (w, h): the frame is a larger device frame of that size (and
        pitch), scaled to the context's size on the GPU before it is encoded
        (cairo_ctx_submit_scaled, see scale_check); crop = (x, y, w, h) scales a
        region of it."""
        return _submit("cairo_ctx", self.h, self.width, self.height, self._keep, rgb, index, inter, quality, on_device,
                       fmt, pitch, src_size, crop)

    def submit_tensor(self, t, index: int, inter: bool, quality: int, sync: bool = True, scaled: bool = False,
                      crop=None, src_size=None, **desc) -> int:
        """Submit a tensor frame in device memory (cairo_ctx_submit_tensor): t
        and the keywords mul, add, value_range are tensor_desc's (or t is a
        TensorDesc).  Produces the bits of submitting the RGB24 frame the input
        map gives.  t is kept alive until the ticket's wait and must not
        change before it.  sync: synchronise the producer's current stream
        first when torch is already imported (the C ABI leaves that ordering to
        the caller).

        scaled=True or crop = (x, y, w, h): t is a larger tensor, which (or
        whose region) is mapped to samples and scaled to the context's size on
        the GPU in one pass (cairo_ctx_submit_tensor_scaled, see
        tensor_scale_check): the bits of Context.submit(..., src_size=...) of
        the packed RGB24 frame.  The source size is t's own; src_size = (w, h)
        gives it for a (ptr, dtype, strides) or a shapeless TensorDesc."""
        return _submit_tensor("cairo_ctx", self.h, self.width, self.height, self._keep, t, index, inter, quality, sync,
                              desc, scaled, crop, src_size)

    def wait(self, ticket: int, copy: bool = True) -> FrameOutputs:
        r = _FrameResult()
        st = self.L.cairo_ctx_wait(self.h, ticket, ctypes.byref(r))
        if st != EVX_SUCCESS:
            raise CairoError("cairo_ctx_wait", st, self.timeout_info() if st == EVX_ERROR_HARDWAREFAIL else None)
        self._keep.pop(ticket, None)
        return self._outputs(r, copy)

    ACCT_FIELDS = ("coder_tasks", "coder_total", "coder_group_wait", "coder_window", "coder_search", "coder_inter",
                   "coder_dequeue", "coder_mbs", "helper_tasks", "helper_total", "helper_wait", "helper_deblock",
                   "helper_search", "helper_catchup", "helper_dequeue", "helper_chunks",
                   "win_bytes", "win_spec_unused_bytes", "zero_mv_bytes", "gran_poll_bytes", "rec_poll_bytes",
                   "win_stages", "searched_tasks", "inter_tasks", "coder_xform", "coder_publish", "coder_drain",
                   "coder_vm0", "coder_records", "coder_prebarrier", "coder_store_tail",
                   "search_eval", "search_barrier", "search_select", "subpel_eval", "subpel_barrier",
                   "subpel_select", "db_inputs", "db_filter", "db_write",
                   "search_passes", "search_mbs_2pass", "search_mbs_3pass", "search_mbs_4pass",
                   "coder_xform_copy", "coder_copy_mbs", "coder_xform_coded", "coder_coded_mbs",
                   "helper_carry", "carry_bytes",
                   "coder_prologue_fresh", "coder_prologue_records", "helper_group_start",
                   "start_older_searched", "start_ref1_searched", "start_older_idle", "start_ref1_idle",
                   "older_searched", "older_idle", "ref1_idle",
                   "flag_set", "fallback_polls", "fallback_full", "lvl2_runs", "idle_groups", "idle_group_time")

    def read_acct(self, reset: bool = False) -> dict:
        """Engine time accounting (set_debug(32) on a CAIRO_ACCT=1 build): 10 ns
        ticks per role and phase summed over all tasks (kernels.h Acct)."""
        w = np.zeros(len(self.ACCT_FIELDS), np.uint64)
        _ck(self.L.cairo_ctx_read_acct(self.h, _ptr(w), len(w), int(reset)), "cairo_ctx_read_acct")
        return {k: int(w[i]) for i, k in enumerate(self.ACCT_FIELDS)}

    def timeout_info(self) -> dict | None:
        """The in-kernel wait that timed out first, as last reported
        (cairo_ctx_timeout_info): kind (WAIT_KINDS name), the waiting frame's
        epoch, index and MB row, the group member, what it needed, what it
        waited on, the last value seen; None if none since create / reset."""
        w = np.zeros(16, np.int32)
        _ck(self.L.cairo_ctx_timeout_info(self.h, _ptr(w), 16), "cairo_ctx_timeout_info")
        if not w[0]:
            return None
        d = {k: int(w[i]) for i, k in enumerate(TIMEOUT_FIELDS)}
        d["kind"] = WAIT_KINDS.get(d["kind"], str(d["kind"]))
        d["seen"] = (d.pop("seen_hi") & 0xFFFFFFFF) << 32 | (d.pop("seen_lo") & 0xFFFFFFFF)
        return d

    def _outputs(self, r, copy: bool) -> FrameOutputs:
        ny, nc = r.wa * r.ha, (r.wa // 2) * (r.ha // 2)
        mbs = r.wmb * r.hmb
        has_coef = bool(r.coef_y)
        feed = _view(r.feed, np.uint32, (r.feed_bits + 31) // 32) if r.feed_status == FEED_VALID else None
        out = FrameOutputs(
            _view(r.block_table, BLOCK_DESC, mbs),
            _view(r.coef_y, np.int16, ny).reshape(r.ha, r.wa) if has_coef else None,
            _view(r.coef_u, np.int16, nc).reshape(r.ha // 2, r.wa // 2) if has_coef else None,
            _view(r.coef_v, np.int16, nc).reshape(r.ha // 2, r.wa // 2) if has_coef else None,
            feed, int(r.feed_bits), int(r.feed_status), int(r.quality),
        )
        if copy:
            cp = lambda a: None if a is None else a.copy()  # noqa: E731
            out = FrameOutputs(cp(out.table), cp(out.coef_y), cp(out.coef_u), cp(out.coef_v), cp(out.feed),
                               out.feed_bits, out.feed_status, out.quality)
        return out

    def set_outputs(self, outputs: int) -> None:
        """OUT_COEF and/or OUT_FEED for frames submitted from now on."""
        _ck(self.L.cairo_ctx_set_outputs(self.h, outputs), "cairo_ctx_set_outputs")

    def fetch_coef(self, ticket: int):
        """(y, u, v) output_cache planes of a waited, unreleased frame (copies)."""
        r = _FrameResult()
        _ck(self.L.cairo_ctx_fetch_coef(self.h, ticket, ctypes.byref(r)), "cairo_ctx_fetch_coef")
        ny, nc = self.wa * self.ha, (self.wa // 2) * (self.ha // 2)
        return (_view(r.coef_y, np.int16, ny).reshape(self.ha, self.wa).copy(),
                _view(r.coef_u, np.int16, nc).reshape(self.ha // 2, self.wa // 2).copy(),
                _view(r.coef_v, np.int16, nc).reshape(self.ha // 2, self.wa // 2).copy())

    def set_metrics(self, sse: bool = True, ssim: bool = True, keep_recon: bool = False, flags: int | None = None) -> None:
        """Per-frame metrics and/or kept reconstructions for frames submitted
        from now on (cairo_ctx_set_metrics; no frame may be in flight).  All
        False turns them off and frees the kept plane sets.  flags: the raw
        METRIC_* / KEEP_RECON bits instead."""
        if flags is None:
            flags = (METRIC_SSE if sse else 0) | (METRIC_SSIM if ssim else 0) | (KEEP_RECON if keep_recon else 0)
        _ck(self.L.cairo_ctx_set_metrics(self.h, flags), "cairo_ctx_set_metrics")

    def set_rate(self, target_bits: int | None, q0: int = 8, qmin: int = 1, qmax: int = 31, window: int = 32) -> None:
        """Target bitrate (cairo_ctx_set_rate): from now on the context chooses
        one quality per launch on the device so that frames average target_bits
        (payload plus the 10-byte frame record); the quality of a submit is
        ignored, FrameOutputs.quality and frame_rate report the choice.
        window: frames over which a debt is paid back.  None turns it off.  No
        frame may be in flight; the outputs must include OUT_FEED."""
        if target_bits is None:
            _ck(self.L.cairo_ctx_set_rate(self.h, None), "cairo_ctx_set_rate")
            return
        cfg = _Rate(target_bits, q0, qmin, qmax, window)
        _ck(self.L.cairo_ctx_set_rate(self.h, ctypes.byref(cfg)), "cairo_ctx_set_rate")

    def frame_rate(self, ticket: int) -> dict:
        """What the rate controller saw and chose for a waited, unreleased
        frame: quality, overflow, feed_bits, ones, est_bits, aim, debt."""
        r = _RateInfo()
        _ck(self.L.cairo_ctx_frame_rate(self.h, ticket, ctypes.byref(r)), "cairo_ctx_frame_rate")
        return _rate_dict(r)

    def set_input_color(self, range: int, matrix: int) -> None:
        """The colour description (RANGE_*, MATRIX_*) of the I420 / NV12 frames
        (and of the NV12 frame a YUY2 / UYVY / P010 frame folds to) submitted
        from now on, also through a Stream; recorded per frame at submit.  RGB
        frames ignore it.  Survives reset()."""
        _ck(self.L.cairo_ctx_set_input_color(self.h, range, matrix), "cairo_ctx_set_input_color")

    def set_output_color(self, range: int, matrix: int) -> None:
        """The colour description fetch_recon and cairo_ctx_decode_frame_fmt
        write I420 / NV12 frames in from now on (YUY2 / UYVY / P010 frames are
        the unfold of that NV12 frame)."""
        _ck(self.L.cairo_ctx_set_output_color(self.h, range, matrix), "cairo_ctx_set_output_color")

    def frame_metrics(self, ticket: int) -> dict:
        """Metrics of a waited, unreleased frame: the raw cairo_frame_metrics
        fields plus psnr_y/u/v/all (dB, inf at SSE 0) and ssim_y/u/v."""
        m = _FrameMetrics()
        _ck(self.L.cairo_ctx_frame_metrics(self.h, ticket, ctypes.byref(m)), "cairo_ctx_frame_metrics")
        return _metrics_dict(m)

    def fetch_recon_planes(self, ticket: int):
        """(y, u, v) kept deblocked reconstruction of a waited, unreleased frame,
        aligned int16 planes as read_planes returns them."""
        y = np.empty((self.ha, self.wa), np.int16)
        u = np.empty((self.ha // 2, self.wa // 2), np.int16)
        v = np.empty_like(u)
        _ck(self.L.cairo_ctx_fetch_recon_planes(self.h, ticket, _ptr(y), _ptr(u), _ptr(v)),
            "cairo_ctx_fetch_recon_planes")
        return y, u, v

    def fetch_recon(self, ticket: int, fmt: int, pitch: int = 0, out: np.ndarray | None = None) -> np.ndarray:
        """The same frame as a flat uint8 buffer of frame_layout(fmt, pitch)
        bytes (split_frame gives its planes): what the decoder shows.  out: a
        buffer to write into (its pitch padding keeps its bytes)."""
        nb, _ = frame_layout(fmt, self.width, self.height, pitch)
        if out is None:
            out = np.zeros(nb, np.uint8)
        elif not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.nbytes != nb or \
                not out.flags["C_CONTIGUOUS"]:
            raise ValueError(f"out must be a C-contiguous uint8 array of {nb} bytes")
        _ck(self.L.cairo_ctx_fetch_recon(self.h, ticket, fmt, pitch, _ptr(out)), "cairo_ctx_fetch_recon")
        return out

    def fetch_recon_tensor(self, ticket: int, t, **desc):
        """The same frame as RGB through the output map into the device tensor
        t (cairo_ctx_fetch_recon_tensor; t and the keywords as tensor_desc's
        with output=True) -> t.  Synchronous; no copy to the host."""
        d = _frame_tensor(t, self.width, self.height, True, desc)
        _ck(self.L.cairo_ctx_fetch_recon_tensor(self.h, ticket, d.ptr, ctypes.byref(d.c)),
            "cairo_ctx_fetch_recon_tensor")
        return t

    def release(self, ticket: int) -> None:
        _ck(self.L.cairo_ctx_release(self.h, ticket), "cairo_ctx_release")

    def encode_frame(self, rgb, index: int, inter: bool, quality: int, on_device: bool = False,
                     fmt: int = FMT_RGB24, pitch: int = 0, src_size=None, crop=None) -> FrameOutputs:
        t = self.submit(rgb, index, inter, quality, on_device, fmt=fmt, pitch=pitch, src_size=src_size, crop=crop)
        try:
            return self.wait(t, copy=True)
        finally:
            self.release(t)

    def decode_frame(self, table: np.ndarray, planes, index: int) -> np.ndarray:
        """cairo_ctx_decode_frame: reconstruct frame `index` from a block table
        and (y, u, v) coefficient planes -> RGB888.  The table must pass
        table_check; one that does not is refused here, not decoded."""
        if not table_check(table, self.wmb, self.hmb, self.ring):
            raise CairoError("decode_frame: table_check refused the table", 3)
        t = np.ascontiguousarray(table).view(np.uint8)
        coef = np.concatenate([np.ascontiguousarray(p, dtype=np.int16).ravel() for p in planes])
        assert coef.size == self.wa * self.ha * 3 // 2
        rgb = np.empty((self.height, self.width, 3), np.uint8)
        _ck(self.L.cairo_ctx_decode_frame(self.h, _ptr(t), _ptr(coef), index, _ptr(rgb)), "cairo_ctx_decode_frame")
        return rgb

    def decode_frame_tensor(self, table: np.ndarray, planes, index: int, t, **desc):
        """decode_frame written through the output map into the device tensor t
        (cairo_ctx_decode_frame_tensor; t and the keywords as tensor_desc's
        with output=True) -> t.  Synchronous; no copy to the host."""
        if not table_check(table, self.wmb, self.hmb, self.ring):
            raise CairoError("decode_frame_tensor: table_check refused the table", 3)
        d = _frame_tensor(t, self.width, self.height, True, desc)
        tb = np.ascontiguousarray(table).view(np.uint8)
        coef = np.concatenate([np.ascontiguousarray(p, dtype=np.int16).ravel() for p in planes])
        assert coef.size == self.wa * self.ha * 3 // 2
        _ck(self.L.cairo_ctx_decode_frame_tensor(self.h, _ptr(tb), _ptr(coef), index, d.ptr, ctypes.byref(d.c)),
            "cairo_ctx_decode_frame_tensor")
        return t

    def sync(self) -> None:
        _ck(self.L.cairo_ctx_sync(self.h), "cairo_ctx_sync")

    def reset(self) -> None:
        """Fresh-encoder state (cairo_ctx_reset): planes zeroed, tickets from 0,
        any group left (its members reset and rejoin together)."""
        _ck(self.L.cairo_ctx_reset(self.h), "cairo_ctx_reset")
        self._keep.clear()

    def read_planes(self, which: int):
        """which: 0 input, 1 output_cache, 2+k ring slot k -> (y, u, v)."""
        y = np.empty((self.ha, self.wa), np.int16)
        u = np.empty((self.ha // 2, self.wa // 2), np.int16)
        v = np.empty_like(u)
        _ck(self.L.cairo_ctx_read_planes(self.h, which, _ptr(y), _ptr(u), _ptr(v)), "read_planes")
        return y, u, v

    def read_inter(self):
        n = self.wmb * self.hmb * max(self.ring - 1, 0)
        d = np.zeros(n, BLOCK_DESC)
        s = np.zeros(n, np.int32)
        if n:
            _ck(self.L.cairo_ctx_read_inter(self.h, _ptr(d), _ptr(s)), "read_inter")
        return d, s

    def read_table(self):
        t = np.zeros(self.wmb * self.hmb, BLOCK_DESC)
        _ck(self.L.cairo_ctx_read_table(self.h, _ptr(t)), "read_table")
        return t

    def set_debug(self, flags: int) -> None:
        _ck(self.L.cairo_ctx_set_debug(self.h, flags), "set_debug")

    def read_predeblock(self):
        y = np.empty((self.ha, self.wa), np.int16)
        u = np.empty((self.ha // 2, self.wa // 2), np.int16)
        v = np.empty_like(u)
        _ck(self.L.cairo_ctx_read_predeblock(self.h, _ptr(y), _ptr(u), _ptr(v)), "read_predeblock")
        return y, u, v

    def read_stamps(self):
        """-> (per-MB stamps (MAX_BATCH, hmb, wmb, 12), per-row deblock chunk stamps (MAX_BATCH, hmb, 256),
        engine [entry, exit], inter-task stamps (MAX_BATCH, hmb, ng, 12): dequeue, ready,
        done, zero-MV checked, window staged, level-2 wait start / end, level-2
        count, step 16 done, integer steps done, sub-pel done) for the frames of the last batch; 100 MHz ticks."""
        n_mb, n_db = self.hmb * self.wmb * 12, self.hmb * 256
        fw = n_mb + n_db
        ng = (self.wmb + 3) // 4
        n_it = MAX_BATCH * self.hmb * ng * 12
        out = np.zeros(MAX_BATCH * fw + 2 + n_it, np.uint64)
        _ck(self.L.cairo_ctx_read_stamps(self.h, _ptr(out)), "read_stamps")
        fr = out[: MAX_BATCH * fw].reshape(MAX_BATCH, fw)
        return (fr[:, :n_mb].reshape(MAX_BATCH, self.hmb, self.wmb, 12), fr[:, n_mb:].reshape(MAX_BATCH, self.hmb, 256),
                out[MAX_BATCH * fw:MAX_BATCH * fw + 2], out[MAX_BATCH * fw + 2:].reshape(MAX_BATCH, self.hmb, ng, 12))

    def engine_variant(self) -> int:
        """The engine of the last launch enqueued: 0 plain, 1 general (diagnostics,
        cross-device groups, decode)."""
        return int(self.L.cairo_ctx_engine_variant(self.h))

    def set_profiling(self, enable: bool) -> None:
        _ck(self.L.cairo_ctx_set_profiling(self.h, int(enable)), "set_profiling")

    def take_timings(self):
        """-> ([convert ms, 0, engine ms summed over launches, engine busy ms
        (union of the launch intervals)], frames) since the last call."""
        ms = (ctypes.c_double * 4)()
        n = ctypes.c_int()
        _ck(self.L.cairo_ctx_take_timings(self.h, ms, ctypes.byref(n)), "take_timings")
        return list(ms), n.value

    def busy_intervals(self) -> np.ndarray:
        """(n, 2) engine launch [start, end) ms since profiling started, not reset."""
        n = ctypes.c_int()
        _ck(self.L.cairo_ctx_busy_intervals(self.h, None, 0, ctypes.byref(n)), "busy_intervals")
        out = np.zeros((max(n.value, 1), 2), np.float64)
        _ck(self.L.cairo_ctx_busy_intervals(self.h, _ptr(out), n.value, ctypes.byref(n)), "busy_intervals")
        return out[: n.value]

    def set_batch(self, frames: int) -> None:
        _ck(self.L.cairo_ctx_set_batch(self.h, frames), "set_batch")

    def set_workgroups(self, rows: int = 0) -> None:
        _ck(self.L.cairo_ctx_set_workgroups(self.h, rows), "set_workgroups")

    def set_helpers(self, helpers: int = 0) -> None:
        _ck(self.L.cairo_ctx_set_helpers(self.h, helpers), "set_helpers")

    def max_workgroups(self) -> int:
        return int(self.L.cairo_ctx_max_workgroups(self.h))

    def flush(self) -> None:
        _ck(self.L.cairo_ctx_flush(self.h), "cairo_ctx_flush")

    # ---- frame-interleaved groups (include/cairo_amd.h) ----
    def peer_info(self, cross_device: bool = False) -> bytes:
        """This member's cairo_peer record (plain bytes, to exchange)."""
        rec = (ctypes.c_uint8 * PEER_SIZE)()
        _ck(self.L.cairo_ctx_peer_info(self.h, int(cross_device), rec), "cairo_ctx_peer_info")
        return bytes(rec)

    def join_group(self, rank: int, peers: list) -> None:
        """Join the group of len(peers) members as `rank` (records in rank order)."""
        buf = b"".join(peers)
        assert len(buf) == PEER_SIZE * len(peers)
        arr = (ctypes.c_uint8 * len(buf)).from_buffer_copy(buf)
        _ck(self.L.cairo_ctx_join_group(self.h, len(peers), rank, arr), "cairo_ctx_join_group")


MIRROR_SLOTS = 16  # kMirrorSlots (backend.hip): reconstruction slots of a member over devices / processes


def group_layout(n: int, size: int, ring: int, stages: int, mirror: bool = False) -> dict:
    """Where frame n of a frame-interleaved group of `size` members lives
    (backend.hip frame_links): its member, that member's ticket, staging
    slot and reconstruction slot, and whether it reconstructs in place over
    frame n - ring (the reference's ring reuse, common.cpp:192-195).  mirror:
    members on other devices or processes, whose rings all share one layout
    (slot (n % N) * S + (n / N) % S: the producer's own block, a mirror block
    on every other member); `readers` are the members its deblock pushes it
    to (the frames n+1..n+R-1 reference it, n+R reads its stale rows)."""
    slots = -(-ring // size)  # S = ceil(R / N) reconstruction slots per member (per block when mirrored)
    t = n // size
    slot = (n % size) * slots + t % slots if mirror else t % slots
    readers = []
    if mirror:
        for d in range(1, ring + 1):
            j = (n + d) % size
            if j != n % size and j not in readers:
                readers.append(j)
    return {"member": n % size, "ticket": t, "staging_slot": t % stages, "recon_slot": slot,
            "recon_slots": slots * size if mirror else slots, "in_place": size * slots == ring, "readers": readers}


class Group:
    """A frame-interleaved group of member contexts in this process (one per
    device, or several on one device) encoding ONE stream: frame n goes to
    member n % N (include/cairo_amd.h).  Processes that each own
    one member exchange Context.peer_info() records themselves."""

    def __init__(self, width: int, height: int, ring: int, devices, stages: int = 64, batch: int = 0):
        self.members = [Context(width, height, ring, device=d, stages=stages) for d in devices]
        n = len(self.members)
        per_dev = {d: list(devices).count(d) for d in devices}
        cross = len(per_dev) > 1
        for m, d in zip(self.members, devices):
            if batch:
                m.set_batch(batch)
            if per_dev[d] > 1:  # members on one device share its workgroup slots
                m.set_workgroups(max(1, m.max_workgroups() // per_dev[d]))
        self.cross = cross
        self._join()
        self.size, self.ring, self.stages = n, ring, stages
        self.tickets = {}

    def _join(self) -> None:
        recs = [m.peer_info(cross_device=self.cross) for m in self.members]
        for r, m in enumerate(self.members):
            m.join_group(r, recs)

    def reset(self) -> None:
        """Every member back to the fresh-encoder state and the group rejoined
        (cairo_ctx_reset leaves it): the next frame is frame 0 of a new stream."""
        for m in self.members:
            m.reset()
        self._join()
        self.tickets = {}

    def submit(self, rgb, index: int, inter: bool, quality: int, on_device: bool = False,
               fmt: int = FMT_RGB24, pitch: int = 0, src_size=None, crop=None) -> None:
        m = self.members[index % self.size]
        self.tickets[index] = m.submit(rgb, index, inter, quality, on_device, fmt=fmt, pitch=pitch,
                                       src_size=src_size, crop=crop)

    def wait(self, index: int, copy: bool = True) -> FrameOutputs:
        """Outputs of frame `index`; launches every member's pending frames first
        (the frame may depend on any earlier frame of the stream)."""
        for m in self.members:
            m.flush()
        return self.members[index % self.size].wait(self.tickets[index], copy)

    def release(self, index: int) -> None:
        self.members[index % self.size].release(self.tickets.pop(index))

    def recon(self, n: int):
        """Frame n's deblocked reconstruction (y, u, v), while still held."""
        lay = group_layout(n, self.size, self.ring, self.stages, mirror=self.cross)
        return self.members[lay["member"]].read_planes(2 + lay["recon_slot"])

    def close(self) -> None:
        for m in self.members:
            m.close()


def default_batch(width: int, height: int) -> int:
    """Frames per engine launch the library uses by default for this frame size."""
    return int(lib().cairo_default_batch(width, height))


def task_order(hmb: int, frames: int):
    """-> (the engine's task order of a launch: int32 (frame << 16 | row) per
    task, the order slope)."""
    out = np.zeros(frames * hmb, np.int32)
    slope = ctypes.c_int()
    _ck(lib().cairo_task_order(hmb, frames, _ptr(out), ctypes.byref(slope)), "cairo_task_order")
    return out, slope.value


def task_queues(hmb: int, frames: int, helpers: int = 192, rows: int = 192, pool: int = 0):
    """-> (one pool's tasks (0 helpers, 1 row coders) of a launch with
    `helpers` + `rows` workers, partitioned into per-label queues: int32
    (frame << 16 | row), the 9 segment bounds, the number of labels) -- the
    layout the engine's launch uses (backend.hip banded_pool)."""
    out = np.zeros(frames * hmb, np.int32)
    seg = np.zeros(9, np.int32)
    nlab = ctypes.c_int()
    _ck(lib().cairo_task_queues(hmb, frames, helpers, rows, pool, _ptr(out), _ptr(seg), ctypes.byref(nlab)),
        "cairo_task_queues")
    return out, seg, nlab.value


def serialize_slice(table: np.ndarray, wmb: int, hmb: int, ring: int, cy, cu, cv, capacity_bytes: int | None = None):
    """Host entropy stage on explicit inputs -> (bytes, nbits)."""
    cap = capacity_bytes or (cy.size * 4 + 65536)
    out = np.zeros(cap, np.uint8)  # bits past the payload's end are left as they are: zeros
    pos = ctypes.c_uint32(0)
    t = np.ascontiguousarray(table).view(np.uint8)
    cy, cu, cv = (np.ascontiguousarray(a, dtype=np.int16) for a in (cy, cu, cv))
    _ck(
        lib().cairo_serialize_slice(_ptr(t), wmb, hmb, ring, _ptr(cy), _ptr(cu), _ptr(cv), _ptr(out), cap, ctypes.byref(pos)),
        "cairo_serialize_slice",
    )
    n = pos.value
    return out[: (n + 7) // 8].tobytes(), n


def serialize_feed(feed: np.ndarray, feed_bits: int, capacity_bytes: int | None = None):
    """The arithmetic coder over a GPU-precoded feed (FrameOutputs.feed) -> (bytes, nbits)."""
    cap = capacity_bytes or (feed_bits // 8 * 2 + 65536)
    out = np.zeros(cap, np.uint8)
    pos = ctypes.c_uint32(0)
    f = np.ascontiguousarray(feed, dtype=np.uint32)
    _ck(lib().cairo_serialize_feed(_ptr(f), feed_bits, _ptr(out), cap, ctypes.byref(pos)), "cairo_serialize_feed")
    return out[: (pos.value + 7) // 8].tobytes(), pos.value


def precode_slice(table: np.ndarray, wmb: int, hmb: int, ring: int, cy, cu, cv):
    """The host precode alone -> (feed words uint32, feed bits): what the GPU
    precode hands over for a FEED_VALID frame."""
    t = np.ascontiguousarray(table).view(np.uint8)
    cy, cu, cv = (np.ascontiguousarray(a, dtype=np.int16) for a in (cy, cu, cv))
    nb = ctypes.c_uint64(0)
    L = lib()
    L.cairo_precode_slice(_ptr(t), wmb, hmb, ring, _ptr(cy), _ptr(cu), _ptr(cv), None, 0, ctypes.byref(nb))
    out = np.zeros((nb.value + 31) // 32 + 1, np.uint32)
    _ck(L.cairo_precode_slice(_ptr(t), wmb, hmb, ring, _ptr(cy), _ptr(cu), _ptr(cv), _ptr(out), out.size,
                              ctypes.byref(nb)), "cairo_precode_slice")
    return out[: (nb.value + 31) // 32], nb.value


FEED_HDR_WORDS = 16  # kFeedHdrWords (precode.h): bits lo, hi; overflow; dropped writes; 11 list starts; unused


def kat_precode(frames, wmb: int, hmb: int, ring: int, slots=None, nslots: int | None = None, prefill: int = 0,
                feed_words: int = 0, guard_words: int = 64, device: int = 0):
    """The GPU precode on host tables and planes, without a context
    (cairo_kat_precode): frames = [(table, (y, u, v)), ...] of one geometry in
    one launch, frame j on staging slot slots[j] of nslots (default: j of
    len(frames)), every buffer holding `prefill` before.
    -> (hdr (n, 16), feed (n, feed_words): each frame's host words after the
    header, guard (n, guard_words): its slot's device words from the feed's end
    on)."""
    n = len(frames)
    slots = np.ascontiguousarray(np.arange(n) if slots is None else slots, dtype=np.int32)
    nslots = n if nslots is None else nslots
    mbs = wmb * hmb
    tables = np.zeros((n, mbs * 16), np.uint8)
    cy = np.zeros((n, hmb * 16, wmb * 16), np.int16)
    cu = np.zeros((n, hmb * 8, wmb * 8), np.int16)
    cv = np.zeros((n, hmb * 8, wmb * 8), np.int16)
    for j, (table, (y, u, v)) in enumerate(frames):
        tables[j] = np.ascontiguousarray(table).view(np.uint8)
        cy[j], cu[j], cv[j] = y, u, v
    hdr = np.zeros((n, FEED_HDR_WORDS), np.uint32)
    feed = np.zeros((n, feed_words), np.uint32)
    guard = np.zeros((n, guard_words), np.uint32)
    _ck(lib().cairo_kat_precode(wmb, hmb, ring, n, nslots, _ptr(slots), _ptr(tables), _ptr(cy), _ptr(cu), _ptr(cv),
                                prefill, _ptr(hdr), _ptr(feed) if feed_words else None, feed_words,
                                _ptr(guard) if guard_words else None, guard_words, device), "cairo_kat_precode")
    return hdr, feed, guard


def kat_quant(coef: np.ndarray, types, qps, device: int = 0):
    """The device quantizer and dequantizer alone (cairo_kat_quant): coef is
    (n, 384) int16 in kat_transform's layout, types[m] the block type (0..3)
    and qps[m] the qp itself (1..31) of macroblock m -> (quant, dequant), both
    (n, 384) int16."""
    coef = np.ascontiguousarray(coef, dtype=np.int16).reshape(-1, 384)
    n = coef.shape[0]
    tq = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(types, np.uint8), (n,)),
                                        np.broadcast_to(np.asarray(qps, np.uint8), (n,))], 1))
    quant, dequant = np.zeros_like(coef), np.zeros_like(coef)
    _ck(lib().cairo_kat_quant(_ptr(coef), _ptr(tq), n, _ptr(quant), _ptr(dequant), device), "cairo_kat_quant")
    return quant, dequant


def unserialize_slice(payload: bytes, nbits: int, wmb: int, hmb: int, ring: int, table=None, planes=None,
                      start: int = 0):
    """Host entropy decode of one frame's payload (bits [start, nbits) of
    payload) into a persistent (table, (y, u, v)) state (zeros when None) ->
    (table, planes, bits consumed)."""
    if table is None:
        table = np.zeros(wmb * hmb, BLOCK_DESC)
    if planes is None:
        planes = (np.zeros((hmb * 16, wmb * 16), np.int16), np.zeros((hmb * 8, wmb * 8), np.int16),
                  np.zeros((hmb * 8, wmb * 8), np.int16))
    buf = np.frombuffer(payload, np.uint8) if len(payload) else np.zeros(1, np.uint8)
    rd = ctypes.c_uint32(start)
    _ck(lib().cairo_unserialize_slice(_ptr(np.ascontiguousarray(buf)), ctypes.byref(rd), nbits, wmb, hmb, ring,
                                      _ptr(table), *(_ptr(p) for p in planes)), "cairo_unserialize_slice")
    return table, planes, rd.value - start


def table_check(table: np.ndarray, wmb: int, hmb: int, ring: int) -> bool:
    """cairo_table_check: may this block table go to the decode-mode engine?"""
    t = np.ascontiguousarray(table).view(np.uint8)
    assert t.size == wmb * hmb * 16
    return bool(lib().cairo_table_check(_ptr(t), wmb, hmb, ring))


def desc_check(descs: np.ndarray, mb_index, wmb: int, hmb: int, ring: int) -> np.ndarray:
    """cairo_desc_check: is descs[k] legal as macroblock mb_index[k]? -> bool array."""
    d = np.ascontiguousarray(descs, dtype=BLOCK_DESC).reshape(-1)
    idx = np.ascontiguousarray(np.broadcast_to(np.asarray(mb_index, np.uint32), d.shape))
    ok = np.zeros(d.size, np.uint8)
    _ck(lib().cairo_desc_check(_ptr(d.view(np.uint8)), _ptr(idx), d.size, wmb, hmb, ring, _ptr(ok)), "cairo_desc_check")
    return ok.astype(bool)


def bits_append(dst: np.ndarray, pos: int, src: bytes, nbits: int) -> int:
    """Append nbits of src (LSB-first) at bit pos of the uint8 array dst -> new pos."""
    p = ctypes.c_uint64(pos)
    s = np.frombuffer(src, np.uint8) if len(src) else np.zeros(1, np.uint8)
    _ck(lib().cairo_bits_append(_ptr(dst), dst.size * 8, ctypes.byref(p), _ptr(s), nbits), "cairo_bits_append")
    return p.value


class Stream:
    """Frame pipeline (``cairo_stream_*``): GPU hot path + host entropy on
    native worker threads.  Drives ``ctx`` exclusively while open."""

    def __init__(self, ctx: "Context", threads: int = 0):
        self.L = lib()
        self.ctx = ctx
        p = ctypes.c_void_p()
        _ck(self.L.cairo_stream_create(ctx.h, threads, ctypes.byref(p)), "cairo_stream_create")
        self.h = p
        self._keep = {}

    def submit(self, rgb, index: int, inter: bool, quality: int, on_device: bool = False,
               fmt: int = FMT_RGB24, pitch: int = 0, src_size=None, crop=None) -> int:
        """src_size / crop: a scaled submit, as Context.submit."""
        return _submit("cairo_stream", self.h, self.ctx.width, self.ctx.height, self._keep, rgb, index, inter, quality,
                       on_device, fmt, pitch, src_size, crop)

    def submit_tensor(self, t, index: int, inter: bool, quality: int, sync: bool = True, scaled: bool = False,
                      crop=None, src_size=None, **desc) -> int:
        """A tensor frame, as Context.submit_tensor (cairo_stream_submit_tensor;
        scaled / crop / src_size: cairo_stream_submit_tensor_scaled); t is kept
        alive until the frame is collected."""
        return _submit_tensor("cairo_stream", self.h, self.ctx.width, self.ctx.height, self._keep, t, index, inter,
                              quality, sync, desc, scaled, crop, src_size)

    def collect(self, ticket: int, out: np.ndarray | None = None, pos: int = 0):
        """Append the frame's payload at bit pos of out -> new pos; with out
        None, return (bytes, nbits) of the payload alone."""
        if out is None:
            p = ctypes.c_uint64(0)
            _ck(self.L.cairo_stream_payload_bits(self.h, ticket, ctypes.byref(p)), "cairo_stream_payload_bits")
            buf = np.zeros(p.value // 8 + 8, np.uint8)
            p = ctypes.c_uint64(0)
            _ck(self.L.cairo_stream_collect(self.h, ticket, _ptr(buf), buf.size, ctypes.byref(p)),
                "cairo_stream_collect")
            self._keep.pop(ticket, None)
            return buf[: (p.value + 7) // 8].tobytes(), p.value
        p = ctypes.c_uint64(pos)
        _ck(self.L.cairo_stream_collect(self.h, ticket, _ptr(out), out.size, ctypes.byref(p)), "cairo_stream_collect")
        self._keep.pop(ticket, None)
        return p.value

    def payload_bits(self, ticket: int) -> int:
        """The frame's payload length in bits (waits for its entropy stage)."""
        p = ctypes.c_uint64(0)
        _ck(self.L.cairo_stream_payload_bits(self.h, ticket, ctypes.byref(p)), "cairo_stream_payload_bits")
        return p.value

    def frame_metrics(self, ticket: int) -> dict:
        """Metrics of a frame whose outputs the pipeline has picked up (a
        collected frame, until ticket + 2 * stages is submitted); the context's
        set_metrics comes before the stream is created."""
        m = _FrameMetrics()
        _ck(self.L.cairo_stream_frame_metrics(self.h, ticket, ctypes.byref(m)), "cairo_stream_frame_metrics")
        return _metrics_dict(m)

    def frame_rate(self, ticket: int) -> dict:
        """Context.frame_rate of a frame whose outputs the pipeline has picked
        up (as frame_metrics); the frame record is the caller's to write, with
        this quality."""
        r = _RateInfo()
        _ck(self.L.cairo_stream_frame_rate(self.h, ticket, ctypes.byref(r)), "cairo_stream_frame_rate")
        return _rate_dict(r)

    def timeline(self, ticket: int):
        """(submitted, outputs on host, entropy start, entropy end, collected), us."""
        t = (ctypes.c_double * 5)()
        _ck(self.L.cairo_stream_timeline(self.h, ticket, t), "cairo_stream_timeline")
        return list(t)

    def close(self) -> None:
        if self.h:
            r = self.L.cairo_stream_destroy(self.h)
            self.h = None
            self._keep.clear()
            _ck(r, "cairo_stream_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BitStream:
    """evx::bit_stream owned from Python."""

    def __init__(self, size_bits: int):
        self.L = lib()
        self.h = self.L.evx_bitstream_create(size_bits)
        if not self.h:
            raise MemoryError("evx_bitstream_create")

    def bits(self) -> int:
        return self.L.evx_bitstream_occupancy(self.h)

    def write(self, data: bytes, nbits: int | None = None) -> None:
        """Append nbits (default: all) of data, LSB-first."""
        n = len(data) * 8 if nbits is None else nbits
        buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
        _ck(self.L.evx_bitstream_write_bits(self.h, _ptr(np.ascontiguousarray(buf)), n), "write_bits")

    def data(self) -> bytes:
        n = (self.bits() + 7) // 8
        return ctypes.string_at(self.L.evx_bitstream_data(self.h), n) if n else b""

    def empty(self) -> None:
        self.L.evx_bitstream_empty(self.h)

    def __del__(self):
        try:
            if self.h:
                self.L.evx_bitstream_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Encoder:
    """The drop-in evx1_encoder (reference evx1.h:66-94) through its C view."""

    def __init__(self, ring: int = 4, device: int = 0):
        self.L = lib()
        p = ctypes.c_void_p()
        _ck(self.L.evx_encoder_create(ctypes.byref(p)), "create_encoder")
        self.h = p
        if ring != 4:
            _ck(self.L.evx_encoder_set_ring(self.h, ring), "set_ring")
        if device:
            _ck(self.L.evx_encoder_set_device(self.h, device), "set_device")

    def set_quality(self, q: int) -> None:
        _ck(self.L.evx_encoder_set_quality(self.h, q), "set_quality")

    def insert_intra(self) -> None:
        _ck(self.L.evx_encoder_insert_intra(self.h), "insert_intra")

    def clear(self) -> None:
        _ck(self.L.evx_encoder_clear(self.h), "clear")

    def set_input_format(self, fmt: int, pitch: int = 0) -> None:
        """The layout encode() reads its frames in from now on (FMT_*, row pitch
        in bytes, 0: tight); callable between frames.  peek() stays RGB888."""
        _ck(self.L.evx_encoder_set_input_format(self.h, fmt, pitch), "set_input_format")
        self._fmt, self._pitch = fmt, pitch

    def set_input_tensor(self, t, **desc) -> None:
        """encode() reads, from now on, device tensors laid out like t
        (tensor_desc's arguments: dtype, strides and the input map are fixed
        here; each encode() brings a tensor of that layout, such as batch[n] of
        an NCHW batch, or a device address with width and height).  None goes
        back to the pixel formats.  Callable between frames."""
        d = None if t is None else tensor_desc(t, output=False, **desc)
        _ck(self.L.evx_encoder_set_input_tensor(self.h, None if d is None else ctypes.byref(d.c)),
            "set_input_tensor")
        self._tensor = d

    def set_input_color(self, range: int, matrix: int) -> None:
        """The colour description (RANGE_*, MATRIX_*) of the I420 / NV12 frames
        encode() reads from now on; callable between frames."""
        _ck(self.L.evx_encoder_set_input_color(self.h, range, matrix), "set_input_color")

    def set_metrics(self, sse: bool = True, ssim: bool = True) -> None:
        """Per-frame metrics for the frames encode() codes from now on."""
        _ck(self.L.evx_encoder_set_metrics(self.h, (METRIC_SSE if sse else 0) | (METRIC_SSIM if ssim else 0)),
            "evx_encoder_set_metrics")

    def last_metrics(self) -> dict:
        """Metrics of the last encoded frame (Context.frame_metrics' dict)."""
        m = _FrameMetrics()
        _ck(self.L.evx_encoder_last_metrics(self.h, ctypes.byref(m)), "evx_encoder_last_metrics")
        return _metrics_dict(m)

    def encode(self, rgb: np.ndarray, bs: BitStream, width: int | None = None, height: int | None = None) -> None:
        """Encode one frame.  With the default input format, rgb is (height,
        width, 3) RGB888.  After set_input_format, it is a uint8 buffer of
        frame_layout(fmt, width, height, pitch) bytes; width and height may be
        left out where the array's shape is (height, width, 3)."""
        if getattr(self, "_tensor", None) is not None:
            # a device tensor laid out as set_input_tensor's, or its address
            if hasattr(rgb, "data_ptr"):
                d = tensor_desc(rgb)
                if tuple(d.c.stride) != tuple(self._tensor.c.stride) or d.c.dtype != self._tensor.c.dtype:
                    raise ValueError("the tensor's dtype or strides differ from set_input_tensor's")
                width, height = d.width, d.height
                _sync_producer(rgb)
                rgb = d.ptr
            if width is None or height is None:
                raise ValueError("width and height are needed with a device address")
            _ck(self.L.evx_encoder_encode(self.h, int(rgb), width, height, bs.h), "encode")
            self._shape = (width, height)
            return
        fmt, pitch = getattr(self, "_fmt", FMT_RGB24), getattr(self, "_pitch", 0)
        if fmt != FMT_RGB24 or pitch:
            if width is None or height is None:
                if not isinstance(rgb, np.ndarray) or rgb.ndim != 3 or rgb.shape[2] != 3:
                    raise ValueError("width and height are needed for a frame that is not shaped (height, width, 3)")
                height, width = rgb.shape[:2]
            ptr = _host_frame_fmt(rgb, fmt, width, height, pitch)
            _ck(self.L.evx_encoder_encode(self.h, ptr, width, height, bs.h), "encode")
            self._shape = (width, height)
            return
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError(f"frame must have shape (height, width, 3), got {rgb.shape}")
        h, w = rgb.shape[:2]
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8) if rgb.dtype == np.uint8 else None
        if rgb is None:
            raise ValueError("frame must be uint8 RGB888")
        _ck(self.L.evx_encoder_encode(self.h, _ptr(rgb), w, h, bs.h), "encode")
        self._shape = (w, h)

    def peek(self, state: int, width: int, height: int) -> np.ndarray:
        """Debug view of the last encoded frame (EVX_PEEK_*, evx1.h) -> RGB (h, w, 3)."""
        # the native peek writes the encoder's frame size: refuse a smaller view
        if getattr(self, "_shape", None) != (width, height):
            raise ValueError(f"peek size {width}x{height} differs from the last encoded frame "
                             f"{getattr(self, '_shape', None)}")
        out = np.zeros((height, width, 3), np.uint8)
        _ck(self.L.evx_encoder_peek(self.h, state, _ptr(out)), "peek")
        return out

    def close(self) -> None:
        if self.h:
            self.L.evx_encoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Decoder:
    """The drop-in evx1_decoder (reference evx1.h:97-112) through its C view."""

    def __init__(self, device: int = 0):
        self.L = lib()
        p = ctypes.c_void_p()
        _ck(self.L.evx_decoder_create(ctypes.byref(p)), "create_decoder")
        self.h = p
        if device:
            _ck(self.L.evx_decoder_set_device(self.h, device), "set_device")

    def set_output_format(self, fmt: int, pitch: int = 0) -> None:
        """The layout decode() returns its frames in from now on (FMT_*, row
        pitch in bytes, 0: tight); callable between frames."""
        _ck(self.L.evx_decoder_set_output_format(self.h, fmt, pitch), "set_output_format")
        self._fmt, self._pitch = fmt, pitch

    def set_output_tensor(self, t, **desc) -> None:
        """decode(..., out=x) writes, from now on, into device tensors laid out
        like t (tensor_desc's arguments with output=True), with no copy to the
        host.  None goes back to the pixel formats.  Callable between frames."""
        d = None if t is None else tensor_desc(t, output=True, **desc)
        _ck(self.L.evx_decoder_set_output_tensor(self.h, None if d is None else ctypes.byref(d.c)),
            "set_output_tensor")
        self._tensor = d

    def set_output_color(self, range: int, matrix: int) -> None:
        """The colour description (RANGE_*, MATRIX_*) decode() writes I420 /
        NV12 frames in from now on; callable between frames."""
        _ck(self.L.evx_decoder_set_output_color(self.h, range, matrix), "set_output_color")

    def decode(self, bs: "BitStream", width: int, height: int, out: np.ndarray | None = None) -> np.ndarray:
        """Decode [header +] one frame record of bs (emptied afterwards) -> RGB
        (h, w, 3) for tight RGB24 / BGR24; for a YUV or pitched output format a
        flat uint8 buffer of frame_layout bytes (split_frame gives its planes).
        out: a buffer to write into (its pitch padding keeps its bytes)."""
        if getattr(self, "_tensor", None) is not None:
            # into a device tensor laid out as set_output_tensor's (or its address) -> out
            if out is None:
                raise ValueError("decode() into a tensor needs out=")
            ptr = out
            if hasattr(out, "data_ptr"):
                d = tensor_desc(out, output=True)
                if tuple(d.c.stride) != tuple(self._tensor.c.stride) or d.c.dtype != self._tensor.c.dtype or \
                        (d.width, d.height) != (width, height):
                    raise ValueError("the tensor's dtype, strides or size differ from set_output_tensor's")
                ptr = d.ptr
            _ck(self.L.evx_decoder_decode(self.h, bs.h, int(ptr)), "decode")
            return out
        fmt, pitch = getattr(self, "_fmt", FMT_RGB24), getattr(self, "_pitch", 0)
        nb, tight = frame_layout(fmt, width, height, pitch)
        if out is None:
            out = np.zeros(nb, np.uint8)
        elif not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.nbytes != nb or \
                not out.flags["C_CONTIGUOUS"]:
            raise ValueError(f"out must be a C-contiguous uint8 array of {nb} bytes")
        _ck(self.L.evx_decoder_decode(self.h, bs.h, _ptr(out)), "decode")
        if fmt in (FMT_RGB24, FMT_BGR24) and (not pitch or pitch == tight):
            return out.reshape(height, width, 3)
        return out

    def clear(self) -> None:
        _ck(self.L.evx_decoder_clear(self.h), "clear")

    def close(self) -> None:
        if self.h:
            self.L.evx_decoder_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def yuv_to_rgb(y: np.ndarray, u: np.ndarray, v: np.ndarray, width: int, height: int) -> np.ndarray:
    """convert_image YUV -> RGB (reference convert.cpp:16-19, 162-223), numpy
    restatement for tests: saturate narrows to int16, then clips to 0..255."""
    yy = y[:height, :width].astype(np.int32) - 16
    uu = np.repeat(np.repeat(u.astype(np.int32) - 128, 2, 0), 2, 1)[:height, :width]
    vv = np.repeat(np.repeat(v.astype(np.int32) - 128, 2, 0), 2, 1)[:height, :width]

    def sat(x):
        x = ((x + 32768) & 0xFFFF) - 32768
        return np.clip(x, 0, 255).astype(np.uint8)

    return np.stack([sat((256 * yy + 358 * vv + 128) >> 8),
                     sat((256 * yy - 88 * uu - 182 * vv + 128) >> 8),
                     sat((256 * yy + 452 * uu + 128) >> 8)], axis=-1)


def device_count() -> int:
    return lib().cairo_device_count()
