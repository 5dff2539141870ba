"""Per-frame metrics without a GPU: the header, the binding and the numpy
restatement (tests/metrics_ref.py) that the GPU tests compare against."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import metrics_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "cairo_amd.h")).read()

NEW_SYMBOLS = ("cairo_ctx_set_metrics", "cairo_ctx_frame_metrics", "cairo_ctx_fetch_recon_planes",
               "cairo_ctx_fetch_recon", "cairo_stream_frame_metrics", "cairo_kat_metrics", "cairo_frame_metrics_size",
               "evx_encoder_set_metrics", "evx_encoder_last_metrics")


def test_flag_values_match_header(cairo):
    flags = {k: int(v) for k, v in re.findall(r"#define (CAIRO_METRIC_\w+|CAIRO_KEEP_RECON) (\d+)", HEADER)}
    assert flags == {"CAIRO_METRIC_SSE": cairo.METRIC_SSE, "CAIRO_METRIC_SSIM": cairo.METRIC_SSIM,
                     "CAIRO_KEEP_RECON": cairo.KEEP_RECON}
    assert (cairo.METRIC_SSE, cairo.METRIC_SSIM, cairo.KEEP_RECON) == (1, 2, 4)


def test_api_version_unchanged(cairo):
    """The feature adds symbols only; callers detect it by them."""
    assert cairo.lib().cairo_api_version() == 4 == cairo.API_VERSION


def test_struct_size(cairo):
    assert cairo.lib().cairo_frame_metrics_size() == ctypes.sizeof(cairo._FrameMetrics) == 112


def test_symbols_declared_and_exported(cairo):
    L = cairo.lib()
    for n in NEW_SYMBOLS:
        assert re.search(r"CAIRO_API\s+int\s+%s\s*\(" % n, HEADER), f"{n} is not declared in the header"
        assert hasattr(L, n), f"{n} is not exported"


def test_header_states_the_constants():
    assert "c1 = 416" in HEADER and "c2 = 235963" in HEADER
    assert (ref.C1, ref.C2) == (round((0.01 * 255) ** 2 * 64), round((0.03 * 255) ** 2 * 64 * 63))


def _planes(rng, w, h, lo=-300, hi=600):
    return (rng.integers(lo, hi + 1, (h, w)).astype(np.int16),
            rng.integers(lo, hi + 1, (h // 2, w // 2)).astype(np.int16),
            rng.integers(lo, hi + 1, (h // 2, w // 2)).astype(np.int16))


@pytest.mark.parametrize("size", [(8, 8), (18, 10), (130, 66)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identical_planes(size):
    w, h = size
    a = _planes(np.random.default_rng(w), w, h)
    m = ref.frame_metrics(a, a, w, h)
    assert m["sse"] == [0, 0, 0]
    assert m["ssim_sum"] == [float(n) for n in m["ssim_windows"]]  # every window is exactly 1.0
    assert m["samples"] == [w * h, w * h // 4, w * h // 4]
    assert ref.psnr(0, w * h) == float("inf")


def test_zero_against_255():
    w, h = 18, 10
    a = (np.full((h, w), 16, np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16))
    b = (np.full((h, w), 271, np.int16), np.full((h // 2, w // 2), 255, np.int16), np.full((h // 2, w // 2), 255, np.int16))
    m = ref.frame_metrics(a, b, w, h)
    assert m["sse"] == [65025 * n for n in m["samples"]]
    assert ref.psnr(m["sse"][0], m["samples"][0]) == 0.0
    # beyond the clamps nothing changes: -300 is 0, 600 is 255
    a2 = tuple(np.full_like(p, -300) for p in a)
    b2 = tuple(np.full_like(p, 600) for p in b)
    assert ref.frame_metrics(a2, b2, w, h) == m


@pytest.mark.parametrize("size,count", [((2, 2), 0), ((8, 8), 1), ((10, 6), 0), ((130, 66), 31 * 15)],
                         ids=lambda v: str(v))
def test_window_counts(size, count):
    pw, ph = size
    assert ref.window_count(pw, ph) == count
    z = np.zeros((ph, pw), np.int64)
    assert ref.ssim_windows(z, z).size == count
    if count:
        assert ref.ssim_windows(z, z).shape == (ph // 4 - 1, pw // 4 - 1)


def test_hand_computed_window():
    """One 8x8 window, worked by hand.
    Flat 100 against flat 110: s1 = 6400, s2 = 7040, ss = 64 * 22100, s12 = 64 * 11000, so vars = covar = 0 and the
    value is (2 * 6400 * 7040 + 416) / (6400^2 + 7040^2 + 416), times c2 / c2.
    A 0 / 255 checkerboard against its inverse: s1 = s2 = 8160, ss = 64 * 65025, s12 = 0, so vars = 133171200,
    covar = -66585600: anti-correlated, close to -1."""
    a = np.full((8, 8), 100, np.int64)
    b = np.full((8, 8), 110, np.int64)
    num, den = 90112416 * 235963, 90522016 * 235963
    got = ref.ssim_windows(a, b)
    assert got.shape == (1, 1) and got[0, 0] == float(num) / float(den)
    assert abs(got[0, 0] - 0.99547513) < 1e-8
    i, j = np.mgrid[0:8, 0:8]
    a = 255 * ((i + j) & 1)
    b = 255 - a
    num, den = 133171616 * (2 * -66585600 + 235963), 133171616 * (133171200 + 235963)
    got = ref.ssim_windows(a, b)
    assert got[0, 0] == float(num) / float(den)
    assert abs(got[0, 0] + 0.99646251) < 1e-8
    m = ref.plane_metrics(a, b)
    assert m == {"sse": 64 * 65025, "ssim_sum": float(num) / float(den), "ssim_windows": 1, "samples": 64}


def test_leftover_columns_count_for_sse_only():
    """10x6: two blocks by one, no window; SSE still covers all 60 samples."""
    a = np.zeros((6, 10), np.int64)
    b = np.zeros((6, 10), np.int64)
    b[5, 9] = 3  # outside every 4x4 block
    assert ref.plane_metrics(a, b) == {"sse": 9, "ssim_sum": 0.0, "ssim_windows": 0, "samples": 60}


def test_binding_derives_psnr_and_ssim(cairo):
    m = cairo._FrameMetrics()
    m.flags, m.width, m.height = 3, 8, 8
    for k, (sse, n) in enumerate(((64, 64), (0, 16), (16 * 65025, 16))):
        m.sse[k], m.samples[k], m.ssim_sum[k], m.ssim_windows[k] = sse, n, 0.5 * (k == 0), int(k == 0)
    d = cairo._metrics_dict(m)
    assert d["psnr_y"] == pytest.approx(20 * np.log10(255.0)) and d["psnr_u"] == float("inf") and d["psnr_v"] == 0.0
    assert d["psnr_all"] == ref.psnr(64 + 16 * 65025, 96)
    assert d["ssim_y"] == 0.5 and d["ssim_u"] is None and d["ssim_v"] is None
    m.flags = 1
    d = cairo._metrics_dict(m)
    assert d["ssim_y"] is None and d["psnr_y"] is not None
