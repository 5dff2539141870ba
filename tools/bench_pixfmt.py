#!/usr/bin/env python3
"""Hot-path rate per input pixel format (include/cairo_amd.h CAIRO_FMT_*).

One process, one context per leg, the plain bench run's shape: frames resident
in HBM, feed outputs, the library's default batch, `--warmup` untimed launches
and `--steps` timed ones, nothing copied to the host in the timed region.  The
same band4 content goes in as RGB24, BGR24, I420 and NV12 (the YUV frames are
the convert's own planes, Y - 16, U, V: tools' content fits 8 bits,
tests/test_pixfmt.py), then RGB24 and NV12 once more from pinned host memory
(the PCIe-inclusive rate).  After timing, each format's block tables of the
first `--check-frames` frames are compared with the RGB24 run's.

Capture and 10-bit layouts: YUY2, UYVY and P010 legs carry
the unfold of the NV12 frames (cairo_frame_fold), whose fold is that NV12 frame
again, so their tables are compared with the same run's; P010 runs from pinned
host memory as well (as many bytes per frame as RGB24).  "capfmt" relates each
resident leg to the NV12 legs of this process and their spread.

Colour descriptions: the resident NV12 leg runs a second time
("nv12_repeat"), so that the identity leg's own run-to-run spread in this
process is known, and then once more with the same bytes *interpreted* as
LIMITED / BT709 ("nv12_limited_bt709": the full colour map in the convert; its
tables are another picture's, so they are not compared).

Prints one JSON line.  The resident pool is `--pool` distinct frames, cycled,
so a rate here is not bench.py's headline (whose frames are all distinct): the
figures are for comparing the formats with each other.

usage: python tools/bench_pixfmt.py [--config 4k] [--steps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"4k": (3840, 2160, 4, 16), "1080p": (1920, 1080, 4, 8), "720p": (1280, 720, 2, 16), "cif": (352, 288, 4, 16)}
NAMES = {0: "rgb24", 1: "bgr24", 2: "i420", 3: "nv12", 8: "yuy2", 9: "uyvy", 10: "p010"}
CAP_FMTS = (8, 9, 10)  # FMT_YUY2, FMT_UYVY, FMT_P010


def yuv_frame(cairo_amd, rgb, fmt):
    """The RGB frame's source planes (the library's own convert, through
    cairo_kat_convert) as a tight I420 / NV12 frame: Y - 16, U, V."""
    h, w = rgb.shape[:2]
    y = np.empty((h, w), np.int16)
    u = np.empty((h // 2, w // 2), np.int16)
    v = np.empty_like(u)
    src = np.ascontiguousarray(rgb)
    st = cairo_amd.lib().cairo_kat_convert(0, cairo_amd.FMT_RGB24, w, h, 0, src.ctypes.data, y.ctypes.data,
                                           u.ctypes.data, v.ctypes.data, 0)
    if st:
        raise RuntimeError(f"cairo_kat_convert: {st}")
    if y.min() < 16 or y.max() > 271 or min(u.min(), v.min()) < 0 or max(u.max(), v.max()) > 255:
        raise RuntimeError("content does not fit 8-bit YUV")
    out = np.empty(w * h * 3 // 2, np.uint8)
    out[:w * h] = (y - 16).reshape(-1)
    if fmt == cairo_amd.FMT_I420:
        out[w * h:w * h * 5 // 4] = u.reshape(-1)
        out[w * h * 5 // 4:] = v.reshape(-1)
    else:
        out[w * h:].reshape(-1, 2)[:, 0] = u.reshape(-1)
        out[w * h:].reshape(-1, 2)[:, 1] = v.reshape(-1)
    return out


def run(ctx, frame_of, first, count, q, on_device, fmt, log=None, tables=None):
    inflight = deque()
    stages = ctx.stages

    def retire():
        f, t = inflight.popleft()
        out = ctx.wait(t, copy=False)
        if tables is not None:
            tb = out.table.copy()
            tb["pad"] = 0
            tables.append(tb)
        ctx.release(t)
        if log is not None:
            log.append(time.perf_counter())

    for f in range(first, first + count):
        if len(inflight) == stages:
            retire()
        inflight.append((f, ctx.submit(frame_of(f), f, f > 0, q, on_device=on_device, fmt=fmt)))
    while inflight:
        retire()


def leg(cairo_amd, w, h, ring, q, batch, warm, timed, frame_of, on_device, fmt, check, color=None):
    ctx = cairo_amd.Context(w, h, ring)
    if color is not None:
        ctx.set_input_color(*color)
    ctx.set_batch(batch)
    ctx.set_outputs(cairo_amd.OUT_FEED)
    run(ctx, frame_of, 0, warm, q, on_device, fmt)
    ctx.sync()
    done = []
    t0 = time.perf_counter()
    run(ctx, frame_of, warm, timed, q, on_device, fmt, log=done)
    ctx.sync()
    el = time.perf_counter() - t0
    out = {"value": round(w * h * timed / el / 1e6, 3), "ms_per_frame": round(el * 1e3 / timed, 4)}
    if timed > batch:  # without the first launch's fill and the last launch's tail (bench.py host_rgb)
        st = done[-1] - done[batch - 1]
        out["steady_value"] = round(w * h * (timed - batch) / st / 1e6, 3)
    tables = []
    if check:  # untimed: the first frames of a fresh stream
        ctx.reset()
        ctx.set_outputs(cairo_amd.OUT_FEED)
        run(ctx, frame_of, 0, check, q, on_device, fmt, tables=tables)
    ctx.close()
    return out, tables


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="4k", choices=sorted(CONFIGS))
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--pool", type=int, default=96, help="distinct resident frames per format, cycled")
    p.add_argument("--host-steps", type=int, default=12, help="timed launches of the host-fed legs (0: skip)")
    p.add_argument("--check-frames", type=int, default=48)
    p.add_argument("--no-color", dest="color", action="store_false",
                   help="skip the NV12 repeat and the NV12 LIMITED / BT709 legs")
    p.add_argument("--no-capfmt", dest="capfmt", action="store_false", help="skip the YUY2, UYVY and P010 legs")
    p.add_argument("--formats", default=None, metavar="NAMES",
                   help="comma-separated resident legs to run alone (for a kernel trace of one format): no host-fed "
                        "legs, no table check, no comparisons")
    a = p.parse_args()
    import torch  # device and pinned memory only; before the library starts HIP

    torch.cuda.set_device(0)
    import cairo_amd

    w, h, ring, q = CONFIGS[a.config]
    batch = cairo_amd.default_batch(w, h)
    warm, timed = a.warmup * batch, a.steps * batch
    pool_n = max(2 * batch, a.pool)
    with ThreadPoolExecutor(8) as pool:
        rgb = list(pool.map(lambda f: cairo_amd.make_band4(w, h, f), range(pool_n)))
    host = {0: rgb, 1: [np.ascontiguousarray(f[..., ::-1]) for f in rgb],
            2: [yuv_frame(cairo_amd, f, cairo_amd.FMT_I420) for f in rgb],
            3: [yuv_frame(cairo_amd, f, cairo_amd.FMT_NV12) for f in rgb]}
    res = {"config": a.config, "width": w, "height": h, "ring": ring, "quality": q, "batch": batch,
           "warmup_frames": warm, "timed_frames": timed, "pool_frames": pool_n, "unit": "Mpix/s", "resident": {},
           "host_fed": {}, "tables_equal_rgb24": {}}
    ref_tables = None
    legs = (0, 1, 2, 3) + (CAP_FMTS if a.capfmt else ())
    if a.formats:
        legs = tuple(f for f in legs if NAMES[f] in a.formats.split(","))
        a.check_frames, a.host_steps, a.color, a.capfmt = 0, 0, False, False
    for fmt in legs:
        if fmt in CAP_FMTS:  # built when its turn comes and dropped after it: a P010 pool is as large as the RGB one
            host[fmt] = [cairo_amd.frame_fold(1, fmt, f, w, h) for f in host[3]]
        nb = host[fmt][0].nbytes
        dev = torch.empty((pool_n, nb), dtype=torch.uint8, device="cuda")
        for i, f in enumerate(host[fmt]):
            dev[i].copy_(torch.from_numpy(f.reshape(-1)))
        torch.cuda.synchronize()
        base = dev.data_ptr()
        out, tables = leg(cairo_amd, w, h, ring, q, batch, warm, timed, lambda f: base + (f % pool_n) * nb, True, fmt,
                          a.check_frames)
        out["source_bytes_per_frame"] = nb
        res["resident"][NAMES[fmt]] = out
        if fmt == 0:
            ref_tables = tables
        elif not a.formats:
            res["tables_equal_rgb24"][NAMES[fmt]] = len(tables) == len(ref_tables) and all(
                np.array_equal(x, y) for x, y in zip(tables, ref_tables))
        if fmt == cairo_amd.FMT_NV12 and a.color:
            frame_of = lambda f: base + (f % pool_n) * nb  # noqa: E731
            rep, tables = leg(cairo_amd, w, h, ring, q, batch, warm, timed, frame_of, True, fmt, a.check_frames)
            rep["source_bytes_per_frame"] = nb
            res["resident"]["nv12_repeat"] = rep
            res["tables_equal_rgb24"]["nv12_repeat"] = len(tables) == len(ref_tables) and all(
                np.array_equal(x, y) for x, y in zip(tables, ref_tables))
            col, _ = leg(cairo_amd, w, h, ring, q, batch, warm, timed, frame_of, True, fmt, 0,
                         color=(cairo_amd.RANGE_LIMITED, cairo_amd.MATRIX_BT709))
            col["source_bytes_per_frame"] = nb
            res["resident"]["nv12_limited_bt709"] = col
            lo, hi = sorted((out["value"], rep["value"]))
            res["color"] = {"identity_runs": [out["value"], rep["value"]], "identity_spread_pct":
                            round(100 * (hi - lo) / lo, 3), "limited_bt709": col["value"],
                            "inside_identity_spread": lo <= col["value"] <= hi,
                            "vs_identity_mean_pct": round(100 * (2 * col["value"] / (lo + hi) - 1), 3)}
            print(f"[bench_pixfmt] nv12_repeat: {rep}\n[bench_pixfmt] nv12_limited_bt709: {col}", file=sys.stderr,
                  flush=True)
        del dev
        torch.cuda.empty_cache()
        if fmt in (8, 9):
            del host[fmt]
        print(f"[bench_pixfmt] {NAMES[fmt]}: {out}", file=sys.stderr, flush=True)
    if a.capfmt:
        nv = [res["resident"][k]["value"] for k in ("nv12", "nv12_repeat") if k in res["resident"]]
        lo, hi = min(nv), max(nv)
        res["capfmt"] = {"nv12_runs": nv, "nv12_spread_pct": round(100 * (hi - lo) / lo, 3)}
        for fmt in CAP_FMTS:
            v = res["resident"][NAMES[fmt]]["value"]
            res["capfmt"][NAMES[fmt]] = {"value": v, "vs_nv12_low_pct": round(100 * (v / lo - 1), 3),
                                         "below_nv12_by_more_than_its_spread": v < lo - (hi - lo)}
    if a.host_steps:
        n = 2 * batch
        for fmt in (0, 3) + ((10,) if a.capfmt else ()):
            nb = host[fmt][0].nbytes
            pinned = torch.empty((n, nb), dtype=torch.uint8, pin_memory=True)
            hv = pinned.numpy()
            for i in range(n):
                hv[i] = host[fmt][i].reshape(-1)
            frames = [hv[i].reshape(h, w, 3) if fmt == 0 else hv[i] for i in range(n)]
            out, tables = leg(cairo_amd, w, h, ring, q, batch, batch, a.host_steps * batch, lambda f: frames[f % n],
                              False, fmt, min(a.check_frames, n))
            out["pcie_bytes_per_frame"] = nb
            out["pcie_GBps"] = round(nb * out["value"] * 1e6 / (w * h) / 1e9, 2)
            if ref_tables is not None:
                m = min(len(tables), len(ref_tables))
                out["tables_equal_rgb24"] = all(np.array_equal(x, y) for x, y in zip(tables[:m], ref_tables[:m]))
            res["host_fed"][NAMES[fmt]] = out
            del frames, hv, pinned
            print(f"[bench_pixfmt] host-fed {NAMES[fmt]}: {out}", file=sys.stderr, flush=True)
    res["ok"] = all(res["tables_equal_rgb24"].values()) and all(
        v.get("tables_equal_rgb24", True) for v in res["host_fed"].values())
    print(json.dumps(res))
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
