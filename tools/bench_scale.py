#!/usr/bin/env python3
"""What the scaled submit costs (include/cairo_amd.h cairo_ctx_submit_scaled).

One process, the plain bench run's shape (frames resident in HBM, feed
outputs, the library's default batch, `--warmup` untimed launches and `--steps`
timed ones, nothing copied to the host in the timed region).  A context of the
rendition's size (default 1080p, q = 8, R = 4) is fed two ways at the same
launch counts:

  (a) resident frames of its own size, scaled beforehand (by the library's own
      scaler through cairo_kat_scale, so both legs encode the same bits);
  (b) the resident 4K source frames through the scaled submit.

Both for RGB24 and for NV12 (the NV12 sources are the convert's own planes of
the RGB content: Y - 16, U, V).  After timing, the block tables of the first
`--check-frames` frames of (b) are compared with (a)'s.  Leg (a) is the
comparison; no ratio is asserted.

Prints one JSON line.  The resident pool is `--pool` distinct frames, cycled,
so a rate here is not bench.py's headline.

usage: python tools/bench_scale.py [--rendition 1080p] [--steps 20] [--warmup 5]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_pixfmt import yuv_frame  # noqa: E402

SOURCE = (3840, 2160)
RENDITIONS = {"1080p": (1920, 1080, 4, 8), "720p": (1280, 720, 2, 16)}


def run(ctx, frame_of, first, count, q, fmt, src_size, log=None, tables=None):
    inflight = deque()
    stages = ctx.stages

    def retire():
        t = inflight.popleft()
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
        inflight.append(ctx.submit(frame_of(f), f, f > 0, q, on_device=True, fmt=fmt, src_size=src_size))
    while inflight:
        retire()


def leg(cairo_amd, w, h, ring, q, batch, warm, timed, frame_of, fmt, src_size, check):
    ctx = cairo_amd.Context(w, h, ring)
    ctx.set_batch(batch)
    ctx.set_outputs(cairo_amd.OUT_FEED)
    run(ctx, frame_of, 0, warm, q, fmt, src_size)
    ctx.sync()
    done = []
    t0 = time.perf_counter()
    run(ctx, frame_of, warm, timed, q, fmt, src_size, log=done)
    ctx.sync()
    el = time.perf_counter() - t0
    out = {"value": round(w * h * timed / el / 1e6, 3), "ms_per_frame": round(el * 1e3 / timed, 4)}
    if timed > batch:  # without the first launch's fill and the last launch's tail
        st = done[-1] - done[batch - 1]
        out["steady_value"] = round(w * h * (timed - batch) / st / 1e6, 3)
    tables = []
    if check:
        ctx.reset()
        ctx.set_outputs(cairo_amd.OUT_FEED)
        run(ctx, frame_of, 0, check, q, fmt, src_size, tables=tables)
    ctx.close()
    return out, tables


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rendition", default="1080p", choices=sorted(RENDITIONS))
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--pool", type=int, default=64, help="distinct resident frames per leg, cycled")
    p.add_argument("--check-frames", type=int, default=48)
    p.add_argument("--only", default="", help="comma list of legs to run (rgb24, nv12; default both)")
    p.add_argument("--out", default="", help="also write the JSON line to this file")
    a = p.parse_args()
    import torch  # device memory only; before the library starts HIP

    torch.cuda.set_device(0)
    import cairo_amd

    sw, sh = SOURCE
    w, h, ring, q = RENDITIONS[a.rendition]
    batch = cairo_amd.default_batch(w, h)
    warm, timed = a.warmup * batch, a.steps * batch
    pool_n = max(2 * batch, a.pool)
    with ThreadPoolExecutor(8) as pool:
        rgb = list(pool.map(lambda f: cairo_amd.make_band4(sw, sh, f), range(pool_n)))
    res = {"source": list(SOURCE), "rendition": a.rendition, "width": w, "height": h, "ring": ring, "quality": q,
           "batch": batch, "warmup_frames": warm, "timed_frames": timed, "pool_frames": pool_n, "unit": "Mpix/s",
           "legs": {}, "tables_equal_prescaled": {}}
    names = {cairo_amd.FMT_RGB24: "rgb24", cairo_amd.FMT_NV12: "nv12"}
    only = [s for s in a.only.split(",") if s]
    for fmt, name in names.items():
        if only and name not in only:
            continue
        big = [f.reshape(-1) if fmt == cairo_amd.FMT_RGB24 else yuv_frame(cairo_amd, f, fmt) for f in rgb]
        nb_small = cairo_amd.frame_layout(fmt, w, h)[0]
        small = [cairo_amd.kat_scale(f, fmt, SOURCE, w, h)[:nb_small] for f in big]
        tables = {}
        for tag, frames, src_size in (("prescaled", small, None), ("scaled_submit", big, SOURCE)):
            nb = frames[0].nbytes
            dev = torch.empty((pool_n, nb), dtype=torch.uint8, device="cuda")
            for i, f in enumerate(frames):
                dev[i].copy_(torch.from_numpy(np.ascontiguousarray(f)))
            torch.cuda.synchronize()
            base = dev.data_ptr()
            out, tables[tag] = leg(cairo_amd, w, h, ring, q, batch, warm, timed, lambda f: base + (f % pool_n) * nb,
                                   fmt, src_size, a.check_frames)
            out["source_bytes_per_frame"] = nb
            res["legs"][f"{name}_{tag}"] = out
            del dev
            torch.cuda.empty_cache()
            print(f"[bench_scale] {name} {tag}: {out}", file=sys.stderr, flush=True)
        x, y = tables["prescaled"], tables["scaled_submit"]
        res["tables_equal_prescaled"][name] = len(x) == len(y) and all(np.array_equal(i, j) for i, j in zip(x, y))
        pa, pb = res["legs"][f"{name}_prescaled"], res["legs"][f"{name}_scaled_submit"]
        res["legs"][f"{name}_scaled_vs_prescaled_pct"] = round(100.0 * (pb["value"] / pa["value"] - 1.0), 3)
    res["ok"] = all(res["tables_equal_prescaled"].values())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
