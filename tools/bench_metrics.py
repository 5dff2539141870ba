#!/usr/bin/env python3
"""Hot-path rate with kept reconstructions and per-frame metrics on
(cairo_ctx_set_metrics) against the same build with them off.

One process, one context per leg, the plain bench run's shape (as
tools/bench_pixfmt.py): tight RGB24 frames resident in HBM, feed outputs, the
library's default batch, `--warmup` untimed launches and `--steps` timed ones.
Legs: off, keep only, SSE, SSE + SSIM, and off once more at the end (the
session's drift).  A leg with a metric reads every frame's result
(Context.frame_metrics) as a caller would; the means of the timed frames'
PSNR / SSIM are reported with the rate, and must be equal between the legs
that compute them.

Prints one JSON line.  The resident pool is `--pool` distinct frames, cycled,
so a rate here is not bench.py's headline: the figures are for comparing the
legs with each other.

usage: python tools/bench_metrics.py [--config 4k] [--steps 20] [--warmup 5]
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


def run(ctx, frame_of, first, count, q, metrics, log=None, seen=None):
    inflight = deque()
    stages = ctx.stages

    def retire():
        f, t = inflight.popleft()
        ctx.wait(t, copy=False)
        if metrics:
            m = ctx.frame_metrics(t)
            if seen is not None:
                seen.append(m)
        ctx.release(t)
        if log is not None:
            log.append(time.perf_counter())

    for f in range(first, first + count):
        if len(inflight) == stages:
            retire()
        inflight.append((f, ctx.submit(frame_of(f), f, f > 0, q, on_device=True)))
    while inflight:
        retire()


def leg(cairo_amd, w, h, ring, q, batch, warm, timed, frame_of, flags):
    ctx = cairo_amd.Context(w, h, ring)
    ctx.set_batch(batch)
    ctx.set_outputs(cairo_amd.OUT_FEED)
    if flags:
        ctx.set_metrics(flags=flags)
    metrics = bool(flags & (cairo_amd.METRIC_SSE | cairo_amd.METRIC_SSIM))
    run(ctx, frame_of, 0, warm, q, metrics)
    ctx.sync()
    done, seen = [], []
    t0 = time.perf_counter()
    run(ctx, frame_of, warm, timed, q, metrics, log=done, seen=seen)
    ctx.sync()
    el = time.perf_counter() - t0
    ctx.close()
    out = {"flags": flags, "value": round(w * h * timed / el / 1e6, 3), "ms_per_frame": round(el * 1e3 / timed, 4)}
    if timed > batch:  # without the first launch's fill and the last launch's tail
        out["steady_value"] = round(w * h * (timed - batch) / (done[-1] - done[batch - 1]) / 1e6, 3)
    if seen and seen[0]["psnr_y"] is not None:
        for k in ("psnr_y", "psnr_u", "psnr_v", "psnr_all"):
            out["mean_" + k] = round(float(np.mean([m[k] for m in seen])), 4)
    if seen and seen[0]["ssim_y"] is not None:
        for k in ("ssim_y", "ssim_u", "ssim_v"):
            out["mean_" + k] = round(float(np.mean([m[k] for m in seen])), 6)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--config", default="4k", choices=sorted(CONFIGS))
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--pool", type=int, default=96, help="distinct resident frames, cycled")
    a = p.parse_args()
    import torch  # device memory only; before the library starts HIP

    torch.cuda.set_device(0)
    import cairo_amd

    w, h, ring, q = CONFIGS[a.config]
    batch = cairo_amd.default_batch(w, h)
    warm, timed = a.warmup * batch, a.steps * batch
    pool_n = max(2 * batch, a.pool)
    with ThreadPoolExecutor(8) as pool:
        rgb = list(pool.map(lambda f: cairo_amd.make_band4(w, h, f), range(pool_n)))
    nb = rgb[0].nbytes
    dev = torch.empty((pool_n, nb), dtype=torch.uint8, device="cuda")
    for i, f in enumerate(rgb):
        dev[i].copy_(torch.from_numpy(f.reshape(-1)))
    torch.cuda.synchronize()
    base = dev.data_ptr()
    res = {"config": a.config, "width": w, "height": h, "ring": ring, "quality": q, "batch": batch,
           "warmup_frames": warm, "timed_frames": timed, "pool_frames": pool_n, "unit": "Mpix/s", "legs": {}}
    S, M, K = cairo_amd.METRIC_SSE, cairo_amd.METRIC_SSIM, cairo_amd.KEEP_RECON
    for name, flags in (("off", 0), ("keep", K), ("sse", S), ("sse_ssim", S | M), ("off_again", 0)):
        out = leg(cairo_amd, w, h, ring, q, batch, warm, timed, lambda f: base + (f % pool_n) * nb, flags)
        res["legs"][name] = out
        print(f"[bench_metrics] {name}: {out}", file=sys.stderr, flush=True)
    off = res["legs"]["off"]["value"]
    for name in ("keep", "sse", "sse_ssim", "off_again"):
        res["legs"][name]["vs_off_percent"] = round(100.0 * (res["legs"][name]["value"] / off - 1.0), 2)
    res["ok"] = res["legs"]["sse"].get("mean_psnr_all") == res["legs"]["sse_ssim"].get("mean_psnr_all")
    print(json.dumps(res))
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
