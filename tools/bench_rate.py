#!/usr/bin/env python3
"""Hot-path rate with the target-bitrate controller on (cairo_ctx_set_rate;
DESIGN.md §4.20) against the same build with it off.

One process, one context per leg, the plain bench run's shape (as
tools/bench_metrics.py): tight RGB24 frames resident in HBM, feed outputs, the
library's default batch, `--warmup` untimed launches and `--steps` timed ones.
Legs: off; on with the quality pinned (qmin = qmax = q0 = the configuration's
quality, so the engine's work is the off leg's and the difference is what the
controller costs: one read of each frame's feed and two small kernels per
launch, plus one more behind the convert); off once more (the session's
drift); on and free, aiming at the pinned leg's mean estimated bits per frame.
A leg with the controller on reads every frame's record (Context.frame_rate)
as a caller would.

Prints one JSON line.  The resident pool is `--pool` distinct frames, cycled,
so a rate here is not bench.py's headline: the figures are for comparing the
legs with each other.

usage: python tools/bench_rate.py [--config 4k] [--steps 20] [--warmup 5]
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


def run(ctx, frame_of, first, count, q, rated, log=None, seen=None):
    inflight = deque()
    stages = ctx.stages

    def retire():
        f, t = inflight.popleft()
        ctx.wait(t, copy=False)
        if rated:
            r = ctx.frame_rate(t)
            if seen is not None:
                seen.append(r)
        ctx.release(t)
        if log is not None:
            log.append(time.perf_counter())

    for f in range(first, first + count):
        if len(inflight) == stages:
            retire()
        inflight.append((f, ctx.submit(frame_of(f), f, f > 0, q, on_device=True)))
    while inflight:
        retire()


def leg(cairo_amd, w, h, ring, q, batch, warm, timed, frame_of, rate):
    ctx = cairo_amd.Context(w, h, ring)
    ctx.set_batch(batch)
    ctx.set_outputs(cairo_amd.OUT_FEED)
    if rate:
        ctx.set_rate(**rate)
    run(ctx, frame_of, 0, warm, q, bool(rate))
    ctx.sync()
    done, seen = [], []
    t0 = time.perf_counter()
    run(ctx, frame_of, warm, timed, q, bool(rate), log=done, seen=seen)
    ctx.sync()
    el = time.perf_counter() - t0
    ctx.close()
    out = {"rate": rate, "value": round(w * h * timed / el / 1e6, 3), "ms_per_frame": round(el * 1e3 / timed, 4)}
    if timed > batch:  # without the first launch's fill and the last launch's tail
        out["steady_value"] = round(w * h * (timed - batch) / (done[-1] - done[batch - 1]) / 1e6, 3)
    if seen:
        out["mean_quality"] = round(float(np.mean([r["quality"] for r in seen])), 3)
        out["mean_est_bits"] = round(float(np.mean([r["est_bits"] for r in seen])), 1)
        out["mean_feed_bits"] = round(float(np.mean([r["feed_bits"] for r in seen])), 1)
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
    frame_of = lambda f: base + (f % pool_n) * nb  # noqa: E731
    pinned = dict(target_bits=1 << 20, q0=q, qmin=q, qmax=q, window=32)
    for name, rate in (("off", None), ("on_pinned", pinned), ("off_again", None), ("on_free", "free")):
        if rate == "free":
            target = int(min(max(res["legs"]["on_pinned"]["mean_est_bits"], 1), 1 << 28))
            rate = dict(target_bits=target, q0=q, qmin=1, qmax=31, window=2 * batch)
        out = leg(cairo_amd, w, h, ring, q, batch, warm, timed, frame_of, rate)
        res["legs"][name] = out
        print(f"[bench_rate] {name}: {out}", file=sys.stderr, flush=True)
    off = res["legs"]["off"]["value"]
    for name in ("on_pinned", "off_again", "on_free"):
        res["legs"][name]["vs_off_percent"] = round(100.0 * (res["legs"][name]["value"] / off - 1.0), 2)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
