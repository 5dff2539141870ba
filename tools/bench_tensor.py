#!/usr/bin/env python3
"""What tensor frames cost (include/cairo_amd.h cairo_ctx_submit_tensor,
cairo_ctx_decode_frame_tensor).

One process, the plain bench run's shape (frames resident in HBM, feed
outputs, batch 32, `--warmup` untimed launches and `--steps` timed ones,
nothing copied to the host in the timed region).  A 4K q = 16 R = 4 context is
fed four ways at the same launch counts:

  (a) rgb24        resident RGB24 device frames (cairo_ctx_submit);
  (b) f16_tensor   resident float16 CHW tensors in [0, 1] through submit_tensor;
  (c) f32_tensor   the same as float32;
  (d) f16_torch    the float16 tensors converted frame by frame with the usual
                   torch chain (permute, mul, round, clamp, to(uint8),
                   contiguous) and submitted as RGB24: what callers do today.

All four encode the same bits: after timing, the block tables of the first
`--check-frames` frames of each leg are compared with (a)'s.

Then decode: `--decode-frames` frames decoded on a fresh context each way,
  decode_tensor   cairo_ctx_decode_frame_tensor into a float16 CHW tensor;
  decode_torch    cairo_ctx_decode_frame to the host, then H2D and the torch
                  chain (to(float16), div, permute, contiguous) into the same
                  kind of tensor;
both results compared.  Each figure is one run; no spread is taken.

Prints one JSON line.  The resident pool is `--pool` distinct frames, cycled,
so a rate here is not bench.py's headline.

usage: python tools/bench_tensor.py [--steps 20] [--warmup 5] [--only rgb24,f16_tensor]
"""
import argparse
import ctypes
import json
import os
import sys
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, RING, Q, BATCH = 3840, 2160, 4, 16, 32
LEGS = ("rgb24", "f16_tensor", "f32_tensor", "f16_torch")


def run(ctx, submit, first, count, log=None, tables=None):
    inflight = deque()
    stages = ctx.stages

    def retire():
        t, keep = inflight.popleft()
        out = ctx.wait(t, copy=False)
        if tables is not None:
            tb = out.table.copy()
            tb["pad"] = 0
            tables.append(tb)
        ctx.release(t)
        del keep
        if log is not None:
            log.append(time.perf_counter())

    for f in range(first, first + count):
        if len(inflight) == stages:
            retire()
        inflight.append(submit(ctx, f))
    while inflight:
        retire()


def leg(cairo_amd, submit, warm, timed, check):
    ctx = cairo_amd.Context(W, H, RING)
    ctx.set_batch(BATCH)
    ctx.set_outputs(cairo_amd.OUT_FEED)
    run(ctx, submit, 0, warm)
    ctx.sync()
    done = []
    t0 = time.perf_counter()
    run(ctx, submit, warm, timed, log=done)
    ctx.sync()
    el = time.perf_counter() - t0
    out = {"value": round(W * H * timed / el / 1e6, 3), "ms_per_frame": round(el * 1e3 / timed, 4)}
    if timed > BATCH:  # without the first launch's fill and the last launch's tail
        st = done[-1] - done[BATCH - 1]
        out["steady_value"] = round(W * H * (timed - BATCH) / st / 1e6, 3)
    tables = []
    if check:
        ctx.reset()
        ctx.set_outputs(cairo_amd.OUT_FEED)
        run(ctx, submit, 0, check, tables=tables)
    ctx.close()
    return out, tables


def decode_legs(cairo_amd, torch, rgb, n):
    """Encode n frames once (tables and coefficients on the host), then decode
    them each way on a fresh context -> per-leg ms per frame, results equal."""
    enc = cairo_amd.Context(W, H, RING, stages=4)
    recs = []
    for t in range(n):
        out = enc.encode_frame(rgb[t], t, t > 0, Q)
        recs.append((np.ascontiguousarray(out.table).view(np.uint8).copy(),
                     np.concatenate([np.ascontiguousarray(p, dtype=np.int16).ravel()
                                     for p in (out.coef_y, out.coef_u, out.coef_v)])))
    enc.close()
    res, outs = {}, {}
    for name in ("decode_tensor", "decode_torch"):
        ctx = cairo_amd.Context(W, H, RING, stages=2)
        dst = [torch.zeros((3, H, W), dtype=torch.float16, device="cuda") for _ in range(n)]
        host = np.empty((H, W, 3), np.uint8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t, (table, coef) in enumerate(recs):
            if name == "decode_tensor":
                d = cairo_amd.tensor_desc(dst[t], output=True)
                st = ctx.L.cairo_ctx_decode_frame_tensor(ctx.h, table.ctypes.data, coef.ctypes.data, t, d.ptr,
                                                         ctypes.byref(d.c))
            else:
                st = ctx.L.cairo_ctx_decode_frame(ctx.h, table.ctypes.data, coef.ctypes.data, t, host.ctypes.data)
                u8 = torch.from_numpy(host).to("cuda")
                dst[t].copy_(u8.to(torch.float16).div(255.0).permute(2, 0, 1).contiguous())
            assert st == 0, (name, t, st)
        torch.cuda.synchronize()
        res[name] = {"ms_per_frame": round((time.perf_counter() - t0) * 1e3 / n, 4)}
        outs[name] = [x.cpu() for x in dst]
        ctx.close()
        del dst
        torch.cuda.empty_cache()
    res["frames"] = n
    # s / 255 in float32 rounded to float16 (the library) against float16(s) / 255 in float16 (torch's chain)
    res["max_abs_difference"] = max(float((a.float() - b.float()).abs().max())
                                    for a, b in zip(outs["decode_tensor"], outs["decode_torch"]))
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--pool", type=int, default=64, help="distinct resident frames per leg, cycled")
    p.add_argument("--check-frames", type=int, default=48)
    p.add_argument("--decode-frames", type=int, default=8)
    p.add_argument("--only", default="", help="comma list of legs to run (default all)")
    p.add_argument("--out", default="", help="also write the JSON line to this file")
    a = p.parse_args()
    import torch  # before the library starts HIP; submit_tensor finds it in sys.modules

    torch.cuda.set_device(0)
    import cairo_amd

    warm, timed = a.warmup * BATCH, a.steps * BATCH
    pool_n = max(2 * BATCH, a.pool)
    with ThreadPoolExecutor(8) as pool:
        rgb = list(pool.map(lambda f: cairo_amd.make_band4(W, H, f), range(pool_n)))
    res = {"width": W, "height": H, "ring": RING, "quality": Q, "batch": BATCH, "warmup_frames": warm,
           "timed_frames": timed, "pool_frames": pool_n, "unit": "Mpix/s", "legs": {}, "tables_equal_rgb24": {},
           "note": "each leg is one run; no spread taken"}
    only = [s for s in a.only.split(",") if s] or list(LEGS) + ["decode"]
    tables = {}
    for name in LEGS:
        if name not in only:
            continue
        if name == "rgb24":
            dev = torch.empty((pool_n, H, W, 3), dtype=torch.uint8, device="cuda")
            for i, f in enumerate(rgb):
                dev[i].copy_(torch.from_numpy(f))
        else:
            dt = torch.float32 if name == "f32_tensor" else torch.float16
            dev = torch.empty((pool_n, 3, H, W), dtype=dt, device="cuda")
            for i, f in enumerate(rgb):
                dev[i].copy_(torch.from_numpy(f).to("cuda").permute(2, 0, 1).to(torch.float32).div(255.0).to(dt))
        torch.cuda.synchronize()
        nb = dev[0].numel() * dev[0].element_size()
        if name == "rgb24":
            base = dev.data_ptr()
            submit = lambda ctx, f: (ctx.submit(base + (f % pool_n) * nb, f, f > 0, Q, on_device=True), None)  # noqa: E731
        elif name == "f16_torch":
            def submit(ctx, f):
                u8 = dev[f % pool_n].permute(1, 2, 0).mul(255.0).round().clamp(0, 255).to(torch.uint8).contiguous()
                torch.cuda.current_stream().synchronize()  # the chain before the library's launch stream reads it
                return ctx.submit(u8.data_ptr(), f, f > 0, Q, on_device=True), u8
        else:
            # resident and idle: no producer to order (sync=False)
            submit = lambda ctx, f: (ctx.submit_tensor(dev[f % pool_n], f, f > 0, Q, sync=False), None)  # noqa: E731
        out, tables[name] = leg(cairo_amd, submit, warm, timed, a.check_frames)
        out["source_bytes_per_frame"] = nb
        res["legs"][name] = out
        del dev
        torch.cuda.empty_cache()
        print(f"[bench_tensor] {name}: {out}", file=sys.stderr, flush=True)
    if "rgb24" in tables:
        x = tables["rgb24"]
        for name, y in tables.items():
            if name != "rgb24":
                res["tables_equal_rgb24"][name] = len(x) == len(y) and all(np.array_equal(i, j) for i, j in zip(x, y))
                res["legs"][f"{name}_vs_rgb24_pct"] = round(
                    100.0 * (res["legs"][name]["value"] / res["legs"]["rgb24"]["value"] - 1.0), 3)
    if "decode" in only:
        res["decode"] = decode_legs(cairo_amd, torch, rgb, a.decode_frames)
        print(f"[bench_tensor] decode: {res['decode']}", file=sys.stderr, flush=True)
    res["ok"] = all(res["tables_equal_rgb24"].values())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["ok"] else 1


if __name__ == "__main__":
    sys.exit(main())
