#!/usr/bin/env python3
"""What the scaled tensor submit's kernel costs (include/cairo_amd.h
cairo_ctx_submit_tensor_scaled), from a kernel trace.

Run mode (under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR
-o run -- python tools/bench_tensor_scale.py`, a run of its own, no counters):
resident 3840x2160 tensors, a pool larger than the Infinity Cache, one frame
per launch, in phases of `--frames` submits that the parse mode finds again by
their order:

  fused     k_tensor_scale_batch   f16 CHW -> 1920x1080, f16 CHW -> 1280x720,
                                   f32 HWC -> 1920x1080, f32 HWC -> 1280x720
  baseline  k_tensor_pack_batch    f16 CHW, f32 HWC into a 3840x2160 context (what
                                   a caller without the fused kernel runs first)
            k_scale_batch          the packed RGB24 frame -> 1920x1080, -> 1280x720

Parse mode (`--parse DIR`): per phase the median and minimum kernel duration
without the first `--skip` launches, the fused kernel's source bandwidth, and
fused against pack + scale.  Prints one JSON line.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, RING, Q = 3840, 2160, 4, 16
RUNGS = ((1920, 1080), (1280, 720))
SOURCES = (("f16_chw", 2), ("f32_hwc", 4))  # name, element size


def run(a):
    import torch  # before the library starts HIP; submit_tensor finds it in sys.modules

    torch.cuda.set_device(0)
    import cairo_amd

    rgb = [cairo_amd.make_band4(W, H, f) for f in range(a.pool)]
    u8 = torch.stack([torch.from_numpy(f) for f in rgb]).to("cuda")  # (pool, H, W, 3)
    pools = {"f16_chw": u8.permute(0, 3, 1, 2).to(torch.float32).div(255.0).to(torch.float16).contiguous(),
             "f32_hwc": u8.to(torch.float32).div(255.0).contiguous()}
    torch.cuda.synchronize()

    def phase(ctx, submit):
        for f in range(a.frames):
            t = submit(ctx, f)
            ctx.wait(t, copy=False)
            ctx.release(t)
        ctx.sync()

    def context(w, h):
        ctx = cairo_amd.Context(w, h, RING, stages=4)
        ctx.set_batch(1)
        ctx.set_outputs(cairo_amd.OUT_FEED)
        return ctx

    # fused: one context per rendition, the phases in the order the parse expects
    ctxs = {r: context(*r) for r in RUNGS}
    for name, _ in SOURCES:
        for r in RUNGS:
            phase(ctxs[r], lambda ctx, f, p=pools[name]: ctx.submit_tensor(p[f % a.pool], f, f > 0, Q, sync=False,
                                                                           scaled=True))
    # baseline, second half: the packed frame through the scaled submit
    nb = 3 * W * H
    for r in RUNGS:
        phase(ctxs[r], lambda ctx, f: ctx.submit(u8.data_ptr() + (f % a.pool) * nb, f, f > 0, Q, on_device=True,
                                                 src_size=(W, H)))
    for c in ctxs.values():
        c.close()
    # baseline, first half: the tensor packed at full size
    big = context(W, H)
    for name, _ in SOURCES:
        phase(big, lambda ctx, f, p=pools[name]: ctx.submit_tensor(p[f % a.pool], f, f > 0, Q, sync=False))
    big.close()
    print(json.dumps({"frames_per_phase": a.frames, "pool": a.pool}))
    return 0


def parse(a):
    files = glob.glob(os.path.join(a.parse, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {a.parse}")
    rows = list(csv.DictReader(open(files[0])))

    def phases(kernel, names):
        d = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) for r in rows
                   if kernel in r["Kernel_Name"])
        if len(d) != a.frames * len(names):
            raise SystemExit(f"{kernel}: {len(d)} dispatches, expected {a.frames * len(names)}")
        out = {}
        for i, n in enumerate(names):
            us = [x[1] / 1e3 for x in d[i * a.frames + a.skip:(i + 1) * a.frames]]
            out[n] = {"median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "launches": len(us)}
        return out

    rung = lambda r: f"{r[0]}x{r[1]}"  # noqa: E731
    fused = phases("k_tensor_scale_batch", [f"{s}->{rung(r)}" for s, _ in SOURCES for r in RUNGS])
    pack = phases("k_tensor_pack_batch", [s for s, _ in SOURCES])
    scale = phases("k_scale_batch", [f"rgb24->{rung(r)}" for r in RUNGS])
    res = {"source": f"{W}x{H}", "frames_per_phase": a.frames, "skipped": a.skip, "fused": fused, "pack": pack,
           "scale": scale, "compare": {}}
    for s, es in SOURCES:
        for r in RUNGS:
            k = f"{s}->{rung(r)}"
            src_bytes = 3 * W * H * es
            f = fused[k]["median_us"]
            two = pack[s]["median_us"] + scale[f"rgb24->{rung(r)}"]["median_us"]
            fused[k]["source_GB_per_s"] = round(src_bytes / f / 1e3, 1)
            res["compare"][k] = {"fused_us": f, "pack_plus_scale_us": round(two, 2), "fused_over_two": round(f / two, 3)}
    print(json.dumps(res))
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=12, help="submits per phase")
    p.add_argument("--skip", type=int, default=2, help="parse: launches of each phase left out (warm-up)")
    p.add_argument("--pool", type=int, default=8, help="distinct resident 4K frames per source, cycled")
    p.add_argument("--parse", default="", help="directory of a kernel trace of a run with the same --frames")
    a = p.parse_args()
    return parse(a) if a.parse else run(a)


if __name__ == "__main__":
    sys.exit(main())
