"""Steady-state time accounting of the engine's workers (diagnostic).

Needs a library built with CAIRO_ACCT=1 (tools/build_variant.sh acct
-DCAIRO_ACCT=1): --lib variants/ab/acct.so loads it in place of
cairo_amd/_lib/libcairo_amd.so, which stays untouched.
Runs bench.py's timed configuration (default frames per launch, overlapping
launches, feed outputs, frames resident in HBM), zeroes the counters after the
warm-up and prints where the row coders' and row helpers' time goes, per
macroblock / per inter group, summed over every task of the measured launches
(kernels.h Acct).
usage: python tools/acct.py [--config 4k] [--content band4] [--steps 10] [--warmup 3] [--lib PATH]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="4k", choices=sorted(bench.CONFIGS))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--helpers", type=int, default=0, help="helper workgroups of a launch (0 = default)")
    ap.add_argument("--content", default="band4", choices=["band4", "noise", "static"], help="bench.py's content kinds")
    ap.add_argument("--lib", default="", help="the accounting build to load instead of the in-tree library")
    a = ap.parse_args()
    import numpy as np
    import torch

    import cairo_amd

    if a.lib:
        cairo_amd.LIB_PATH = os.path.abspath(a.lib)
    w, h, ring, q, _ = bench.CONFIGS[a.config]
    batch = cairo_amd.default_batch(w, h)
    warm, timed = a.warmup * batch, a.steps * batch
    n = warm + timed
    pool = bench.content_pool(a.content, n)  # distinct resident frames; frame f is frame f % pool
    frames = torch.empty((pool, h, w, 3), dtype=torch.uint8, device="cuda:0")
    for f in range(pool):
        frames[f].copy_(torch.from_numpy(bench.content_frame(a.content, w, h, f)))
    torch.cuda.synchronize()
    base, stride = frames.data_ptr(), w * h * 3
    ctx = cairo_amd.Context(w, h, ring)
    ctx.set_outputs(cairo_amd.OUT_FEED)
    ctx.set_debug(32)
    if a.helpers:
        ctx.set_helpers(a.helpers)
    bench.run_hot_path(ctx, lambda f: base + (f % pool) * stride, 0, warm, q, ctx.stages)
    ctx.sync()
    ctx.read_acct(reset=True)
    t0 = time.perf_counter()
    bench.run_hot_path(ctx, lambda f: base + (f % pool) * stride, warm, timed, q, ctx.stages)
    ctx.sync()
    el = time.perf_counter() - t0
    c = ctx.read_acct()
    ctx.close()
    us = lambda ticks: ticks / 100.0  # noqa: E731  (10 ns ticks)
    mbs = max(c["coder_mbs"], 1)
    groups = max(c["helper_tasks"] * ((w + 63) // 64), 1)
    parts = ("group_wait", "window", "search", "inter", "xform", "publish", "drain", "vm0", "records", "prebarrier",
             "store_tail")
    coder = {k: round(us(c["coder_" + k]) / mbs, 3) for k in ("total",) + parts}
    coder["rest"] = round(coder["total"] - sum(coder[k] for k in parts), 3)
    coder["dequeue_per_task"] = round(us(c["coder_dequeue"]) / max(c["coder_tasks"], 1), 2)
    # "xform" by macroblock kind: the copy macroblocks' phase (the output_cache carry, where the coder does
    # it) and the coded ones' (the transform chain), each per macroblock of its kind, and the kinds' shares
    kinds = max(c["coder_copy_mbs"] + c["coder_coded_mbs"], 1)
    coder["xform_by_kind"] = {
        "copy_us_per_copy_mb": round(us(c["coder_xform_copy"]) / max(c["coder_copy_mbs"], 1), 3),
        "coded_us_per_coded_mb": round(us(c["coder_xform_coded"]) / max(c["coder_coded_mbs"], 1), 3),
        "copy_share": round(c["coder_copy_mbs"] / kinds, 4),
        "copy_us_per_mb": round(us(c["coder_xform_copy"]) / kinds, 3),
        "coded_us_per_mb": round(us(c["coder_xform_coded"]) / kinds, 3)}
    # inside "search": thread 0's wave per stage phase (evaluation + LDS stores, barrier, LDS reads + replay)
    coder["search_phases"] = {k: round(us(c[k]) / mbs, 3) for k in
                              ("search_eval", "search_barrier", "search_select", "subpel_eval", "subpel_barrier",
                               "subpel_select")}
    # evaluation passes (one barrier each) per macroblock: stage 0's, then 2..4 for stages 1-4 (5 = no
    # speculated stage was ever reused), and the share of macroblocks at each count
    coder["search_passes"] = {"per_mb": round(c["search_passes"] / mbs, 3)}
    coder["search_passes"].update({k: round(c["search_mbs_" + k] / mbs, 4) for k in ("2pass", "3pass", "4pass")})
    # the prologue (inside "rest" and "records"): macroblock start to the fresh granule's load issued, per
    # macroblock, and from there to the record loads issued, per macroblock that is not a group start (at a
    # group start they go out after the search)
    in_group = max(mbs - c["coder_tasks"] * ((w + 63) // 64), 1)
    coder["prologue"] = {"to_fresh_load": round(us(c["coder_prologue_fresh"]) / mbs, 3),
                         "to_record_loads_in_group": round(us(c["coder_prologue_records"]) / in_group, 3)}
    helper = {k: round(us(c["helper_" + k]) / groups, 3) for k in ("total", "wait", "deblock", "search", "catchup")}
    helper["rest"] = round(helper["total"] - sum(helper[k] for k in ("wait", "deblock", "search", "catchup")), 3)
    helper["dequeue_per_task"] = round(us(c["helper_dequeue"]) / max(c["helper_tasks"], 1), 2)
    helper["carry"] = round(us(c["helper_carry"]) / groups, 3)  # first load .. last store issued; inside "rest"
    # a searched inter task's entry to its first window DMA (inside "search"), per searched task
    helper["group_start_per_searched_task"] = round(us(c["helper_group_start"]) / max(c["searched_tasks"], 1), 3)
    # the group start by reference and by searched / not: a task's entry to its first window
    # DMA, or to its record stores when nothing searches, per task of that kind; what the wait's flag said for
    # the tasks that needed it; the groups in which no task searched (a library from before §4.12 has none of
    # these counters and reads zeros)
    if "idle_groups" in c:
        ref1_searched = c["searched_tasks"] - c["older_searched"]
        asked = max(c["flag_set"] + c["fallback_polls"], 1)
        helper["group_start"] = {
            "older_searched_us": round(us(c["start_older_searched"]) / max(c["older_searched"], 1), 3),
            "ref1_searched_us": round(us(c["start_ref1_searched"]) / max(ref1_searched, 1), 3),
            "older_idle_us": round(us(c["start_older_idle"]) / max(c["older_idle"], 1), 3),
            "ref1_idle_us": round(us(c["start_ref1_idle"]) / max(c["ref1_idle"], 1), 3),
            "tasks": {"older_searched": c["older_searched"], "ref1_searched": ref1_searched,
                      "older_idle": c["older_idle"], "ref1_idle": c["ref1_idle"]},
            "flag_set_frac": round(c["flag_set"] / asked, 4),
            "fallback_polls_frac": round(c["fallback_polls"] / asked, 4),
            "fallback_found_full_frac": round(c["fallback_full"] / max(c["fallback_polls"], 1), 4),
            "lvl2_runs_per_searched_task": round(c["lvl2_runs"] / max(c["searched_tasks"], 1), 4),
            "idle_group_frac": round(c["idle_groups"] / groups, 4),
            "idle_group_us": round(us(c["idle_group_time"]) / max(c["idle_groups"], 1), 3)}
    helper["deblock_phases"] ={k: round(us(c[k]) / groups, 3) for k in ("db_inputs", "db_filter", "db_write")}
    helper["chunks_per_group"] = round(c["helper_chunks"] / groups, 3)
    mb = 1e6
    traffic = {k: round(c[k] / timed / mb, 2) for k in
               ("win_bytes", "win_spec_unused_bytes", "zero_mv_bytes", "gran_poll_bytes", "rec_poll_bytes",
                "carry_bytes")}
    traffic["unit"] = "MB per frame (requested)"
    traffic["searched_task_frac"] = round(c["searched_tasks"] / max(c["inter_tasks"], 1), 3)
    traffic["win_stages_per_frame"] = round(c["win_stages"] / timed, 1)
    out = {"config": a.config, "content": a.content, "timed_frames": timed, "mpix_s": round(w * h * timed / el / 1e6, 1),
           "coder_us_per_mb": coder, "helper_us_per_group": helper, "traffic": traffic, "raw": c}
    print(json.dumps(out))
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
