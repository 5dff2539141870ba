#!/usr/bin/env python3
"""CPU simulation of the target-bitrate controller.

Runs the oracle encoder, the host precode and cairo_amd.RateModel over a
sequence of frames cut into launches, exactly as a Context with set_rate does
on the device: launch L is stepped with the estimated bits of the frames of
launch L-2, every frame of a launch is coded at the launch's quality.  It is
the reference the GPU path must equal (tests/test_gpu_rate.py), and where the
gains of the law are justified: no GPU is needed.

    python tools/rate_sim.py --kind band4 --size 352x288 --frames 64 --batch 4 \
        --target 55000 --q0 8 --window 32

prints the quality of every launch and the mean bits per frame (estimate + 80
and real payload + 80).  --fixed Q codes every frame at Q instead (no
controller), for the means a target is chosen from.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import cairo_amd  # noqa: E402
from oracle import oracle as orc  # noqa: E402

STREAM_HEADER_BITS = 14 * 8  # before the first frame's record
FRAME_RECORD_BITS = cairo_amd.RATE_FRAME_RECORD_BITS


def make_frames(kind: str, w: int, h: int, n: int):
    if kind == "band4":
        return [orc.make_frame(w, h, t) for t in range(n)]
    from tests import content

    return [content.make(kind, w, h, t) for t in range(n)]


def launches_of(n: int, batch: int):
    """n frames in launches of `batch`, the last one partial."""
    return [min(batch, n - i) for i in range(0, n, batch)]


def popcount(words: np.ndarray, nbits: int) -> int:
    """Set bits among the first nbits of the LSB-first uint32 words."""
    if not nbits:
        return 0
    return int(np.unpackbits(np.ascontiguousarray(words, dtype="<u4").view(np.uint8), bitorder="little")[:nbits].sum())


def simulate(frames, launches, ring: int = 4, rate: dict | None = None, fixed_q: int | None = None):
    """-> one record per frame: launch, quality, aim, debt (after its launch's
    step), feed_bits, ones, est_bits (estimate + 80), payload_bits and payload
    (the oracle's payload of the frame coded at that quality, without the
    stream header and the frame record).  rate: RateModel's keywords; or
    fixed_q, with no controller (aim and debt 0)."""
    assert sum(launches) == len(frames) and all(n >= 1 for n in launches)
    assert (rate is None) != (fixed_q is None)
    model = cairo_amd.RateModel(**rate) if rate is not None else None
    enc = orc.OracleEncoder(ring)
    out, per_launch, t = [], [], 0
    for L, n in enumerate(launches):
        if model is not None:
            obs = sum(r["est_bits"] for r in per_launch[L - 2]) if L >= 2 else 0
            q, aim, debt = model.step(n, obs), model.aim, model.debt
        else:
            q, aim, debt = fixed_q, 0, 0
        recs = []
        for _ in range(n):
            enc.set_quality(q)
            data, nbits = enc.encode(frames[t])
            head = FRAME_RECORD_BITS + (STREAM_HEADER_BITS if t == 0 else 0)
            wa, ha, _, _ = enc.dims()
            wmb, hmb = wa // 16, ha // 16
            feed, fbits = cairo_amd.precode_slice(enc.block_table(), wmb, hmb, ring, *enc.planes(1))
            ones = popcount(feed, fbits)
            recs.append(dict(launch=L, quality=q, aim=aim, debt=debt, feed_bits=fbits, ones=ones,
                             est_bits=cairo_amd.rate_estimate(fbits, fbits - ones) + FRAME_RECORD_BITS,
                             payload_bits=nbits - head, payload=data[head // 8:]))
            t += 1
        per_launch.append(recs)
        out += recs
    return out


def summary(recs):
    """-> (quality per launch, mean est_bits, mean payload_bits + 80)."""
    qs = []
    for r in recs:
        if r["launch"] == len(qs):
            qs.append(r["quality"])
    return (qs, float(np.mean([r["est_bits"] for r in recs])),
            float(np.mean([r["payload_bits"] + FRAME_RECORD_BITS for r in recs])))


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kind", default="band4")
    ap.add_argument("--size", default="352x288")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--launches", default="", help="launch sizes, e.g. 3,3,2,3,3 (instead of --batch)")
    ap.add_argument("--target", type=int, default=0, help="bits per frame")
    ap.add_argument("--q0", type=int, default=8)
    ap.add_argument("--qmin", type=int, default=1)
    ap.add_argument("--qmax", type=int, default=31)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--fixed", type=int, default=0, help="no controller: every frame at this quality")
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.split("x"))
    launches = [int(x) for x in a.launches.split(",")] if a.launches else launches_of(a.frames, a.batch)
    frames = make_frames(a.kind, w, h, sum(launches))
    if a.fixed:
        recs = simulate(frames, launches, a.ring, fixed_q=a.fixed)
    else:
        if a.target < 1:
            ap.error("--target or --fixed is needed")
        recs = simulate(frames, launches, a.ring,
                        rate=dict(target_bits=a.target, q0=a.q0, qmin=a.qmin, qmax=a.qmax, window=a.window))
    qs, est, real = summary(recs)
    half = recs[len(recs) // 2:]
    print(f"{a.kind} {w}x{h} frames={len(recs)} launches={launches if a.launches else a.batch} "
          + (f"fixed q={a.fixed}" if a.fixed else f"T={a.target} q0={a.q0} q=[{a.qmin},{a.qmax}] W={a.window}"))
    print("q per launch:", " ".join(str(q) for q in qs))
    print(f"mean bits/frame: estimate {est:.0f}, payload {real:.0f}; second half payload {summary(half)[2]:.0f}"
          + ("" if a.fixed else f" ({100.0 * (real / a.target - 1):+.1f} % of target); final debt {recs[-1]['debt']}"))


if __name__ == "__main__":
    main()
