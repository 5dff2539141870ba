"""One member of a two-process group on one device, reporting which engine its
launches ran (run by tests/test_gpu_engine_variants.py, GPU test infrastructure).

The group is set up as tests/group_worker.py's xproc mode sets one up: this
process is member RANK of N, its buffers shared through IPC handles
(fine-grained memory, system-scope hand-offs), records exchanged over gloo.
Members in different processes make every frame's view sys, so every launch
must take the general engine: cairo_ctx_engine_variant is sampled after each
launch is enqueued (a submit that fills the batch, and the final flush).
Every frame's block table and coefficients and the final reconstructions are
compared with the oracle's.  Prints one JSON line; exit status 0 = bit-exact.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import cairo_amd  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests.group_worker import oracle_stream, table_mismatch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=2)
    ap.add_argument("--rank", type=int, default=0)
    ap.add_argument("--store", required=True)
    ap.add_argument("--w", type=int, default=352)
    ap.add_argument("--h", type=int, default=288)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--q", type=int, default=16)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--batch", type=int, default=2)
    a = ap.parse_args()
    w, h, ring, q, F, N = a.w, a.h, a.ring, a.q, a.frames, a.members
    ref, final = oracle_stream(w, h, ring, q, F, 0)
    bad, variants = [], []
    import torch.distributed as dist

    dist.init_process_group("gloo", init_method=f"file://{a.store}", rank=a.rank, world_size=N)
    ctx = cairo_amd.Context(w, h, ring)
    ctx.set_batch(a.batch)
    ctx.set_workgroups(max(1, ctx.max_workgroups() // N))  # N members share the device
    recs = [None] * N
    dist.all_gather_object(recs, ctx.peer_info(cross_device=True))
    ctx.join_group(a.rank, recs)
    mine = [t for t in range(F) if t % N == a.rank]
    frames = {t: orc.make_frame(w, h, t) for t in mine}
    dist.barrier()  # every member ready: in-kernel waits on the others are bounded (2 s)
    tk = {}
    for k, t in enumerate(mine):
        tk[t] = ctx.submit(frames[t], t, not ref[t][0], q)
        if (k + 1) % a.batch == 0:  # the batch is full: this submit enqueued a launch
            variants.append(ctx.engine_variant())
    if len(mine) % a.batch:
        ctx.flush()
        variants.append(ctx.engine_variant())
    for t in mine:
        out = ctx.wait(tk[t])
        if table_mismatch(out.table, ref[t][1]) or any(
                not np.array_equal(x, y) for x, y in zip((out.coef_y, out.coef_u, out.coef_v), ref[t][2])):
            bad.append(t)
        ctx.release(tk[t])
    ctx.sync()
    dist.barrier()  # every member's frames encoded: their pushes into this member's mirrors are done
    for t, planes in final.items():  # its own frames, and the mirrors other members pushed here
        lay = cairo_amd.group_layout(t, N, ring, ctx.stages, mirror=True)
        if lay["member"] == a.rank or a.rank in lay["readers"]:
            got = ctx.read_planes(2 + lay["recon_slot"])
            if any(not np.array_equal(x, y) for x, y in zip(got, planes)):
                bad.append(f"recon {t}" + ("" if lay["member"] == a.rank else " (mirror)"))
    dist.barrier()  # the others may still read this member's buffers until they finish
    ctx.close()
    dist.destroy_process_group()
    print(json.dumps({"rank": a.rank, "members": N, "frames": F, "launches": len(variants), "variants": variants,
                      "mismatched": bad}), flush=True)
    sys.exit(1 if bad or any(v != 1 for v in variants) else 0)


if __name__ == "__main__":
    main()
