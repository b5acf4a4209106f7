#!/usr/bin/env python3
"""What the closed loop costs: the stand-alone retarget call at the real shape, and a C3 drag edit run plain, tracked, closed-loop
and closed-loop with a stop that never fires.

  python tools/closed_loop_bench.py [--reps 4] [--warmup 1] [--call-reps 200] [--skip-edit]

Call: DragKernels.retarget_raw (ishap_drag_batch_retarget with E = 1: one launch of one 1024-thread workgroup) on prepared buffers at W = 64,
ld = 512, r = 12, voxel = 2 / 256, for 1 / 4 / 16 handles with a lead of 2 voxels, between two device events (median of `call-reps`
calls after 10 warm-up calls), and as the time per call of 50 calls enqueued back to back between two events
(`burst_ms_per_call`: the larger of the device's time per call and the host's time to enqueue one).  Next to them the lattice
tuples the workgroup marks and the bytes of LDS it holds.
Edits: one warm-up of each kind, then `reps` timed edits of each kind, interleaved (plain, tracked, closed, stop, plain, ...) so
that drift hits all; a device synchronise before each clock reading, as in bench.py (its shape, weights and handles).  `closed`
is closed_loop=True; `stop` is closed_loop={"stop": True, "arrive": 0.0}: the same device work plus the pinned copy, the event and
the host's wait for the event of two steps ago, with a flag that never fires -- its difference to `closed` is what the lag-2
wait costs the host.  Prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from track_bench import BURST, event_ms  # noqa: E402  (tools/ is this script's own directory)


def call_times(device, reps):
    from ishapediting_amd.drag_utils import DragKernels, feat_channel_map
    W, ld, r, voxel, step = 64, 512, 12, 2.0 / 256, 2.0
    gen = torch.Generator().manual_seed(5)
    out = {"W": W, "ld": ld, "r": r, "voxel": voxel, "step": step, "calls": []}
    for B in (1, 4, 16):
        src = torch.rand(B, 3, generator=gen) * 1.2 - 0.6
        tgt = src + (torch.rand(B, 3, generator=gen) - 0.5) * 0.3
        dk = DragKernels(device, W, ld, feat_channel_map(ld), r, voxel)
        dk.setup(src.numpy(), tgt.numpy(), 0.4)
        K = torch.randint(-3, 4, (B, 3), generator=gen).to(device=device, dtype=torch.int32)
        dk.retarget(K, step, 1.0)
        ptrs = (K.data_ptr(), dk.goals.data_ptr(), dk.remaining.data_ptr(), dk.arrived.data_ptr(), dk.done.data_ptr(), step, 1.0)
        t = event_ms(lambda: dk.retarget_raw(*ptrs), 10, reps)

        def burst(n=BURST):
            for _ in range(n):
                dk.retarget_raw(*ptrs)
        t["burst_ms_per_call"] = round(event_ms(burst, 2, max(3, reps // BURST))["median_ms"] / BURST, 4)
        out["calls"].append({"handles": B, **t, "workgroups": 1, "threads": 1024, "lattice_tuples": 6 * (2 * r + 1) ** 2 * B,
                             "lds_bytes": 3 * W * W, "bytes_stored": 3 * W * W + 24 * B})
    return out


KINDS = (("plain", {}), ("tracked", {"track": True}), ("closed", {"closed_loop": True}),
         ("stop", {"closed_loop": {"stop": True, "arrive": 0.0}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--call-reps", type=int, default=200)
    ap.add_argument("--skip-edit", action="store_true", help="time the stand-alone call only")
    a = ap.parse_args()
    from ishapediting_amd import synthetic
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    torch.manual_seed(bench.RNG_SEED)
    np.random.seed(bench.RNG_SEED)
    res = {"metric": "closed-loop drag", "device": torch.cuda.get_device_name(device), "call": call_times(device, a.call_reps)}
    if not a.skip_edit:
        ds = bench.make_dragstuff(device, 1234)
        ds.update_latent_params(img=synthetic.latent(0))
        src, tgt = synthetic.handles(bench.HANDLES, seed=7)
        stops = {}

        def edit(kind, kw):
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in ds.training(src, tgt, scale=1200, cof=0.4, **kw):       # bench.one_edit's arguments
                pass
            torch.cuda.synchronize()
            stops[kind] = ds.last_stop
            return time.time() - t0
        for _ in range(a.warmup):
            for kind, kw in KINDS:
                edit(kind, kw)
        times = {kind: [] for kind, _ in KINDS}
        for _ in range(a.reps):
            for kind, kw in KINDS:
                times[kind].append(edit(kind, kw))
        tr = ds.last_track
        res["edit"] = {"guided_steps": bench.GUIDED_STEPS, "res": bench.RES, "handles": bench.HANDLES, "reps": a.reps, "warmup": a.warmup,
                       **{f"{kind}_s": [round(t, 4) for t in times[kind]] for kind, _ in KINDS},
                       **{f"{kind}_median_s": round(float(np.median(times[kind])), 4) for kind, _ in KINDS},
                       "stop_fired": stops["stop"], "tracked_rows": len(tr["steps"]),
                       "remaining_voxels_first": [round(float(v), 3) for v in tr["remaining"][0]],
                       "remaining_voxels_after": [round(float(v), 3) for v in tr["remaining_after"]]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
