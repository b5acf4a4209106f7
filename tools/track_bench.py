#!/usr/bin/env python3
"""What handle tracking costs: the stand-alone call at the real shape, and a C3 drag edit with tracking on against the same edit
without it.

  python tools/track_bench.py [--reps 3] [--warmup 1] [--call-reps 200] [--skip-edit]

Call: HandleTracker.run_ptr (ishap_drag_track: two launches) on prepared buffers at W = 64, ld = 512, Cc = 170, voxel = 2 / 256,
for 1 / 4 / 16 handles, at the default search (R = 4, rp = 2) and the largest (R = 8, rp = 4), between two device events (median of
`call-reps` calls after 10 warm-up calls), and as the time per call of 50 calls enqueued back to back between two events
(`burst_ms_per_call`).  A call is two short launches: the single-call figure holds the host's enqueue of both behind the first
event, the burst figure is the larger of the device's time per call and the host's time to enqueue one.  Next to them the bytes the
call reads from the taps and the LDS one workgroup holds.
Edits: warm-up steps, then `reps` timed steps of each kind, interleaved (plain, tracked, plain, tracked, ...) so that drift hits
both; a device synchronise before each clock reading, as in bench.py (its shape, weights and handles).  Prints ONE JSON line.
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


def event_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.sort(np.asarray(ms))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms[0]), 4), "max_ms": round(float(ms[-1]), 4), "calls": reps}


BURST = 50       # calls enqueued back to back between two events


def call_times(device, reps):
    from ishapediting_amd.drag_utils import HandleTracker, feat_channel_map
    W, ld, voxel = 64, 512, 2.0 / 256
    gen = torch.Generator().manual_seed(5)
    orig = torch.randn(W * W, ld, generator=gen).half().to(device)
    edit = (orig.float() + 0.3 * torch.randn(W * W, ld, generator=gen).to(device)).half()
    out = {"W": W, "ld": ld, "Cc": int(feat_channel_map(ld).shape[1]), "voxel": voxel, "calls": []}
    for R, rp in ((4, 2), (8, 4)):
        for B in (1, 4, 16):
            tr = HandleTracker(device, W, ld, feat_channel_map(ld), voxel, radius=R, patch=rp)
            tr.setup([(torch.rand(B, 3, generator=gen) * 1.2 - 0.6).numpy()])
            k_in = torch.zeros((B, 3), dtype=torch.int32, device=device)
            k_out, dist, dist0 = torch.empty_like(k_in), torch.empty(B, device=device), torch.empty(B, device=device)
            ptrs = (edit.data_ptr(), orig.data_ptr(), 0, k_in.data_ptr(), k_out.data_ptr(), dist.data_ptr(), dist0.data_ptr())
            t = event_ms(lambda: tr.run_raw(*ptrs), 10, reps)

            def burst(n=BURST):
                for _ in range(n):
                    tr.run_raw(*ptrs)
            t["burst_ms_per_call"] = round(event_ms(burst, 2, max(3, reps // BURST))["median_ms"] / BURST, 4)
            positions = (2 * (R + rp) + 1) ** 2 + (2 * rp + 1) ** 2
            cw = 64 if positions * 64 * 4 <= 65536 else 32 if positions * 32 * 4 <= 65536 else 16
            out["calls"].append({"R": R, "rp": rp, "handles": B, **t, "candidates": (2 * R + 1) ** 3, "chunk_channels": cw,
                                 "workgroups": B * 3 * -(-tr.Cc // cw), "lds_bytes": positions * cw * 4,
                                 "tap_bytes_read": B * 3 * tr.Cc * positions * 4 * 2})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--call-reps", type=int, default=200)
    ap.add_argument("--skip-edit", action="store_true", help="time the stand-alone call only")
    a = ap.parse_args()
    from ishapediting_amd import synthetic
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    torch.manual_seed(bench.RNG_SEED)
    np.random.seed(bench.RNG_SEED)
    res = {"metric": "handle tracking", "device": torch.cuda.get_device_name(device), "call": call_times(device, a.call_reps)}
    if not a.skip_edit:
        ds = bench.make_dragstuff(device, 1234)
        ds.update_latent_params(img=synthetic.latent(0))
        src, tgt = synthetic.handles(bench.HANDLES, seed=7)

        def edit(track):
            kw = {"track": True} if track else {}
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in ds.training(src, tgt, scale=1200, cof=0.4, **kw):       # bench.one_edit's arguments
                pass
            torch.cuda.synchronize()
            return time.time() - t0
        for _ in range(a.warmup):
            edit(False), edit(True)
        times = {False: [], True: []}
        for _ in range(a.reps):
            for r in (False, True):
                times[r].append(edit(r))
        err = ds.handle_error()
        res["edit"] = {"guided_steps": bench.GUIDED_STEPS, "res": bench.RES, "handles": bench.HANDLES, "reps": a.reps, "warmup": a.warmup,
                       "plain_s": [round(t, 4) for t in times[False]], "tracked_s": [round(t, 4) for t in times[True]],
                       "plain_median_s": round(float(np.median(times[False])), 4),
                       "tracked_median_s": round(float(np.median(times[True])), 4),
                       "tracked_rows": len(ds.last_track["steps"]), "error_voxels": [round(float(v), 3) for v in err["error"]],
                       "fraction": [round(float(v), 3) for v in err["fraction"]]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
