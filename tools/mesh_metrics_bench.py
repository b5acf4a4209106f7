#!/usr/bin/env python3
"""Timing of the device mesh metrics (ishapediting_amd/metrics.py; not part of bench.py): calc_implicit_field (signed
distance) of 100 000 points uniform in [-1,1]^3 against the 256^3 sphere mesh (~300 k triangles), and calc_local_distance
with 8 handles x 10 000 points on the same mesh and a deformed copy.  Prints one JSON line of milliseconds (median of
--reps after a warm-up; host clock around calls that end in a device synchronise).

    python tools/mesh_metrics_bench.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--handles", type=int, default=8)
    ap.add_argument("--local-points", type=int, default=10_000)
    a = ap.parse_args()
    import torch
    from ishapediting_amd.mesh import extract_surface
    from ishapediting_amd.metrics import calc_implicit_field, calc_local_distance, mesh_distance
    from ishapediting_amd.mesh import mesh_occupancy
    dev = torch.device("cuda", 0)
    res, r = 256, 90.4
    ax = torch.arange(res, dtype=torch.float32, device=dev) - (res - 1) / 2
    vol = r - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    v, f = extract_surface(vol)
    v = (v / (res - 1) * 2 - 1).contiguous()
    g = torch.Generator().manual_seed(0)
    pts = (torch.rand((a.points, 3), generator=g) * 2 - 1).to(dev)
    vb = (v * torch.tensor([1.1, 1.0, 0.95], device=dev)).contiguous()
    hidx = torch.randint(0, v.shape[0], (a.handles,), generator=g).to(dev)
    ha = v[hidx]
    hb = vb[hidx]
    out = {"triangles": int(f.shape[0]), "points": a.points,
           "implicit_field_sdf_ms": timed(lambda: calc_implicit_field((v, f), pts), a.reps),
           "unsigned_distance_ms": timed(lambda: mesh_distance(v, f, pts, sdf=False), a.reps),
           "occupancy_ms": timed(lambda: mesh_occupancy(v, f, pts), a.reps),
           "local_handles": a.handles, "local_points": a.local_points,
           "local_distance_iou_ms": timed(lambda: calc_local_distance((v, f), (vb, f), ha, hb, 0.1, a.local_points, "IoU"), a.reps)}
    print(json.dumps({k: (round(x, 3) if isinstance(x, float) else x) for k, x in out.items()}))


if __name__ == "__main__":
    main()
