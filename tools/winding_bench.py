#!/usr/bin/env python3
"""Timing of the generalized winding number (ishapediting_amd/mesh.py, csrc/winding.hip; not part of bench.py): inside /
outside of 200 000 points against the 256^3 sphere mesh (~300 k triangles) by ray parity and by winding number, the same
queries against a 100 000-point oriented cloud, the cloud's k = 8 areas, and cloud_to_mesh at 128^3 and 256^3.  Prints one
JSON line of milliseconds (median of --reps after a warm-up; cloud_to_mesh: one run each, it is long; host clock around
calls that end in a device synchronise).

    python tools/winding_bench.py [--reps 5] [--skip-mesh-256]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warm=True):
    import torch
    if warm:
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
    ap.add_argument("--queries", type=int, default=200_000)
    ap.add_argument("--cloud-points", type=int, default=100_000)
    ap.add_argument("--skip-mesh-256", action="store_true", help="leave out cloud_to_mesh at 256^3 (1.7e12 pairs)")
    a = ap.parse_args()
    import torch
    from ishapediting_amd.mesh import (cloud_areas, cloud_to_mesh, cloud_winding_number, extract_surface, mesh_occupancy,
                                       mesh_winding_number)
    dev = torch.device("cuda", 0)
    res, r = 256, 90.4
    ax = torch.arange(res, dtype=torch.float32, device=dev) - (res - 1) / 2
    vol = r - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    v, f = extract_surface(vol)
    v = (v / (res - 1) * 2 - 1).contiguous()
    g = torch.Generator().manual_seed(0)
    pts = (torch.rand((a.queries, 3), generator=g) * 2 - 1).to(dev)
    # Fibonacci sphere of radius 0.7 with outward normals
    i = torch.arange(a.cloud_points, dtype=torch.float64) + 0.5
    z = 1 - 2 * i / a.cloud_points
    phi = i * math.pi * (3 - math.sqrt(5))
    s = torch.sqrt(1 - z * z)
    nrm = torch.stack([s * torch.cos(phi), s * torch.sin(phi), z], dim=1).float().to(dev).contiguous()
    cloud = (0.7 * nrm).contiguous()
    areas = cloud_areas(cloud)
    out = {"triangles": int(f.shape[0]), "queries": a.queries, "cloud_points": a.cloud_points,
           "occupancy_parity_ms": timed(lambda: mesh_occupancy(v, f, pts), a.reps),
           "occupancy_winding_ms": timed(lambda: mesh_occupancy(v, f, pts, method="winding"), a.reps),
           "mesh_winding_number_ms": timed(lambda: mesh_winding_number(v, f, pts), a.reps),
           "cloud_winding_number_ms": timed(lambda: cloud_winding_number(cloud, nrm, pts, areas), a.reps),
           "cloud_areas_k8_ms": timed(lambda: cloud_areas(cloud), a.reps),
           "cloud_to_mesh_128_ms": timed(lambda: cloud_to_mesh(cloud, nrm, res=128), 1, warm=False)}
    if not a.skip_mesh_256:
        out["cloud_to_mesh_256_ms"] = timed(lambda: cloud_to_mesh(cloud, nrm, res=256), 1, warm=False)
    agree = float((mesh_occupancy(v, f, pts) == mesh_occupancy(v, f, pts, method="winding")).float().mean())
    out["parity_winding_agreement"] = agree
    print(json.dumps({k: (round(x, 3) if isinstance(x, float) and k.endswith("_ms") else x) for k, x in out.items()}))


if __name__ == "__main__":
    main()
