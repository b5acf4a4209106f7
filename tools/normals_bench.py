#!/usr/bin/env python3
"""Timing of the front end for clouds without normals (ishapediting_amd/mesh.py, csrc/normals.hip; not part of bench.py):
on Fibonacci-sphere clouds of 10 000 and 100 000 points (radius 0.7) the three device calls one by one -- ishap_cloud_knn at
k = 8 and k = 12, ishap_cloud_normals and ishap_cloud_orient at k = 12 -- next to cloud_areas(k = 8) in the same run, then
estimate_normals(k = 12) end to end and cloud_to_mesh(points) without normals at 128^3.  Prints one JSON line: milliseconds
(median of --reps after one warm-up; cloud_to_mesh: one run after a warm-up at 32^3; host clock around calls that end in a
device synchronise), rounds and seeds per cloud, the share of estimate_normals the orientation rounds take, and how many
estimated normals point against the radius.

    python tools/normals_bench.py [--reps 5] [--sizes 10000 100000]
"""
import argparse
import ctypes as C
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


def fibonacci_sphere(n, radius, dev):
    import torch
    i = torch.arange(n, dtype=torch.float64) + 0.5
    z = 1 - 2 * i / n
    phi = i * math.pi * (3 - math.sqrt(5))
    s = torch.sqrt(1 - z * z)
    nrm = torch.stack([s * torch.cos(phi), s * torch.sin(phi), z], dim=1).float().to(dev).contiguous()
    return (radius * nrm).contiguous(), nrm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--mesh-res", type=int, default=128)
    a = ap.parse_args()
    import torch
    from ishapediting_amd import _lib
    from ishapediting_amd.mesh import cloud_areas, cloud_knn, cloud_to_mesh, estimate_normals
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    out = {"reps": a.reps}
    for n in a.sizes:
        p, radial = fibonacci_sphere(n, 0.7, dev)
        k = 12
        idx, _ = cloud_knn(p, k)
        raw = torch.empty_like(p)
        var = torch.empty(n, dtype=torch.float32, device=dev)
        stream = _lib.stream_ptr(dev)

        def normals():
            _lib.check(L.ishap_cloud_normals(p.data_ptr(), n, idx.data_ptr(), k, raw.data_ptr(), var.data_ptr(), stream))

        normals()
        nbytes = int(L.ishap_cloud_orient_scratch_bytes(n))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        info = (C.c_int * 2)()
        work = torch.empty_like(raw)

        def orient():
            work.copy_(raw)                                # the call orients in place: every repeat starts from the raw normals
            _lib.check(L.ishap_cloud_orient(p.data_ptr(), work.data_ptr(), idx.data_ptr(), n, k, scratch.data_ptr(), nbytes, info,
                                            stream))

        r = {"cloud_areas_k8_ms": timed(lambda: cloud_areas(p, 8), a.reps),
             "cloud_knn_k8_ms": timed(lambda: cloud_knn(p, 8), a.reps),
             "cloud_knn_k12_ms": timed(lambda: cloud_knn(p, k), a.reps),
             "cloud_normals_k12_ms": timed(normals, a.reps),
             "cloud_orient_k12_ms": timed(orient, a.reps),
             "estimate_normals_k12_ms": timed(lambda: estimate_normals(p, k), a.reps)}
        r["rounds"], r["seeds"] = int(info[0]), int(info[1])
        r["knn_k8_over_areas_k8"] = r["cloud_knn_k8_ms"] / r["cloud_areas_k8_ms"]
        r["orient_share_of_estimate"] = r["cloud_orient_k12_ms"] / r["estimate_normals_k12_ms"]
        cos = (estimate_normals(p, k) * radial).sum(dim=1)
        r["normals_against_the_radius"] = int((cos <= 0).sum())
        r["smallest_cos_to_the_radius"] = float(cos.min())
        out[str(n)] = r
    n = a.sizes[-1]
    p, _ = fibonacci_sphere(n, 0.7, dev)
    cloud_to_mesh(p, res=32)
    out[f"cloud_to_mesh_{a.mesh_res}_bare_{n}_ms"] = timed(lambda: cloud_to_mesh(p, res=a.mesh_res), 1, warm=False)

    def rnd(x):
        if isinstance(x, dict):
            return {k: rnd(v) for k, v in x.items()}
        return round(x, 4) if isinstance(x, float) else x
    print(json.dumps(rnd(out)))


if __name__ == "__main__":
    main()
