#!/usr/bin/env python3
"""What quadric vertex clustering costs on the meshes the sparse surface makes.

  python tools/simplify_bench.py [--res 512 1024] [--cells 2 4] [--reps 7] [--inner 4] [--out profiles/simplify_bench.txt]

The surface is tools/sparse_surface_bench.py's closed shape-like one (`blobs`), cut by extract_surface_sparse at R from the 256^3
volume of the same planes; its vertices are in grid units, and the cells are `cell` voxels from origin 0, as OccupancyMesh's
`simplify` keyword places them.  In one process, per R: two warm-up extractions and `reps` timed ones; then per cell size and
contraction two warm-up calls of mesh.simplify_vertex_clustering and `reps` timed windows of `inner` calls each, quadric and
average alternating, a device synchronise before every clock reading (every call also ends in its own read-back of the sizes).
Reported per row: ms per call (median, min, max over the windows), vertices and triangles in / out, clusters, the peak device
memory of one call above what was resident (torch's allocator), the bytes the call held, the extraction time of the same mesh,
and the accumulation pass:
  atomic bytes (algorithmic) = triangles of non-zero area x 3 corners x 11 slots x 8 bytes (ten quadric entries and the guard);
  atomic bytes (per triangle) = the same after the corners of a triangle that share a cluster were summed: an UPPER bound of what
                               is issued, because consecutive triangles of one cluster are summed too before the atomic (how
                               many that saves depends on the order of the input and is not counted here);
  pass time                  = ms(quadric) - ms(average): contraction "average" skips exactly the quadric pass and the guard
                               check (one load per possible cluster), everything else is the same launches on the same data.
The rate is therefore a difference of two end-to-end medians, not a kernel trace, and it is algorithmic bytes over the time of a
pass that also does the float64 arithmetic: what this kernel achieved with 64-bit integer atomics of this shape (sixteen-lane
groups, one 128-byte row per group, eleven lanes of each adding), not what the hardware can do.
Writes a JSON line and a readable table to --out and prints the JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

COARSE = 256
SLOT_BYTES = 11 * 8          # per triangle corner: ten quadric entries and the guard, 64 bits each


def window(fn, inner):
    """ms per call over `inner` calls, and the peak bytes above what was resident"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(inner):
        r = fn()
        del r
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner, torch.cuda.max_memory_allocated() - base


def atomic_bytes(verts, tris, vmap):
    """(algorithmic, after the in-triangle sums) atomic bytes of the quadric pass: float64 torch ops on the device, outside every timed window"""
    t = tris.long()
    p = verts.double()
    n = torch.cross(p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]], dim=1).norm(dim=1)
    ok = (n > 0) & torch.isfinite(n)
    c = vmap.long()[t[ok]]
    # clusters without an output vertex (-1) cannot be told apart here: their corners count as one cluster, a handful at most
    distinct = 1 + (c[:, 1] != c[:, 0]).long() + ((c[:, 2] != c[:, 0]) & (c[:, 2] != c[:, 1])).long()
    return int(ok.sum()) * 3 * SLOT_BYTES, int(distinct.sum()) * SLOT_BYTES


def run(dec, planes, R, cells, reps, inner):
    from ishapediting_amd.mesh import extract_surface_sparse, simplify_vertex_clustering
    from ishapediting_amd.triplane_decoder import decode_planes_grid
    coarse = decode_planes_grid(dec, planes, COARSE)
    nb = (R - 1 + 7) // 8

    def extract():
        return extract_surface_sparse(dec, planes, R, coarse, max_bricks=nb ** 3)

    for _ in range(2):
        window(extract, 1)
    te = [window(extract, 1)[0] for _ in range(reps)]
    v, t, _ = extract()
    rows = []
    for cell in cells:
        dims = [int(np.floor((R - 1) / cell)) + 1] * 3

        def call(contraction):
            return simplify_vertex_clustering(v, t, float(cell), contraction, origin=(0.0, 0.0, 0.0), dims=dims, return_map=True)

        calls = {"quadric": lambda: call("quadric"), "average": lambda: call("average")}
        outs = {}
        for c, fn in calls.items():
            window(fn, 1)
            outs[c] = fn()
        times, peaks = {c: [] for c in calls}, {c: [] for c in calls}
        for _ in range(reps):
            for c, fn in calls.items():
                ms, peak = window(fn, inner)
                times[c].append(ms)
                peaks[c].append(peak)
        algo, per_tri = atomic_bytes(v, t, outs["quadric"][3])
        pass_ms = float(np.median(times["quadric"])) - float(np.median(times["average"]))
        for c in calls:
            info = outs[c][2]
            row = {"res": R, "cell": cell, "contraction": c, "ms": round(float(np.median(times[c])), 3),
                   "ms_min_max": [round(min(times[c]), 3), round(max(times[c]), 3)], "reps": reps, "calls_per_window": inner,
                   "vertices_in": info.vertices_in, "vertices_out": info.vertices_out, "triangles_in": info.triangles_in,
                   "triangles_nondegenerate": info.triangles_nondegenerate, "triangles_out": info.triangles_out, "clusters": info.clusters,
                   "peak_bytes": int(max(peaks[c])), "held_bytes": info.bytes, "extract_ms": round(float(np.median(te)), 2),
                   "extract_ms_min_max": [round(min(te), 2), round(max(te), 2)]}
            if c == "quadric":
                row["atomic_bytes_algorithmic"] = algo
                row["atomic_bytes_per_triangle"] = per_tri
                row["quadric_pass_ms"] = round(pass_ms, 3)
                row["atomic_GBps_algorithmic"] = round(algo / pass_ms / 1e6, 1) if pass_ms > 0 else None
                row["atomic_GBps_per_triangle"] = round(per_tri / pass_ms / 1e6, 1) if pass_ms > 0 else None
            rows.append(row)
        del outs
    return rows


def table_line(r):
    gib = 1024.0 ** 3
    lo, hi = r["ms_min_max"]
    left = (f"{r['res']:5d} {r['cell']:5g} {r['contraction']:>11} {r['ms']:8.3f} {lo:8.3f} {hi:8.3f} {r['extract_ms']:10.2f} "
            f"{r['vertices_in']:10d} {r['vertices_out']:10d} {r['triangles_in']:10d} {r['triangles_out']:10d} {r['peak_bytes'] / gib:9.3f}")
    if r["contraction"] != "quadric":
        return left + f" {'-':>8} {'-':>8} {'-':>9} {'-':>12}"
    pass_ms, algo_gb = f"{r['quadric_pass_ms']:.3f}", f"{r['atomic_bytes_algorithmic'] / 1e9:.3f}"
    rate_algo = "-" if r["atomic_GBps_algorithmic"] is None else f"{r['atomic_GBps_algorithmic']:.1f}"
    rate_tri = "-" if r["atomic_GBps_per_triangle"] is None else f"{r['atomic_GBps_per_triangle']:.1f}"
    return left + f" {pass_ms:>8} {algo_gb:>8} {rate_algo:>9} {rate_tri:>12}"


def report(a, results):
    out = {"metric": "quadric vertex clustering of a sparse-surface mesh (ms per call, wall clock around a device synchronise)",
           "device": torch.cuda.get_device_name(0), "coarse_seed_res": COARSE, "results": results}
    lines = [json.dumps(out), "",
             f"{out['device']}; shape `blobs` of tools/sparse_surface_bench.py; median of {a.reps} windows of {a.inner} calls, quadric and "
             "average alternating, after two warm-up calls each; pass ms = ms(quadric) - ms(average)", "",
             f"{'R':>5} {'cell':>5} {'contraction':>11} {'ms':>8} {'min':>8} {'max':>8} {'extract ms':>10} {'verts in':>10} {'verts out':>10} "
             f"{'tris in':>10} {'tris out':>10} {'peak GiB':>9} {'pass ms':>8} {'algo GB':>8} {'GB/s algo':>9} {'GB/s per-tri':>12}"]
    lines += [table_line(r) for r in results]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    p.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0])
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--inner", type=int, default=4)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "simplify_bench.txt"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("simplify_bench needs a GPU: nothing here is measured on a CPU")
    device = torch.device("cuda", 0)
    from sparse_surface_bench import shapes
    dec, planes = shapes(device, ["blobs"])["blobs"]
    results, lines = [], []
    for R in a.res:
        rows = run(dec, planes, R, a.cells, a.reps, a.inner)
        results += rows
        for r in rows:
            print(json.dumps(r), flush=True)
        lines = report(a, results)               # rewritten after every resolution: a later one that fails loses nothing
    print("\n".join(lines[2:]))


if __name__ == "__main__":
    main()
