#!/usr/bin/env python3
"""What the sparse high-resolution surface costs next to the dense path at the same resolution.

  python tools/sparse_surface_bench.py [--res 512 1024] [--reps 5] [--shapes c3 blobs] [--out profiles/sparse_surface_bench.txt]

Per shape and resolution R, in one process, after one warm-up of each path, `reps` repeats of each, alternating, a device
synchronise before every clock reading:
  dense   decode_planes_grid(decoder, planes, R) + extract_surface (the parent's path: R^3 logits + 6 bytes of scan scratch a voxel)
  sparse  extract_surface_sparse(decoder, planes, R, coarse) seeded from the 256^3 volume of the same planes (decoded outside
          the timed window: get_mesh has it anyway)
with the peak device memory of each path above what was resident before it (torch's allocator: both paths allocate through
it), the brick counts, the growth rounds, and the decoded points against R^3 (the derived expectation: 729 bricks / R^3).
Both meshes are compared: the vertex and triangle counts, and (up to 64 M vertices) the sorted vertex rows bit for bit -- equal
when the coarse grid sees every component of the fine surface.
Shapes: `c3`, bench.py's synthetic C3 shape (random decoder weights: the volume is noise and the surface passes through almost
every cell -- the worst case, every brick is active); `blobs`, low-pass planes (S = 8, 0.005 randn) under the same decoder with
its output bias moved to the median logit -- a closed, shape-like surface, where only O(R^2) of the bricks are near it.
Writes a JSON line and a readable table to --out and prints the JSON line.
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

COARSE = 256


def shapes(device, which):
    from ishapediting_amd import synthetic
    from ishapediting_amd.triplane_decoder import MultiTriplane, decode_planes_grid, prepare_planes
    out = {}
    if "blobs" in which:
        sd = {k: v.clone() for k, v in synthetic.decoder_state_dict(4321).items()}
        dec = MultiTriplane(1, device=device)
        dec.net.load_state_dict(sd)
        planes = (torch.randn((3, 8, 8, 32), generator=torch.Generator().manual_seed(1)) * 0.005).to(device)
        med = decode_planes_grid(dec, planes, 64).median()
        sd["5.bias"] = sd["5.bias"] - med.cpu()
        dec.net.load_state_dict(sd)
        out["blobs"] = (dec, planes)
    if "c3" in which:
        import bench
        ds = bench.make_dragstuff(device, 1234)
        ds.update_latent_params(img=synthetic.latent(0))
        out["c3"] = (ds.decoder, prepare_planes(ds.tri_feat0.to(device), ds.range, ds.middle))
        del ds
    return out


def timed(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return res, (time.perf_counter() - t0) * 1e3, torch.cuda.max_memory_allocated() - base


COMPARE_MAX = 64_000_000     # vertices up to which the two vertex sets are sorted and compared (three stable sorts of int64 indices)


def rows_sorted(v):
    idx = torch.arange(v.shape[0], device=v.device)
    for c in (2, 1, 0):          # lexicographic: stable sorts from the last key to the first
        idx = idx[torch.argsort(v[idx, c], stable=True)]
    return v[idx]


def run(device, name, dec, planes, R, reps):
    from ishapediting_amd.mesh import extract_surface, extract_surface_sparse
    from ishapediting_amd.triplane_decoder import decode_planes_grid
    coarse = decode_planes_grid(dec, planes, COARSE)
    nb = (R - 1 + 7) // 8

    def dense():
        return extract_surface(decode_planes_grid(dec, planes, R))

    def sparse():
        return extract_surface_sparse(dec, planes, R, coarse, max_bricks=nb ** 3)

    (dv, dt), _, _ = timed(dense)
    (sv, st, info), _, _ = timed(sparse)
    same_counts = (int(dv.shape[0]), int(dt.shape[0])) == (int(sv.shape[0]), int(st.shape[0]))
    equal = None if dv.shape[0] > COMPARE_MAX else bool(same_counts and torch.equal(rows_sorted(dv), rows_sorted(sv)))
    counts = {"dense": (int(dv.shape[0]), int(dt.shape[0])), "sparse": (int(sv.shape[0]), int(st.shape[0]))}
    del dv, dt, sv, st
    td, ts, md, ms = [], [], [], []
    for _ in range(reps):
        r, t, m = timed(dense)
        del r
        td.append(t); md.append(m)
        r, t, m = timed(sparse)
        del r
        ts.append(t); ms.append(m)
    med = lambda x: float(np.median(x))      # noqa: E731
    return {"shape": name, "res": R, "reps": reps, "dense_ms": round(med(td), 2), "dense_ms_min_max": [round(min(td), 2), round(max(td), 2)],
            "sparse_ms": round(med(ts), 2), "sparse_ms_min_max": [round(min(ts), 2), round(max(ts), 2)],
            "dense_peak_bytes": int(max(md)), "sparse_peak_bytes": int(max(ms)), "sparse_held_bytes": info.bytes,
            "bricks_active": info.bricks, "bricks_total": nb ** 3, "rounds": info.rounds, "points_decoded": info.points,
            "points_dense": R ** 3, "points_ratio": round(info.points / R ** 3, 4), "time_ratio_sparse_over_dense": round(med(ts) / med(td), 3),
            "vertices_triangles": counts, "vertex_sets_bitwise_equal": equal}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--res", type=int, nargs="+", default=[512, 1024])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--shapes", nargs="+", default=["blobs", "c3"], choices=["c3", "blobs"])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_surface_bench.txt"))
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_surface_bench needs a GPU: nothing here is measured on a CPU")
    device = torch.device("cuda", 0)
    results = []
    for name, (dec, planes) in shapes(device, a.shapes).items():
        for R in a.res:
            results.append(run(device, name, dec, planes, R, a.reps))
            print(json.dumps(results[-1]), flush=True)
            lines = report(a, results)           # rewritten after every row: a later row that fails loses nothing
    print("\n".join(lines[2:]))


def report(a, results):
    out = {"metric": "sparse against dense level-set surface at one resolution (ms per mesh, wall clock around a device synchronise)",
           "device": torch.cuda.get_device_name(0), "coarse_seed_res": COARSE, "results": results}
    gib = 1024.0 ** 3
    lines = [json.dumps(out), "", f"{out['device']}; seeds: the {COARSE}^3 volume of the same planes (outside the timed window); median of "
             f"{a.reps} alternating repeats after a warm-up", "",
             f"{'shape':6} {'R':>5} {'dense ms':>10} {'sparse ms':>10} {'sparse/dense':>13} {'dense GiB':>10} {'sparse GiB':>11} "
             f"{'bricks':>18} {'rounds':>6} {'points/R^3':>11} {'vertices':>10} {'same set':>8}"]
    for r in results:
        lines.append(f"{r['shape']:6} {r['res']:5d} {r['dense_ms']:10.2f} {r['sparse_ms']:10.2f} {r['time_ratio_sparse_over_dense']:13.3f} "
                     f"{r['dense_peak_bytes'] / gib:10.3f} {r['sparse_peak_bytes'] / gib:11.3f} "
                     f"{str(r['bricks_active']) + '/' + str(r['bricks_total']):>18} {r['rounds']:6d} {r['points_ratio']:11.4f} "
                     f"{r['vertices_triangles']['sparse'][0]:10d} {str(r['vertex_sets_bitwise_equal']):>8}")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return lines


if __name__ == "__main__":
    main()
