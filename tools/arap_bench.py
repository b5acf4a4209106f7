#!/usr/bin/env python3
"""Timing of the device ARAP deformation (ishapediting_amd/deform.py: arap at 50 iterations; not part of bench.py) on two
meshes: the marching-cubes mesh of an analytic 256^3 sphere, and get_mesh's surface (decode + marching cubes + 10
smoothing passes) of a synthetic-weight triplane at --decoded-res.  Handles: the nearest vertices of a few points, moved
by 0.1; static: every vertex farther than 0.5 from all handles.  Prints one JSON line per mesh: V, F, free vertices, the
median total time over --reps after a warm-up (host clock around a call that ends in a device synchronise), time per outer
iteration and the CG iterations of every outer iteration.

    python tools/arap_bench.py [--reps 3] [--iters 50] [--decoded-res 128]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sphere_mesh(dev, res=256, r=90.4):
    import torch
    from ishapediting_amd.mesh import extract_surface
    ax = torch.arange(res, dtype=torch.float32, device=dev) - (res - 1) / 2
    vol = r - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    v, f = extract_surface(vol)
    return (v / (res - 1) * 2 - 1).contiguous(), f


def decoded_mesh(dev, res):
    import torch
    from ishapediting_amd import synthetic
    from ishapediting_amd.mesh import volume_to_mesh
    from ishapediting_amd.metrics import device_mesh
    from ishapediting_amd.triplane_decoder import MultiTriplane, decode_volume
    dec = MultiTriplane(1, device=dev)
    dec.net.load_state_dict(synthetic.decoder_state_dict())
    lat = torch.from_numpy(synthetic.latent(0)) * 0.5
    return device_mesh(volume_to_mesh(decode_volume(dec, lat.to(dev), 1.0, 0.0, res), res, smooth_iterations=10))


def case(name, v, f, picks, reps, iters):
    import torch
    from ishapediting_amd.deform import deform_as_rigid_as_possible, nearest_vertices
    handles = torch.unique(nearest_vertices((v, f), picks))
    d = torch.cdist(v.double(), v[handles].double()).min(dim=1).values
    static = torch.nonzero(d > 0.5).flatten()
    ids = torch.cat([static, handles]).cpu().numpy()
    pos = torch.cat([v[static], v[handles] + torch.tensor([0.1, 0.0, 0.0], device=v.device)]).contiguous()
    deform_as_rigid_as_possible(v, f, ids, pos, max_iter=iters)
    torch.cuda.synchronize()
    ts, info = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        _, info = deform_as_rigid_as_possible(v, f, ids, pos, max_iter=iters)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    total = ts[len(ts) // 2]
    cg = info["cg_iters"]
    return {"mesh": name, "V": int(v.shape[0]), "F": int(f.shape[0]), "handles": int(handles.numel()),
            "static": int(static.numel()), "free": int(v.shape[0] - len(ids)), "iters": iters,
            "total_s": round(total, 4), "per_iter_ms": round(total / max(iters, 1) * 1e3, 3),
            "cg_per_iter": cg.tolist(), "cg_total": int(cg.sum()),
            "us_per_cg_iter": round(total / max(int(cg.sum()), 1) * 1e6, 2), "converged": bool(info["converged"].all()),
            "energy_first_last": [float(info["energy"][0]), float(info["energy"][-1])] if iters else []}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--decoded-res", type=int, default=128)
    a = ap.parse_args()
    import torch
    from ishapediting_amd import synthetic
    dev = torch.device("cuda", 0)
    v, f = sphere_mesh(dev)
    picks = torch.tensor([[0.0, 0.0, 0.75], [0.25, 0.0, 0.7], [0.0, 0.25, 0.7], [-0.2, -0.2, 0.7]])
    print(json.dumps(case("sphere256", v, f, picks, a.reps, a.iters)), flush=True)
    if a.decoded_res > 0:
        v, f = decoded_mesh(dev, a.decoded_res)
        src, _ = synthetic.handles(3, seed=7)
        print(json.dumps(case(f"decoded{a.decoded_res}", v, f, torch.from_numpy(src), a.reps, a.iters)), flush=True)


if __name__ == "__main__":
    main()
