#!/usr/bin/env python3
"""What a region costs: a C3 drag edit (DragStuff.training, bench.py's shape, weights and handles) with a keep region against the
same edit without one, and the time to build a weight map from voxel grids at D = 256, W = 64.

  python tools/region_edit_bench.py [--reps 3] [--warmup 1] [--map-reps 50] [--skip-edit]

Edits: warm-up steps, then `reps` timed steps of each kind, interleaved (plain, keep, plain, keep, ...) so that drift hits both;
a device synchronise before each clock reading, as in bench.py.  The keep region is a box around the first handle.
Map: regions.plane_weights(keep = Voxels of a 256^3 ball, free = Voxels of a second ball + a Box, dilate 1) at W = 64, between
two device events (median of `map-reps` calls after 5 warm-up calls; the call includes the upload of the primitives, the
allocations and the read-back of the shadow counts), and the library call alone on prepared buffers.  Prints ONE JSON line.
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


def map_times(device, reps):
    import ctypes as C
    from ishapediting_amd import _lib
    from ishapediting_amd.regions import Box, Voxels, plane_weights
    D, W = 256, 64
    ax = torch.linspace(-1, 1, D, device=device)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    keep = Voxels(((x + 0.3) ** 2 + y ** 2 + z ** 2) < 0.16)
    free = [Voxels(((x - 0.5) ** 2 + (y - 0.2) ** 2 + z ** 2) < 0.09), Box((0.2, -0.8, -0.1), (0.7, -0.3, 0.4))]
    out = {"D": D, "W": W, "set_voxels": [int(keep.mask.sum()), int(free[0].mask.sum())]}
    out["plane_weights_call"] = event_ms(lambda: plane_weights(keep=keep, free=free, W=W, dilate=1, device=device), 5, reps)
    # the library call alone: two 256^3 grids reduced onto three 64^2 maps, one primitive, dilate 1
    L = _lib.lib()
    prim = (_lib.RegionPrimC * 1)()
    prim[0].kind, prim[0].role = 0, 1
    prim[0].a[:], prim[0].b[:] = (0.2, -0.8, -0.1), (0.7, -0.3, 0.4)
    prims = torch.frombuffer(bytearray(bytes(prim)), dtype=torch.uint8).to(device)
    kg, fg = keep.mask.view(torch.uint8), free[0].mask.view(torch.uint8)
    wout = torch.empty((3, W, W), dtype=torch.float32, device=device)
    counts = torch.zeros(2, dtype=torch.int32, device=device)
    nb = int(L.ishap_region_plane_weights_scratch_bytes(W))
    scratch = torch.empty(nb, dtype=torch.uint8, device=device)

    def call():
        _lib.check(L.ishap_region_plane_weights(prims.data_ptr(), 1, kg.data_ptr(), fg.data_ptr(), D, W, 1, 4.0, 0.0, wout.data_ptr(),
                                                counts.data_ptr(), scratch.data_ptr(), nb, _lib.stream_ptr(device)))
    out["library_call"] = event_ms(call, 5, reps)
    out["library_call"]["volume_bytes_read"] = 3 * 2 * D ** 3        # each grid is read once per plane
    assert torch.equal(wout, plane_weights(keep=keep, free=free, W=W, dilate=1, device=device))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--map-reps", type=int, default=50)
    ap.add_argument("--skip-edit", action="store_true", help="time the map builder only")
    a = ap.parse_args()
    from ishapediting_amd import synthetic
    from ishapediting_amd.regions import Box
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    torch.manual_seed(bench.RNG_SEED)
    np.random.seed(bench.RNG_SEED)
    res = {"metric": "region-constrained drag edit", "device": torch.cuda.get_device_name(device), "map": map_times(device, a.map_reps)}
    if not a.skip_edit:
        ds = bench.make_dragstuff(device, 1234)
        ds.update_latent_params(img=synthetic.latent(0))
        src, tgt = synthetic.handles(bench.HANDLES, seed=7)
        c = np.asarray(src[0], np.float64)
        keep = [Box(c - 0.3, c + 0.3)]

        def edit(with_region):
            kw = {"keep": keep} if with_region else {}
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
        res["edit"] = {"guided_steps": bench.GUIDED_STEPS, "res": bench.RES, "reps": a.reps, "warmup": a.warmup,
                       "plain_s": [round(t, 4) for t in times[False]], "keep_s": [round(t, 4) for t in times[True]],
                       "plain_median_s": round(float(np.median(times[False])), 4), "keep_median_s": round(float(np.median(times[True])), 4),
                       "keep_texels": int((ds._dk.weights != 1).sum()), "losses_finite": bool(all(bool(torch.isfinite(l).all()) for l in ds.last_losses))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
