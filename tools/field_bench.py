#!/usr/bin/env python3
"""Timing of the decoder's field kernels (csrc/decode_field.hip; not part of bench.py) and of the mesh refinement built on them.

  field_grad / project   ishap_triplane_field_grad and ishap_triplane_project (4 iterations) at 1 000, 40 000 and 160 000
                         points drawn near the surface of a shape-like field: a smooth synthetic triplane (S = 128) through
                         the synthetic-weight decoder whose output bias is moved so that the field's median is its zero level.
                         Milliseconds, median of --reps after one warm-up, host clock around calls that end in a device
                         synchronise; next to ishap_triplane_decode_points of the same points.
  get_mesh               DragStuff.get_mesh of that latent at --res (default 256) with refine = None and with
                         refine = {"iterations": 4, "max_move": one voxel}, each including the mesh build (surface, ten
                         smoothing sweeps, and for the refined one the projection).
  level set              of the refined mesh's vertices: the share with |logit| <= tol and the mean |logit|, before (the
                         smoothed vertices) and after the projection, and the share of vertices that moved.
One JSON line.

    python tools/field_bench.py [--reps 5] [--res 256]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TOL = 1e-4


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


def shape_like(dev, res):
    """(DragStuff with the decoder loaded, latent [1,96,128,128]): tools/components_bench.py's smooth field, with the decoder's
    output bias lowered by the field's median so that the level set the mesh is made at is the decoder's own zero"""
    import torch
    from ishapediting_amd import synthetic
    from ishapediting_amd.drag_utils import DragStuff, get_args
    from ishapediting_amd.triplane_decoder import decode_volume
    S = 128
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
    g = torch.Generator().manual_seed(17)
    lat = torch.zeros(1, 96, S, S)
    for c in range(96):
        a, b, p, q = torch.randn(4, generator=g)
        lat[0, c] = 0.005 * (a * torch.cos(1.5 * xx + p) + b * torch.cos(1.5 * yy + q))
    lat = lat.to(dev)
    ds = DragStuff(dev, args=get_args(["--shape_resolution", str(res)]))
    sd = synthetic.decoder_state_dict(4321)
    ds.decoder.net.load_state_dict(sd)
    median = decode_volume(ds.decoder, lat, 1.0, 0.0, 64).median()
    sd["5.bias"] = sd["5.bias"] - median.cpu()
    ds.decoder.net.load_state_dict(sd)
    return ds, lat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=256)
    a = ap.parse_args()
    import torch
    from ishapediting_amd.triplane_decoder import field_grad_planes, prepare_planes, project_to_surface
    dev = torch.device("cuda", 0)
    res = a.res
    voxel = 2.0 / (res - 1)
    out = {"res": res, "reps": a.reps, "tol": TOL, "device": torch.cuda.get_device_name(0)}
    ds, lat = shape_like(dev, res)
    planes = prepare_planes(lat, 1.0, 0.0)

    ds.refine = None
    out["get_mesh_plain_ms"] = timed(lambda: ds.get_mesh(tri_feat=lat).vertices, a.reps)
    ds.refine = {"iterations": 4, "max_move": voxel}
    out["get_mesh_refined_ms"] = timed(lambda: ds.get_mesh(tri_feat=lat).vertices, a.reps)
    mesh = ds.get_mesh(tri_feat=lat)
    verts = mesh.vertices
    start, p = mesh.refinement
    z0 = field_grad_planes(ds.decoder, planes, start).logits.abs()
    z1 = p.logits.abs()
    out["mesh"] = {"vertices": int(verts.shape[0]), "triangles": int(mesh.triangles.shape[0]),
                   "share_within_tol_before": float((z0 <= TOL).float().mean()), "share_within_tol_after": float((z1 <= TOL).float().mean()),
                   "mean_abs_logit_before": float(z0.mean()), "mean_abs_logit_after": float(z1.mean()),
                   "share_moved": float((p.accepted > 0).float().mean()),
                   "mean_move_voxels": float((p.points - start).norm(dim=1).mean() / voxel)}

    # points near the surface: the smoothed vertices again, repeated or cut to the size asked for
    for n in (1000, 40000, 160000):
        idx = torch.arange(n, device=dev) % start.shape[0]
        pts = start[idx].contiguous()
        r = {"field_grad_ms": timed(lambda: field_grad_planes(ds.decoder, planes, pts), a.reps),
             "project4_ms": timed(lambda: project_to_surface(ds.decoder, planes, pts, iterations=4, step_max=0.5 * voxel, max_move=voxel, tol=TOL),
                                  a.reps),
             "project0_ms": timed(lambda: project_to_surface(ds.decoder, planes, pts, iterations=0), a.reps),
             "decode_points_ms": timed(lambda: _decode_points(ds.decoder, planes, pts), a.reps)}
        out[f"n{n}"] = r

    def rnd(v):
        if isinstance(v, dict):
            return {k: rnd(w) for k, w in v.items()}
        return round(v, 5) if isinstance(v, float) else v
    print(json.dumps(rnd(out)))


def _decode_points(decoder, planes, pts):
    """ishap_triplane_decode_points on explicit planes (MultiTriplane.forward without the re-layout of its embeddings)"""
    import ctypes as C
    import torch
    from ishapediting_amd import _lib
    outp = torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device)
    w = decoder.net.weights_c()
    _lib.check(_lib.lib().ishap_triplane_decode_points(planes.data_ptr(), planes.shape[1], C.byref(w), pts.data_ptr(), pts.shape[0],
                                                       outp.data_ptr(), _lib.stream_ptr(pts.device)))
    return outp


if __name__ == "__main__":
    main()
