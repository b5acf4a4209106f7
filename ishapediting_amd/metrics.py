"""Mesh metrics on the device: the reference's evaluation helpers (meshProcess.py:7-118) without Open3D or scipy.

The reference builds them on Open3D's RaycastingScene (signed distance, occupancy, closest points) and scipy's cKDTree;
neither is a dependency here.  Every distance, sign, maximum and per-group statistic comes from libishap_hip.so
(csrc/surface.hip: ishap_mesh_distance, ishap_mesh_occupancy, ishap_hausdorff, ishap_group_field_stats); torch only draws
the random samples and moves tensors.

A mesh may be an OccupancyMesh, a (vertices, triangles) pair, any object with `.vertices` / `.triangles` (an Open3D
TriangleMesh the GUI holds) or the path of an OBJ file (read with mesh.read_obj).

Sampling: every function that samples takes `seed` (default 0) and draws from its own torch.Generator, so a call is
reproducible; the reference draws from numpy's global state and Open3D's sampler, so its samples -- not their
distribution -- differ from these.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .mesh import (OCCUPANCY_METHODS, OccupancyMesh, _check_choice, mesh_arrays, mesh_chamfer, mesh_occupancy, orientation_sign,
                   read_obj, sample_surface_points)

METRICS = ("IoU", "L2", "CD")


def device_mesh(mesh, device=None):
    """(vertices [V,3] float32, triangles [F,3] int32) on the device from any accepted mesh form."""
    dev = _lib.need_gpu(device, "mesh metrics", "run")
    if isinstance(mesh, str):
        v, t = read_obj(mesh)
    elif isinstance(mesh, OccupancyMesh) and mesh.vertices.device == dev:
        return _lib.tensor(mesh.vertices, torch.float32), _lib.tensor(mesh.triangles, torch.int32)
    elif isinstance(mesh, tuple) and all(torch.is_tensor(x) and x.device == dev for x in mesh):
        return _lib.tensor(mesh[0], torch.float32), _lib.tensor(mesh[1], torch.int32)
    else:
        v, t = mesh_arrays(mesh)
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev), torch.from_numpy(np.ascontiguousarray(t)).to(dev)


def mesh_distance(verts: torch.Tensor, tris: torch.Tensor, points: torch.Tensor, sdf=True, orientation: str = "auto"):
    """(distance [P] float32, closest triangle [P] int32) of device points to a device mesh: signed (negative inside,
    inside by the ray parity of mesh_occupancy) when `sdf`, else unsigned.  sdf=2: the sign comes from the winding number
    instead (inside where mesh_winding_number > 0.5, negated first when mesh.orientation_sign(..., orientation) is -1), for
    meshes that are not watertight.  The closest triangle is the lowest index on exact ties."""
    winding = sdf is not True and sdf is not False and int(sdf) == 2
    dev = verts.device
    v = _lib.tensor(verts, torch.float32)
    t = _lib.tensor(tris, torch.int32, dev)
    p = _lib.tensor(points, torch.float32, dev, (-1, 3))
    dist = torch.empty(p.shape[0], dtype=torch.float32, device=dev)
    tri = torch.empty(p.shape[0], dtype=torch.int32, device=dev)
    if p.shape[0] == 0:
        return dist, tri
    if t.shape[0] == 0:
        raise ValueError("mesh_distance: the mesh has no triangles")
    mode = 2 * orientation_sign(v, t, orientation) if winding else int(bool(sdf))
    scratch, nbytes = _lib.scratch(dev, "ishap_mesh_distance_scratch_bytes_sdf", t.shape[0], p.shape[0], mode)
    _lib.call(dev, "ishap_mesh_distance", v.data_ptr(), t.data_ptr(), t.shape[0], p.data_ptr(), p.shape[0], mode,
              dist.data_ptr(), tri.data_ptr(), scratch.data_ptr(), nbytes)
    return dist, tri


def field_stats(fa: torch.Tensor, fb: torch.Tensor, groups: int, occupancy: bool = False) -> torch.Tensor:
    """ishap_group_field_stats: fa, fb [groups * P] on the device -> [2 groups + 2]: per-group IoU, per-group mean squared
    difference, then the means of both over the groups (inside: < 0, or != 0 for occupancy)."""
    a = _lib.tensor(fa, torch.float32)
    b = _lib.tensor(fb, torch.float32, a.device)
    assert a.numel() == b.numel() and a.numel() % groups == 0 and a.numel() > 0
    out = torch.empty(2 * groups + 2, dtype=torch.float32, device=a.device)
    _lib.call(a.device, "ishap_group_field_stats", a.data_ptr(), b.data_ptr(), groups, a.numel() // groups, int(bool(occupancy)),
              out.data_ptr())
    return out


def hausdorff_sq(pa: torch.Tensor, pb: torch.Tensor):
    """(max over a of min_b |a-b|^2, max over b of min_a |a-b|^2, per-point minima [na + nb]) of two device point sets."""
    a = _lib.tensor(pa, torch.float32, pa.device, (-1, 3))
    b = _lib.tensor(pb, torch.float32, a.device, (-1, 3))
    nearest = torch.empty(a.shape[0] + b.shape[0], dtype=torch.float32, device=a.device)
    out2 = torch.empty(2, dtype=torch.float32, device=a.device)
    _lib.call(a.device, "ishap_hausdorff", a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], nearest.data_ptr(), out2.data_ptr())
    d = out2.tolist()
    return d[0], d[1], nearest


# ---------------------------------------------------------------- meshProcess.py's call surface


def calc_implicit_field(mesh, points, sdf: bool = True, device=None, sign: str = "parity") -> torch.Tensor:
    """meshProcess.py:7-14: the signed distance of every point (negative inside), or with sdf=False the 0/1 occupancy.
    sign: where inside comes from -- "parity" (ray crossings, closed meshes) or "winding" (winding number > 0.5, any mesh).
    Returns a [P] float32 device tensor."""
    _check_choice("sign", sign, OCCUPANCY_METHODS)
    v, t = device_mesh(mesh, device)
    p = _lib.tensor(points, torch.float32, v.device, (-1, 3))
    if sdf:
        return mesh_distance(v, t, p, sdf=2 if sign == "winding" else True)[0]
    return mesh_occupancy(v, t, p, method=sign)


def calc_chamfer(mesh_a, mesh_b, point_num: int, seed: int = 0, device=None) -> float:
    """meshProcess.py:18-35: mesh.mesh_chamfer (area-uniform samples, mean squared nearest-neighbour distance both ways)."""
    return mesh_chamfer(device_mesh(mesh_a, device), device_mesh(mesh_b, device), point_num, seed)


def calc_hausdorff(mesh_a, mesh_b, point_num: int, seed: int = 0, device=None) -> float:
    """meshProcess.py:39-55: `point_num` area-uniform samples on each surface, the larger of the two directed maxima of
    the nearest-neighbour distance (not squared)."""
    va, ta = device_mesh(mesh_a, device)
    vb, tb = device_mesh(mesh_b, va.device)
    g = torch.Generator(device="cpu").manual_seed(seed)
    pa = sample_surface_points(va, ta, point_num, g)
    pb = sample_surface_points(vb, tb, point_num, g)
    h_ab, h_ba, _ = hausdorff_sq(pa, pb)
    return float(np.sqrt(max(h_ab, h_ba)))


def iou_points(mesh_a, mesh_b, point_num: int, seed: int = 0, device=None) -> torch.Tensor:
    """calc_iou's sample set (meshProcess.py:64-69): int(0.2 point_num) uniform in [-1,1]^3, then int(0.4 point_num)
    area-uniform samples of each surface plus N(0, 0.01) noise.  [N,3] float32 on the device."""
    va, ta = device_mesh(mesh_a, device)
    vb, tb = device_mesh(mesh_b, va.device)
    dev = va.device
    g = torch.Generator(device="cpu").manual_seed(seed)
    uniform = (torch.rand((int(point_num * 0.2), 3), generator=g) * 2 - 1).to(dev)
    n_s = int(point_num * 0.4)
    pa = sample_surface_points(va, ta, n_s, g)
    pa = pa + 0.01 * torch.randn(pa.shape, generator=g).to(dev)
    pb = sample_surface_points(vb, tb, n_s, g)
    pb = pb + 0.01 * torch.randn(pb.shape, generator=g).to(dev)
    return torch.cat([uniform, pa, pb], dim=0).contiguous()


def calc_iou(mesh_a, mesh_b, point_num: int, seed: int = 0, device=None, sign: str = "parity") -> float:
    """meshProcess.py:59-77: |A and B| / |A or B| over iou_points(mesh_a, mesh_b, point_num, seed), inside by occupancy
    (sign: "parity" or "winding", as calc_implicit_field)."""
    _check_choice("sign", sign, OCCUPANCY_METHODS)
    va, ta = device_mesh(mesh_a, device)
    vb, tb = device_mesh(mesh_b, va.device)
    pts = iou_points((va, ta), (vb, tb), point_num, seed)
    oa, ob = mesh_occupancy(va, ta, pts, method=sign), mesh_occupancy(vb, tb, pts, method=sign)
    return float(field_stats(oa, ob, 1, occupancy=True)[0])


def calc_local_distance(mesh_a, mesh_b, points_a, points_b, r: float, point_num: int, metric: str = "IoU", seed: int = 0,
                        device=None, sign: str = "parity") -> float:
    """meshProcess.py:80-105: for every handle i, the signed distance of mesh_a at points_a[i] + offsets against that of
    mesh_b at points_b[i] + offsets (one set of `point_num` offsets uniform in [-r, r]^3, shared by all handles); the mean
    over the handles of
      'IoU'  |A and B| / |A or B| with inside = signed distance < 0 (NaN when neither mesh has a sample inside),
      'L2'   the mean of (d_b - d_a)^2,
      'CD'   0: the reference's branch is `pass`, so every handle contributes nothing.
    sign: "parity" or "winding", where the signed distances take their sign from (calc_implicit_field).
    All handles go to the device in one distance launch per mesh and one statistics launch."""
    pa = points_a if torch.is_tensor(points_a) else np.asarray(points_a)
    pb = points_b if torch.is_tensor(points_b) else np.asarray(points_b)
    if tuple(pa.shape) != tuple(pb.shape):
        raise ArithmeticError("The 'points_a' and 'points_b' should have the same shape!")
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    _check_choice("sign", sign, OCCUPANCY_METHODS)
    if metric == "CD":
        return 0.0
    va, ta = device_mesh(mesh_a, device)
    vb, tb = device_mesh(mesh_b, va.device)
    dev = va.device
    ha, hb = _lib.tensor(pa, torch.float32, dev, (-1, 3)), _lib.tensor(pb, torch.float32, dev, (-1, 3))
    G = ha.shape[0]
    g = torch.Generator(device="cpu").manual_seed(seed)
    offs = ((torch.rand((point_num, 3), generator=g) * 2 - 1) * r).to(dev)
    qa = (ha[:, None, :] + offs[None]).reshape(-1, 3).contiguous()
    qb = (hb[:, None, :] + offs[None]).reshape(-1, 3).contiguous()
    sdf = 2 if sign == "winding" else True
    da = mesh_distance(va, ta, qa, sdf=sdf)[0]
    db = mesh_distance(vb, tb, qb, sdf=sdf)[0]
    out = field_stats(da, db, G)
    return float(out[2 * G] if metric == "IoU" else out[2 * G + 1])


def calc_mesh_points_normals(mesh, pcd=None, seed: int = 0, device=None) -> dict:
    """meshProcess.py:108-118: 2048 area-uniform surface samples (or the given points: an array, a tensor or an object
    with `.points`) and the unit normal cross(b - a, c - a) of each one's closest triangle.  numpy float32 arrays."""
    v, t = device_mesh(mesh, device)
    dev = v.device
    if pcd is None:
        pts = sample_surface_points(v, t, 2048, torch.Generator(device="cpu").manual_seed(seed))
    else:
        pts = _lib.tensor(pcd.points if hasattr(pcd, "points") else pcd, torch.float32, dev, (-1, 3))
    _, tri = mesh_distance(v, t, pts, sdf=False)
    f = t[tri.long()].long()
    n = torch.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=1)
    n = n / n.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return {"points": pts.cpu().numpy().astype(np.float32), "normals": n.cpu().numpy().astype(np.float32)}
