"""As-rigid-as-possible deformation on the device: the reference's meshProcess.arap (meshProcess.py:222-236) without Open3D.

The reference calls Open3D's TriangleMesh.deform_as_rigid_as_possible(constraint_ids, constraint_pos, max_iter=50); Open3D
is not a dependency here.  libishap_hip.so (csrc/deform.hip: ishap_arap) runs Sorkine & Alexa 2007 with the spokes energy
(Open3D's default) and cotangent weights w_ij = max(0, 1/2 sum cot), all in fp64:
  local   a rotation per vertex from the SVD of S_i = sum_j w_ij e_ij e'_ij^T (det fixed, identity when S_i has rank < 2),
  global  L_ff x_f = b_f - L_fc x_c, Jacobi-preconditioned CG warm-started from the previous positions.
Unconstrained vertices whose connected component (of the w > 0 edges) holds no constraint come back bit for bit at rest,
where Open3D's system would be singular.  Parity with Open3D itself is not pinned (it cannot run here); the statement the
device is tested against is tests/arap_ref.py.

nearest_vertices is the GUI's KD-tree pick (main.py:525-527) that turns drag handles into vertex ids.

A mesh may be anything metrics.device_mesh accepts: an OccupancyMesh, a (vertices, triangles) pair, an object with
`.vertices` / `.triangles` (an Open3D TriangleMesh) or the path of an OBJ file.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .mesh import OccupancyMesh, _write_obj, read_obj
from .metrics import device_mesh


def _host_ids(ids, name: str) -> np.ndarray:
    """int64 [n] on the host from a list, an array or a tensor"""
    a = ids.detach().cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids)
    if a.size == 0:
        return np.zeros(0, np.int64)
    if a.ndim != 1 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must be a 1-D list of vertex indices, got shape {a.shape} / {a.dtype}")
    return a.astype(np.int64)


def _host_positions(pos, n: int, name: str):
    """(positions, is_tensor): [n, 3] positions checked on the host side of the call (a tensor is checked by shape only)"""
    if torch.is_tensor(pos):
        shape = tuple(pos.shape)
    else:
        pos = np.asarray(pos, dtype=np.float32)
        shape = pos.shape
    if n == 0 and (len(shape) == 0 or int(np.prod(shape)) == 0):
        return np.zeros((0, 3), np.float32)
    if shape != (n, 3):
        raise ValueError(f"{name} must have shape ({n}, 3) for {n} vertex ids, got {shape}")
    return pos


def _check_ids(ids: np.ndarray, nverts: int, name: str):
    if ids.size and (ids.min() < 0 or ids.max() >= nverts):
        raise ValueError(f"{name}: vertex ids must lie in [0, {nverts}), got [{ids.min()}, {ids.max()}]")
    if np.unique(ids).size != ids.size:
        raise ValueError(f"{name}: repeated vertex ids")


def _num_vertices(mesh) -> int:
    """the vertex count of any accepted mesh form, without device work"""
    if isinstance(mesh, str):
        return int(read_obj(mesh)[0].shape[0])
    if isinstance(mesh, OccupancyMesh):
        return int(mesh.vertices.shape[0])
    v = mesh[0] if isinstance(mesh, tuple) else mesh.vertices
    return int(v.shape[0]) if torch.is_tensor(v) else int(np.asarray(v).reshape(-1, 3).shape[0])


def deform_as_rigid_as_possible(verts, tris, constraint_ids, constraint_pos, max_iter: int = 50, tol: float = 1e-8,
                                max_cg=None, device=None):
    """Open3D's deform_as_rigid_as_possible(constraint_ids, constraint_pos, max_iter) (spokes energy) on the device.

    verts [V,3], tris [F,3] (tensors or arrays), constraint_ids [C] distinct, constraint_pos [C,3].  tol: a CG column
    stops when |r| <= tol max(|rhs|, 1e-300); max_cg: the CG cap per outer iteration (None: 4 free vertices + 100).
    Returns (new vertices [V,3] float32 on the device, info) with info = {"energy": float64 [max_iter] (E_k at the
    rotations of step k and the positions before it), "cg_iters": int64 [max_iter], "converged": bool [max_iter] (every
    column met tol within max_cg)}."""
    ids = _host_ids(constraint_ids, "constraint_ids")
    pos = _host_positions(constraint_pos, ids.size, "constraint_pos")
    nv = int(verts.shape[0]) if torch.is_tensor(verts) else int(np.asarray(verts).reshape(-1, 3).shape[0])
    _check_ids(ids, nv, "constraint_ids")
    if int(max_iter) < 0 or not tol >= 0:
        raise ValueError(f"max_iter >= 0 and tol >= 0 required, got {max_iter}, {tol}")
    if max_cg is not None and not 0 < int(max_cg) < 2 ** 31:
        raise ValueError(f"max_cg must be in [1, 2^31), got {max_cg}")
    dev = verts.device if torch.is_tensor(verts) and verts.is_cuda else _lib.need_gpu(device, "mesh metrics", "run")
    v = _lib.tensor(verts, torch.float32, dev, (-1, 3))
    t = _lib.tensor(tris, torch.int32, dev, (-1, 3))
    if v.shape[0] == 0 or t.shape[0] == 0:
        raise ValueError("deform_as_rigid_as_possible: the mesh has no vertices or no triangles")
    c = torch.from_numpy(ids.astype(np.int32)).to(dev)
    cp = _lib.tensor(pos, torch.float32, dev, (-1, 3)) if ids.size else torch.zeros((0, 3), dtype=torch.float32, device=dev)
    K = int(max_iter)
    out = torch.empty_like(v)
    energy = torch.zeros(max(K, 1), dtype=torch.float64, device=dev)
    iters = torch.zeros(max(K, 1), dtype=torch.int32, device=dev)
    scratch, nbytes = _lib.scratch(dev, "ishap_arap_scratch_bytes", v.shape[0], t.shape[0], c.shape[0])
    _lib.call(dev, "ishap_arap", v.data_ptr(), v.shape[0], t.data_ptr(), t.shape[0], c.data_ptr() if ids.size else None,
              cp.data_ptr() if ids.size else None, c.shape[0], K, float(tol), 0 if max_cg is None else int(max_cg),
              out.data_ptr(), energy.data_ptr(), iters.data_ptr(), scratch.data_ptr(), nbytes)
    it = iters[:K].cpu().numpy().astype(np.int64)
    info = {"energy": energy[:K].cpu().numpy(), "cg_iters": np.abs(it), "converged": it >= 0}
    return out, info


def arap(mesh, static_ids, handle_ids, handle_pos, max_iter: int = 50, path=None, device=None):
    """meshProcess.arap (meshProcess.py:222-236): static vertices stay at rest, handles go to handle_pos, max_iter
    alternations.  Returns (vertices [V,3] float32, triangles [F,3] int32) on the device.  The reference always writes
    the result to '1.obj' in the working directory; here an OBJ is written only when `path` is given."""
    static = _host_ids(static_ids, "static_ids")
    handles = _host_ids(handle_ids, "handle_ids")
    hp = _host_positions(handle_pos, handles.size, "handle_pos")
    both = np.intersect1d(static, handles)
    if both.size:
        raise ValueError(f"vertices both static and handle: {both[:8].tolist()}")
    nv = _num_vertices(mesh)
    _check_ids(static, nv, "static_ids")
    _check_ids(handles, nv, "handle_ids")
    v, t = device_mesh(mesh, device)
    dev = v.device
    ids = np.concatenate([static, handles])
    pos = torch.cat([v[torch.from_numpy(static).to(dev)], _lib.tensor(hp, torch.float32, dev, (-1, 3)) if handles.size else v[:0]]).contiguous()
    new_v, _ = deform_as_rigid_as_possible(v, t, ids, pos, max_iter=max_iter)
    if path is not None:
        _write_obj(path, new_v, t)
    return new_v, t


def nearest_vertices(mesh, points, device=None) -> torch.Tensor:
    """For every point the index of its nearest mesh vertex (fp64 squared distance), the lowest index on ties: main.py's
    KD-tree pick of drag handles.  int64 [P] on the device."""
    v, _ = device_mesh(mesh, device)
    p = _lib.tensor(points, torch.float32, v.device, (-1, 3))
    idx = torch.empty(p.shape[0], dtype=torch.int32, device=v.device)
    if p.shape[0] == 0:
        return idx.long()
    if v.shape[0] == 0:
        raise ValueError("nearest_vertices: the mesh has no vertices")
    _lib.call(v.device, "ishap_nearest_vertices", v.data_ptr(), v.shape[0], p.data_ptr(), p.shape[0], idx.data_ptr())
    return idx.long()
