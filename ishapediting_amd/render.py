"""Headless rendering and pixel picking on the device: what the reference asks of Open3D's scene widget, without Open3D.

  render_mesh      render_to_image + render_to_depth_image (main.py:345-360): colour, depth and triangle id per pixel
  unproject        camera.unproject(x, y, depth, w, h) (main.py:501-505)
  pick             the Ctrl-click handler (main.py:492-509): pixel -> nearest mesh vertex, or a point at the source's depth
  Camera.fit       setup_camera(60, bounds, center) (main.py:611-612)
  marker_sphere / marker_arrow / edit_parts   draw_point / draw_arrow (main.py:539-590)
  save_picture     _save_pic_done (main.py:345-360): white wherever depth == 1, written as PNG

Every pixel comes from libishap_hip.so (csrc/render.hip: ishap_render_mesh, ishap_unproject); there is no CPU fallback.  The
projection, coverage, depth and shading are this library's own statement (include/ishap.h; in fp64: tests/render_ref.py).
Parity with Open3D's pictures (Filament's lighting, its camera framing) is unpinned: Open3D cannot run here.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import zlib
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .mesh import OccupancyMesh
from .metrics import device_mesh

MESH_COLOUR = (0.7, 0.7, 0.7)
RED, BLUE, GREEN = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0)      # main.py:513, 516, 550


@dataclass
class Camera:
    """Looks from `eye` at `centre`; `fov` is the vertical field of view in degrees; pixels are square."""
    eye: tuple
    centre: tuple = (0.0, 0.0, 0.0)
    up: tuple = (0.0, 1.0, 0.0)
    fov: float = 60.0
    near: float = 0.1
    far: float = 10.0

    @classmethod
    def fit(cls, bounds_min, bounds_max, fov: float = 60.0, aspect: float = 1.0) -> "Camera":
        """setup_camera(fov, bounds, center): look at the centre of the bounds along -z from centre + (0, 0, 1.25 *
        max_extent), up (0, 1, 0) -- the eye placement is after Open3D's behaviour, unpinned.  Where that distance would
        leave part of the bounding box outside a picture of width / height = `aspect` (a cube at fov 60 needs 1.37
        extents), the eye moves back along +z just far enough.  near / far enclose the bounding sphere strictly."""
        lo, hi = np.asarray(bounds_min, np.float64).reshape(3), np.asarray(bounds_max, np.float64).reshape(3)
        centre, half = (lo + hi) / 2, (hi - lo) / 2
        if not (half >= 0).all() or not half.max() > 0:
            raise ValueError(f"Camera.fit: empty bounds {lo} .. {hi}")
        t = math.tan(math.radians(fov) / 2)
        dist = max(1.25 * 2 * half.max(), half[2] + 1.02 * max(half[1] / t, half[0] / (t * aspect)))
        radius = float(np.linalg.norm(half))
        return cls(eye=tuple(centre + (0, 0, dist)), centre=tuple(centre), up=(0.0, 1.0, 0.0), fov=float(fov),
                   near=0.9 * (dist - radius), far=1.1 * (dist + radius))

    def _c(self) -> _lib.CameraC:
        c = _lib.CameraC()
        for k in range(3):
            c.eye[k], c.centre[k], c.up[k] = float(self.eye[k]), float(self.centre[k]), float(self.up[k])
        c.fov_y_deg, c.near, c.far = float(self.fov), float(self.near), float(self.far)
        return c


class RenderResult(NamedTuple):
    rgb: torch.Tensor        # uint8 [H, W, 3], background (0, 0, 0)
    depth: torch.Tensor      # float32 [H, W], background exactly 1
    tri_id: torch.Tensor     # int32 [H, W], background -1; indices into the concatenated triangle list


def _vertex_normals(v: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    """mesh.vertex_normals (area-weighted face normals summed per vertex, normalised) with the sums kept in fp64: the device's
    scatter-add has no fixed order, and an fp64 sum rounds to the same fp32 normal whatever the order, so that two renders of
    one mesh give the same bits."""
    p, idx = v.double(), t.long()
    fn = torch.cross(p[idx[:, 1]] - p[idx[:, 0]], p[idx[:, 2]] - p[idx[:, 0]], dim=1)
    out = torch.zeros_like(p)
    for k in range(3):
        out.index_add_(0, idx[:, k], fn)
    return (out / out.norm(dim=1, keepdim=True).clamp_min(1e-300)).float().contiguous()


def _part_arrays(mesh, lit: bool, dev):
    v, t = device_mesh(mesh, dev)
    if not lit:
        return v, t, torch.zeros_like(v)
    if isinstance(mesh, OccupancyMesh) and mesh._vnormals is not None and mesh._vnormals.device == v.device:
        return v, t, mesh._vnormals.detach().float().contiguous()
    return v, t, _vertex_normals(v, t)


def render_mesh(mesh_or_parts, camera: Camera, width: int, height: int, device=None) -> RenderResult:
    """Renders a mesh (anything mesh.mesh_arrays accepts, or an OBJ path), or a LIST of (mesh, colour, lit) parts
    (colour: r, g, b in [0, 1]; lit parts are shaded with their area-weighted vertex normals, unlit ones are painted flat),
    in one call: the parts are concatenated, `tri_id` counts through them in order."""
    dev = _lib.need_gpu(device, "mesh metrics", "run")
    parts = mesh_or_parts if isinstance(mesh_or_parts, list) else [(mesh_or_parts, MESH_COLOUR, True)]
    vs, ts, ns, ids, table, base = [], [], [], [], [], 0
    for k, (m, colour, lit) in enumerate(parts):
        v, t, n = _part_arrays(m, bool(lit), dev)
        vs.append(v); ts.append(t + base); ns.append(n)
        ids.append(torch.full((t.shape[0],), k, dtype=torch.int32, device=dev))
        table.append([float(colour[0]), float(colour[1]), float(colour[2]), 1.0 if lit else 0.0])
        base += v.shape[0]
    v = torch.cat(vs).contiguous() if vs else torch.zeros((0, 3), dtype=torch.float32, device=dev)
    t = torch.cat(ts).to(torch.int32).contiguous() if ts else torch.zeros((0, 3), dtype=torch.int32, device=dev)
    n = torch.cat(ns).contiguous() if ns else v
    part = torch.cat(ids).contiguous() if ids else torch.zeros(0, dtype=torch.int32, device=dev)
    table = torch.tensor(table or [[0.0, 0.0, 0.0, 0.0]], dtype=torch.float32, device=dev)
    return render_arrays(v, t, camera, width, height, normals=n, tri_part=part, parts=table)


def render_arrays(verts: torch.Tensor, tris: torch.Tensor, camera: Camera, width: int, height: int, normals=None,
                  tri_part=None, parts=None) -> RenderResult:
    """ishap_render_mesh on device arrays: verts [V,3] float32, tris [F,3] int32, normals [V,3] or None (flat face normals),
    tri_part [F] int32 or None, parts [P,4] (r, g, b, lit) or None (one lit grey part)."""
    dev = _lib.need_gpu(verts, "render")
    width, height = int(width), int(height)
    v = _lib.tensor(verts, torch.float32, shape=(-1, 3))
    t = _lib.tensor(tris, torch.int32, dev, (-1, 3))
    nrm = None if normals is None else _lib.tensor(normals, torch.float32, dev, (-1, 3))
    tp = None if tri_part is None else _lib.tensor(tri_part, torch.int32, dev)
    if parts is None:
        parts = torch.tensor([[*MESH_COLOUR, 1.0]], dtype=torch.float32, device=dev)
    pt = _lib.tensor(parts, torch.float32, dev, (-1, 4))
    if nrm is not None and nrm.shape != v.shape:
        raise ValueError(f"normals {tuple(nrm.shape)} do not match vertices {tuple(v.shape)}")
    if tp is not None and tp.shape[0] != t.shape[0]:
        raise ValueError(f"tri_part has {tp.shape[0]} entries for {t.shape[0]} triangles")
    try:
        scratch, nbytes = _lib.scratch(dev, "ishap_render_scratch_bytes", v.shape[0], t.shape[0], width, height)
    except _lib.ScratchError:
        raise ValueError(f"render: invalid sizes ({v.shape[0]} vertices, {t.shape[0]} triangles, {width} x {height})") from None
    rgb = torch.empty((height, width, 3), dtype=torch.uint8, device=dev)
    depth = torch.empty((height, width), dtype=torch.float32, device=dev)
    tri_id = torch.empty((height, width), dtype=torch.int32, device=dev)
    cam = camera._c()
    _lib.call(dev, "ishap_render_mesh", _lib.ptr(v) if v.shape[0] else None, v.shape[0], _lib.ptr(t) if t.shape[0] else None,
              t.shape[0], _lib.ptr(nrm), _lib.ptr(tp) if tp is not None and tp.shape[0] else None, pt.data_ptr(), pt.shape[0],
              C.byref(cam), width, height, scratch.data_ptr(), nbytes, rgb.data_ptr(), depth.data_ptr(), tri_id.data_ptr())
    return RenderResult(rgb, depth, tri_id)


def unproject(camera: Camera, x, y, depth, width: int, height: int, device=None) -> torch.Tensor:
    """camera.unproject(x, y, depth, width, height): the world point of pixel (x, y) -- its centre -- at `depth`.  Scalars
    give a [3] tensor, arrays of n values an [n, 3] tensor, float32 on the device."""
    dev = _lib.need_gpu(device, "mesh metrics", "run")
    scalar = np.ndim(x) == 0 and np.ndim(y) == 0 and np.ndim(depth) == 0

    def host(a):
        return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    xyd = np.stack(np.broadcast_arrays(host(x), host(y), host(depth)), axis=-1).astype(np.float32).reshape(-1, 3)
    d_xyd = torch.from_numpy(np.ascontiguousarray(xyd)).to(dev)
    world = torch.empty((xyd.shape[0], 3), dtype=torch.float32, device=dev)
    cam = camera._c()
    _lib.call(dev, "ishap_unproject", C.byref(cam), int(width), int(height), _lib.ptr(d_xyd) if xyd.shape[0] else None,
              xyd.shape[0], _lib.ptr(world) if xyd.shape[0] else None)
    return world[0] if scalar else world


def pick(mesh, camera: Camera, depth_image, x: int, y: int, source_depth=None):
    """The Ctrl-click of main.py:496-509 on pixel (x, y) of `depth_image` (a render's depth, [H, W]).
    On the surface: (vertex position float32 [3], vertex index, depth) -- the mesh vertex nearest to the unprojected point
    (deform.nearest_vertices); keep `depth` as the next call's source_depth, as the GUI does for a target.
    On background (depth == 1): the point unprojected at `source_depth` (float32 [3]) when one is given, else None."""
    from .deform import nearest_vertices
    h, w = int(depth_image.shape[0]), int(depth_image.shape[1])
    depth = float(depth_image[int(y), int(x)])
    if depth == 1.0:
        if source_depth is None:
            return None
        return unproject(camera, int(x), int(y), float(source_depth), w, h).cpu().numpy()
    world = unproject(camera, int(x), int(y), depth, w, h)
    v, t = device_mesh(mesh, world.device)
    idx = int(nearest_vertices((v, t), world.reshape(1, 3))[0])
    return v[idx].cpu().numpy(), idx, depth


# ---------------------------------------------------------------- markers (host generators of closed triangle meshes)
def marker_sphere(point, radius: float = 0.04, segments: int = 16):
    """draw_point's sphere (main.py:541, radius 0.04) around `point`: a closed latitude / longitude mesh, 2 * segments
    meridians by `segments` parallels.  (vertices [V,3] float32, triangles [F,3] int32)."""
    n_lon, n_lat = 2 * segments, segments
    p = np.asarray(point, np.float64).reshape(3)
    theta = np.pi * np.arange(1, n_lat) / n_lat                       # the rings between the poles
    phi = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.sin(theta)[:, None] * np.cos(phi)[None], np.sin(theta)[:, None] * np.sin(phi)[None],
                     np.repeat(np.cos(theta)[:, None], n_lon, 1)], axis=-1).reshape(-1, 3)
    verts = np.concatenate([[[0, 0, 1.0]], ring, [[0, 0, -1.0]]]) * radius + p
    south = 1 + (n_lat - 1) * n_lon
    tris = []
    for j in range(n_lon):
        k = (j + 1) % n_lon
        tris.append((0, 1 + j, 1 + k))
        for i in range(n_lat - 2):
            a, b = 1 + i * n_lon, 1 + (i + 1) * n_lon
            tris.append((a + j, b + j, b + k))
            tris.append((a + j, b + k, a + k))
        last = 1 + (n_lat - 2) * n_lon
        tris.append((south, last + k, last + j))
    return verts.astype(np.float32), np.asarray(tris, np.int32)


def marker_arrow(start, end, segments: int = 20):
    """draw_arrow's arrow from `start` to `end` (main.py:576-583): a cylinder of radius 0.02 under a cone of radius 0.04 and
    height min(0.1, half the length), as ONE closed mesh (base disc, shaft, the ring under the cone, the cone)."""
    a, b = np.asarray(start, np.float64).reshape(3), np.asarray(end, np.float64).reshape(3)
    length = float(np.linalg.norm(b - a))
    if not length > 0:
        raise ValueError("marker_arrow: start and end coincide")
    cone_h = min(0.1, 0.5 * length)
    shaft_h = length - cone_h
    z = (b - a) / length
    x = np.cross(z, (1.0, 0, 0) if abs(z[0]) < 0.9 else (0, 1.0, 0))
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    phi = 2 * np.pi * np.arange(segments) / segments
    circle = np.cos(phi)[:, None] * x[None] + np.sin(phi)[:, None] * y[None]
    n = segments
    verts = np.concatenate([a[None], a + 0.02 * circle, a + shaft_h * z + 0.02 * circle, a + shaft_h * z + 0.04 * circle, b[None]])
    r0, r1, r2, tip = 1, 1 + n, 1 + 2 * n, 1 + 3 * n
    tris = []
    for j in range(n):
        k = (j + 1) % n
        tris.append((0, r0 + k, r0 + j))
        for lo, hi in ((r0, r1), (r1, r2)):
            tris.append((lo + j, lo + k, hi + k))
            tris.append((lo + j, hi + k, hi + j))
        tris.append((r2 + j, r2 + k, tip))
    return verts.astype(np.float32), np.asarray(tris, np.int32)


_PRISM_TRIS = np.array([[0, 2, 1], [0, 3, 2], [4, 5, 6], [4, 6, 7], [0, 1, 5], [0, 5, 4], [1, 2, 6], [1, 6, 5], [2, 3, 7], [2, 7, 6],
                        [3, 0, 4], [3, 4, 7]], np.int32)


def marker_box(lo, hi, thickness: float = 0.012):
    """The wire frame of the axis-aligned box lo..hi (a keep / free region of an edit): its twelve edges as thin square prisms
    of side `thickness`, each a closed mesh of 8 vertices and 12 triangles that overlaps its neighbours at the corners.
    (vertices [96,3] float32, triangles [144,3] int32)."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi >= lo).all()):
        raise ValueError(f"marker_box: need finite lo <= hi, got {lo.tolist()} and {hi.tolist()}")
    h = 0.5 * float(thickness)
    verts, tris = [], []
    for axis in range(3):                                   # the four edges along each axis
        o1, o2 = (axis + 1) % 3, (axis + 2) % 3
        for c1 in (lo[o1], hi[o1]):
            for c2 in (lo[o2], hi[o2]):
                a, b = np.empty(3), np.empty(3)
                a[axis], b[axis] = lo[axis] - h, hi[axis] + h
                a[o1], b[o1], a[o2], b[o2] = c1 - h, c1 + h, c2 - h, c2 + h
                x0, y0, z0, x1, y1, z1 = *a, *b
                tris.append(_PRISM_TRIS + len(verts) * 8)
                verts.append(np.array([[x0, y0, z0], [x1, y0, z0], [x1, y1, z0], [x0, y1, z0],
                                       [x0, y0, z1], [x1, y0, z1], [x1, y1, z1], [x0, y1, z1]]))
    return np.concatenate(verts).astype(np.float32), np.concatenate(tris).astype(np.int32)


KEEP_COLOUR = (1.0, 0.7, 0.0)        # amber: the frame of a keep region
FREE_COLOUR = (0.0, 0.7, 0.7)        # teal: the frame of a free region


def edit_parts(mesh, sources, targets, mesh_colour=MESH_COLOUR, boxes=()):
    """The scene of an edit as render_mesh parts: the mesh (lit), a red sphere at every source and a blue one at every
    target (unlit, main.py:513-516, 543-545), a green arrow from each source to its target (lit, main.py:517, 587).
    boxes: region frames to draw, each a marker_box mesh or a (marker_box mesh, colour) pair (default colour KEEP_COLOUR)."""
    src = np.asarray(sources, np.float64).reshape(-1, 3)
    tgt = np.asarray(targets, np.float64).reshape(-1, 3)
    if src.shape != tgt.shape:
        raise ValueError(f"{src.shape[0]} sources for {tgt.shape[0]} targets")
    parts = [(mesh, mesh_colour, True)]
    parts += [(marker_sphere(p), RED, False) for p in src]
    parts += [(marker_sphere(p), BLUE, False) for p in tgt]
    parts += [(marker_arrow(s, e), GREEN, True) for s, e in zip(src, tgt) if np.linalg.norm(e - s) > 0]
    for b in boxes:
        frame, colour = b if isinstance(b[1], tuple) and len(b[1]) == 3 and not hasattr(b[1], "shape") else (b, KEEP_COLOUR)
        parts.append((frame, colour, False))
    return parts


# ---------------------------------------------------------------- pictures
def _png(rgb: np.ndarray) -> bytes:
    h, w, _ = rgb.shape

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    rows = np.concatenate([np.zeros((h, 1), np.uint8), rgb.reshape(h, w * 3)], axis=1)      # filter type 0 on every row
    return (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
            chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))


def save_picture(path, result) -> np.ndarray:
    """_save_pic_done (main.py:345-360): the colour picture with white wherever depth == 1, written as an 8-bit RGB PNG
    (standard library only).  `result`: a RenderResult or an (rgb, depth) pair, tensors or arrays.  Returns the pixels."""
    rgb, depth = result[0], result[1]
    rgb = rgb.detach().cpu().numpy() if torch.is_tensor(rgb) else np.asarray(rgb)
    depth = depth.detach().cpu().numpy() if torch.is_tensor(depth) else np.asarray(depth)
    img = np.ascontiguousarray(rgb, dtype=np.uint8).copy()
    if img.ndim != 3 or img.shape[2] != 3 or depth.shape != img.shape[:2]:
        raise ValueError(f"save_picture: rgb {img.shape} / depth {depth.shape}")
    img[depth == 1.0] = 255
    with open(path, "wb") as fh:
        fh.write(_png(img))
    return img
