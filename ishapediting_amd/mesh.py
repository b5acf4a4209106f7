"""Mesh side of get_mesh (reference: triplane_decoder/visualize.py:100-104 = PyMCubes marching cubes at level 0 +
vertices/res*2-1; drag_utils.py:300 = Open3D filter_smooth_simple(10); meshProcess.py:18-35 = Chamfer distance).

Those are third-party CPU calls outside the kernel path.  Here the surface is produced ON THE
DEVICE by csrc/surface.hip (marching cubes on the resident volume, smoothing, nearest-neighbour Chamfer on area-uniform
surface samples) through the C ABI (ishap_surface_count / _emit, ishap_mesh_smooth, ishap_chamfer); this module only
allocates the outputs.  extract_surface_sparse / SparseOccupancyMesh cut the same surface at resolutions the dense volume cannot
reach, from bricks near the surface only (csrc/sparse_surface.hip).  The backend is an explicit choice, never an import probe: BACKEND = "device" (default) or
"third_party" (the reference's own PyMCubes / Open3D calls on the host, for users who have them and want that exact mesh).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np
import torch

from . import _lib


MAX_OBJ_VERTICES = 4_000_000      # text export of a DENSE volume's mesh: more is noise, not a surface (a 256^3 shape has well under
                                  # a million vertices); sparse high-resolution meshes have their own limit, MAX_SPARSE_OBJ_VERTICES
BACKEND = "device"                # "device" | "open3d" | "third_party"; set explicitly, results never depend on what happens to be installed
METHODS = {"marching_tetrahedra": 0, "marching_cubes": 1}


def extract_surface(volume: torch.Tensor, level: float = 0.0, method: str = "marching_cubes"):
    """Level-`level` triangle mesh of a [res,res,res] volume: (vertices [V,3] float32 in grid coordinates,
    triangles [F,3] int32), both on the device, in voxel order (deterministic).  method: "marching_cubes" (what the
    reference calls, visualize.py:100) or "marching_tetrahedra"."""
    meth = METHODS[method]
    _lib.need_gpu(volume, "extract_surface")
    assert volume.dim() == 3 and volume.shape[0] == volume.shape[1] == volume.shape[2]
    res = volume.shape[0]
    dev = volume.device
    vol = _lib.tensor(volume, torch.float32)
    scratch, _ = _lib.scratch(dev, "ishap_surface_scratch_bytes", res)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.call(dev, "ishap_surface_count", vol.data_ptr(), res, float(level), meth, scratch.data_ptr(), counts.data_ptr())
    nv, nt = (int(c) for c in counts.tolist())                 # the one host read-back: output sizes
    verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    tris = torch.empty((nt, 3), dtype=torch.int32, device=dev)
    if nv and nt:
        _lib.call(dev, "ishap_surface_emit", vol.data_ptr(), res, float(level), meth, scratch.data_ptr(), verts.data_ptr(),
                  tris.data_ptr())
    return verts, tris


def surface_counts(volume: torch.Tensor, level: float = 0.0, method: str = "marching_cubes"):
    """(vertices, triangles) of the level surface without emitting it."""
    meth = METHODS[method]
    _lib.need_gpu(volume, "surface_counts")
    res = volume.shape[0]
    dev = volume.device
    vol = _lib.tensor(volume, torch.float32)
    scratch, _ = _lib.scratch(dev, "ishap_surface_scratch_bytes", res)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.call(dev, "ishap_surface_count", vol.data_ptr(), res, float(level), meth, scratch.data_ptr(), counts.data_ptr())
    nv, nt = counts.tolist()
    return int(nv), int(nt)


def smooth_mesh(verts: torch.Tensor, tris: torch.Tensor, iterations: int = 10, box_max: float = 0.0) -> torch.Tensor:
    """filter_smooth_simple (drag_utils.py:300) on the device; returns new vertex positions.  box_max > 0: `verts` are grid
    coordinates of a [0, box_max]^3 volume whose surface may be cut open by the box (each neighbour still counts once)."""
    _lib.need_gpu(verts, "smooth_mesh")
    out = _lib.tensor(verts, torch.float32).clone()
    tris = _lib.tensor(tris, torch.int32)
    if out.shape[0] == 0 or tris.shape[0] == 0 or iterations <= 0:
        return out
    try:
        scratch, nbytes = _lib.scratch(out.device, "ishap_mesh_smooth_scratch_bytes", out.shape[0], tris.shape[0])
    except _lib.ScratchError:
        raise RuntimeError("ishap_mesh_smooth_scratch_bytes: invalid sizes") from None
    _lib.call(out.device, "ishap_mesh_smooth", out.data_ptr(), out.shape[0], tris.data_ptr(), tris.shape[0], int(iterations),
              float(box_max), scratch.data_ptr(), nbytes)
    return out


class SimplifyInfo(NamedTuple):
    """simplify_vertex_clustering: non-empty cells, vertices in / out, triangles in / with three distinct clusters / out (the
    difference of the last two is the duplicates dropped) and the bytes of device memory the call held at its end (scratch,
    counts and the outputs)"""
    clusters: int
    vertices_in: int
    vertices_out: int
    triangles_in: int
    triangles_nondegenerate: int
    triangles_out: int
    bytes: int


CONTRACTIONS = {"quadric": 0, "average": 1}
SIMPLIFY_MAX_CELLS = 1 << 30


def _checked_simplify(simplify) -> dict:
    """the `simplify` keyword of the mesh classes: None, a cell size in voxels, or {"cell": voxels, "contraction": ...,
    "regularization": ...}"""
    if simplify is None:
        return None
    if not isinstance(simplify, dict):
        simplify = {"cell": simplify}
    unknown = [k for k in simplify if k not in ("cell", "contraction", "regularization")]
    if unknown or "cell" not in simplify:
        raise ValueError(f'simplify must be None, a cell size or a dict with "cell" (and "contraction", "regularization"); got {simplify!r}')
    out = dict(simplify)
    out["cell"] = float(out["cell"])
    if not (out["cell"] > 0 and np.isfinite(out["cell"])):
        raise ValueError(f"simplify: the cell size must be positive and finite, not {out['cell']}")
    _check_choice("simplify contraction", out.get("contraction", "quadric"), tuple(CONTRACTIONS))
    return out


def simplify_vertex_clustering(verts: torch.Tensor, tris: torch.Tensor, cell: float, contraction: str = "quadric", origin=None,
                               dims=None, regularization: float = 1e-3, return_map: bool = False, return_clusters: bool = False):
    """Open3D's simplify_vertex_clustering(voxel_size=cell, contraction=Quadric | Average) on the device (csrc/simplify.hip; the
    rule: include/ishap.h, "Mesh simplification"): the vertices of each cell of the grid `origin + cell * [0, dims)` become one
    vertex -- the point that minimises the area-weighted squared distance to the planes of the cluster's triangles, pulled
    towards the cluster's mean by `regularization` and kept inside the cell ("quadric"), or the mean ("average") -- triangles
    with two corners in one cell go, and of several triangles on the same three cells in the same orientation the first stays.
    Returns (vertices [Vo,3] float32, triangles [Fo,3] int32, SimplifyInfo), with return_map also vertex_map [V] int32 (the
    output vertex of each input vertex, -1 where its cell is touched by no kept triangle), with return_clusters after it
    vertex_cluster [V] int32 (the cluster of each input vertex, clusters numbered in ascending cell id: the partition itself,
    also where no triangle is kept), all on the device.  Only integer
    atomics: the result is bit for bit the same from run to run and does not depend on the order of the input triangles or
    vertices (the output rows follow the cell ids and the input triangle order).
    origin: default verts.amin(0) as float64; dims: default floor((max - origin) / cell) + 1 per axis; vertices outside the
    grid are clamped into its border cells.  At most 2^30 cells.
    Memory: the scratch is sized before the number of clusters is known, 132 bytes for each of min(V, cells) POSSIBLE clusters
    besides 8 bytes per 32 cells, 4 per vertex and 8 to 20 per triangle -- about 1.3 GB of rows for a 10 M vertex mesh, of which
    the clusters there are use a fraction (SimplifyInfo.bytes reports what was held).
    Host read-backs: ONE for the output sizes (with the status word and the info counts); one more, before it, for the bounding
    box when origin or dims is left to the default.
    Raises RuntimeError if the accumulated triangle area of a cluster could overflow the 64-bit sums (2^26 cell faces in one
    cell): use a larger cell or contraction="average".
    Clustering can leave non-manifold edges and vertices where a feature is thinner than a cell (two sheets that fall into one
    cell are joined); nothing here repairs that."""
    _lib.need_gpu(verts, "simplify_vertex_clustering")
    _check_choice("contraction", contraction, tuple(CONTRACTIONS))
    cell, regularization = float(cell), float(regularization)
    if not (cell > 0 and np.isfinite(cell)):
        raise ValueError(f"simplify_vertex_clustering: the cell size must be positive and finite, not {cell}")
    if not (regularization > 0 and np.isfinite(regularization)):
        raise ValueError(f"simplify_vertex_clustering: regularization must be positive and finite, not {regularization}")
    dev = verts.device
    v = _lib.tensor(verts, torch.float32, shape=(-1, 3))
    t = _lib.tensor(tris, torch.int32, dev, (-1, 3))
    nv, nt = int(v.shape[0]), int(t.shape[0])
    if nv > 0x7fffffff or 3 * nt > 0x7fffffff:
        raise ValueError("simplify_vertex_clustering: vertex indices and 3 * triangles must fit int32")
    i32 = dict(dtype=torch.int32, device=dev)
    if nv == 0 or nt == 0:
        out = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), **i32), SimplifyInfo(0, nv, 0, nt, 0, 0, 0))
        out = out + (torch.full((nv,), -1, **i32),) if return_map else out
        return out + (torch.full((nv,), -1, **i32),) if return_clusters else out
    if origin is None or dims is None:
        box = torch.stack([v.amin(0), v.amax(0)]).to(torch.float64).cpu().numpy()          # the bounding-box read-back
        if not np.isfinite(box).all():
            raise ValueError("simplify_vertex_clustering: the vertices are not finite; pass origin and dims")
        if origin is None:
            origin = box[0]
    lo = np.asarray(origin, dtype=np.float64).reshape(3)
    if dims is None:
        dims = np.maximum(np.floor((box[1] - lo) / cell), 0).astype(np.int64) + 1
    dims = [int(d) for d in np.asarray(dims).reshape(3)]
    if min(dims) < 1 or dims[0] * dims[1] * dims[2] > SIMPLIFY_MAX_CELLS:
        raise ValueError(f"simplify_vertex_clustering: dims {dims} must be >= 1 with at most 2^30 cells; use a larger cell")
    lo_c, dims_c = (C.c_double * 3)(*lo.tolist()), (C.c_int * 3)(*dims)
    try:
        scratch, nbytes = _lib.scratch(dev, "ishap_mesh_simplify_scratch_bytes", nv, nt, dims_c)
    except _lib.ScratchError:
        raise RuntimeError("ishap_mesh_simplify_scratch_bytes: invalid sizes") from None
    counts = torch.empty(3, **i32)
    common = (v.data_ptr(), nv, t.data_ptr(), nt, lo_c, cell, dims_c, CONTRACTIONS[contraction])
    _lib.call(dev, "ishap_mesh_simplify_count", *common, scratch.data_ptr(), nbytes, counts.data_ptr())
    vo, to, status, clusters, nondeg = torch.cat([counts, scratch[:8].view(torch.int32)]).tolist()     # the one host read-back
    if status != 0:
        raise RuntimeError("simplify_vertex_clustering: the triangle area gathered in one cell reaches 2^26 cell faces, the "
                           "64-bit quadric sums could overflow; use a larger cell or contraction=\"average\"")
    out_v = torch.empty((max(vo, 1), 3), dtype=torch.float32, device=dev)      # an empty result still needs an address
    out_t = torch.empty((max(to, 1), 3), **i32)
    vmap = torch.empty(nv, **i32)
    vclus = torch.empty(nv, **i32) if return_clusters else None
    _lib.call(dev, "ishap_mesh_simplify_emit", *common, regularization, scratch.data_ptr(), nbytes, out_v.data_ptr(),
              out_t.data_ptr(), vmap.data_ptr(), _lib.ptr(vclus))
    out_v, out_t = out_v[:vo], out_t[:to]
    held = sum(x.numel() * x.element_size() for x in (scratch, counts, out_v, out_t, vmap))
    info = SimplifyInfo(int(clusters), nv, int(vo), nt, int(nondeg), int(to), held)
    out = (out_v, out_t, info, vmap) if return_map else (out_v, out_t, info)
    return out + (vclus,) if return_clusters else out


def chamfer_distance(pa: torch.Tensor, pb: torch.Tensor, point_num=20000, seed: int = 0, query_num=None) -> float:
    """meshProcess.py:18-35: mean squared nearest-neighbour distance a->b plus b->a on `point_num` samples per side
    (the reference samples mesh surfaces with Open3D; here the samples are drawn from the given point sets).
    point_num=None uses every point (no sampling floor).  query_num (with point_num=None): only the QUERY side of each
    direction is a random subset of that many points, the nearest neighbour is searched in the COMPLETE other set -- an
    unbiased estimate of the all-points value without its quadratic cost and without a sampling floor (the floor of the
    sampled form comes from thinning the target set)."""
    _lib.need_gpu(pa, "chamfer_distance")
    g = torch.Generator(device="cpu").manual_seed(seed)

    def pick(p, n):
        if n is None or p.shape[0] <= n:
            return p
        return p[torch.randperm(p.shape[0], generator=g)[:n].to(p.device)]

    def run(a, b):
        nearest = torch.empty(max(a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
        out2 = torch.empty(2, dtype=torch.float32, device=a.device)
        _lib.call(a.device, "ishap_chamfer", a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], nearest.data_ptr(), out2.data_ptr())
        return out2.tolist()
    a = _lib.tensor(pick(pa, point_num), torch.float32)
    b = _lib.tensor(pick(pb, point_num), torch.float32, a.device)
    if a.shape[0] == 0 or b.shape[0] == 0:
        return float("nan")
    if query_num is not None and point_num is None:
        return float(run(pick(a, query_num).contiguous(), b)[0] + run(pick(b, query_num).contiguous(), a)[0])
    d = run(a, b)
    return float(d[0] + d[1])


def mesh_chamfer(mesh_a, mesh_b, point_num: int = 20000, seed: int = 0) -> float:
    """calc_chamfer (meshProcess.py:18-35): `point_num` points sampled uniformly BY AREA on each surface
    (sample_points_uniformly), then the two mean squared nearest-neighbour distances.  mesh_*: (vertices, triangles) pairs
    or OccupancyMesh objects, on the device."""
    def vt(m):
        return (m.vertices, m.triangles) if isinstance(m, OccupancyMesh) else m
    (va, ta), (vb, tb) = vt(mesh_a), vt(mesh_b)
    g = torch.Generator(device="cpu").manual_seed(seed)
    pa = sample_surface_points(va, ta, point_num, g)
    pb = sample_surface_points(vb, tb, point_num, g)
    return chamfer_distance(pa, pb, point_num=None)


class _Points:
    """What `np.asarray(mesh.vertices)` / `len(mesh.vertices)` need (main.py:507): a lazy host view of a device array."""

    def __init__(self, fetch):
        self._fetch = fetch

    def __array__(self, dtype=None, copy=None):
        a = self._fetch()
        return a if dtype is None else a.astype(dtype, copy=False)

    def __len__(self):
        return int(self._fetch().shape[0])


class OccupancyMesh:
    """The mesh get_mesh returns with the default "device" backend: the device volume plus, on first use, its surface
    (vertices in the reference's convention grid/res*2-1, visualize.py:101) after `smooth_iterations` sweeps.

    It carries the part of open3d.geometry.TriangleMesh's surface the reference's GUI touches on `drag_stuff.mesh`
    (main.py:288,314,373,478,507) -- `has_vertex_normals()`, `has_triangle_normals()`, `compute_vertex_normals()`,
    `np.asarray(mesh.vertex_normals)`, `copy.deepcopy` -- and `to_open3d()`, which builds the real TriangleMesh for
    `update_mesh` (Open3D is imported only there, when called).  `.vertices` / `.triangles` stay device tensors (the
    product's own consumers: Chamfer, sampling, OBJ export); `np.asarray` of them works through torch's __array__ only for
    host tensors, so GUI code goes through `to_open3d()` or `vertices_numpy()`.
    clean: None (the volume as given), or a dict of volume.clean_volume keywords: `.volume` is then the cleaned volume.
    refine: None, or a dict {decoder, planes, iterations, max_move}: the decoder and the channels-last planes the volume was
    decoded from.  The smoothed vertices are then put back on the decoder's zero level set
    (triplane_decoder.project_to_surface: `iterations` steps, default 4, none further than `max_move`, default one voxel,
    in decoder coordinates) with the triangles unchanged, and compute_vertex_normals() stores the field's analytic normals
    -grad / |grad| (the direction of decreasing logit: outward, logits are positive inside) instead of the triangle sum.
    Two further keys are passed on to project_to_surface when given: `step_max` (longest single step, default half a voxel)
    and `tol` (|logit| at which a vertex is left alone); any other key raises.
    simplify: None (nothing new runs: the mesh is bit for bit what it was), a cell size in voxels, or a dict {"cell": voxels,
    "contraction": "quadric" | "average", "regularization": 1e-3}: after smoothing and BEFORE refine the mesh goes through
    simplify_vertex_clustering in grid units with origin 0, so the cells line up with the voxel grid; refine then puts the
    fewer, moved vertices back on the level set and the field normals are per output vertex.  `.simplification` is the
    SimplifyInfo once the mesh is built."""

    def __init__(self, volume: torch.Tensor, res: int, smooth_iterations: int = 10, clean=None, refine=None, simplify=None):
        self.volume = volume if clean is None else _cleaned(volume, clean)
        self.res = res
        self.smooth_iterations = smooth_iterations
        self.refine = None if refine is None else _checked_refine(refine)
        self.simplify = _checked_simplify(simplify)
        self.simplification = None    # simplify: the SimplifyInfo once the mesh is built
        self._mesh = None
        self._vnormals = None
        self._field_normals = None
        self.refinement = None        # refine: (start [V,3], triplane_decoder.Projection) once the mesh is built

    def _build(self):
        if self._mesh is None:
            v, t = extract_surface(self.volume, 0.0)
            v = smooth_mesh(v, t, self.smooth_iterations, box_max=float(self.res - 1))     # in grid coordinates: the box is known
            v, t = self._simplified(v, t)
            if self.refine is not None and v.shape[0] > 0:
                v = self._refined(v)
            self._mesh = (v / self.res * 2 - 1, t)
        return self._mesh

    def _simplified(self, v: torch.Tensor, t: torch.Tensor):
        """grid units, origin 0, cells of `cell` voxels over the box [0, res - 1]: aligned with the voxel grid"""
        if self.simplify is None or v.shape[0] == 0 or t.shape[0] == 0:
            return v, t
        sp = self.simplify
        dims = [int(np.floor((self.res - 1) / sp["cell"])) + 1] * 3
        v, t, self.simplification = simplify_vertex_clustering(v, t, sp["cell"], sp.get("contraction", "quadric"), origin=(0.0, 0.0, 0.0),
                                                               dims=dims, regularization=sp.get("regularization", 1e-3))
        return v, t

    def _refined(self, v: torch.Tensor) -> torch.Tensor:
        """grid units -> the decoder coordinates the volume was sampled at (linspace(-1, 1, res): c = 2 g / (res - 1) - 1, NOT
        the vertex convention g / res * 2 - 1), project, and back to grid units"""
        from . import triplane_decoder as td              # triplane_decoder has no need of this module
        r = self.refine
        voxel = 2.0 / (self.res - 1)
        kw = {"iterations": int(r.get("iterations", 4)), "max_move": float(r.get("max_move", voxel))}
        kw["step_max"] = float(r.get("step_max", 0.5 * voxel))
        if "tol" in r:
            kw["tol"] = float(r["tol"])
        start = v * 2 / (self.res - 1) - 1
        p = td.project_to_surface(r["decoder"], r["planes"], start, **kw)
        self._field_normals = p.normals
        self.refinement = (start, p)                     # what went in and what came out, in decoder coordinates
        moved = (p.accepted > 0)[:, None]                # a vertex no step was taken for stays bit for bit where it was
        return torch.where(moved, (p.points + 1) * (self.res - 1) / 2, v)

    @property
    def vertices(self) -> torch.Tensor:
        return self._build()[0]

    @property
    def triangles(self) -> torch.Tensor:
        return self._build()[1]

    def counts(self):
        return surface_counts(self.volume, 0.0)

    # ---- the TriangleMesh surface main.py uses ----
    def vertices_numpy(self) -> np.ndarray:
        return self.vertices.detach().cpu().numpy().astype(np.float64)

    def triangles_numpy(self) -> np.ndarray:
        return self.triangles.detach().cpu().numpy().astype(np.int32)

    def has_vertex_normals(self) -> bool:
        return self._vnormals is not None

    def has_triangle_normals(self) -> bool:
        return False

    def compute_vertex_normals(self, normalized: bool = True):
        """TriangleMesh.compute_vertex_normals: area-weighted sum of the incident triangles' normals, normalised.
        With `refine` the stored normals are the field's analytic unit normals -grad / |grad| (outward), and the NORMALISED
        triangle sum at the vertices where the field has none (a vanishing gradient): unit vectors throughout, so
        `normalized` has no effect there."""
        if self._field_normals is None:
            self._vnormals = vertex_normals(self.vertices, self.triangles, normalized)
            return self
        has = (self._field_normals != 0).any(dim=1, keepdim=True)
        self._vnormals = torch.where(has, self._field_normals, vertex_normals(self.vertices, self.triangles, True))
        return self

    @property
    def vertex_normals(self):
        return _Points(lambda: np.zeros((0, 3)) if self._vnormals is None else self._vnormals.detach().cpu().numpy().astype(np.float64))

    def to_open3d(self):
        """The open3d.geometry.TriangleMesh the reference's get_mesh returns (visualize.py:102-104 + drag_utils.py:300):
        same vertices / triangles, already smoothed on the device.  Imports Open3D here and nowhere else."""
        import open3d as o3d
        m = o3d.geometry.TriangleMesh()
        m.vertices = o3d.utility.Vector3dVector(self.vertices_numpy())
        m.triangles = o3d.utility.Vector3iVector(self.triangles_numpy())
        if self._vnormals is not None:
            m.vertex_normals = o3d.utility.Vector3dVector(np.asarray(self.vertex_normals))
        return m

    def __deepcopy__(self, memo):
        m = OccupancyMesh(self.volume.clone(), self.res, self.smooth_iterations, simplify=self.simplify)
        m.refine = self.refine                           # the decoder and the planes are shared, not copied
        m.simplification = self.simplification
        if self._mesh is not None:
            m._mesh = (self._mesh[0].clone(), self._mesh[1].clone())
        if self._field_normals is not None:
            m._field_normals = self._field_normals.clone()
            m.refinement = self.refinement
        if self._vnormals is not None:
            m._vnormals = self._vnormals.clone()
        return m


class SparseSurfaceInfo(NamedTuple):
    """extract_surface_sparse: active bricks at the end, growth rounds that changed something (may vary from run to run with the
    scheduling of a round's workgroups; the other fields and the mesh do not), points decoded (729 per brick) and the bytes of
    device memory the call held at its end (maps, lists, values and reached bits with their reserve, scratch, the mesh)"""
    bricks: int
    rounds: int
    points: int
    bytes: int


SPARSE_MIN_RES, SPARSE_MAX_RES = 9, 2048
SPARSE_MAX_RATIO = 64      # a coarse seed volume [Rc]^3 serves fine grids with res - 1 <= 64 (Rc - 1): a coarse cell then marks at most 10^3 bricks


def extract_surface_sparse(decoder, planes: torch.Tensor, res: int, seeds, level: float = 0.0, max_rounds: int = 64,
                           max_bricks: int = 1 << 20):
    """The marching-cubes surface of the decoder's field on the FINE grid linspace(-1, 1, res)^3 (9 <= res <= 2048) without its
    dense volume: only bricks of 8^3 cells near the surface are decoded (triplane_decoder.decode_bricks) and cut
    (csrc/sparse_surface.hip; include/ishap.h states the scheme).  -> (vertices [V,3] float32 in fine-grid coordinates,
    triangles [F,3] int32, SparseSurfaceInfo), on the device.
    seeds: a coarse dense volume [Rc,Rc,Rc] of the same field (every brick that overlaps one of its crossing cells), "all"
    (every brick), or an int tensor [n,3] of brick coordinates (bx, by, bz), each in 0 .. ceil((res - 1) / 8) - 1.
    The result is exactly the connected components (triangles joined through shared vertices) of
    extract_surface(decode_planes_grid(decoder, planes, res), level) that cut a cell of a seeded brick, followed to their end
    through bricks the seeds did not name; with seeds="all" it is that mesh (the same vertices and triangles bit for bit, in
    brick order instead of voxel order).  Repeats bit for bit, whatever the order of the seeds.
    The growth stops when a round changes nothing; more than `max_rounds` rounds or `max_bricks` active bricks (2916 bytes of
    values each) raise RuntimeError -- never a partial mesh.  The host waits for the device at the count read-backs only: the
    seed count (coarse seeds only: the first decode has to be sized), one per growth round, one before the mesh is allocated.
    A coarse seed volume [Rc]^3 must satisfy res - 1 <= 64 (Rc - 1).
    info.rounds is NOT a property of the field: whether a brick sees a neighbour's newly reached edges in the same round or the
    next depends on how the round's workgroups were scheduled.  The mesh, info.bricks and info.points are (the reached set is a
    least fixed point); rounds has a lower bound (the brick distance the surface travels from the seeds) and may differ run to run."""
    from . import triplane_decoder as td              # triplane_decoder has no need of this module
    _lib.need_gpu(planes, "extract_surface_sparse")
    res, max_rounds, max_bricks = int(res), int(max_rounds), int(max_bricks)
    L = _lib.lib()
    nb = int(L.ishap_sparse_bricks_per_axis(res))
    if nb < 0:
        raise ValueError(f"extract_surface_sparse: res = {res} is outside {SPARSE_MIN_RES} .. {SPARSE_MAX_RES}")
    assert planes.dtype == torch.float32 and planes.is_contiguous() and planes.dim() == 4 and planes.shape[0] == 3 and planes.shape[3] == 32
    dev = planes.device
    N = nb ** 3
    i32 = dict(dtype=torch.int32, device=dev)
    bmap = torch.zeros(N, dtype=torch.uint8, device=dev)
    slot_map = torch.empty(N, **i32)
    blist = torch.empty(N + 1, **i32)                  # slot -> brick id, discovery order
    counters = torch.zeros(2, **i32)                   # {edge bits a growth round recorded, bricks a compaction listed}
    cscratch, cbytes = _lib.scratch(dev, "ishap_sparse_compact_scratch_bytes", res)
    axis = torch.linspace(-1, 1, res).to(dev)          # the table decode_planes_grid reads
    held = [bmap, slot_map, blist, cscratch]
    n0 = None
    if isinstance(seeds, str):
        if seeds != "all":
            raise ValueError(f'extract_surface_sparse: seeds must be a coarse volume, "all" or brick coordinates [n,3], not {seeds!r}')
        bmap.fill_(1)
        n0 = N
    elif torch.is_tensor(seeds) and seeds.is_floating_point():
        if seeds.dim() != 3 or not (seeds.shape[0] == seeds.shape[1] == seeds.shape[2]) or not 2 <= seeds.shape[0] <= SPARSE_MAX_RES:
            raise ValueError(f"extract_surface_sparse: a coarse seed volume is [Rc,Rc,Rc] with 2 <= Rc <= {SPARSE_MAX_RES}, not {tuple(seeds.shape)}")
        if res - 1 > SPARSE_MAX_RATIO * (seeds.shape[0] - 1):
            raise ValueError(f"extract_surface_sparse: a coarse volume of {seeds.shape[0]}^3 seeds fine grids up to "
                             f"{SPARSE_MAX_RATIO * (seeds.shape[0] - 1) + 1} (res - 1 <= {SPARSE_MAX_RATIO} (Rc - 1)), not {res}")
        coarse = _lib.tensor(seeds, torch.float32, dev)
        _lib.call(dev, "ishap_sparse_seed_volume", coarse.data_ptr(), coarse.shape[0], float(level), res, bmap.data_ptr())
    else:
        b = torch.as_tensor(seeds)
        if b.is_floating_point() or b.dim() != 2 or b.shape[1] != 3:
            raise ValueError("extract_surface_sparse: explicit seeds are an int tensor [n,3] of brick coordinates")
        b = b.detach().to(torch.int64).cpu()
        if b.numel() and (int(b.min()) < 0 or int(b.max()) >= nb):
            raise ValueError(f"extract_surface_sparse: brick coordinates must lie in 0 .. {nb - 1} (res = {res})")
        ids = torch.unique((b[:, 0] * nb + b[:, 1]) * nb + b[:, 2])
        bmap[ids.to(dev)] = 1
        n0 = int(ids.numel())
    _lib.call(dev, "ishap_sparse_compact", bmap.data_ptr(), res, 0, 0, slot_map.data_ptr(), blist.data_ptr(), N,
              counters[1:].data_ptr(), cscratch.data_ptr(), cbytes)
    if n0 is None:
        n0 = int(counters[1])                      # read-back: the seed count
    empty = (torch.empty((0, 3), dtype=torch.float32, device=dev), torch.empty((0, 3), **i32))
    if n0 == 0:
        return empty[0], empty[1], SparseSurfaceInfo(0, 0, 0, sum(t.numel() * t.element_size() for t in held))
    if n0 > max_bricks:
        raise RuntimeError(f"extract_surface_sparse: the seeds name {n0} bricks, more than max_bricks = {max_bricks}")
    n, rounds = n0, 0
    rbytes = int(L.ishap_sparse_reach_bytes(1))
    # values and reached bits live in buffers with room to grow: a round that adds bricks decodes them in place behind the
    # others; a full buffer is replaced by one half as large again (a copy per growth of 1.5x, not per round)
    cap = min(N, n + n // 4 + 16)
    values = torch.empty((cap, 729), dtype=torch.float32, device=dev)
    reach = torch.zeros((cap, rbytes), dtype=torch.uint8, device=dev)
    td._decode_bricks_into(decoder, planes, axis, res, blist[:n], values[:n])
    while True:
        counters.zero_()
        _lib.call(dev, "ishap_sparse_grow", values.data_ptr(), blist.data_ptr(), n, res, float(level), bmap.data_ptr(),
                  slot_map.data_ptr(), reach.data_ptr(), counters.data_ptr())
        _lib.call(dev, "ishap_sparse_compact", bmap.data_ptr(), res, 1, n, slot_map.data_ptr(), blist[n:].data_ptr(), N - n,
                  counters[1:].data_ptr(), cscratch.data_ptr(), cbytes)
        changed, new = (int(c) for c in counters.tolist())     # read-back: one per growth round
        if changed == 0 and new == 0:
            break
        rounds += 1
        if rounds > max_rounds:
            raise RuntimeError(f"extract_surface_sparse: the surface was still growing after max_rounds = {max_rounds} rounds "
                               f"({n} bricks active)")
        if new:
            if n + new > max_bricks:
                raise RuntimeError(f"extract_surface_sparse: round {rounds} reaches {n + new} active bricks, more than "
                                   f"max_bricks = {max_bricks}")
            if n + new > cap:
                cap = min(N, max(n + new, cap + cap // 2))
                grown = torch.empty((cap, 729), dtype=torch.float32, device=dev)
                grown[:n] = values[:n]
                values = grown
                grown = torch.zeros((cap, rbytes), dtype=torch.uint8, device=dev)
                grown[:n] = reach[:n]
                reach = grown
                del grown
            td._decode_bricks_into(decoder, planes, axis, res, blist[n:n + new], values[n:n + new])
            n += new
    # emission order: ascending brick id, so the order of discovery does not show
    ordered = torch.empty(n + 1, **i32)
    _lib.call(dev, "ishap_sparse_compact", bmap.data_ptr(), res, 2, 0, slot_map.data_ptr(), ordered.data_ptr(), n,
              counters[1:].data_ptr(), cscratch.data_ptr(), cbytes)
    escratch, ebytes = _lib.scratch(dev, "ishap_sparse_surface_scratch_bytes", res, n)
    counts = torch.zeros(2, **i32)
    common = (values.data_ptr(), ordered.data_ptr(), n, res, float(level), slot_map.data_ptr(), reach.data_ptr(),
              escratch.data_ptr(), ebytes)
    _lib.call(dev, "ishap_sparse_surface_count", *common, counts.data_ptr())
    nv, nt = (int(c) for c in counts.tolist())                 # read-back: output sizes
    verts = torch.empty((nv, 3), dtype=torch.float32, device=dev)
    tris = torch.empty((nt, 3), **i32)
    if nv and nt:
        _lib.call(dev, "ishap_sparse_surface_emit", *common, verts.data_ptr(), tris.data_ptr())
    held += [values, reach, ordered, escratch, verts, tris]
    return verts, tris, SparseSurfaceInfo(n, rounds, 729 * n, sum(t.numel() * t.element_size() for t in held))


class SparseOccupancyMesh(OccupancyMesh):
    """OccupancyMesh at a resolution the dense volume cannot reach: the surface of the decoder's field on the fine grid
    linspace(-1, 1, res)^3 (res up to 2048), cut by extract_surface_sparse from the bricks that `coarse` -- the dense volume the
    caller has anyway, e.g. DragStuff.volume at shape_resolution, after any cleaning -- shows a crossing in, and followed to its
    end.  `.volume` is that coarse volume; `.info` the SparseSurfaceInfo once the mesh is built.  Same public surface as
    OccupancyMesh: vertices (the reference's convention g / res * 2 - 1 of the fine grid coordinates g), triangles, counts,
    compute_vertex_normals, to_open3d, deepcopy; smoothing with box_max = res - 1.
    refine: None, or OccupancyMesh's dict WITHOUT decoder / planes (they are this mesh's own): the smoothed vertices go back on
    the zero level set through the same projection, by default no further than one FINE voxel.  It inherits what `_refined`
    documents: the projection works at the sampling convention 2 g / (res - 1) - 1, the vertices are handed out at
    g / res * 2 - 1, and the two differ by up to one voxel."""

    def __init__(self, decoder, planes: torch.Tensor, res: int, coarse: torch.Tensor, smooth_iterations: int = 10, refine=None,
                 max_rounds: int = 64, max_bricks: int = 1 << 20, simplify=None):
        if not SPARSE_MIN_RES <= int(res) <= SPARSE_MAX_RES:
            raise ValueError(f"SparseOccupancyMesh: res = {res} is outside {SPARSE_MIN_RES} .. {SPARSE_MAX_RES}")
        super().__init__(coarse, int(res), smooth_iterations,
                         refine=None if refine is None else dict(refine, decoder=decoder, planes=planes), simplify=simplify)
        self.decoder, self.planes = decoder, planes
        self.max_rounds, self.max_bricks = int(max_rounds), int(max_bricks)
        self.info = None

    def _build(self):
        if self._mesh is None:
            v, t, self.info = extract_surface_sparse(self.decoder, self.planes, self.res, self.volume, 0.0, self.max_rounds,
                                                     self.max_bricks)
            v = smooth_mesh(v, t, self.smooth_iterations, box_max=float(self.res - 1))
            v, t = self._simplified(v, t)                # cells in FINE voxels
            if self.refine is not None and v.shape[0] > 0:
                v = self._refined(v)
            self._mesh = (v / self.res * 2 - 1, t)
        return self._mesh

    def counts(self):
        v, t = self._build()
        return int(v.shape[0]), int(t.shape[0])

    def __deepcopy__(self, memo):
        m = SparseOccupancyMesh(self.decoder, self.planes, self.res, self.volume.clone(), self.smooth_iterations,
                                max_rounds=self.max_rounds, max_bricks=self.max_bricks, simplify=self.simplify)      # decoder and planes are shared
        m.refine, m.info, m.simplification = self.refine, self.info, self.simplification
        if self._mesh is not None:
            m._mesh = (self._mesh[0].clone(), self._mesh[1].clone())
        if self._field_normals is not None:
            m._field_normals = self._field_normals.clone()
            m.refinement = self.refinement
        if self._vnormals is not None:
            m._vnormals = self._vnormals.clone()
        return m


def sparse_volume_to_mesh(decoder, planes: torch.Tensor, res: int, coarse: torch.Tensor, smooth_iterations: int = 10,
                          backend: str = None, refine=None, simplify=None):
    """volume_to_mesh's counterpart for a mesh resolution above the decoded volume's: a SparseOccupancyMesh ("device") or its
    open3d.geometry.TriangleMesh ("open3d"); "third_party" has no sparse path and raises.  coarse: the dense volume (cleaned
    by the caller if it is to be), refine: OccupancyMesh's dict, decoder / planes taken from the arguments; simplify:
    OccupancyMesh's keyword, the cell in voxels of the FINE grid."""
    backend = BACKEND if backend is None else backend
    if backend not in ("device", "open3d"):
        raise ValueError(f'a sparse mesh needs the device surface (backend "device" or "open3d"), not {backend!r}')
    if refine is not None:
        refine = {k: v for k, v in refine.items() if k not in ("decoder", "planes")}
    m = SparseOccupancyMesh(decoder, planes, res, coarse, smooth_iterations, refine=refine, simplify=simplify)
    if backend == "device":
        return m
    return (m if refine is None else m.compute_vertex_normals()).to_open3d()


def vertex_normals(verts: torch.Tensor, tris: torch.Tensor, normalized: bool = True) -> torch.Tensor:
    """Per-vertex normals as Open3D's compute_vertex_normals defines them: the sum over incident triangles of the
    (unnormalised, i.e. area-weighted) face normal cross(v1 - v0, v2 - v0), then normalised.  Display-side plumbing in
    torch ops on the device (not on the timed path)."""
    v = verts.detach().to(torch.float32)
    t = tris.detach().to(device=v.device, dtype=torch.long)
    fn = torch.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]], dim=1)
    out = torch.zeros_like(v)
    for k in range(3):
        out.index_add_(0, t[:, k], fn)
    if normalized:
        out = out / out.norm(dim=1, keepdim=True).clamp_min(1e-30)
    return out


def mesh_arrays(mesh):
    """(vertices [V,3] float32, triangles [F,3] int32) as numpy from whatever a caller hands train_triplane(mesh=...):
    a (vertices, triangles) pair, an OccupancyMesh, or any object with `.vertices` / `.triangles` (an
    open3d.geometry.TriangleMesh, main.py:447-451) -- read with np.asarray, nothing Open3D-specific."""
    if isinstance(mesh, OccupancyMesh):
        return mesh.vertices_numpy().astype(np.float32), mesh.triangles_numpy()
    if isinstance(mesh, tuple):
        v, t = mesh
    else:
        v, t = mesh.vertices, mesh.triangles
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    if torch.is_tensor(t):
        t = t.detach().cpu().numpy()
    return np.asarray(v, dtype=np.float32).reshape(-1, 3), np.asarray(t, dtype=np.int32).reshape(-1, 3)


REFINE_KEYS = ("decoder", "planes", "iterations", "max_move", "step_max", "tol")


def _checked_refine(refine: dict) -> dict:
    if not isinstance(refine, dict) or "decoder" not in refine or "planes" not in refine:
        raise ValueError("refine must be a dict with at least `decoder` and `planes` (the channels-last planes of the volume)")
    unknown = [k for k in refine if k not in REFINE_KEYS]
    if unknown:
        raise ValueError(f"refine: unknown keys {unknown}; known: {REFINE_KEYS}")
    return dict(refine)


def _cleaned(volume: torch.Tensor, clean: dict) -> torch.Tensor:
    from . import volume as volume_ops              # volume.py imports this module
    return volume_ops.clean_volume(volume, **clean)


def volume_to_mesh(volume: torch.Tensor, res: int, smooth_iterations: int = 10, backend: str = None, clean=None, refine=None,
                   simplify=None):
    """get_mesh's mesh (drag_utils.py:298-300).  clean: None, or a dict of volume.clean_volume keywords (e.g.
    {"keep": "largest"}): floaters / cavities are taken out of the volume before the surface is made, for every backend.
    backend None -> the module-level BACKEND:
      "device"      OccupancyMesh (surface, smoothing on the device; vertices / triangles stay device tensors)
      "open3d"      the same device surface handed over as an open3d.geometry.TriangleMesh -- what the reference's GUI
                    expects from drag_stuff.mesh (main.py:288,314,373,478,507); only the final vertex / triangle arrays
                    cross PCIe (a few MB, not the 67 MB volume)
      "third_party" the reference's own PyMCubes + Open3D calls on the host.
    refine: None, or OccupancyMesh's refine dict {decoder, planes, iterations, max_move}: vertices back on the decoder's
    level set and analytic normals ("device"; "open3d" hands over that refined mesh with its normals; "third_party" raises).
    simplify: None, or OccupancyMesh's simplify keyword (a cell size in voxels or a dict): the smoothed mesh is reduced by
    quadric vertex clustering before refine ("device" and "open3d"; "third_party" raises)."""
    backend = BACKEND if backend is None else backend
    if clean is not None:
        volume = _cleaned(volume, clean)
    if backend == "device":
        return OccupancyMesh(volume, res, smooth_iterations, refine=refine, simplify=simplify)
    if backend == "open3d":
        m = OccupancyMesh(volume, res, smooth_iterations, refine=refine, simplify=simplify)
        return (m if refine is None else m.compute_vertex_normals()).to_open3d()
    if backend != "third_party":
        raise ValueError(f"unknown mesh backend {backend!r}")
    if refine is not None:
        raise ValueError('refine needs the device surface (backend "device" or "open3d"): the third_party meshes are made on the host')
    if simplify is not None:
        raise ValueError('simplify needs the device surface (backend "device" or "open3d"): the third_party meshes are made on the host')
    import mcubes
    import open3d as o3d
    vertices, triangles = mcubes.marching_cubes(volume.detach().cpu().numpy(), 0)
    vertices = vertices / res * 2 - 1                      # visualize.py:101 (create_obj_o3d's own convention)
    mesh = o3d.geometry.TriangleMesh()
    mesh.vertices = o3d.utility.Vector3dVector(vertices)
    mesh.triangles = o3d.utility.Vector3iVector(triangles)
    return mesh.filter_smooth_simple(number_of_iterations=smooth_iterations) if smooth_iterations > 0 else mesh


EXPORT_CHUNK = 1 << 18                 # rows that cross to the host and become text / bytes at a time
MAX_SPARSE_OBJ_VERTICES = 64_000_000   # a sparse mesh as OBJ text (about 100 bytes per vertex with its faces); beyond: .ply, or an error


def _write_obj(path, verts: torch.Tensor, tris: torch.Tensor):
    """Wavefront OBJ, streamed EXPORT_CHUNK rows at a time: neither the host copy nor the text of a mesh of tens of millions of
    vertices exists as a whole (the bytes are those of writing it in one piece)"""
    with open(path, "w") as fh:
        for s in range(0, verts.shape[0], EXPORT_CHUNK):
            v = verts[s:s + EXPORT_CHUNK].detach().cpu().numpy()
            fh.write("".join(f"v {p[0]:.6f} {p[1]:.6f} {p[2]:.6f}\n" for p in v))
        for s in range(0, tris.shape[0], EXPORT_CHUNK):
            f = tris[s:s + EXPORT_CHUNK].detach().cpu().numpy().astype(np.int64) + 1
            fh.write("".join(f"f {t[0]} {t[1]} {t[2]}\n" for t in f))


PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def write_ply(path, verts: torch.Tensor, tris: torch.Tensor):
    """binary little-endian PLY (float x y z; faces as uchar 3 + int32 indices), streamed EXPORT_CHUNK rows at a time: 12 bytes a
    vertex and 13 a triangle, no text formatting -- the format for meshes of tens of millions of vertices"""
    with open(path, "wb") as fh:
        fh.write((f"ply\nformat binary_little_endian 1.0\nelement vertex {int(verts.shape[0])}\nproperty float x\nproperty float y\n"
                  f"property float z\nelement face {int(tris.shape[0])}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii"))
        for s in range(0, verts.shape[0], EXPORT_CHUNK):
            fh.write(verts[s:s + EXPORT_CHUNK].detach().to(torch.float32).cpu().numpy().astype("<f4").tobytes())
        for s in range(0, tris.shape[0], EXPORT_CHUNK):
            t = tris[s:s + EXPORT_CHUNK].detach().cpu().numpy()
            rec = np.empty(t.shape[0], PLY_FACE)
            rec["n"], rec["v"] = 3, t
            fh.write(rec.tobytes())


def read_ply(path: str):
    """reader of write_ply's files: (vertices [V,3] float32, triangles [F,3] int32)"""
    with open(path, "rb") as fh:
        nv = nf = None
        while True:
            line = fh.readline().decode("ascii").strip()
            if line.startswith("element vertex"):
                nv = int(line.split()[-1])
            elif line.startswith("element face"):
                nf = int(line.split()[-1])
            elif line == "end_header":
                break
            elif not line:
                raise ValueError(f"{path}: no end_header")
        v = np.frombuffer(fh.read(12 * nv), "<f4").reshape(nv, 3)
        f = np.frombuffer(fh.read(PLY_FACE.itemsize * nf), PLY_FACE)
    if nf and not (f["n"] == 3).all():
        raise ValueError(f"{path}: only triangles are read")
    return v.astype(np.float32), f["v"].astype(np.int32).reshape(nf, 3)


def write_surface(path, verts: torch.Tensor, tris: torch.Tensor):
    """A sparse (high-resolution) mesh to a file, whatever its size: binary PLY when `path` ends in .ply, else streamed OBJ text up
    to MAX_SPARSE_OBJ_VERTICES vertices.  More than that as text raises RuntimeError naming the limit -- a mesh is never silently
    replaced by a stub."""
    if str(path).lower().endswith(".ply"):
        write_ply(path, verts, tris)
        return
    if verts.shape[0] > MAX_SPARSE_OBJ_VERTICES:
        raise RuntimeError(f"{path}: {int(verts.shape[0])} vertices / {int(tris.shape[0])} triangles exceed the OBJ text limit "
                           f"MAX_SPARSE_OBJ_VERTICES = {MAX_SPARSE_OBJ_VERTICES}; write a .ply (binary) instead")
    _write_obj(path, verts, tris)


def write_mesh(path, mesh):
    """o3d.io.write_triangle_mesh (drag_utils.py:470) when the mesh is an Open3D object; Wavefront OBJ of the device mesh otherwise.
    A SparseOccupancyMesh goes through write_surface (streamed OBJ, or binary PLY by extension; an error, never a stub, above its text
    limit); the MAX_OBJ_VERTICES stub is for dense volumes that are noise, not a surface."""
    if isinstance(mesh, SparseOccupancyMesh):
        write_surface(path, mesh.vertices, mesh.triangles)
        return
    if isinstance(mesh, OccupancyMesh):
        nv, nt = mesh.counts()
        if nv > MAX_OBJ_VERTICES:
            with open(path, "w") as f:
                f.write(f"# {nv} vertices / {nt} triangles: the volume is not a surface, mesh not written\n")
            return
        _write_obj(path, mesh.vertices, mesh.triangles)
        return
    import open3d as o3d
    o3d.io.write_triangle_mesh(path, mesh)


def read_obj(path: str):
    """Minimal Wavefront OBJ reader (v / f records, polygons fan-triangulated): (vertices [V,3] float32, triangles [F,3] int32)."""
    vs, fs = [], []
    with open(path) as fh:
        for line in fh:
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                vs.append([float(p[1]), float(p[2]), float(p[3])])
            elif p[0] == "f":
                idx = [int(t.split("/")[0]) for t in p[1:]]
                idx = [i - 1 if i > 0 else len(vs) + i for i in idx]
                fs.extend([idx[0], idx[k], idx[k + 1]] for k in range(1, len(idx) - 1))
    return np.asarray(vs, np.float32).reshape(-1, 3), np.asarray(fs, np.int32).reshape(-1, 3)


OCCUPANCY_METHODS = ("parity", "winding")
ORIENTATIONS = ("auto", "ccw", "cw")


def _check_choice(name: str, value, allowed):
    if value not in allowed:
        raise ValueError(f"{name} must be one of {allowed}, got {value!r}")


def mesh_signed_volume(verts: torch.Tensor, tris: torch.Tensor) -> float:
    """sum over the triangles of det(A, B, C) / 6: the enclosed volume, positive when the triangles are counter-clockwise
    seen from outside (fp64 torch ops on the device: one number per call, plumbing)."""
    v = verts.detach().to(torch.float64)
    t = tris.detach().to(device=v.device, dtype=torch.long)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    return float((a * torch.cross(b, c, dim=1)).sum() / 6.0)


def orientation_sign(verts: torch.Tensor, tris: torch.Tensor, orientation: str = "auto") -> int:
    """+1 when the winding number of the mesh is positive inside (triangles counter-clockwise seen from outside), -1 when
    it is negative: "ccw" -> +1, "cw" -> -1, "auto" -> the sign of the mesh's signed volume, so a consistently inverted
    mesh gives the same inside as its mirror twin."""
    _check_choice("orientation", orientation, ORIENTATIONS)
    if orientation == "auto":
        return -1 if mesh_signed_volume(verts, tris) < 0 else 1
    return 1 if orientation == "ccw" else -1


def mesh_winding_number(verts: torch.Tensor, tris: torch.Tensor, points: torch.Tensor) -> torch.Tensor:
    """Generalized winding number of `points` about the triangle mesh (ishap_mesh_winding; Jacobson et al. 2013):
    1 inside / 0 outside a closed mesh that is counter-clockwise seen from outside, -1 inside a clockwise one, and a
    smooth value in between where the surface is open.  verts [V,3], tris [F,3], points [P,3] -> [P] float32."""
    _lib.need_gpu(verts, "mesh_winding_number")
    dev = verts.device
    v = _lib.tensor(verts, torch.float32)
    t = _lib.tensor(tris, torch.int32, dev)
    p = _lib.tensor(points, torch.float32, dev, (-1, 3))
    w = torch.empty(p.shape[0], dtype=torch.float32, device=dev)
    if p.shape[0] == 0:
        return w
    if t.shape[0] == 0:
        raise ValueError("mesh_winding_number: the mesh has no triangles")
    scratch, nbytes = _lib.scratch(dev, "ishap_winding_scratch_bytes", t.shape[0], p.shape[0])
    _lib.call(dev, "ishap_mesh_winding", v.data_ptr(), t.data_ptr(), t.shape[0], p.data_ptr(), p.shape[0], w.data_ptr(),
              scratch.data_ptr(), nbytes)
    return w


def cloud_areas(points: torch.Tensor, k: int = 8) -> torch.Tensor:
    """The surface area each point of a cloud stands for, from its k-th nearest other point: pi d_k^2 / k
    (ishap_cloud_areas; brute force on the device).  points [N,3] -> [N] float32; 1 <= k <= 16, k < N."""
    if not (1 <= int(k) <= 16):
        raise ValueError(f"cloud_areas: k must be in 1..16, got {k!r}")
    _lib.need_gpu(points, "cloud_areas")
    p = _lib.tensor(points, torch.float32, shape=(-1, 3))
    if p.shape[0] <= int(k):
        raise ValueError(f"cloud_areas: k = {k} needs more than {k} points, got {p.shape[0]}")
    a = torch.empty(p.shape[0], dtype=torch.float32, device=p.device)
    _lib.call(p.device, "ishap_cloud_areas", p.data_ptr(), p.shape[0], int(k), a.data_ptr())
    return a


def _check_cloud_k(what: str, points, k):
    """host-side checks shared by the kNN / normal calls: (k, N); raises before any device work"""
    if not (1 <= int(k) <= 16):
        raise ValueError(f"{what}: k must be in 1..16, got {k!r}")
    if not torch.is_tensor(points) or points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what}: points must be a [N,3] tensor, got {tuple(points.shape) if torch.is_tensor(points) else type(points).__name__}")
    if points.shape[0] <= int(k):
        raise ValueError(f"{what}: k = {k} needs more than {k} points, got {points.shape[0]}")
    return int(k), points.shape[0]


def _knn_launch(p: torch.Tensor, k: int):
    idx = torch.empty((p.shape[0], k), dtype=torch.int32, device=p.device)
    d2 = torch.empty((p.shape[0], k), dtype=torch.float32, device=p.device)
    _lib.call(p.device, "ishap_cloud_knn", p.data_ptr(), p.shape[0], k, idx.data_ptr(), d2.data_ptr())
    return idx, d2


def _orient_launch(p: torch.Tensor, n: torch.Tensor, idx: torch.Tensor, k: int):
    """orients n in place; (rounds, seeds)"""
    scratch, nbytes = _lib.scratch(p.device, "ishap_cloud_orient_scratch_bytes", p.shape[0])
    info = (C.c_int * 2)()
    _lib.call(p.device, "ishap_cloud_orient", p.data_ptr(), n.data_ptr(), idx.data_ptr(), p.shape[0], k, scratch.data_ptr(), nbytes, info)
    return int(info[0]), int(info[1])


def cloud_knn(points: torch.Tensor, k: int = 8):
    """The k nearest OTHER points of every point of a cloud (ishap_cloud_knn; brute force on the device), ascending by
    (squared distance, index): equal distances go to the smaller index, equal points are neighbours at distance 0.
    points [N,3] -> (idx [N,k] int32, d2 [N,k] float32); 1 <= k <= 16, k < N."""
    k, _ = _check_cloud_k("cloud_knn", points, k)
    _lib.need_gpu(points, "cloud_knn")
    return _knn_launch(_lib.tensor(points, torch.float32), k)


def estimate_normals(points: torch.Tensor, k: int = 12, orient: bool = True, return_info: bool = False):
    """Unit normals [N,3] float32 of a cloud that has none (the device counterpart of Open3D's estimate_normals +
    orient_normals_consistent_tangent_plane): the direction of least spread of every point's k nearest neighbours
    (ishap_cloud_knn, ishap_cloud_normals), then, with `orient`, made consistent along the kNN graph from the topmost point
    of every component (ishap_cloud_orient): OUTWARD for a closed surface that is not nested inside another; a cavity's
    surface comes out pointing away from the cavity.  orient=False: the sign is a rule on the components (the largest in
    magnitude is positive), not an orientation.  return_info: also a dict with `variation` [N] (l0 / (l0 + l1 + l2), 0 on a
    plane), `rounds` and `seeds` (None without `orient`).  1 <= k <= 16, k < N."""
    k, _ = _check_cloud_k("estimate_normals", points, k)
    _lib.need_gpu(points, "estimate_normals")
    p = _lib.tensor(points, torch.float32)
    idx, _ = _knn_launch(p, k)
    n = torch.empty_like(p)
    var = torch.empty(p.shape[0], dtype=torch.float32, device=p.device) if return_info else None
    _lib.call(p.device, "ishap_cloud_normals", p.data_ptr(), p.shape[0], idx.data_ptr(), k, n.data_ptr(), _lib.ptr(var))
    rounds, seeds = _orient_launch(p, n, idx, k) if orient else (None, None)
    return (n, {"variation": var, "rounds": rounds, "seeds": seeds}) if return_info else n


def orient_normals(points: torch.Tensor, normals: torch.Tensor, k: int = 12, return_info: bool = False):
    """`normals` [N,3] of any length and sign, normalised and oriented as estimate_normals orients its own
    (ishap_cloud_orient over the k nearest neighbours): each comes back as its unit vector or the negation of it.
    A zero normal raises.  return_info: also {"rounds", "seeds"}."""
    k, N = _check_cloud_k("orient_normals", points, k)
    if not torch.is_tensor(normals) or tuple(normals.shape) != (N, 3):
        raise ValueError(f"orient_normals: {N} points but normals of shape "
                         f"{tuple(normals.shape) if torch.is_tensor(normals) else type(normals).__name__}")
    n = normals.detach().to(torch.float32)
    length = torch.linalg.norm(n, dim=1, keepdim=True)
    if not bool((length > 0).all()):                       # also false for NaN
        raise ValueError(f"orient_normals: {int((~(length > 0)).sum())} normals are zero or not a number")
    _lib.need_gpu(points, "orient_normals")
    p = _lib.tensor(points, torch.float32)
    n = (n / length).to(p.device).contiguous()
    idx, _ = _knn_launch(p, k)
    rounds, seeds = _orient_launch(p, n, idx, k)
    return (n, {"rounds": rounds, "seeds": seeds}) if return_info else n


def cloud_winding_number(points: torch.Tensor, normals: torch.Tensor, query: torch.Tensor, areas=None) -> torch.Tensor:
    """Winding number of `query` about an oriented point cloud (ishap_cloud_winding; Barill et al. 2018): about 1 inside,
    0 outside when `normals` are unit and point outward.  areas [N]: the area each point stands for, cloud_areas(points)
    when None.  points, normals [N,3], query [P,3] -> [P] float32."""
    _lib.need_gpu(points, "cloud_winding_number")
    dev = points.device
    p = _lib.tensor(points, torch.float32, shape=(-1, 3))
    n = _lib.tensor(normals, torch.float32, dev, (-1, 3))
    if n.shape != p.shape:
        raise ValueError(f"cloud_winding_number: {p.shape[0]} points but {n.shape[0]} normals")
    a = cloud_areas(p) if areas is None else _lib.tensor(areas, torch.float32, dev, (-1,))
    if a.shape[0] != p.shape[0]:
        raise ValueError(f"cloud_winding_number: {p.shape[0]} points but {a.shape[0]} areas")
    q = _lib.tensor(query, torch.float32, dev, (-1, 3))
    w = torch.empty(q.shape[0], dtype=torch.float32, device=dev)
    if q.shape[0] == 0:
        return w
    scratch, nbytes = _lib.scratch(dev, "ishap_winding_scratch_bytes", p.shape[0], q.shape[0])
    _lib.call(dev, "ishap_cloud_winding", p.data_ptr(), n.data_ptr(), a.data_ptr(), p.shape[0], q.data_ptr(), q.shape[0],
              w.data_ptr(), scratch.data_ptr(), nbytes)
    return w


def mesh_occupancy(verts: torch.Tensor, tris: torch.Tensor, points: torch.Tensor, method: str = "parity",
                   orientation: str = "auto") -> torch.Tensor:
    """RaycastingScene.compute_occupancy of the reference (drag_utils.py:437-440) on the device: 1 inside / 0 outside the
    triangle mesh.  verts [V,3], tris [F,3], points [P,3] -> [P] float32.
    method "parity" (default): the parity of +x ray crossings; needs a closed mesh -- a missing, doubled or interior
    face flips whole rays.  method "winding": mesh_winding_number > 0.5, which degrades smoothly where the surface is
    open; `orientation` (this method only, orientation_sign): "auto" negates w for a mesh whose signed volume is negative."""
    _check_choice("method", method, OCCUPANCY_METHODS)
    _check_choice("orientation", orientation, ORIENTATIONS)
    _lib.need_gpu(verts, "mesh_occupancy")
    dev = verts.device
    v = _lib.tensor(verts, torch.float32)
    t = _lib.tensor(tris, torch.int32, dev)
    p = _lib.tensor(points, torch.float32, dev)
    if method == "winding":
        w = mesh_winding_number(v, t, p)
        return ((-w if orientation_sign(v, t, orientation) < 0 else w) > 0.5).to(torch.float32)
    occ = torch.empty(p.shape[0], dtype=torch.float32, device=dev)
    _lib.call(dev, "ishap_mesh_occupancy", v.data_ptr(), t.data_ptr(), t.shape[0], p.data_ptr(), p.shape[0], occ.data_ptr())
    return occ


def sample_surface_points(verts: torch.Tensor, tris: torch.Tensor, n: int, generator=None,
                          multinomial_max: int = 1 << 24) -> torch.Tensor:
    """mesh.sample_points_uniformly(n) (drag_utils.py:432): triangles drawn with probability proportional to their area,
    a uniform point on each.  The random draws are torch's (plumbing); areas and points are computed by the library.
    Above `multinomial_max` triangles (torch.multinomial's category limit, 2^24) the triangle is drawn by inverse CDF instead:
    the same distribution from ONE uniform per sample, so the samples of a given seed differ between the two branches
    (only meshes beyond 16.7 M triangles -- random-weight noise surfaces -- take the second)."""
    _lib.need_gpu(verts, "sample_surface_points")
    dev = verts.device
    v = _lib.tensor(verts, torch.float32)
    t = _lib.tensor(tris, torch.int32, dev)
    areas = torch.empty(t.shape[0], dtype=torch.float32, device=dev)
    _lib.call(dev, "ishap_mesh_tri_areas", v.data_ptr(), t.data_ptr(), t.shape[0], areas.data_ptr())
    if areas.numel() <= multinomial_max:
        idx = torch.multinomial(areas.double().cpu(), n, replacement=True, generator=generator).to(device=dev, dtype=torch.int32)
    else:      # torch.multinomial stops at 2^24 categories (a 256^3 noise surface has 3e7 triangles): inverse CDF instead
        cdf = torch.cumsum(areas.double().cpu(), 0)
        u = torch.rand(n, generator=generator, dtype=torch.float64) * cdf[-1]
        # right=True: triangle i owns [cdf[i-1], cdf[i]) -- a draw that lands ON a cdf value (u = 0 in front of leading
        # zero-area triangles included) goes to the next triangle with area, never to a degenerate one
        idx = torch.searchsorted(cdf, u, right=True).clamp_(max=areas.numel() - 1).to(device=dev, dtype=torch.int32)
    uw = torch.rand((n, 2), generator=generator).to(dev).contiguous()
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    _lib.call(dev, "ishap_mesh_points_on_tris", v.data_ptr(), t.data_ptr(), idx.data_ptr(), uw.data_ptr(), n, pts.data_ptr())
    return pts


def _center_rule_scaled(v: torch.Tensor):
    """drag_utils.py:420-428: points that leave [-1,1]^3 are moved to their mean and, if wider than 2, scaled to fit.
    Returns (points, the factor they were scaled by: 1.0 unless they were wider than 2)."""
    mx, mn = v.max(dim=0).values, v.min(dim=0).values
    scale = 1.0
    if bool((mn > 1).any() or (mn < -1).any() or (mx > 1).any() or (mx < -1).any()):
        v = v - v.mean(dim=0)                                # get_center() = mean of the vertices
        ext = float((mx - mn).max())
        if ext > 2:
            scale = 2. / (ext + 1e-2)
            v = v * scale
    return v, scale


def _center_rule(v: torch.Tensor) -> torch.Tensor:
    return _center_rule_scaled(v)[0]


def sample_occupancy(mesh, mesh_path, center_mesh, points_size, uniform_ratio, device=None, generator=None,
                     occupancy: str = "parity"):
    """drag_utils.py:411-440: `points_size` samples (a `uniform_ratio` share uniform in [-1,1]^3, the rest on the surface
    plus N(0, 0.01) noise) with their occupancy.  BACKEND "third_party": Open3D (RaycastingScene) exactly as the
    reference; "device" (default): the mesh -- an OBJ file, a (vertices, triangles) pair, an OccupancyMesh or ANY object
    with `.vertices` / `.triangles` such as the open3d TriangleMesh the GUI passes (main.py:447-451) -- is sampled on
    the device.  occupancy (device route): "parity" (default) or "winding" -- mesh_occupancy's `method`, for meshes that are
    not watertight.  Returns (None, None) when no mesh is given."""
    _check_choice("occupancy", occupancy, OCCUPANCY_METHODS)
    if mesh is None and mesh_path is None:
        return None, None
    o3d = None
    if BACKEND == "third_party":
        if occupancy != "parity" and not isinstance(mesh, tuple):    # compute_occupancy is ray parity: no quiet parity labels
            raise ValueError('sample_occupancy: occupancy="winding" needs the device route (mesh.BACKEND = "device" or a '
                             '(vertices, triangles) pair); the third_party route labels by Open3D ray casting')
        import open3d as o3d
    if o3d is not None and not isinstance(mesh, tuple):
        if mesh is None:
            mesh = o3d.io.read_triangle_mesh(mesh_path)
        if center_mesh:
            max_bound, min_bound = mesh.get_max_bound(), mesh.get_min_bound()
            axis_extent = max_bound - min_bound
            if np.any(min_bound > 1) or np.any(min_bound < -1) or np.any(max_bound > 1) or np.any(max_bound < -1):
                mesh.translate(-mesh.get_center())
                if axis_extent.max() > 2:
                    mesh.scale(2. / (axis_extent.max() + 1e-2), center=np.array([0., 0, 0]))
        n_uniform = int(points_size * uniform_ratio)
        uniform = (np.random.rand(n_uniform, 3) * 2 - 1).astype(np.float32)
        surf = np.asarray(mesh.sample_points_uniformly(points_size - n_uniform).points, dtype=np.float32)
        surf += 0.01 * np.random.randn(surf.shape[0], 3)
        pts = np.concatenate([uniform, surf], axis=0).astype(np.float32)
        scene = o3d.t.geometry.RaycastingScene()
        scene.add_triangles(o3d.t.geometry.TriangleMesh().from_legacy(mesh_legacy=mesh))
        occ = scene.compute_occupancy(pts).numpy().reshape(-1, 1).astype(np.float32)
        return pts, occ
    # ---- device route ----
    if mesh is not None:
        v_np, t_np = mesh_arrays(mesh)
    else:
        v_np, t_np = read_obj(mesh_path)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    v = torch.from_numpy(v_np).to(dev)
    t = torch.from_numpy(t_np).to(dev)
    if center_mesh:                                              # drag_utils.py:420-428
        v = _center_rule(v)
    n_uniform = int(points_size * uniform_ratio)
    uniform = (torch.rand((n_uniform, 3), generator=generator) * 2 - 1).to(dev)
    surf = sample_surface_points(v, t, points_size - n_uniform, generator)
    surf = surf + 0.01 * torch.randn(surf.shape, generator=generator).to(dev)
    pts = torch.cat([uniform, surf], dim=0).contiguous()
    occ = mesh_occupancy(v, t, pts, method=occupancy)
    return pts.cpu().numpy(), occ.reshape(-1, 1).cpu().numpy()


def load_cloud(cloud):
    """(points [N,3], normals [N,3]) float32 numpy from a (points, normals) pair or the path of an .npz with those two
    arrays (the reference's pointcloud.npz, meshProcess.py cloud2mesh).  A cloud without normals -- a bare [N,3] array or
    tensor, a (points, None) pair or an .npz with `points` only -- gives (points, None): sample_cloud_occupancy and
    cloud_to_mesh then estimate them (estimate_normals).  (An array of shape [2,3] is still read as one point and its
    normal, as before.)"""
    def host(x):
        return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    if isinstance(cloud, (str, bytes)) or hasattr(cloud, "__fspath__"):
        with np.load(cloud) as z:
            pts, nrm = z["points"], (z["normals"] if "normals" in z.files else None)
    elif (torch.is_tensor(cloud) or isinstance(cloud, np.ndarray)) and cloud.ndim == 2 and tuple(cloud.shape) != (2, 3):
        pts, nrm = cloud, None
    else:
        pts, nrm = cloud
    pts = host(pts).astype(np.float32).reshape(-1, 3)
    if nrm is None:
        return pts, None
    nrm = host(nrm).astype(np.float32).reshape(-1, 3)
    if pts.shape != nrm.shape:
        raise ValueError(f"cloud: {pts.shape[0]} points but {nrm.shape[0]} normals")
    return pts, nrm


def sample_cloud_occupancy(points, normals=None, points_size=None, uniform_ratio=None, center=True, areas=None, generator=None,
                           device=None, normals_k: int = 12):
    """sample_occupancy for an oriented point cloud, without meshing it: `points_size` samples -- a `uniform_ratio` share
    uniform in [-1,1]^3, the rest cloud points drawn with probability proportional to their area plus N(0, 0.01) noise --
    labelled by cloud_winding_number > 0.5.  center: the mesh route's rule (_center_rule) on the cloud's points; a
    translation leaves given `areas` as they are, a rescale by s multiplies them by s^2 (areas=None: cloud_areas of the
    centred points).  normals=None: a cloud without normals; they are estimated and oriented on the device from
    `normals_k` neighbours (estimate_normals), on the points after the centring rule -- a translation and a uniform scale
    leave normals as they are.
    Returns (points [P,3], occupancies [P,1]) float32 numpy, as sample_occupancy."""
    if points_size is None or uniform_ratio is None:
        raise ValueError("sample_cloud_occupancy: points_size and uniform_ratio are required")
    if normals is None and not (1 <= int(normals_k) <= 16):
        raise ValueError(f"sample_cloud_occupancy: normals_k must be in 1..16, got {normals_k!r}")
    p_np, n_np = load_cloud((points, normals))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    p = torch.from_numpy(p_np).to(dev)
    scale = 1.0
    if center:
        p, scale = _center_rule_scaled(p)
        p = p.contiguous()
    n = estimate_normals(p, k=int(normals_k)) if n_np is None else torch.from_numpy(n_np).to(dev)
    if areas is None:
        a = cloud_areas(p)
    else:
        a = torch.as_tensor(areas, dtype=torch.float32).reshape(-1).to(dev)
        if a.shape[0] != p.shape[0]:
            raise ValueError(f"sample_cloud_occupancy: {p.shape[0]} points but {a.shape[0]} areas")
        if scale != 1.0:
            a = a * (scale * scale)
    n_uniform = int(points_size * uniform_ratio)
    uniform = (torch.rand((n_uniform, 3), generator=generator) * 2 - 1).to(dev)
    n_surf = points_size - n_uniform
    parts = [uniform]
    if n_surf > 0:
        idx = torch.multinomial(a.double().cpu(), n_surf, replacement=True, generator=generator).to(dev)
        parts.append(p[idx] + 0.01 * torch.randn((n_surf, 3), generator=generator).to(dev))
    pts = torch.cat(parts, dim=0).contiguous()
    occ = (cloud_winding_number(p, n, pts, a) > 0.5).to(torch.float32)
    return pts.cpu().numpy(), occ.reshape(-1, 1).cpu().numpy()


def cloud_to_mesh(points, normals=None, res: int = 256, smooth_iterations: int = 10, chunk: int = 1 << 21, normals_k: int = 12):
    """Mesh of an oriented point cloud (the reference's meshProcess.cloud2mesh, here by winding number): cloud_winding_number
    on the linspace(-1, 1, res)^3 grid in chunks of `chunk` queries, extract_surface at level 0.5, vertices rescaled to
    [-1, 1], smooth_mesh.  Returns (vertices [V,3] float32, triangles [F,3] int32) on the device, counter-clockwise seen
    from outside.  Glue over existing calls, and brute force: res^3 x N pairs.  Measured on one MI355X with a 100 000-point
    cloud: 0.24 s at 128^3 and 1.6 s at 256^3 (1.7e12 pairs), linear in both counts -- a million-point
    cloud at 256^3 takes about 16 s.  Fitting from sample_cloud_occupancy labels needs no mesh and is the main route.
    normals=None: a cloud without normals; estimate_normals(points, k=normals_k) supplies them."""
    _lib.need_gpu(points, "cloud_to_mesh")
    dev = points.device
    p = _lib.tensor(points, torch.float32, shape=(-1, 3))
    n = estimate_normals(p, k=normals_k) if normals is None else _lib.tensor(normals, torch.float32, dev, (-1, 3))
    a = cloud_areas(p)
    ax = torch.linspace(-1, 1, res, device=dev)
    vol = torch.empty(res ** 3, dtype=torch.float32, device=dev)
    for i0 in range(0, res ** 3, chunk):
        idx = torch.arange(i0, min(res ** 3, i0 + chunk), device=dev)
        q = torch.stack([ax[idx // (res * res)], ax[(idx // res) % res], ax[idx % res]], dim=1)
        vol[i0:i0 + idx.numel()] = cloud_winding_number(p, n, q, a)
    v, t = extract_surface(vol.reshape(res, res, res), 0.5)
    v = smooth_mesh(v / (res - 1) * 2 - 1, t, smooth_iterations)
    return v, (t[:, [0, 2, 1]].contiguous() if mesh_signed_volume(v, t) < 0 else t)


def export_obj(volume: torch.Tensor, path: str, scale_div: float = 255.0, backend: str = None):
    """visualize.py:71-73 (create_obj): surface at 0, vertices / 255 * 2 - 1, Wavefront OBJ."""
    backend = BACKEND if backend is None else backend
    if backend == "third_party":
        import mcubes
        vertices, triangles = mcubes.marching_cubes(volume.detach().cpu().numpy(), 0)
        vertices = vertices / scale_div * 2 - 1
        mcubes.export_obj(vertices, triangles, path)
        return
    nv, nt = surface_counts(volume, 0.0)
    if nv > MAX_OBJ_VERTICES:                      # not a surface (e.g. random weights decode to noise): do not write GBs of text
        with open(path, "w") as f:
            f.write(f"# {nv} vertices / {nt} triangles: the volume is not a surface, mesh not written\n")
        return
    verts, tris = extract_surface(volume, 0.0)
    _write_obj(path, verts / scale_div * 2 - 1, tris)
