"""Region-constrained drag edits: 3-D keep / free regions -> the weight map of the drag loss's preservation ("mask") term.

A drag edit balances the motion term at the handle lattices against a preservation term on every plane texel no lattice
touches.  A weight map w [3, W, W] (one [row, col] slice per triplane plane, indexed like the kernels' `touched`) scales that
term per texel: 1 is the plain loss, 0 frees a texel, > 1 holds it harder.  Users give 3-D regions in the coordinates handles
use, [-1, 1]^3: a region is a list of `Box`, `Sphere` and `Voxels`, and its SHADOW on a plane is the set of texels it projects
onto (include/ishap.h, ishap_region_plane_weights, states the rule of every primitive).  `plane_weights` builds the map on the
device (csrc/regions.hip): keep_weight in the shadow of `keep`, else free_weight in the shadow of `free`, else 1.

The inherent limit: a plane texel stands for a whole COLUMN through the shape -- the three planes are projections -- so a region
constrains its three shadows, not only its own volume.  Keeping a box also holds whatever lies in front of and behind it along
each axis on the texels the box projects to; freeing one frees those columns.

Part edits (the second half of this file; csrc/parts.hip): `select_part` names a part of a decoded volume, `Rigid` is a rigid
motion, `sample_handles` spreads handles over the part, `transform_region` moves it, and `plan_part_edit` puts them together
into what DragStuff.training takes -- sources, targets and free = [part, moved].

Distances (csrc/edt.hip, volume.distance_transform): `grow`, `shrink`, `open_region`, `close_region` and `shell` change a Voxels
region in 3-D by a Euclidean radius in voxels; `plan_part_edit(margin=)` grows the free regions, `select_part(neck=)` cuts a
selection at thin necks, and `plane_weights(falloff=)` feathers the edges of the map.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib


def _vec3(v, what):
    a = np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1)
    if a.shape != (3,) or not np.isfinite(a).all():
        raise ValueError(f"{what} must be three finite numbers, got {v!r}")
    return tuple(float(x) for x in a)


@dataclass(frozen=True)
class Box:
    """The axis-aligned box lo <= (x, y, z) <= hi.  Its shadow on a plane: the texels whose centre lies in the projected
    rectangle, boundaries inclusive."""
    lo: Sequence[float]
    hi: Sequence[float]

    def __post_init__(self):
        lo, hi = _vec3(self.lo, "Box.lo"), _vec3(self.hi, "Box.hi")
        if any(h < l for l, h in zip(lo, hi)):
            raise ValueError(f"Box: hi {hi} is below lo {lo}")
        object.__setattr__(self, "lo", lo)
        object.__setattr__(self, "hi", hi)


@dataclass(frozen=True)
class Sphere:
    """The ball of `radius` around `centre`.  Its shadow on a plane: the texels whose centre lies in the projected disc."""
    centre: Sequence[float]
    radius: float

    def __post_init__(self):
        object.__setattr__(self, "centre", _vec3(self.centre, "Sphere.centre"))
        r = float(self.radius)
        if not (np.isfinite(r) and r >= 0):
            raise ValueError(f"Sphere: radius must be finite and >= 0, got {self.radius!r}")
        object.__setattr__(self, "radius", r)


@dataclass(frozen=True, eq=False)
class Voxels:
    """A bool [D, D, D] grid indexed [ix][iy][iz] on linspace(-1, 1, D), as decoded volumes are.  Every set voxel marks the
    texel nearest to it on each plane (an integer index map); the grid must be at least as fine as the map (D >= W)."""
    mask: torch.Tensor

    def __post_init__(self):
        m = self.mask
        if not torch.is_tensor(m):
            m = torch.as_tensor(np.asarray(m))
        if m.dim() != 3 or not (m.shape[0] == m.shape[1] == m.shape[2]) or m.shape[0] < 2:
            raise ValueError(f"Voxels: mask must be a [D, D, D] grid with D >= 2, got {tuple(m.shape)}")
        object.__setattr__(self, "mask", m if m.dtype == torch.bool else m != 0)

    @property
    def D(self) -> int:
        return int(self.mask.shape[0])


def _as_list(region, name):
    if region is None:
        return []
    if isinstance(region, (Box, Sphere, Voxels)):
        return [region]
    items = list(region)
    for it in items:
        if not isinstance(it, (Box, Sphere, Voxels)):
            raise ValueError(f"{name}: a region is a Box, a Sphere, a Voxels or a list of them, got {type(it).__name__}")
    return items


def _split(region, name, role, W, device):
    """-> (primitive records, the region's one voxel grid as uint8 on the device or None, D)"""
    prims, grid, D = [], None, 0
    for it in _as_list(region, name):
        if isinstance(it, Box):
            prims.append((0, role, it.lo, it.hi))
        elif isinstance(it, Sphere):
            prims.append((1, role, it.centre, (it.radius, 0.0, 0.0)))
        else:
            if it.D < W:
                raise ValueError(f"{name}: a Voxels grid must be at least as fine as the weight map (D = {it.D} < W = {W})")
            if grid is not None and it.D != D:
                raise ValueError(f"{name}: the Voxels grids of one region must have one size ({D} and {it.D})")
            m = it.mask.to(device)
            grid, D = (m if grid is None else grid | m), it.D        # several grids of a region: their union
    if grid is not None:
        grid = grid.contiguous().view(torch.uint8)
    return prims, grid, D


def check_weight(value, name):
    v = float(value)
    if not (np.isfinite(v) and v >= 0):
        raise ValueError(f"{name} must be finite and >= 0, got {value!r}")
    return v


def check_dilate(value):
    if isinstance(value, bool) or int(value) != value or int(value) < 0:
        raise ValueError(f"dilate must be an integer >= 0, got {value!r}")
    return int(value)


MAX_FALLOFF = 64.0


def check_falloff(value):
    v = float(value)
    if not (np.isfinite(v) and 0.0 <= v <= MAX_FALLOFF):
        raise ValueError(f"falloff must be in 0..{MAX_FALLOFF:g} texels, got {value!r}")
    return v


def falloff_table(falloff: float) -> np.ndarray:
    """float64 [ceil(falloff^2)]: A[d2] = max(0, 1 - sqrt(d2) / falloff), the ramp of a feathered map by squared texel
    distance.  Taken here, on the host: the device looks it up, so its map is bitwise this formula's."""
    n = int(np.ceil(falloff * falloff))
    return np.maximum(0.0, 1.0 - np.sqrt(np.arange(max(n, 1), dtype=np.float64)) / falloff)


def plane_weights(keep=None, free=None, W: Optional[int] = None, keep_weight: float = 4.0, free_weight: float = 0.0, dilate: int = 0,
                  device=None, falloff: float = 0.0) -> torch.Tensor:
    """float32 [3, W, W] on the device: keep_weight on the texels in the shadow of `keep`, else free_weight on those in the shadow
    of `free`, else 1 (keep overrides free).  keep / free: a Box, Sphere or Voxels, or a list of them (their union), or None.
    dilate: grow every shadow by that many texels (Chebyshev), clipped at the map.  A region whose shadow is empty on all three
    planes -- thinner than the texel pitch, or outside the cube -- raises ValueError.
    falloff > 0 (texels, at most 64) feathers the edges: with a = max(0, 1 - distance / falloff) to the keep and to the free
    shadow, w = (1 + (keep_weight - 1) a_k) + ((free_weight - 1) a_f) (1 - a_k), in double, rounded once; distances are exact
    Euclidean ones on each plane (csrc/edt.hip).  falloff <= 1 is the hard map; falloff = 0 is the call it always was.
    A plane texel stands for a whole column through the shape: a region constrains its three shadows, not only its own volume."""
    if W is None or isinstance(W, bool) or int(W) != W or int(W) < 2:
        raise ValueError(f"plane_weights: W (the side of the tap) must be an integer >= 2, got {W!r}")
    W = int(W)
    keep_weight, free_weight = check_weight(keep_weight, "keep_weight"), check_weight(free_weight, "free_weight")
    dilate = check_dilate(dilate)
    falloff = check_falloff(falloff)
    return _plane_map(keep, free, W, keep_weight, free_weight, dilate, device, falloff, False)


def plane_marks(keep=None, free=None, W: Optional[int] = None, dilate: int = 0, device=None) -> torch.Tensor:
    """uint8 [3, W, W] on the device: bit 0 on the texels in the shadow of `keep`, bit 1 on those in the shadow of `free`, both
    after `dilate` -- the sets plane_weights turns into weights.  Arguments and errors as plane_weights."""
    if W is None or isinstance(W, bool) or int(W) != W or int(W) < 2:
        raise ValueError(f"plane_marks: W (the side of the tap) must be an integer >= 2, got {W!r}")
    return _plane_map(keep, free, int(W), 0.0, 0.0, check_dilate(dilate), device, 0.0, True)


def _plane_map(keep, free, W, keep_weight, free_weight, dilate, device, falloff, marks):
    # the regions are validated before anything touches the device
    for region, name in ((keep, "keep"), (free, "free")):
        for it in _as_list(region, name):
            if isinstance(it, Voxels) and it.D < W:
                raise ValueError(f"{name}: a Voxels grid must be at least as fine as the weight map (D = {it.D} < W = {W})")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    kp, kgrid, kD = _split(keep, "keep", 0, W, dev)
    fp, fgrid, fD = _split(free, "free", 1, W, dev)
    if kgrid is not None and fgrid is not None and kD != fD:
        raise ValueError(f"the Voxels grids of keep and free must have one size ({kD} and {fD})")
    D = kD or fD
    recs = kp + fp
    prims = None
    if recs:
        arr = (_lib.RegionPrimC * len(recs))()
        for r, (kind, role, a, b) in zip(arr, recs):
            r.kind, r.role = kind, role
            r.a[:], r.b[:] = a, b
        prims = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    out = torch.empty((3, W, W), dtype=torch.uint8 if marks else torch.float32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    nbytes = int(getattr(_lib.lib(), f"ishap_region_plane_{'feather' if falloff > 0 else 'weights'}_scratch_bytes")(W))
    if nbytes <= 0:
        raise ValueError(f"plane_weights: W = {W} is out of range")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    region = (_lib.ptr(prims), len(recs), _lib.ptr(kgrid), _lib.ptr(fgrid), D, W, dilate)
    if marks:
        _lib.call(dev, "ishap_region_plane_marks", *region, out.data_ptr(), counts.data_ptr(), scratch.data_ptr(), nbytes)
    elif falloff > 0:
        table = torch.from_numpy(falloff_table(falloff)).to(dev)                # uploaded with the call
        _lib.call(dev, "ishap_region_plane_feather", *region, keep_weight, free_weight, table.data_ptr(), table.numel(),
                  out.data_ptr(), counts.data_ptr(), scratch.data_ptr(), nbytes)
    else:
        _lib.call(dev, "ishap_region_plane_weights", *region, keep_weight, free_weight, out.data_ptr(), counts.data_ptr(),
                  scratch.data_ptr(), nbytes)
    nk, nf = (int(v) for v in counts.cpu())
    for region, name, n in ((keep, "keep", nk), (free, "free", nf)):
        if _as_list(region, name) and n == 0:
            raise ValueError(f"the {name} region has an empty shadow on all three planes: it is thinner than the texel pitch "
                             f"(2 / {W - 1}) or lies outside [-1, 1]^3")
    return out


def component_region(volume: torch.Tensor, point, level: float = 0.0) -> Voxels:
    """The connected inside component of `volume` (a decoded [D, D, D] volume, inside where volume - level > 0) under a picked
    point in [-1, 1]^3 -- e.g. a vertex position render.pick returns -- as a Voxels region (volume.label_volume names it).
    Raises ValueError when the voxel nearest to the point is outside the shape."""
    from .volume import label_volume
    if not torch.is_tensor(volume) or volume.dim() != 3 or not (volume.shape[0] == volume.shape[1] == volume.shape[2]):
        raise ValueError("component_region: volume must be a [D, D, D] tensor")
    D = int(volume.shape[0])
    p = np.asarray(_vec3(point, "component_region: point"))
    idx = np.rint((p + 1.0) * (D - 1) / 2.0).astype(np.int64)
    if (idx < 0).any() or (idx > D - 1).any():
        raise ValueError(f"component_region: the point {tuple(p)} lies outside [-1, 1]^3")
    labels = label_volume(volume, level=level, phase="inside", connectivity=6)
    root = int(labels[idx[0], idx[1], idx[2]])
    if root < 0:
        raise ValueError(f"component_region: the point {tuple(p)} (voxel {tuple(int(i) for i in idx)}) is outside the shape")
    return Voxels(labels == root)


# ------------------------------------------------------------------------------------------------ morphology (csrc/edt.hip)
# Growing, shrinking, opening and closing a Voxels region in 3-D, by Euclidean radii in voxels: thresholds of the exact squared
# distance transform (volume.distance_transform).  Nothing lies outside the grid: the cube's walls do not erode a region.
def _radius2(r, what):
    """floor(r^2), taken on the host in double: the integer the squared distances are compared with"""
    v = float(r)
    if not (np.isfinite(v) and v >= 0):
        raise ValueError(f"{what}: the radius must be finite and >= 0 voxels, got {r!r}")
    from .volume import EDT_INF
    return min(int(np.floor(v * v)), EDT_INF - 1)


def _morph_mask(region, what):
    if not isinstance(region, Voxels):
        raise ValueError(f"{what}: region must be a Voxels region, got {type(region).__name__}")
    if region.mask.device.type != "cuda":
        raise ValueError(f"{what}: the region's mask must be on the GPU (there is no CPU path)")
    return region.mask


def grow(region: Voxels, r: float) -> Voxels:
    """The voxels within r of the region: {d^2 <= floor(r^2)}, d^2 the exact squared distance to the region.  r = 0 returns the
    region itself and launches nothing."""
    from .volume import distance_transform
    k, mask = _radius2(r, "grow"), _morph_mask(region, "grow")
    return region if k == 0 else Voxels(distance_transform(mask) <= k)


def shrink(region: Voxels, r: float) -> Voxels:
    """The voxels farther than r from everything outside the region: the complement of the complement's grow.  The walls of the
    cube do not erode.  r = 0 returns the region itself and launches nothing."""
    from .volume import distance_transform
    k, mask = _radius2(r, "shrink"), _morph_mask(region, "shrink")
    return region if k == 0 else Voxels(distance_transform(mask, invert=True) > k)


def open_region(region: Voxels, r: float) -> Voxels:
    """grow(shrink(region, r), r): necks and spurs thinner than 2 r go, convex edges are rounded; a subset of the region."""
    return grow(shrink(region, r), r)


def close_region(region: Voxels, r: float) -> Voxels:
    """shrink(grow(region, r), r): gaps and holes narrower than 2 r fill; a superset of the region."""
    return shrink(grow(region, r), r)


def shell(region: Voxels, inner: float, outer: float) -> Voxels:
    """grow(region, outer) & ~shrink(region, inner): the band from `inner` voxels inside the region's boundary to `outer` outside."""
    return Voxels(grow(region, outer).mask & ~shrink(region, inner).mask)


# ------------------------------------------------------------------------------------------------ part edits (csrc/parts.hip)
# From a region and a rigid motion to handles, targets and free regions.  A rotation stays within what the drag loss can do:
# every handle's lattice still only translates; the part's rotation is carried by handles spread over the part, each with its
# own displacement -- an approximation by translated lattices, better the more handles share the part.  The free regions are
# the part and the place it moves to; like every region they constrain their three shadows, not only their volume.
_PARTS_MAX_D, _PARTS_MAX_HANDLES = 1024, 4096


def _device_volume(volume, what):
    if not torch.is_tensor(volume) or volume.dim() != 3 or not (volume.shape[0] == volume.shape[1] == volume.shape[2]):
        raise ValueError(f"{what}: volume must be a [D, D, D] tensor")
    D = int(volume.shape[0])
    if not 2 <= D <= _PARTS_MAX_D:
        raise ValueError(f"{what}: D = {D} is outside 2..{_PARTS_MAX_D}")
    if volume.device.type != "cuda":
        raise ValueError(f"{what}: the volume must be on the GPU (there is no CPU path)")
    return volume.to(torch.float32).contiguous(), D


def _part_grid(part, what):
    if not isinstance(part, Voxels):
        raise ValueError(f"{what}: part must be a Voxels region, got {type(part).__name__}")
    if part.D > _PARTS_MAX_D:
        raise ValueError(f"{what}: D = {part.D} is above {_PARTS_MAX_D}")
    if part.mask.device.type != "cuda":
        raise ValueError(f"{what}: the part's mask must be on the GPU (there is no CPU path)")
    return part.mask.contiguous().view(torch.uint8), part.D


def _nearest_voxel(point, D, what):
    p = np.asarray(_vec3(point, what))
    idx = np.rint((p + 1.0) * (D - 1) / 2.0).astype(np.int64)
    if (idx < 0).any() or (idx > D - 1).any():
        raise ValueError(f"{what}: the point {tuple(p)} lies outside [-1, 1]^3")
    return tuple(int(i) for i in idx)


def _neck_component(sel: torch.Tensor, vol, level, vox, r, connectivity, point) -> Voxels:
    """select_part's `neck`: the selection cut at necks thinner than 2 r.  E = shrink(selection, r) is labelled; the piece is
    the component of E owning the voxel of E nearest to the pick voxel among those with d^2 <= floor(r^2) (ties: the lowest
    linear index), found in a small cube of labels read back around the pick; grown back by r inside the selection."""
    from .volume import label_volume
    k, D = _radius2(r, "select_part: neck"), int(sel.shape[0])
    whole = Voxels(sel)
    core = shrink(whole, r).mask
    masked = torch.where(core, vol, torch.full((), float(level), dtype=torch.float32, device=vol.device))
    labels = label_volume(masked, level=level, phase="inside", connectivity=connectivity)
    R = int(np.floor(np.sqrt(float(k))))
    lo = [max(v - R, 0) for v in vox]
    hi = [min(v + R, D - 1) for v in vox]
    cube = labels[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1].cpu().numpy()                 # the one host read
    ix, iy, iz = np.meshgrid(*(np.arange(l, h + 1, dtype=np.int64) for l, h in zip(lo, hi)), indexing="ij")
    d2 = (ix - vox[0]) ** 2 + (iy - vox[1]) ** 2 + (iz - vox[2]) ** 2
    ok = (cube >= 0) & (d2 <= k)
    if not ok.any():
        raise ValueError(f"select_part: the point {tuple(_vec3(point, 'point'))} (voxel {vox}) sits on something thinner than "
                         f"2 x neck = {2 * float(r):g} voxels: nothing of the selection within {float(r):g} voxels of it survives")
    key = np.where(ok, d2 * (D ** 3) + (ix * D + iy) * D + iz, np.iinfo(np.int64).max)      # nearest first, then lowest index
    root = int(cube.reshape(-1)[int(np.argmin(key))])
    return Voxels(grow(Voxels(labels == root), r).mask & sel)


def select_part(volume: torch.Tensor, within, level: float = 0.0, point=None, connectivity: int = 6, neck: float = 0.0) -> Voxels:
    """The part of a decoded [D, D, D] volume inside `within` (a Box, Sphere or Voxels, or a list: their union): the voxels with
    volume - level > 0 whose centre lies in a primitive (box bounds inclusive, sphere <= r^2, in double) or that are set in a
    grid.  With `point` (in [-1, 1]^3, e.g. what render.pick returns): only the connected piece of that selection which holds
    the voxel nearest to the point (volume.label_volume with `connectivity`).  Raises ValueError for an empty selection and
    for a point whose voxel is not selected.  On the device; the host reads one count.
    neck = r > 0 (voxels, with `point`) cuts the selection at necks thinner than 2 r, so that an armrest joined to the seat by
    a thin neck is a part of its own: the selection is shrunk by r, the piece of what is left nearest to the pick (within r of
    it; ValueError if there is none -- the pick sits on something thinner than 2 r) is grown back by r inside the selection.
    The result is that piece opened by r: its convex edges are rounded.  neck = 0 is the call it always was."""
    vol, D = _device_volume(volume, "select_part")
    neck2 = _radius2(neck, "select_part: neck")
    if neck2 > 0 and point is None:
        raise ValueError("select_part: neck needs a point: it names the piece on the pick's side of the neck")
    items = _as_list(within, "within")
    if not items:
        raise ValueError("select_part: `within` names no region")
    if connectivity not in (6, 18, 26):
        raise ValueError(f"select_part: connectivity must be 6, 18 or 26, got {connectivity!r}")
    vox = _nearest_voxel(point, D, "select_part: point") if point is not None else None
    dev = vol.device
    recs, grid = [], None
    for it in items:
        if isinstance(it, Box):
            recs.append((0, 0, it.lo, it.hi))
        elif isinstance(it, Sphere):
            recs.append((1, 0, it.centre, (it.radius, 0.0, 0.0)))
        else:
            if it.D != D:
                raise ValueError(f"select_part: a Voxels grid of size {it.D} for a volume of size {D}")
            m = it.mask.to(dev)
            grid = m if grid is None else grid | m
    if grid is not None:
        grid = grid.contiguous().view(torch.uint8)
    prims = None
    if recs:
        arr = (_lib.RegionPrimC * len(recs))()
        for r, (kind, role, a, b) in zip(arr, recs):
            r.kind, r.role = kind, role
            r.a[:], r.b[:] = a, b
        prims = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    out = torch.empty((D, D, D), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call(dev, "ishap_region_select", vol.data_ptr(), D, float(level), _lib.ptr(prims), len(recs), _lib.ptr(grid), out.data_ptr(),
              count.data_ptr())
    if int(count.cpu()) == 0:
        raise ValueError("select_part: the selection is empty: no voxel of the shape lies in the region")
    sel = out.view(torch.bool)
    if vox is None:
        return Voxels(sel)
    if neck2 > 0:
        return _neck_component(sel, vol, level, vox, neck, connectivity, point)
    from .volume import label_volume
    # the shape masked to the selection: outside it volume - level is 0, which is not inside
    masked = torch.where(sel, vol, torch.full((), float(level), dtype=torch.float32, device=dev))
    labels = label_volume(masked, level=level, phase="inside", connectivity=connectivity)
    root = int(labels[vox[0], vox[1], vox[2]])
    if root < 0:
        raise ValueError(f"select_part: the point {tuple(_vec3(point, 'point'))} (voxel {vox}) is not in the selection")
    return Voxels(labels == root)


def _axis_angle(axis, degrees):
    k = np.asarray(_vec3(axis, "Rigid: rotation axis"))
    norm = float(np.sqrt((k * k).sum()))
    if norm == 0.0:
        raise ValueError("Rigid: the rotation axis is the zero vector")
    k = k / norm
    deg = float(degrees)
    if not np.isfinite(deg):
        raise ValueError(f"Rigid: degrees must be finite, got {degrees!r}")
    quarter = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}.get(deg % 360.0)
    c, s = quarter if quarter is not None else (float(np.cos(np.deg2rad(deg))), float(np.sin(np.deg2rad(deg))))
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return c * np.eye(3) + s * K + (1.0 - c) * np.outer(k, k) + 0.0          # + 0.0: no negative zeros


@dataclass(frozen=True, eq=False)
class Rigid:
    """The rigid motion x -> R (x - pivot) + pivot + translation.  rotation: None, (axis, degrees) -- right-handed about `axis`,
    which need not be a unit vector -- or a 3 x 3 matrix, which must be a rotation (|R^T R - I| <= 1e-9 entrywise, det > 0: no
    scale, no reflection).  Whole multiples of 90 degrees about a coordinate axis give entries that are exactly 0 and +-1.
    Sines and cosines are taken here, on the host, in double."""
    rotation: object = None
    pivot: Sequence[float] = (0.0, 0.0, 0.0)
    translation: Sequence[float] = (0.0, 0.0, 0.0)

    def __post_init__(self):
        object.__setattr__(self, "pivot", _vec3(self.pivot, "Rigid.pivot"))
        object.__setattr__(self, "translation", _vec3(self.translation, "Rigid.translation"))
        rot = self.rotation
        if rot is None:
            R = np.eye(3)
        elif isinstance(rot, (tuple, list)) and len(rot) == 2 and np.ndim(rot[1]) == 0:
            R = _axis_angle(rot[0], rot[1])
        else:
            R = np.array(rot.detach().cpu() if torch.is_tensor(rot) else rot, dtype=np.float64)
            if R.shape != (3, 3) or not np.isfinite(R).all():
                raise ValueError(f"Rigid: rotation must be (axis, degrees) or a finite 3 x 3 matrix, got {rot!r}")
            err = float(np.abs(R.T @ R - np.eye(3)).max())
            if err > 1e-9 or np.linalg.det(R) <= 0:
                raise ValueError(f"Rigid: the matrix is not a rotation (|R^T R - I| = {err:.3e}, det = {np.linalg.det(R):.6f}): "
                                 "a part moves rigidly, without scale or reflection")
        R.setflags(write=False)
        object.__setattr__(self, "_matrix", R)

    @property
    def matrix(self) -> np.ndarray:
        """float64 [3, 3]"""
        return self._matrix

    def apply(self, points) -> np.ndarray:
        """float64 [..., 3]: R (x - pivot) + pivot + translation, summed left to right"""
        x = np.asarray(points.detach().cpu() if torch.is_tensor(points) else points, dtype=np.float64)
        if x.shape[-1:] != (3,):
            raise ValueError(f"Rigid.apply: points must end in 3 coordinates, got shape {x.shape}")
        R, p, t = self._matrix, np.asarray(self.pivot), np.asarray(self.translation)
        d = x - p
        return np.stack([((R[a, 0] * d[..., 0] + R[a, 1] * d[..., 1]) + R[a, 2] * d[..., 2]) + p[a] + t[a] for a in range(3)], axis=-1)


@dataclass(frozen=True, eq=False)
class Handles:
    """sample_handles' result.  points: float32 [n, 3] on the device, the picked voxels' centres; voxels: int32 [n, 3] on the
    device, their indices (ix, iy, iz); spacing: the smallest distance between two picks (0 for a single pick)."""
    points: torch.Tensor
    voxels: torch.Tensor
    spacing: float


@dataclass(frozen=True, eq=False)
class PartEdit:
    """plan_part_edit's result: what DragStuff.training takes.  sources, targets: float32 [n, 3] arrays; free: [part, moved];
    spacing: the handles' spacing; moved: the part after the motion, a Voxels region."""
    sources: np.ndarray
    targets: np.ndarray
    free: list
    spacing: float
    moved: Voxels


def handle_voxels(part: Voxels, n: int, start_voxel=None):
    """The launch under sample_handles, as the kernels leave it on the device: (voxels int32 [n, 3], tail int32 [n + 1]), the
    tail holding the squared distance at each pick (uint32 bits) and then M, the part's voxel count.  start_voxel: (ix, iy, iz)
    or None.  Rounds beyond M are (-1, -1, -1) and 0: there is no n <= M check here and no read-back."""
    grid, D = _part_grid(part, "sample_handles")
    if isinstance(n, bool) or int(n) != n or not 1 <= int(n) <= _PARTS_MAX_HANDLES:
        raise ValueError(f"sample_handles: n must be an integer in 1..{_PARTS_MAX_HANDLES}, got {n!r}")
    n = int(n)
    st = None
    if start_voxel is not None:
        st = tuple(int(v) for v in start_voxel)
        if len(st) != 3 or any(v < 0 or v >= D for v in st):
            raise ValueError(f"sample_handles: the start voxel {st} lies outside the grid of size {D}")
        st = (C.c_int * 3)(*st)
    dev = grid.device
    nbytes = int(_lib.lib().ishap_region_handles_scratch_bytes(D, n))
    if nbytes <= 0:
        raise ValueError(f"sample_handles: D = {D}, n = {n} is out of range")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    picks = torch.empty((n, 3), dtype=torch.int32, device=dev)
    tail = torch.empty(n + 1, dtype=torch.int32, device=dev)
    _lib.call(dev, "ishap_region_handles", grid.data_ptr(), D, n, st, picks.data_ptr(), tail.data_ptr(), tail[n:].data_ptr(),
              scratch.data_ptr(), nbytes)
    return picks, tail


def sample_handles(part: Voxels, n: int, start=None) -> Handles:
    """n handles spread over a part by farthest-point sampling on the device (csrc/parts.hip): the first is the voxel nearest
    to `start` (a point in [-1, 1]^3, in the part or not) or, without one, the voxel farthest from the centre of the part's
    bounding box; every later one is the voxel farthest from those picked so far.  Distances are exact integers and every tie
    goes to the lowest voxel index, so the picks repeat bit for bit.  points are the voxel centres 2 i / (D - 1) - 1, formed in
    double and rounded once to float32.  Raises ValueError when the part has fewer than n voxels."""
    D = part.D if isinstance(part, Voxels) else 0
    st = _nearest_voxel(start, D, "sample_handles: start") if start is not None and D >= 2 else None
    picks, tail = handle_voxels(part, n, st)
    n = int(n)
    last, M = (int(v) for v in tail[n - 1:].cpu())                    # the one read-back
    if n > M:
        raise ValueError(f"sample_handles: {n} handles asked of a part of {M} voxels")
    points = (2.0 * picks.to(torch.float64) / (D - 1) - 1.0).to(torch.float32)
    return Handles(points=points, voxels=picks, spacing=float(np.sqrt(float(last)) * 2.0 / (D - 1)))


def transform_region(part: Voxels, rigid: Rigid) -> Voxels:
    """The part moved by `rigid`, on the part's grid, as an inverse map: every destination voxel looks up the source voxel
    nearest to its pre-image (round half to even), so the moved region has no holes.  What leaves the cube is cut off; a
    region that leaves it entirely raises ValueError."""
    grid, D = _part_grid(part, "transform_region")
    if not isinstance(rigid, Rigid):
        raise ValueError(f"transform_region: rigid must be a Rigid, got {type(rigid).__name__}")
    dev = grid.device
    out = torch.empty((D, D, D), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    args = (C.c_double * 15)(*rigid.matrix.reshape(-1), *rigid.pivot, *rigid.translation)
    _lib.call(dev, "ishap_region_transform", grid.data_ptr(), D, args, out.data_ptr(), count.data_ptr())
    if int(count.cpu()) == 0:
        raise ValueError("transform_region: the moved region is empty: the motion takes the part out of [-1, 1]^3 (or the part is empty)")
    return Voxels(out.view(torch.bool))


def handle_targets(sources: np.ndarray, rigid: Rigid) -> np.ndarray:
    """float32(rigid.apply(float64 sources)) for float32 [n, 3] sources; a target outside [-1, 1]^3 raises ValueError naming
    the handle (a lattice cannot be placed outside the cube)."""
    sources = np.asarray(sources, np.float32)
    targets = rigid.apply(sources.astype(np.float64)).astype(np.float32)
    bad = np.nonzero((np.abs(targets) > 1.0).any(axis=1))[0]
    if len(bad):
        k = int(bad[0])
        raise ValueError(f"plan_part_edit: handle {k} at {sources[k].tolist()} would move to {targets[k].tolist()}, outside [-1, 1]^3")
    return targets


def plan_part_edit(part: Voxels, rigid: Rigid, handles: int = 16, start=None, margin: float = 0.0) -> PartEdit:
    """A part edit as a drag edit: `handles` sources spread over the part (sample_handles), each one's target where `rigid`
    takes it -- float32(rigid.apply(float64 sources)) -- and free = [part, moved]: the part's old and new place may change.
    A target outside [-1, 1]^3 raises ValueError naming the handle.  The lattices of the drag loss only translate: a rotation
    is approximated by the handles' different displacements.  The free regions constrain their three shadows, not only their
    volume.  margin (voxels): free = [grow(part, margin), grow(moved, margin)], so that the surface which blends the moved part
    into the rest, just outside both sets, may change too; `moved` stays the ungrown region and margin = 0 is the plan it always
    was.  Several planned edits run in one loop through training_batch, which takes per-edit lists:
        plans = [plan_part_edit(part_a, rigid_a), plan_part_edit(part_b, rigid_b)]
        ds.training_batch([p.sources for p in plans], [p.targets for p in plans], free=[p.free for p in plans])"""
    if not isinstance(rigid, Rigid):
        raise ValueError(f"plan_part_edit: rigid must be a Rigid, got {type(rigid).__name__}")
    _radius2(margin, "plan_part_edit: margin")
    h = sample_handles(part, handles, start=start)
    sources = h.points.cpu().numpy()
    targets = handle_targets(sources, rigid)
    moved = transform_region(part, rigid)
    return PartEdit(sources=sources, targets=targets, free=[grow(part, margin), grow(moved, margin)], spacing=h.spacing, moved=moved)
