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
"""
from __future__ import annotations

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


def plane_weights(keep=None, free=None, W: Optional[int] = None, keep_weight: float = 4.0, free_weight: float = 0.0, dilate: int = 0,
                  device=None) -> torch.Tensor:
    """float32 [3, W, W] on the device: keep_weight on the texels in the shadow of `keep`, else free_weight on those in the shadow
    of `free`, else 1 (keep overrides free).  keep / free: a Box, Sphere or Voxels, or a list of them (their union), or None.
    dilate: grow every shadow by that many texels (Chebyshev), clipped at the map.  A region whose shadow is empty on all three
    planes -- thinner than the texel pitch, or outside the cube -- raises ValueError.
    A plane texel stands for a whole column through the shape: a region constrains its three shadows, not only its own volume."""
    if W is None or isinstance(W, bool) or int(W) != W or int(W) < 2:
        raise ValueError(f"plane_weights: W (the side of the tap) must be an integer >= 2, got {W!r}")
    W = int(W)
    keep_weight, free_weight = check_weight(keep_weight, "keep_weight"), check_weight(free_weight, "free_weight")
    dilate = check_dilate(dilate)
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
    L = _lib.lib()
    prims = None
    if recs:
        arr = (_lib.RegionPrimC * len(recs))()
        for r, (kind, role, a, b) in zip(arr, recs):
            r.kind, r.role = kind, role
            r.a[:], r.b[:] = a, b
        prims = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    out = torch.empty((3, W, W), dtype=torch.float32, device=dev)
    counts = torch.zeros(2, dtype=torch.int32, device=dev)
    nbytes = int(L.ishap_region_plane_weights_scratch_bytes(W))
    if nbytes <= 0:
        raise ValueError(f"plane_weights: W = {W} is out of range")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.ishap_region_plane_weights(_lib.ptr(prims), len(recs), _lib.ptr(kgrid), _lib.ptr(fgrid), D, W, dilate,
                                                keep_weight, free_weight, out.data_ptr(), counts.data_ptr(), scratch.data_ptr(),
                                                nbytes, _lib.stream_ptr(dev)))
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
