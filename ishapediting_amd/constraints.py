"""Volume constraints of a drag edit: keep, carve and fill true 3-D regions through the decoder.

The keep / free regions of regions.py weight the preservation term in the UNet's feature tap, which is three 2-D planes: they
constrain a region's three shadows.  A volume constraint is stated where the shape lives instead: at sample points q_j of the
volume, with a target occupancy g_j and a weight w_j, as the loss
    L_vol = -(1 / sum w) sum_j w_j BCEWithLogits(decoder(planes of pred_xstart)(q_j), g_j)
which every guided step differentiates onto its planes (csrc/constrain.hip) and pulls back to the latent by the full-depth
backward, beside the drag gradient (DragStuff.training: volume_keep, carve, fill).

  keep   "do not change this volume":   g_j = the occupancy of the unedited shape at q_j
  carve  "this volume must end empty":  g_j = 0
  fill   "this volume must end solid":  g_j = 1

`volume_constraints` rasterises the regions of each role to a [D]^3 mask on the device and takes the centres of the set voxels
as the points.  The points stay the same for the whole edit.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib
from .regions import Box, Sphere, Voxels, _as_list

MAX_POINTS = 1 << 20          # ishap_constraint_setup's limit on the points of one edit
ROLES = ("keep", "carve", "fill")


@dataclass(frozen=True, eq=False)
class VolumeConstraints:
    """points float32 [M, 3] in [-1, 1]^3, targets float32 [M] in {0, 1}, weights float32 [M] >= 0, on one device."""
    points: torch.Tensor
    targets: torch.Tensor
    weights: torch.Tensor

    def __post_init__(self):
        p, t, w = self.points, self.targets, self.weights
        if not (torch.is_tensor(p) and torch.is_tensor(t) and torch.is_tensor(w)):
            raise ValueError("VolumeConstraints: points, targets and weights are tensors")
        if p.dim() != 2 or p.shape[1] != 3 or not 1 <= p.shape[0] <= MAX_POINTS:
            raise ValueError(f"VolumeConstraints: points must be [M, 3] with 1 <= M <= {MAX_POINTS}, got {tuple(p.shape)}")
        if tuple(t.shape) != (p.shape[0],) or tuple(w.shape) != (p.shape[0],):
            raise ValueError(f"VolumeConstraints: targets and weights must be [{p.shape[0]}], got {tuple(t.shape)} and {tuple(w.shape)}")

    @property
    def M(self) -> int:
        return int(self.points.shape[0])


def check_role_weights(weights) -> tuple:
    """(keep, carve, fill) weights: three finite numbers >= 0"""
    try:
        w = tuple(float(v) for v in weights)
    except TypeError:
        raise ValueError(f"weights must be three numbers (keep, carve, fill), got {weights!r}") from None
    if len(w) != 3 or not all(np.isfinite(v) and v >= 0 for v in w):
        raise ValueError(f"weights must be three finite numbers >= 0 (keep, carve, fill), got {weights!r}")
    return w


def check_builder_args(keep, carve, fill, D, max_points, weights):
    """The argument checks of volume_constraints that need no device -> (lists of the three roles, D, max_points, weights)."""
    roles = [_as_list(r, n) for r, n in zip((keep, carve, fill), ROLES)]
    if not any(roles):
        raise ValueError("volume constraints: no region given (keep, carve and fill are all empty)")
    if isinstance(D, bool) or int(D) != D or not 2 <= int(D) <= 1024:
        raise ValueError(f"volume constraints: D must be an integer in 2..1024, got {D!r}")
    if isinstance(max_points, bool) or int(max_points) != max_points or int(max_points) < 1:
        raise ValueError(f"volume constraints: max_points must be an integer >= 1, got {max_points!r}")
    if 3 * int(max_points) > MAX_POINTS:
        raise ValueError(f"volume constraints: max_points = {max_points} per role is above {MAX_POINTS // 3}")
    w = check_role_weights(weights)
    for items, n in zip(roles, ROLES):
        for it in items:
            if isinstance(it, Voxels) and it.D != int(D):
                raise ValueError(f"volume constraints: {n} holds a Voxels grid of size {it.D}, the constraint grid has D = {int(D)}")
    return roles, int(D), int(max_points), w


def rasterise(items, D: int, device) -> torch.Tensor:
    """bool [D, D, D] on the device: the voxels of linspace(-1, 1, D)^3 whose centre lies in a Box (bounds inclusive) or a
    Sphere of `items`, or that are set in one of its Voxels grids (ishap_region_select over a volume of ones)."""
    dev = torch.device(device)
    recs, grid = [], None
    for it in items:
        if isinstance(it, Box):
            recs.append((0, 0, it.lo, it.hi))
        elif isinstance(it, Sphere):
            recs.append((1, 0, it.centre, (it.radius, 0.0, 0.0)))
        else:
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
    ones = torch.ones((D, D, D), dtype=torch.float32, device=dev)
    out = torch.empty((D, D, D), dtype=torch.uint8, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    _lib.call(dev, "ishap_region_select", ones.data_ptr(), D, 0.0, _lib.ptr(prims), len(recs), _lib.ptr(grid), out.data_ptr(),
              count.data_ptr())
    return out.view(torch.bool)


def mask_points(mask: torch.Tensor, max_points: int) -> torch.Tensor:
    """Centres 2 i / (D - 1) - 1 (formed in double, rounded once) of the set voxels of a bool [D, D, D] mask in ascending
    linear index; of C > max_points voxels every ceil(C / max_points)-th is kept."""
    D = int(mask.shape[0])
    idx = torch.nonzero(mask)                       # [C, 3] in ascending linear index
    c = int(idx.shape[0])
    if c > max_points:
        idx = idx[::-(-c // max_points)]
    return (2.0 * idx.to(torch.float64) / (D - 1) - 1.0).to(torch.float32)


def volume_constraints(keep=None, carve=None, fill=None, reference_logits_fn: Optional[Callable] = None, D: int = 128,
                       max_points: int = 16384, weights=(1.0, 1.0, 1.0), device=None) -> VolumeConstraints:
    """The constraint points of an edit.  keep / carve / fill: regions.Box, Sphere, Voxels (of grid size D) or lists of them.
    Each role is rasterised to a [D]^3 mask; carve and fill override keep where they overlap, a voxel in both carve and fill
    is a ValueError, and so is a role that was given but holds no voxel.  The points are the centres of the set voxels in
    ascending linear index (every ceil(C / max_points)-th of a role with C > max_points voxels), keep first, then carve, then
    fill.  Targets: carve 0, fill 1, keep reference_logits_fn(points [n, 3]) > 0 -- the logits of the UNEDITED shape (needed
    only with keep).  weights: (keep, carve, fill), one weight per role."""
    roles, D, max_points, w = check_builder_args(keep, carve, fill, D, max_points, weights)
    if roles[0] and reference_logits_fn is None:
        raise ValueError("volume constraints: keep needs reference_logits_fn (the logits of the unedited shape)")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    masks = [rasterise(items, D, dev) if items else None for items in roles]
    if masks[1] is not None and masks[2] is not None and bool((masks[1] & masks[2]).any()):
        raise ValueError(f"volume constraints: carve and fill overlap in {int((masks[1] & masks[2]).sum())} voxel(s) at D = {D}")
    for m, n in zip(masks, ROLES):
        if m is not None and not bool(m.any()):
            raise ValueError(f"volume constraints: {n} rasterises to no voxel at D = {D}")
    if masks[0] is not None:
        for o in masks[1:]:
            if o is not None:
                masks[0] = masks[0] & ~o
        if not bool(masks[0].any()):
            masks[0] = None             # carve and fill cover all of keep: nothing is left to keep
    pts, tgt, wts = [], [], []
    for k, m in enumerate(masks):
        if m is None:
            continue
        p = mask_points(m, max_points)
        if k == 0:
            z = reference_logits_fn(p)
            t = (torch.as_tensor(z).to(dev).reshape(-1) > 0).to(torch.float32)
            if t.shape[0] != p.shape[0]:
                raise ValueError(f"volume constraints: reference_logits_fn returned {t.shape[0]} values for {p.shape[0]} points")
        else:
            t = torch.full((p.shape[0],), float(k - 1), dtype=torch.float32, device=dev)
        pts.append(p)
        tgt.append(t)
        wts.append(torch.full((p.shape[0],), w[k], dtype=torch.float32, device=dev))
    out = VolumeConstraints(torch.cat(pts).contiguous(), torch.cat(tgt).contiguous(), torch.cat(wts).contiguous())
    if not float(out.weights.double().sum()) > 0:
        raise ValueError("volume constraints: every point has weight 0")
    return out
