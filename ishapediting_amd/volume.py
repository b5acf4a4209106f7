"""Connected components of the decoded occupancy volume, on the device (csrc/components.hip through the C ABI:
ishap_volume_label, ishap_volume_components_count / _emit, ishap_volume_flip): which pieces a volume has, and the cleaning
that runs BEFORE the surface is extracted -- floaters (small islands of volume > level) removed, closed cavities (pockets of
volume <= level inside solid parts) filled -- by reflecting their voxels across the level, so the kept surface is bit for bit
the surface it was.  This module only allocates and selects; the voxel work is the library's.

A voxel is inside where `volume - level > 0` (extract_surface's rule: a NaN is outside).  connectivity 6 joins face
neighbours, 26 face, edge and corner neighbours.  A component is named by its ROOT, the lowest linear index
(x * ny + y) * nz + z of its voxels.

Distances (csrc/edt.hip, ishap_edt): `distance_transform` is the exact squared Euclidean distance from every voxel to a set, as
integers; `signed_distance` the voxel-grid signed distance of a decoded volume, negative inside.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from . import _lib

PHASES = {"outside": 0, "inside": 1}
CONNECTIVITIES = (6, 26)


def _check(volume, phase, connectivity, what):
    if phase not in PHASES:
        raise ValueError(f"{what}: phase must be 'inside' or 'outside', got {phase!r}")
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"{what}: connectivity must be 6 or 26, got {connectivity!r}")
    if not torch.is_tensor(volume) or volume.dim() != 3 or volume.numel() == 0:
        raise ValueError(f"{what}: volume must be a non-empty 3-D tensor, got "
                         f"{tuple(volume.shape) if torch.is_tensor(volume) else type(volume).__name__}")
    if volume.numel() >= 1 << 31:
        raise ValueError(f"{what}: {volume.numel()} voxels, the limit is 2^31 - 1")
    _lib.need_gpu(volume, what)
    return _lib.tensor(volume, torch.float32)


def _label(vol: torch.Tensor, level: float, phase: str, connectivity: int) -> torch.Tensor:
    labels = torch.empty(vol.shape, dtype=torch.int32, device=vol.device)
    nx, ny, nz = vol.shape
    _lib.call(vol.device, "ishap_volume_label", vol.data_ptr(), nx, ny, nz, float(level), PHASES[phase], int(connectivity),
              labels.data_ptr())
    return labels


def _scratch(vol: torch.Tensor) -> torch.Tensor:
    try:
        return _lib.scratch(vol.device, "ishap_volume_components_scratch_bytes", vol.numel())[0]
    except _lib.ScratchError:
        raise RuntimeError("ishap_volume_components_scratch_bytes: invalid size") from None


def _table(labels: torch.Tensor, scratch: torch.Tensor) -> torch.Tensor:
    """int32 [C, 9] rows (root, voxels, xmin, xmax, ymin, ymax, zmin, zmax, border) in ascending root order"""
    nx, ny, nz = labels.shape
    dev = labels.device
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.call(dev, "ishap_volume_components_count", labels.data_ptr(), nx, ny, nz, scratch.data_ptr(), count.data_ptr())
    c = int(count.item())                                          # the one host read-back: the table's size
    table = torch.empty((c, 9), dtype=torch.int32, device=dev)
    if c:
        _lib.call(dev, "ishap_volume_components_emit", labels.data_ptr(), nx, ny, nz, scratch.data_ptr(), table.data_ptr())
    return table


def _flip(vol_in: torch.Tensor, vol_out: torch.Tensor, labels: torch.Tensor, level: float, roots: torch.Tensor, scratch: torch.Tensor):
    nx, ny, nz = vol_in.shape
    roots = _lib.tensor(roots, torch.int32, vol_in.device)
    _lib.call(vol_in.device, "ishap_volume_flip", vol_in.data_ptr(), vol_out.data_ptr(), labels.data_ptr(), nx, ny, nz, float(level),
              roots.data_ptr(), roots.numel(), scratch.data_ptr())
    return vol_out


def label_volume(volume: torch.Tensor, level: float = 0.0, phase: str = "inside", connectivity: int = 6) -> torch.Tensor:
    """int32 tensor of the volume's shape (any 3-D shape): every voxel of `phase` carries the root of its component, every
    other voxel -1.  A function of the input alone: two runs give the same bits."""
    return _label(_check(volume, phase, connectivity, "label_volume"), level, phase, connectivity)


@dataclass
class Components:
    """The components of one phase of a volume, in ascending root order.  roots, voxels, border: int32 [C]; bbox: int32 [C, 6]
    (xmin, xmax, ymin, ymax, zmin, zmax, inclusive); border[c] = 1 when the component touches a face of the box; labels: what
    label_volume returns.  len() is the component count."""
    roots: torch.Tensor
    voxels: torch.Tensor
    bbox: torch.Tensor
    border: torch.Tensor
    labels: torch.Tensor

    def __len__(self):
        return int(self.roots.shape[0])


def _components(vol, level, phase, connectivity, scratch) -> Components:
    labels = _label(vol, level, phase, connectivity)
    t = _table(labels, scratch)
    return Components(t[:, 0].contiguous(), t[:, 1].contiguous(), t[:, 2:8].contiguous(), t[:, 8].contiguous(), labels)


def volume_components(volume: torch.Tensor, level: float = 0.0, phase: str = "inside", connectivity: int = 6) -> Components:
    """Labels the volume and tabulates its components (voxel counts, boxes, border flags: exact integers)."""
    vol = _check(volume, phase, connectivity, "volume_components")
    return _components(vol, level, phase, connectivity, _scratch(vol))


def select_components(voxels: torch.Tensor, keep="largest", min_voxels: int = 0, min_fraction: float = 0.0) -> torch.Tensor:
    """clean_volume's rule on a table's voxel counts (rows in ascending root order): a bool mask of the rows kept.
    keep: "largest", an int k (the k largest) or None (all); equal sizes go to the lower root.  Kept rows with fewer than
    max(min_voxels, min_fraction * largest) voxels are then dropped."""
    c = voxels.shape[0]
    if keep is None:
        k = c
    elif keep == "largest":
        k = 1
    elif isinstance(keep, int) and not isinstance(keep, bool) and keep >= 0:
        k = min(keep, c)
    else:
        raise ValueError(f"keep must be 'largest', a non-negative int or None, got {keep!r}")
    kept = torch.zeros(c, dtype=torch.bool, device=voxels.device)
    if c == 0:
        return kept
    order = torch.sort(voxels, descending=True, stable=True).indices      # stable: ties stay in root order
    kept[order[:k]] = True
    largest = int(voxels.max())
    return kept & (voxels.to(torch.float64) >= max(float(min_voxels), float(min_fraction) * largest))


def clean_volume(volume: torch.Tensor, level: float = 0.0, keep="largest", min_voxels: int = 0, min_fraction: float = 0.0,
                 fill_cavities: bool = False, connectivity: int = 6, return_info: bool = False):
    """A new volume without floaters and, with `fill_cavities`, without enclosed cavities.
    Floaters first: the inside components are chosen by select_components (keep / min_voxels / min_fraction) and every
    other one is reflected across the level (out = level - (in - level): it becomes outside, at the same distance).  A volume
    with no inside voxel, or with a single inside component, is left as it is by this step.  Then, with `fill_cavities`, the
    OUTSIDE phase of the result is labelled with the same connectivity and every outside component that touches no face of
    the box is reflected to the inside (a voxel exactly at the level gets the next float above it).  Voxels of kept
    components, and NaN voxels, keep their bits, so the surface of what is kept is unchanged.
    return_info: also a dict with `components` (inside components found), `removed`, `removed_voxels`, `cavities`
    (outside components filled) and `filled_voxels`."""
    vol = _check(volume, "inside", connectivity, "clean_volume")
    out = vol.clone()
    scratch = _scratch(vol)
    info = {"components": 0, "removed": 0, "removed_voxels": 0, "cavities": 0, "filled_voxels": 0}
    comps = _components(vol, level, "inside", connectivity, scratch)
    info["components"] = len(comps)
    if len(comps) > 1:
        gone = ~select_components(comps.voxels, keep, min_voxels, min_fraction)
        info["removed"] = int(gone.sum())
        info["removed_voxels"] = int(comps.voxels[gone].sum())
        if info["removed"]:
            _flip(out, out, comps.labels, level, comps.roots[gone], scratch)
    else:
        select_components(comps.voxels, keep, min_voxels, min_fraction)       # the arguments are checked all the same
    if fill_cavities:
        outside = _components(out, level, "outside", connectivity, scratch)
        closed = outside.border == 0
        info["cavities"] = int(closed.sum())
        info["filled_voxels"] = int(outside.voxels[closed].sum())
        if info["cavities"]:
            _flip(out, out, outside.labels, level, outside.roots[closed], scratch)
    return (out, info) if return_info else out


# ------------------------------------------------------------------------------------------------ distances (csrc/edt.hip)
EDT_INF = 1 << 30          # ISHAP_EDT_INF: the squared distance where a slice holds no seed
EDT_MAX_AXIS = 1024


def _edt(seeds: torch.Tensor, axes: int, invert: bool) -> torch.Tensor:
    """ishap_edt on a contiguous uint8 [n0, n1, n2] device tensor -> int32 of that shape, on torch's current stream"""
    n0, n1, n2 = seeds.shape
    nbytes = int(_lib.lib().ishap_edt_scratch_bytes(n0, n1, n2, axes))
    if nbytes <= 0:
        raise ValueError(f"distance_transform: a grid of {(n0, n1, n2)} with axes mask {axes} is outside the limits (every "
                         f"measured axis <= {EDT_MAX_AXIS}, fewer than 2^31 voxels)")
    out = torch.empty((n0, n1, n2), dtype=torch.int32, device=seeds.device)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=seeds.device)
    _lib.call(seeds.device, "ishap_edt", seeds.data_ptr(), n0, n1, n2, axes, int(bool(invert)), out.data_ptr(), scratch.data_ptr(),
              nbytes)
    return out


def distance_transform(mask: torch.Tensor, axes=None, invert: bool = False) -> torch.Tensor:
    """The exact squared Euclidean distance, in voxels, from every element of `mask` to the nearest set one (with `invert`: to
    the nearest one that is not set): int32 of mask's shape, EDT_INF where there is none.  mask: a bool or uint8 tensor of 1 to
    3 dimensions on the device.  axes: the dimensions of `mask` along which distance is measured (default: all); the others are
    batch dimensions whose slices never see each other -- axes=(1, 2) on a [3, W, W] stack is three 2-D transforms.  Integer
    arithmetic on the device (csrc/edt.hip): two runs give the same bits."""
    if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8) or not 1 <= mask.dim() <= 3 or mask.numel() == 0:
        raise ValueError("distance_transform: mask must be a non-empty bool or uint8 tensor of 1 to 3 dimensions")
    _lib.need_gpu(mask, "distance_transform")
    nd = mask.dim()
    if axes is None:
        axes = tuple(range(nd))
    if isinstance(axes, int) and not isinstance(axes, bool):
        axes = (axes,)
    axes = tuple(axes)
    if not axes or any(isinstance(a, bool) or int(a) != a or not -nd <= a < nd for a in axes):
        raise ValueError(f"distance_transform: axes must name at least one of the {nd} dimensions of mask, got {axes!r}")
    bits = 0
    for a in axes:
        bits |= 1 << (int(a) % nd + 3 - nd)
    seeds = mask.contiguous().view(torch.uint8).reshape((1,) * (3 - nd) + tuple(mask.shape))
    return _edt(seeds, bits, invert).reshape(mask.shape)


def signed_distance(volume: torch.Tensor, level: float = 0.0) -> torch.Tensor:
    """float32 [D, D, D]: the signed distance, in voxels, of every voxel of a decoded volume to the shape's boundary on the grid:
    sqrt(d^2 to the nearest inside voxel) - sqrt(d^2 to the nearest outside voxel), inside where volume - level > 0.  Negative
    inside (the sign of metrics.calc_implicit_field(sdf=True)), +inf with no inside voxel, -inf with no outside voxel.  The
    squared distances are exact integers; the square roots are taken in float64 and the difference is rounded once."""
    vol = _check(volume, "inside", 6, "signed_distance")
    inside = ((vol - float(level)) > 0).view(torch.uint8)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=vol.device)

    def root(invert):
        d2 = _edt(inside, 7, invert)
        return torch.where(d2 >= EDT_INF, inf, torch.sqrt(d2.to(torch.float64)))
    return (root(False) - root(True)).to(torch.float32)
