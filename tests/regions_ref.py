"""The statements the region-constrained drag loss is checked against: numpy shadows and weight maps (the rules of
include/ishap.h, ishap_region_plane_weights, written out literally), the float64 oracle and the float32 yardstick of the WEIGHTED
drag loss (built from the pieces of tests/drag_ref.py), and the table of cases with their seeded weight maps.

Regions are plain tuples here, independent of the product's classes:
    ("box", lo, hi)   ("sphere", centre, radius)   ("voxels", bool ndarray [D, D, D] indexed [ix][iy][iz])
tests/test_regions_host.py asserts the conditions the inputs must meet; tests/test_gpu_regions.py runs them on the device.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from tests import drag_ref as R

PLANE_AXES = ((0, 1), (1, 2), (0, 2))        # (col axis, row axis) of planes xy, yz, xz -- plane_axes() of csrc/drag.hip
BOUNDARY_MARGIN = 1e-6                       # no texel centre of a device case is this close to a primitive's boundary


# ------------------------------------------------------------------------------------------------ shadows and maps
def texel_centres(W):
    return 2.0 * np.arange(W, dtype=np.float64) / (W - 1) - 1.0


def voxel_to_texel(i, D, W):
    return (2 * i * (W - 1) + (D - 1)) // (2 * (D - 1))


def shadow_ref(region, W):
    """bool [3, W, W] indexed [plane][row][col]: the union of the shadows of the region's items (a list of tuples, or None)."""
    out = np.zeros((3, W, W), bool)
    t = texel_centres(W)
    u, v = t[None, :], t[:, None]                       # u along columns, v along rows
    for item in region or []:
        kind = item[0]
        for p, (ac, ar) in enumerate(PLANE_AXES):
            if kind == "box":
                lo, hi = np.asarray(item[1], np.float64), np.asarray(item[2], np.float64)
                out[p] |= (u >= lo[ac]) & (u <= hi[ac]) & (v >= lo[ar]) & (v <= hi[ar])
            elif kind == "sphere":
                c, r = np.asarray(item[1], np.float64), float(item[2])
                out[p] |= (u - c[ac]) ** 2 + (v - c[ar]) ** 2 <= r * r
            elif kind == "voxels":
                m = np.asarray(item[1], bool)
                D = m.shape[0]
                assert m.shape == (D, D, D) and D >= W, "a voxel grid must be at least as fine as the map"
                idx = np.nonzero(m)
                out[p, voxel_to_texel(idx[ar], D, W), voxel_to_texel(idx[ac], D, W)] = True
            else:
                raise ValueError(kind)
    return out


def dilate_ref(shadow, d):
    """Chebyshev dilation by d texels per plane, clipped at the map."""
    if d == 0:
        return shadow.copy()
    out = np.zeros_like(shadow)
    _, W, _ = shadow.shape
    for p, r, c in zip(*np.nonzero(shadow)):
        out[p, max(r - d, 0):min(r + d, W - 1) + 1, max(c - d, 0):min(c + d, W - 1) + 1] = True
    return out


def plane_weights_ref(keep, free, W, keep_weight=4.0, free_weight=0.0, dilate=0):
    """float32 [3, W, W]: keep_weight in the (dilated) shadow of keep, else free_weight in that of free, else 1.  A region that
    is given but has an empty shadow on all three planes raises ValueError."""
    if dilate < 0 or not all(np.isfinite(x) and x >= 0 for x in (keep_weight, free_weight)):
        raise ValueError("dilate >= 0 and finite weights >= 0")
    sk, sf = shadow_ref(keep, W), shadow_ref(free, W)
    for name, region, s in (("keep", keep, sk), ("free", free, sf)):
        if region and not s.any():
            raise ValueError(f"the {name} region has an empty shadow")
    sk, sf = dilate_ref(sk, dilate), dilate_ref(sf, dilate)
    w = np.ones((3, W, W), np.float32)
    w[sf] = np.float32(free_weight)
    w[sk] = np.float32(keep_weight)
    return w


def boundary_distance(region, W):
    """The least distance of a texel centre to a boundary of a box or sphere of the region (in the comparison's own terms:
    coordinate difference for a box face, radius difference for a disc); inf without primitives."""
    best = np.inf
    t = texel_centres(W)
    u, v = np.meshgrid(t, t)
    for item in region or []:
        for ac, ar in PLANE_AXES:
            if item[0] == "box":
                lo, hi = np.asarray(item[1], np.float64), np.asarray(item[2], np.float64)
                best = min(best, *(float(np.abs(t - b).min()) for b in (lo[ac], hi[ac], lo[ar], hi[ar])))
            elif item[0] == "sphere":
                c, r = np.asarray(item[1], np.float64), float(item[2])
                best = min(best, float(np.abs(np.sqrt((u - c[ac]) ** 2 + (v - c[ar]) ** 2) - r).min()))
    return best


# ------------------------------------------------------------------------------------------------ the weighted loss
def _weighted_mask_sum(fe, fo, setup, wmap, loss_type):
    tot = 0
    for p in range(3):
        dm = (fe[p] - fo[p])[:, setup.masks[p]]
        w = wmap[p][setup.masks[p]]
        tot = tot + ((dm.abs() * w).sum() if loss_type == "l1" else ((dm ** 2) * w).sum())
    return tot


def drag_loss_grad64_weighted(edit_tap, orig_tap, chmap, sources, targets, r, voxel, W, cof, loss_type, wmap):
    """drag_ref.drag_loss_grad64 with the preservation term weighted per untouched texel by wmap [3, W, W] (float32 values, taken
    to float64); the divisor stays Cc * nmask.  Same return value."""
    setup = O.DragSetup(sources, targets, r, voxel, W)
    cof = float(np.float32(cof))
    w64 = torch.as_tensor(np.asarray(wmap, np.float32)).double()
    e = edit_tap.detach().double().requires_grad_(True)
    fe, fo = R.gather_planes(e, chmap, W), R.gather_planes(orig_tap.detach().double(), chmap, W)
    patch = R.sample_bilinear(fo, setup.patch_grid.to(fo.dtype))
    shift = R.sample_bilinear(fe, setup.shift_grid.to(fe.dtype))
    d = shift - patch.detach()
    motion = d.abs().mean() if loss_type == "l1" else (d ** 2).mean()
    nmask = sum(int(m.sum()) for m in setup.masks)
    mask_term = torch.zeros((), dtype=fe.dtype)
    if cof > 0:
        mask_term = _weighted_mask_sum(fe, fo, setup, w64, loss_type) / (fe.shape[1] * nmask)
    loss = -motion - cof * mask_term
    grad, = torch.autograd.grad(loss, e)
    return SimpleNamespace(loss=float(loss.detach()), grad=grad, d=d.detach(), setup=setup, nmask=nmask)


def drag_loss_grad32_weighted(edit_tap, orig_tap, chmap, sources, targets, r, voxel, W, cof, loss_type, wmap):
    """The float32 yardstick: the arithmetic of O.drag_loss (F.grid_sample, float32, autograd) with the weighted preservation
    term.  Returns (loss, grad)."""
    setup = O.DragSetup(sources, targets, r, voxel, W)
    cof = float(np.float32(cof))
    w32 = torch.as_tensor(np.asarray(wmap, np.float32))
    e = edit_tap.detach().float().requires_grad_(True)
    edit, orig = R.gather_planes(e, chmap, W), R.gather_planes(orig_tap.detach().float(), chmap, W)
    patch = F.grid_sample(orig, setup.patch_grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    shift = F.grid_sample(edit, setup.shift_grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    C = orig.shape[1]
    nmask = sum(int(m.sum()) for m in setup.masks)
    if cof <= 0:
        mask_loss = 0.0
    else:
        tot = 0.0
        for p in range(3):
            d = (edit[p] - orig[p])[:, setup.masks[p]]
            w = w32[p][setup.masks[p]]
            tot = tot + ((d.abs() * w).sum() if loss_type == "l1" else ((d ** 2) * w).sum())
        mask_loss = tot / (C * nmask)
    if loss_type == "l1":
        loss = -F.l1_loss(shift, patch.detach()) - cof * mask_loss
    else:
        loss = -((shift.reshape(-1) - patch.detach().reshape(-1)) ** 2).mean() - cof * mask_loss
    grad, = torch.autograd.grad(loss, e)
    return float(loss.detach()), grad


# ------------------------------------------------------------------------------------------------ the cases
COF = 0.4
WEIGHT_VALUES = (0.0, 0.25, 1.0, 4.0)
CASES = ("A", "B", "F", "H", "J")            # drag_ref cases: plain; second channel chunk + dead lanes; every padding situation;
#                                              repeated and shared channels; the product's shape
COMBOS = tuple((c, lt) for c in CASES for lt in ("l2", "l1") if c != "J" or lt == "l2")
_SEEDS = {"A": 501, "B": 502, "F": 503, "H": 504, "J": 505}


@lru_cache(maxsize=None)
def weight_map(name):
    """float32 [3, W, W], every texel drawn from WEIGHT_VALUES (seeded per case; the planes differ)."""
    W = R.make_case(name).W
    rng = np.random.default_rng(_SEEDS[name])
    return np.asarray(WEIGHT_VALUES, np.float32)[rng.integers(0, len(WEIGHT_VALUES), size=(3, W, W))]


def _args(name, loss_type, wmap):
    c = R.make_case(name)
    return (c.edit, c.orig, c.chmap, c.sources, c.targets, c.r, c.voxel, c.W, COF, loss_type, wmap)


@lru_cache(maxsize=None)
def oracle(name, loss_type):
    """The weighted float64 result of a case, computed once per session; callers do not modify it."""
    return drag_loss_grad64_weighted(*_args(name, loss_type, weight_map(name)))


@lru_cache(maxsize=None)
def reference32(name, loss_type):
    return drag_loss_grad32_weighted(*_args(name, loss_type, weight_map(name)))


@lru_cache(maxsize=None)
def batch_map():
    """The map of edit 1 of drag_ref.make_batch() (case B's tap shape)."""
    rng = np.random.default_rng(506)
    W = R.make_batch().W
    return np.asarray(WEIGHT_VALUES, np.float32)[rng.integers(0, len(WEIGHT_VALUES), size=(3, W, W))]


def structural_zero(name):
    """bool [W*W, ld]: tap elements whose weighted gradient is zero by construction, in three classes (a dict of masks):
      unmapped   channels no (plane, c) pair maps to (padding included);
      touched    mapped elements of texels outside every target footprint that are touched on every plane mapping the channel;
      freed      the same with at least one such plane untouched at weight 0 (and none untouched at a weight > 0).
    `outside every target footprint`: the whole texel row of the motion-only float64 gradient (L2, cof 0) is zero."""
    c = R.make_case(name)
    res = R.oracle(name, "l2", 0.0)
    outside = ~(res.grad != 0).any(dim=1).numpy()                               # [W*W]
    wmap = weight_map(name).reshape(3, -1)
    untouched = np.stack([m.numpy().reshape(-1) for m in res.setup.masks])      # [3, W*W]
    maps = np.zeros((3, c.ld), bool)
    for p in range(3):
        maps[p, c.chmap[p]] = True
    live = untouched & (wmap > 0)                                               # planes on which the mask term acts
    acts = np.einsum("pt,pc->tc", live.astype(np.int64), maps.astype(np.int64)) > 0
    frees = np.einsum("pt,pc->tc", (untouched & (wmap == 0)).astype(np.int64), maps.astype(np.int64)) > 0
    mapped = maps.any(axis=0)[None, :]
    quiet = outside[:, None] & mapped & ~acts
    return {"unmapped": np.broadcast_to(~mapped, (c.W * c.W, c.ld)).copy(), "touched": quiet & ~frees, "freed": quiet & frees}


# ------------------------------------------------------------------------------------------------ the weight-map cases
MAP_SIZES = ((32, 16), (24, 24), (40, 16))          # (D, W): D = 2 W, D = W, D no multiple of W
MAP_DILATES = (0, 1, 2)
MAP_GRIDS = ("both", "keep", "free", "none")        # which regions carry a voxel grid
MAP_WEIGHTS = ((4.0, 0.0), (2.5, 0.5))


def _corner_and_rod_grids(D):
    """keep: a single set voxel at each of the eight corners and a one-voxel rod along x; free: one-voxel rods along y and z."""
    k, f = np.zeros((D, D, D), bool), np.zeros((D, D, D), bool)
    for ix in (0, D - 1):
        for iy in (0, D - 1):
            for iz in (0, D - 1):
                k[ix, iy, iz] = True
    k[:, D // 3, (2 * D) // 3 + 1] = True
    f[D // 2 + 1, :, D // 5] = True
    f[(3 * D) // 4, D // 4 + 1, :] = True
    return k, f


def map_regions(D, grids):
    """(keep, free) of a weight-map case.  keep: a box that sticks out of the cube, a sphere wholly inside one texel cell (no
    texel centre in it at W = 16 or 24: it adds nothing), [the corner / x-rod grid]; free: a sphere that sticks out, a box thinner
    than a texel along x but not along y and z (a shadow on plane yz only), [the y- / z-rod grid].  The two overlap."""
    kg, fg = _corner_and_rod_grids(D)
    keep = [("box", (-1.3, -0.41, 0.31), (-0.52, 1.7, 0.77)), ("sphere", (0.011, 0.013, 0.017), 0.008)]
    free = [("sphere", (0.9, 0.85, -0.2), 0.43), ("box", (0.01, -0.83, -0.29), (0.03, 0.37, 0.55))]
    if grids in ("both", "keep"):
        keep.append(("voxels", kg))
    if grids in ("both", "free"):
        free.append(("voxels", fg))
    return keep, free
