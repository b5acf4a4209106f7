"""The numpy statement of csrc/components.hip and ishapediting_amd/volume.py that the tests compare with, by equality:
lowest-index labels by union-find over the forward neighbour offsets, the component table, the flip, clean_volume's rule,
and the seeded case generators.

A voxel is inside where float32(vol) - float32(level) > 0 (a NaN is outside); p = (x * ny + y) * nz + z."""
import functools

import numpy as np

TILE = (4, 8, 32)            # csrc/components.hip: CC_TX, CC_TY, CC_TZ


def forward_offsets(connectivity):
    """the 3 (connectivity 6) or 13 (26) offsets (dx, dy, dz) > (0, 0, 0) in lexicographic order"""
    assert connectivity in (6, 26)
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if (dx, dy, dz) > (0, 0, 0) and (connectivity == 26 or abs(dx) + abs(dy) + abs(dz) == 1):
                    out.append((dx, dy, dz))
    assert len(out) == (3 if connectivity == 6 else 13)
    return out


def phase_mask(vol, level, phase):
    with np.errstate(invalid="ignore"):
        inside = (np.asarray(vol, np.float32) - np.float32(level)) > np.float32(0)
    return inside if phase in (1, "inside") else ~inside


def _edges(mask, connectivity):
    """(a, b) linear indices of every pair of member voxels one forward offset apart"""
    nx, ny, nz = mask.shape
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    aa, bb = [], []
    for dx, dy, dz in forward_offsets(connectivity):
        def cut(d, n):          # (slice of the first voxel, slice of its neighbour) along one axis
            return (slice(0, n - d), slice(d, n)) if d >= 0 else (slice(-d, n), slice(0, n + d))
        (sx, tx), (sy, ty), (sz, tz) = cut(dx, nx), cut(dy, ny), cut(dz, nz)
        both = mask[sx, sy, sz] & mask[tx, ty, tz]
        aa.append(idx[sx, sy, sz][both])
        bb.append(idx[tx, ty, tz][both])
    return np.concatenate(aa), np.concatenate(bb)


def union_find(n, a, b):
    """parent array after joining every pair (a[i], b[i]): each element's parent is the lowest element of its set.  Union by
    lowest root (np.minimum.at hangs the higher root under the lowest root that asks for it) with full path compression
    between rounds; the trees at least halve in number per round."""
    parent = np.arange(n, dtype=np.int64)
    while True:
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        ra, rb = parent[a], parent[b]
        open_ = ra != rb
        if not open_.any():
            return parent
        a, b, ra, rb = a[open_], b[open_], ra[open_], rb[open_]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))


def label(vol, level=0.0, phase=1, connectivity=6):
    """int32 labels of vol's shape: the lowest linear index of the voxel's component, -1 for voxels of the other phase"""
    mask = phase_mask(vol, level, phase)
    a, b = _edges(mask, connectivity)
    parent = union_find(mask.size, a, b)
    return np.where(mask.reshape(-1), parent, -1).astype(np.int32).reshape(mask.shape)


def flood_fill_label(vol, level=0.0, phase=1, connectivity=6):
    """the same labels by brute force: voxels in index order, each unlabelled member starts a stack-based flood fill"""
    mask = phase_mask(vol, level, phase)
    nx, ny, nz = mask.shape
    fwd = forward_offsets(connectivity)
    nbrs = fwd + [(-dx, -dy, -dz) for dx, dy, dz in fwd]
    out = np.full(mask.shape, -1, np.int32)
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                if not mask[x, y, z] or out[x, y, z] >= 0:
                    continue
                root = (x * ny + y) * nz + z
                out[x, y, z] = root
                stack = [(x, y, z)]
                while stack:
                    cx, cy, cz = stack.pop()
                    for dx, dy, dz in nbrs:
                        qx, qy, qz = cx + dx, cy + dy, cz + dz
                        if 0 <= qx < nx and 0 <= qy < ny and 0 <= qz < nz and mask[qx, qy, qz] and out[qx, qy, qz] < 0:
                            out[qx, qy, qz] = root
                            stack.append((qx, qy, qz))
    return out


def table(labels):
    """int32 [C, 9] rows (root, voxels, xmin, xmax, ymin, ymax, zmin, zmax, border), ascending root order"""
    nx, ny, nz = labels.shape
    flat = labels.reshape(-1)
    member = flat >= 0
    roots, inv, counts = np.unique(flat[member], return_inverse=True, return_counts=True)
    out = np.zeros((len(roots), 9), np.int32)
    out[:, 0], out[:, 1] = roots, counts
    p = np.nonzero(member)[0]
    coords = (p // (ny * nz), (p // nz) % ny, p % nz)
    border = np.zeros(len(roots), bool)
    for axis, (c, n) in enumerate(zip(coords, (nx, ny, nz))):
        lo = np.full(len(roots), np.iinfo(np.int32).max, np.int64)
        hi = np.full(len(roots), -1, np.int64)
        np.minimum.at(lo, inv, c)
        np.maximum.at(hi, inv, c)
        out[:, 2 + 2 * axis], out[:, 3 + 2 * axis] = lo, hi
        border |= (lo == 0) | (hi == n - 1)
    out[:, 8] = border
    return out


def flip(vol, labels, level, roots):
    """the listed components reflected across the level, in float32; everything else, and every NaN, bit for bit"""
    vol = np.asarray(vol, np.float32)
    level = np.float32(level)
    hit = np.isin(labels, np.asarray(roots, np.int64)) & (labels >= 0) & ~np.isnan(vol)
    with np.errstate(invalid="ignore"):
        was_in = (vol - level) > 0
        mirrored = (level - (vol - level)).astype(np.float32)
        stuck = hit & ~was_in & ~((mirrored - level) > 0)
    mirrored[stuck] = np.nextafter(level, np.float32(np.inf))
    out = vol.copy()
    out[hit] = mirrored[hit]
    return out


def select(voxels, keep="largest", min_voxels=0, min_fraction=0.0):
    """bool mask of the table rows clean_volume keeps: the `keep` largest (ties to the lower root = the earlier row), then
    those with at least max(min_voxels, min_fraction * largest) voxels"""
    voxels = np.asarray(voxels, np.int64)
    c = len(voxels)
    k = c if keep is None else (1 if keep == "largest" else min(int(keep), c))
    kept = np.zeros(c, bool)
    if c == 0:
        return kept
    order = sorted(range(c), key=lambda i: (-voxels[i], i))
    kept[order[:k]] = True
    return kept & (voxels.astype(np.float64) >= max(float(min_voxels), float(min_fraction) * int(voxels.max())))


def clean(vol, level=0.0, keep="largest", min_voxels=0, min_fraction=0.0, fill_cavities=False, connectivity=6):
    """(cleaned volume, info) as volume.clean_volume(..., return_info=True)"""
    out = np.asarray(vol, np.float32).copy()
    info = {"components": 0, "removed": 0, "removed_voxels": 0, "cavities": 0, "filled_voxels": 0}
    lab = label(out, level, 1, connectivity)
    tab = table(lab)
    info["components"] = len(tab)
    if len(tab) > 1:
        gone = ~select(tab[:, 1], keep, min_voxels, min_fraction)
        info["removed"], info["removed_voxels"] = int(gone.sum()), int(tab[gone, 1].sum())
        out = flip(out, lab, level, tab[gone, 0])
    if fill_cavities:
        lab = label(out, level, 0, connectivity)
        tab = table(lab)
        closed = tab[:, 8] == 0
        info["cavities"], info["filled_voxels"] = int(closed.sum()), int(tab[closed, 1].sum())
        out = flip(out, lab, level, tab[closed, 0])
    return out, info


def mesh_components(triangles, nverts):
    """number of connected components of a triangle mesh: union-find over the triangles' vertex ids (unused vertices not counted)"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if len(t) == 0:
        return 0
    parent = union_find(nverts, np.concatenate([t[:, 0], t[:, 1]]), np.concatenate([t[:, 1], t[:, 2]]))
    return len(np.unique(parent[np.unique(t)]))


# ---------------------------------------------------------------------------------------------------- cases
def boxes():
    tx, ty, tz = TILE
    return [(1, 1, 1), (tx - 1, ty, tz + 1), (2 * tx + 1, ty + 1, 3 * tz - 1), (64, 64, 64)]


def _signed(mask, rng):
    """float32 volume with the given inside mask at level 0: magnitudes in [0.1, 1)"""
    mag = rng.uniform(0.1, 1.0, mask.shape).astype(np.float32)
    return np.where(mask, mag, -mag).astype(np.float32)


def serpentine_mask(shape):
    """one voxel wide: every second z row of the box (y even, every x), consecutive rows of a plane joined at alternating ends.
    One component of about n / 2 voxels that crosses every tile seam; inside a plane the only way from row to row is along
    the rows, ny * nz / 2 steps from end to end."""
    nx, ny, nz = shape
    m = np.zeros(shape, bool)
    m[:, 0::2, :] = True
    for k, y in enumerate(range(1, ny - 1, 2)):
        m[:, y, (nz - 1) if k % 2 == 0 else 0] = True
    return m


def path_mask(shape):
    """a single path: the serpentine of every second PLANE (x even), consecutive planes joined by one voxel at alternating ends
    of the plane's snake: about n / 4 voxels, every one (but the ends) with exactly two face neighbours"""
    nx, ny, nz = shape
    m = np.zeros(shape, bool)
    m[0::2] = serpentine_mask((1, ny, nz))[0]
    rows = list(range(0, ny, 2))
    start = (0, 0)
    last_k = len(rows) - 1                       # the snake enters row k at z = 0 when k is even, at z = nz - 1 when odd
    end = (rows[-1], (nz - 1) if last_k % 2 == 0 else 0)
    for j, x in enumerate(range(1, nx - 1, 2)):
        y, z = end if j % 2 == 0 else start
        m[x, y, z] = True
    return m


def combs_mask(shape):
    """two combs whose teeth interleave diagonally: A = teeth at (x even, y even) on a spine in the plane z = 0, B = teeth at
    (x odd, y odd) hanging from a spine in the plane z = nz - 1.  They touch across voxel edges and corners only."""
    nx, ny, nz = shape
    x, y, z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    yl = ny - 1 if (ny - 1) % 2 == 1 else ny - 2          # an odd row for B's cross bar
    a = ((z == 0) & ((x % 2 == 0) | (y == 0))) | ((x % 2 == 0) & (y % 2 == 0) & (z <= nz - 2))
    b = ((z == nz - 1) & ((x % 2 == 1) | (y == yl))) | ((x % 2 == 1) & (y % 2 == 1) & (z >= 1))
    if nz < 3 or yl < 1:
        return a
    return a | b


def checkerboard_mask(shape):
    x, y, z = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return (x + y + z) % 2 == 0


CASES = [          # (name, connectivities)
    ("all_outside", (6, 26)), ("all_inside", (6, 26)), ("bernoulli31", (6,)), ("bernoulli10", (26,)), ("serpentine", (6, 26)),
    ("path", (6,)), ("combs", (6, 26)), ("checkerboard", (6, 26)), ("nans", (6, 26)), ("level", (6, 26)),
]


@functools.lru_cache(maxsize=None)
def case(name, shape):
    """(float32 volume, level) of a named case; seeded by the name and the shape"""
    rng = np.random.default_rng([sum(map(ord, name))] + list(shape))
    level = 0.0
    if name == "all_outside":
        vol = _signed(np.zeros(shape, bool), rng)
    elif name == "all_inside":
        vol = _signed(np.ones(shape, bool), rng)
    elif name == "bernoulli31":
        vol = _signed(rng.random(shape) < 0.31, rng)
    elif name == "bernoulli10":
        vol = _signed(rng.random(shape) < 0.10, rng)
    elif name == "serpentine":
        vol = _signed(serpentine_mask(shape), rng)
    elif name == "path":
        vol = _signed(path_mask(shape), rng)
    elif name == "combs":
        vol = _signed(combs_mask(shape), rng)
    elif name == "checkerboard":
        vol = _signed(checkerboard_mask(shape), rng)
    elif name == "nans":
        vol = _signed(rng.random(shape) < 0.45, rng)
        vol[rng.random(shape) < 0.08] = np.nan
    elif name == "level":
        level = 0.37
        vol = rng.normal(0.37, 0.5, shape).astype(np.float32)
        vol[rng.random(shape) < 0.05] = np.float32(0.37)         # exactly at the level: outside
    else:
        raise KeyError(name)
    vol.setflags(write=False)
    return vol, level


@functools.lru_cache(maxsize=None)
def case_labels(name, shape, phase, connectivity):
    vol, level = case(name, shape)
    lab = label(vol, level, phase, connectivity)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def scene40():
    """The clean_volume scene, 40^3, analytic (value = signed distance-like, positive inside):
    a ball of radius 13 at (20, 20, 20) with an enclosed cavity of radius 6, a floater of radius 2 inside the cavity, two
    floaters of equal size (2 x 2 x 2 boxes) outside the ball -- the tie --, and a slab two voxels thick on the face x = 0.
    One cavity voxel sits exactly at the level."""
    n = 40
    x, y, z = np.meshgrid(*[np.arange(n, dtype=np.float32)] * 3, indexing="ij")
    r = np.sqrt((x - 20) ** 2 + (y - 20) ** 2 + (z - 20) ** 2)
    vol = np.minimum(13.2 - r, r - 6.3)                      # the shell: inside for 6.3 < r < 13.2
    vol = np.maximum(vol, 2.2 - r)                            # the floater in the cavity
    vol = np.minimum(vol, 3.0)
    vol[vol <= 0] = np.minimum(vol[vol <= 0], -0.05)
    vol[36:38, 5:7, 5:7] = 0.8                                # two equal floaters: roots ascending in this order
    vol[36:38, 30:32, 30:32] = 0.6
    vol[0:2, :, :] = np.maximum(vol[0:2, :, :], 0.5)          # the slab on the face x = 0
    vol[20, 20, 24] = 0.0                                     # a cavity voxel exactly at the level
    vol = vol.astype(np.float32)
    vol.setflags(write=False)
    return vol
