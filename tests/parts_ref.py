"""The numpy statement of the part-edit kernels (csrc/parts.hip; include/ishap.h states the rules) and of regions.Rigid /
plan_part_edit, plus the cases the CPU and the GPU tests share.

  select_ref      float32 `volume - level > 0`, voxel centres 2 i / (D - 1) - 1 in float64, box bounds inclusive, sphere
                  (dx dx + dy dy) + dz dz <= r r, a grid ORed in.
  fps_ref         farthest-point picks over integer coordinates: exact integer distances, every tie to the lowest linear index.
                  fps_brute is the definition (all pairwise distances again each round), fps_ref the incremental form.
  transform_ref   the inverse map in float64, in exactly the operation order of the header.
"""
import numpy as np


def centres(D):
    return 2.0 * np.arange(D, dtype=np.float64) / np.float64(D - 1) - 1.0


# ------------------------------------------------------------------------------------------------ (a) select
def select_ref(volume, level, prims, grid=None):
    """prims: [("box", lo, hi) | ("sphere", centre, radius)]; grid: bool / uint8 [D, D, D] or None -> uint8 [D, D, D]"""
    volume = np.asarray(volume, np.float32)
    D = volume.shape[0]
    c = centres(D)
    x, y, z = c[:, None, None], c[None, :, None], c[None, None, :]
    inside = (volume - np.float32(level)) > np.float32(0)
    reg = np.zeros((D, D, D), bool)
    for p in prims:
        if p[0] == "box":
            lo, hi = np.asarray(p[1], np.float64), np.asarray(p[2], np.float64)
            reg |= (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1]) & (z >= lo[2]) & (z <= hi[2])
        else:
            ce, r = np.asarray(p[1], np.float64), np.float64(p[2])
            dx, dy, dz = x - ce[0], y - ce[1], z - ce[2]
            reg |= ((dx * dx + dy * dy) + dz * dz) <= r * r
    if grid is not None:
        reg |= np.asarray(grid) != 0
    return (inside & reg).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ (b) farthest-point handles
def candidates(mask):
    """int64 [M, 3] coordinates of the set voxels in ascending linear index (np.argwhere's order for a C array)"""
    return np.argwhere(np.asarray(mask) != 0).astype(np.int64)


def _lin(coords, D):
    return (coords[:, 0] * D + coords[:, 1]) * D + coords[:, 2]


def _argmax_lowest(values, lin):
    """the entry with the largest value; among equals the lowest linear index"""
    best = np.nonzero(values == values.max())[0]
    return int(best[np.argmin(lin[best])])


def _first(coords, D, start):
    lin = _lin(coords, D)
    if start is not None:
        d = ((coords - np.asarray(start, np.int64)) ** 2).sum(axis=1)
        return _argmax_lowest(-d, lin)
    lo, hi = coords.min(axis=0), coords.max(axis=0)
    d = ((2 * coords - (lo + hi)) ** 2).sum(axis=1)
    return _argmax_lowest(d, lin)


def fps_ref(coords, D, n, start=None):
    """-> (picks int64 [n, 3], dist2 int64 [n], M).  Rounds beyond M: (-1, -1, -1) and 0."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    M = len(coords)
    picks, d2 = -np.ones((n, 3), np.int64), np.zeros(n, np.int64)
    if M == 0:
        return picks, d2, 0
    lin = _lin(coords, D)
    k = _first(coords, D, start)
    picks[0] = coords[k]
    mind = np.full(M, np.iinfo(np.int64).max)
    for r in range(1, min(n, M)):
        mind = np.minimum(mind, ((coords - picks[r - 1]) ** 2).sum(axis=1))
        k = _argmax_lowest(mind, lin)
        picks[r], d2[r] = coords[k], mind[k]
    return picks, d2, M


def fps_brute(coords, D, n, start=None):
    """The definition: every round recomputes the distance of every candidate to every pick made so far."""
    coords = np.asarray(coords, np.int64).reshape(-1, 3)
    M = len(coords)
    picks, d2 = -np.ones((n, 3), np.int64), np.zeros(n, np.int64)
    if M == 0:
        return picks, d2, 0
    lin = _lin(coords, D)
    picks[0] = coords[_first(coords, D, start)]
    for r in range(1, min(n, M)):
        pair = ((coords[:, None, :] - picks[None, :r, :]) ** 2).sum(axis=2)          # [M, r]
        mind = pair.min(axis=1)
        k = _argmax_lowest(mind, lin)
        picks[r], d2[r] = coords[k], mind[k]
    return picks, d2, M


def min_pairwise_dist2(picks):
    p = np.asarray(picks, np.int64)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
    d[np.arange(len(p)), np.arange(len(p))] = np.iinfo(np.int64).max
    return int(d.min())


def handle_points(voxels, D):
    """float32 voxel centres: float64, rounded once"""
    return (2.0 * np.asarray(voxels, np.float64) / np.float64(D - 1) - 1.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ (c) transform
def rotation_ref(axis, degrees):
    """Rodrigues in float64; whole multiples of 90 degrees use exact sines and cosines"""
    k = np.asarray(axis, np.float64)
    k = k / np.sqrt((k * k).sum())
    quarter = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}.get(float(degrees) % 360.0)
    c, s = quarter if quarter is not None else (np.cos(np.deg2rad(float(degrees))), np.sin(np.deg2rad(float(degrees))))
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return c * np.eye(3) + s * K + (1.0 - c) * np.outer(k, k) + 0.0


def apply_ref(R, pivot, t, points):
    """float64: R (x - pivot) + pivot + t, summed left to right"""
    R, p, t = np.asarray(R, np.float64), np.asarray(pivot, np.float64), np.asarray(t, np.float64)
    d = np.asarray(points, np.float64) - p
    return np.stack([((R[a, 0] * d[..., 0] + R[a, 1] * d[..., 1]) + R[a, 2] * d[..., 2]) + p[a] + t[a] for a in range(3)], axis=-1)


def source_indices(D, R, pivot, t):
    """float64 [3][D, D, D]: for every destination voxel the source index BEFORE rounding, (y_a + 1) (D - 1) / 2"""
    R, p, t = np.asarray(R, np.float64), np.asarray(pivot, np.float64), np.asarray(t, np.float64)
    c = centres(D)
    x = (c[:, None, None], c[None, :, None], c[None, None, :])
    d = [x[b] - p[b] - t[b] for b in range(3)]
    out = []
    for a in range(3):
        y = ((R[0, a] * d[0] + R[1, a] * d[1]) + R[2, a] * d[2]) + p[a]          # row a of R^T
        out.append(np.broadcast_to((y + 1.0) * np.float64(D - 1) / 2.0, (D, D, D)))
    return out


def transform_ref(mask, R, pivot, t):
    mask = np.asarray(mask) != 0
    D = mask.shape[0]
    f = [np.rint(v) for v in source_indices(D, R, pivot, t)]              # rint: half to even
    ok = np.ones((D, D, D), bool)
    for v in f:
        ok &= (v >= 0) & (v <= D - 1)
    i = [np.where(ok, v, 0).astype(np.int64) for v in f]
    return (ok & mask[i[0], i[1], i[2]]).astype(np.uint8)


def half_integer_margin(D, R, pivot, t):
    """the smallest distance of any pre-rounding index from a half-integer"""
    return min(float(np.abs(v - np.floor(v) - 0.5).min()) for v in source_indices(D, R, pivot, t))


def plan_ref(mask, R, pivot, t, n, start=None):
    """plan_part_edit: (sources float32 [n, 3], targets float32 [n, 3], moved uint8 grid, spacing).  ValueError for n > M, for
    a target outside the cube and for a region that leaves the cube."""
    mask = np.asarray(mask)
    D = mask.shape[0]
    picks, d2, M = fps_ref(candidates(mask), D, n, start)
    if n > M:
        raise ValueError(f"{n} handles asked of a part of {M} voxels")
    sources = handle_points(picks, D)
    targets = apply_ref(R, pivot, t, sources.astype(np.float64)).astype(np.float32)
    bad = np.nonzero((np.abs(targets) > 1.0).any(axis=1))[0]
    if len(bad):
        raise ValueError(f"handle {int(bad[0])} would move outside [-1, 1]^3")
    moved = transform_ref(mask, R, pivot, t)
    if not moved.any():
        raise ValueError("the moved region is empty")
    return sources, targets, moved, float(np.sqrt(float(d2[n - 1])) * 2.0 / (D - 1))


# ------------------------------------------------------------------------------------------------ shared cases
SIZES = (16, 33, 64)
# the general transforms of the GPU test: (axis, degrees, pivot, translation) -- off-centre pivots, a translation, no axis or
# angle that lands a source index on a half-integer (tests/test_parts_host.py asserts the margin at every size)
GENERAL = (((0.3, -0.5, 0.8), 23.0, (0.21, -0.13, 0.07), (0.11, 0.05, -0.09)),
           ((-0.7, 0.2, 0.4), 141.0, (-0.17, 0.29, 0.12), (-0.06, 0.13, 0.04)))


def l_volume(D):
    """An L of two boxes, +1 inside and -1 outside, float32 [D, D, D]"""
    c = centres(D)
    x, y, z = c[:, None, None], c[None, :, None], c[None, None, :]
    upright = (x >= -0.6) & (x <= -0.2) & (y >= -0.6) & (y <= 0.7) & (z >= -0.3) & (z <= 0.3)
    foot = (x >= -0.6) & (x <= 0.6) & (y >= -0.6) & (y <= -0.2) & (z >= -0.3) & (z <= 0.3)
    return np.where(upright | foot, 1.0, -1.0).astype(np.float32)


def two_blobs_volume(D):
    """Two disconnected boxes, +1 inside and -1 outside"""
    c = centres(D)
    x, y, z = c[:, None, None], c[None, :, None], c[None, None, :]
    a = (x >= -0.8) & (x <= -0.3) & (np.abs(y) <= 0.4) & (np.abs(z) <= 0.4)
    b = (x >= 0.3) & (x <= 0.8) & (np.abs(y) <= 0.4) & (np.abs(z) <= 0.4)
    return np.where(a | b, 1.0, -1.0).astype(np.float32)


def cube_mask(D, lo, hi):
    m = np.zeros((D, D, D), np.uint8)
    m[lo:hi, lo:hi, lo:hi] = 1
    return m


def cross_mask(D, arm):
    """A symmetric 3-D cross about the centre voxel of an odd grid: arms of `arm` voxels along every axis"""
    assert D % 2 == 1
    c = D // 2
    m = np.zeros((D, D, D), np.uint8)
    m[c - arm:c + arm + 1, c, c] = 1
    m[c, c - arm:c + arm + 1, c] = 1
    m[c, c, c - arm:c + arm + 1] = 1
    return m


def first_voxels_mask(D, M):
    """the first M voxels in linear order: the candidates fill whole scan blocks up to M"""
    m = np.zeros(D * D * D, np.uint8)
    m[:M] = 1
    return m.reshape(D, D, D)


def scattered_mask(D, M, seed):
    m = np.zeros(D * D * D, np.uint8)
    m[np.random.default_rng(seed).choice(D * D * D, size=M, replace=False)] = 1
    return m.reshape(D, D, D)
