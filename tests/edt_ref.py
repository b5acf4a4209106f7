"""numpy references of the exact squared Euclidean distance transform (csrc/edt.hip), of the feathered weight map
(region_feather_kernel) and of the morphology built on them (ishapediting_amd/regions.py).  Integers are int64 here; the
feather is float64 operation by operation, rounded once."""
import numpy as np

INF = 1 << 30          # ISHAP_EDT_INF


def seeds_of(grid, invert=False):
    s = np.asarray(grid) != 0
    return ~s if invert else s


def edt_brute(grid, axes=7, invert=False):
    """All pairs: for every voxel the minimum over the seeds of its slice of the squared distance along the measured axes."""
    s = seeds_of(grid, invert)
    assert s.ndim == 3
    meas = [a for a in range(3) if (axes >> a) & 1]
    batch = [a for a in range(3) if not (axes >> a) & 1]
    out = np.full(s.shape, INF, np.int64)
    coords = np.stack(np.meshgrid(*(np.arange(n) for n in s.shape), indexing="ij"), -1).reshape(-1, 3)
    flat = out.reshape(-1)
    sv = coords[s.reshape(-1)]
    for c0 in range(0, len(coords), 2048):                       # chunked: 2048 voxels against all seeds
        v = coords[c0:c0 + 2048]
        if len(sv) == 0:
            continue
        d = np.zeros((len(v), len(sv)), np.int64)
        for a in meas:
            d += (v[:, None, a] - sv[None, :, a]) ** 2
        same = np.ones((len(v), len(sv)), bool)
        for a in batch:
            same &= v[:, None, a] == sv[None, :, a]
        d = np.where(same, d, INF)
        flat[c0:c0 + 2048] = np.minimum(d.min(1), INF)
    return out


def edt_separable(grid, axes=7, invert=False):
    """One min-plus per measured axis, by broadcasting: out[i] = min_j (i - j)^2 + f[j]."""
    f = np.where(seeds_of(grid, invert), 0, INF).astype(np.int64)
    assert f.ndim == 3
    for a in range(3):
        if not (axes >> a) & 1:
            continue
        n = f.shape[a]
        i = np.arange(n)
        cost = (i[:, None] - i[None, :]) ** 2                      # [out i][from j]
        g = np.moveaxis(f, a, -1)                                  # [..., j]
        out = np.empty_like(g)
        for i0 in range(0, n, 32):                                 # chunks of output rows keep the broadcast small
            out[..., i0:i0 + 32] = (g[..., None, :] + cost[i0:i0 + 32]).min(-1)
        f = np.moveaxis(np.minimum(out, INF), -1, a)
    return f


def falloff_table(falloff):
    n = max(int(np.ceil(np.float64(falloff) * np.float64(falloff))), 1)
    return np.maximum(0.0, 1.0 - np.sqrt(np.arange(n, dtype=np.float64)) / np.float64(falloff))


def feather_ref(marks, kw, fw, falloff):
    """float32 [3, W, W] from marks uint8 [3, W, W] (bit 0 keep, bit 1 free, after dilation): the rule of
    ishap_region_plane_feather in float64, one operation at a time."""
    marks = np.asarray(marks)
    A = falloff_table(falloff)

    def ramp(bit):
        d2 = edt_separable((marks & bit) != 0, axes=6)
        return np.where(d2 < len(A), A[np.minimum(d2, len(A) - 1)], 0.0)
    ak, af = ramp(1), ramp(2)
    kw64, fw64 = np.float64(np.float32(kw)), np.float64(np.float32(fw))
    hold = 1.0 + (kw64 - 1.0) * ak
    loose = ((fw64 - 1.0) * af) * (1.0 - ak)
    w = (hold + loose).astype(np.float32)
    w = np.where((ak == 0.0) & (af == 0.0), np.float32(1.0), w)
    w = np.where((ak == 0.0) & (af == 1.0), np.float32(fw), w)
    return np.where(ak == 1.0, np.float32(kw), w).astype(np.float32)


def hard_ref(marks, kw, fw):
    marks = np.asarray(marks)
    return np.where(marks & 1, np.float32(kw), np.where(marks & 2, np.float32(fw), np.float32(1.0))).astype(np.float32)


# ---- morphology on bool [D, D, D] grids, r in voxels
def radius2(r):
    return int(np.floor(np.float64(r) * np.float64(r)))


def grow(mask, r):
    mask = np.asarray(mask, bool)
    return mask.copy() if radius2(r) == 0 else edt_separable(mask) <= radius2(r)


def shrink(mask, r):
    mask = np.asarray(mask, bool)
    return mask.copy() if radius2(r) == 0 else edt_separable(mask, invert=True) > radius2(r)


def open_(mask, r):
    return grow(shrink(mask, r), r)


def close_(mask, r):
    return shrink(grow(mask, r), r)


def shell(mask, inner, outer):
    return grow(mask, outer) & ~shrink(mask, inner)


def signed_distance(inside):
    """float32: sqrt(d2 to the nearest inside voxel) - sqrt(d2 to the nearest outside voxel), roots in float64"""
    inside = np.asarray(inside, bool)

    def root(invert):
        d2 = edt_separable(inside, invert=invert)
        return np.where(d2 >= INF, np.inf, np.sqrt(d2.astype(np.float64)))
    return (root(False) - root(True)).astype(np.float32)


def components6(mask):
    """labels (int64, -1 outside) of the 6-connected components of a bool grid, by flood fill; a label is its lowest linear index"""
    mask = np.asarray(mask, bool)
    lab = np.full(mask.shape, -1, np.int64)
    n0, n1, n2 = mask.shape
    for start in zip(*np.nonzero(mask)):
        if lab[start] >= 0:
            continue
        root = (start[0] * n1 + start[1]) * n2 + start[2]
        stack = [start]
        lab[start] = root
        while stack:
            x, y, z = stack.pop()
            for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                q = (x + dx, y + dy, z + dz)
                if 0 <= q[0] < n0 and 0 <= q[1] < n1 and 0 <= q[2] < n2 and mask[q] and lab[q] < 0:
                    lab[q] = root
                    stack.append(q)
    return lab


def neck(sel, vox, r):
    """select_part(point=, neck=r) on a bool selection: None where no voxel of shrink(sel, r) lies within r of the pick voxel"""
    sel = np.asarray(sel, bool)
    k = radius2(r)
    lab = components6(shrink(sel, r))
    idx = np.stack(np.meshgrid(*(np.arange(n) for n in sel.shape), indexing="ij"), -1)
    d2 = ((idx - np.asarray(vox)) ** 2).sum(-1)
    ok = (lab >= 0) & (d2 <= k)
    if not ok.any():
        return None
    lin = (idx[..., 0] * sel.shape[1] + idx[..., 1]) * sel.shape[2] + idx[..., 2]
    key = np.where(ok, d2 * sel.size + lin, np.iinfo(np.int64).max)
    root = lab.reshape(-1)[int(np.argmin(key))]
    return grow(lab == root, r) & sel


# ---- the cases of the device tests
SHAPES = [(1, 1, 1), (2, 3, 5), (1, 1, 70), (70, 1, 1), (17, 33, 65), (64, 64, 64), (65, 1, 130)]
SMALL_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 1, 70), (70, 1, 1)]          # those the all-pairs reference does in no time


def seed_sets(shape, seed=0):
    """name -> uint8 grid: none, all, the eight corners in turn, a full plane, random 1 % and 50 %"""
    n0, n1, n2 = shape
    out = {"none": np.zeros(shape, np.uint8), "all": np.full(shape, 255, np.uint8)}
    for c in range(8):
        g = np.zeros(shape, np.uint8)
        g[(n0 - 1) * (c >> 2 & 1), (n1 - 1) * (c >> 1 & 1), (n2 - 1) * (c & 1)] = 1 + c
        out[f"corner{c}"] = g
    g = np.zeros(shape, np.uint8)
    g[:, n1 // 2, :] = 7
    out["plane"] = g
    rng = np.random.default_rng(1000 * seed + n0 * 31 + n1 * 7 + n2)
    for name, p in (("rand1", 0.01), ("rand50", 0.5)):
        out[name] = (rng.random(shape) < p).astype(np.uint8) * 3
    return out
