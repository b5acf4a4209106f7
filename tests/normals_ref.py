"""TEST INFRASTRUCTURE ONLY -- numpy statement of the front end for clouds without normals (csrc/normals.hip):

  knn          the k nearest OTHER points of every point, ascending by (squared distance, index)
  pca_normals  C_i = sum over {p_i} + its k neighbours of (q - m)(q - m)^T, q relative to p_i, m their mean; the unit
               eigenvector of the smallest eigenvalue, its component of largest magnitude positive (ties: the lowest axis);
               variation l0 / (l0 + l1 + l2); the relative eigen-gap (l1 - l0) / l2 that conditions the eigenvector
  orient       round r: every point without a level takes, among its OWN neighbours with a level in [1, r), the one with
               the largest |n_i . n_j| (ties: first in neighbour order), flips where that dot is negative, gets level r; a
               round that orients nothing while points remain seeds the remaining point of largest z (ties: smallest
               index), flipped to n_z >= 0, at level r.  rounds = the rounds in which propagation oriented a point.

`dtype=np.float64` is the statement the device is held to; `dtype=np.float32` evaluates the SAME formulas in fp32 (LAPACK's
ssyevd for the eigenvectors): a yardstick for how far fp32 rounding alone moves the result on given inputs, not the code
under test."""
from __future__ import annotations

import numpy as np

from tests.winding_ref import fibonacci_sphere  # noqa: F401  (re-exported: the sphere clouds of the tests)


def knn(points, k: int):
    """(idx [N, k] int64, d2 [N, k] float64)"""
    p = np.asarray(points, np.float64)
    N = len(p)
    idx = np.empty((N, k), np.int64)
    d2o = np.empty((N, k))
    step = max(1, (1 << 22) // N)
    for i in range(0, N, step):
        d2 = ((p[i:i + step, None, :] - p[None]) ** 2).sum(-1)
        rows = np.arange(len(d2))
        d2[rows, np.arange(i, i + len(d2))] = np.inf                   # not itself; equal points stay, at distance 0
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]           # stable: equal distances keep index order
        idx[i:i + step] = order
        d2o[i:i + step] = d2[rows[:, None], order]
    return idx, d2o


def distinct_ranks(d2, k: int, rel: float = 1e-5):
    """[N, k] bool from d2 [N, > k]: ranks whose distance differs from the rank before AND the rank after (rank k, the
    first one outside the list, included) by more than `rel` relative -- where a last-bit change cannot swap two indices"""
    d2 = np.asarray(d2, np.float64)
    far = np.diff(d2[:, :k + 1], axis=1) > rel * d2[:, 1:k + 1]          # [N, k]: rank c against rank c + 1
    return far & np.concatenate([np.ones((len(d2), 1), bool), far[:, :-1]], axis=1)


def signed_by_convention(n):
    """n or -n, row by row: the component of largest magnitude positive, ties to the lowest axis"""
    lead = np.take_along_axis(n, np.argmax(np.abs(n), axis=1)[:, None], axis=1)     # argmax: the first maximum
    return np.where(lead < 0, -n, n)


def pca_normals(points, idx, dtype=np.float64):
    """(normals [N, 3], variation [N], gap [N]) in `dtype`"""
    p = np.asarray(points, dtype)
    q = p[np.asarray(idx, np.int64)] - p[:, None, :]                   # relative to the point before any product
    nb = np.concatenate([np.zeros((len(p), 1, 3), dtype), q], axis=1)
    d = nb - nb.mean(axis=1, keepdims=True, dtype=dtype)
    C = np.einsum("nka,nkb->nab", d, d).astype(dtype)
    w, v = np.linalg.eigh(C)
    n = v[:, :, 0]
    n = n / np.sqrt((n * n).sum(axis=1, keepdims=True))
    s = w.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        var = np.where(s > 0, np.maximum(w[:, 0], 0) / s, 0)
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0)
    return signed_by_convention(n).astype(dtype), var.astype(dtype), gap.astype(dtype)


def orient(points, normals, idx):
    """(signs [N] of +1 / -1 to multiply `normals` by, rounds, seeds)"""
    p = np.asarray(points, np.float64)
    n = np.asarray(normals, np.float64).copy()
    idx = np.asarray(idx, np.int64)
    N = len(p)
    level = np.zeros(N, np.int64)
    signs = np.ones(N, np.int64)
    rounds = seeds = 0
    r = 1
    while True:
        un = np.flatnonzero(level == 0)
        if len(un) == 0:
            return signs, rounds, seeds
        nb = idx[un]
        ok = (level[nb] >= 1) & (level[nb] < r)
        dots = np.einsum("ua,uka->uk", n[un], n[nb])                   # parents have a level below r: nobody flips them now
        a = np.where(ok, np.abs(dots), -1.0)
        c = np.argmax(a, axis=1)                                       # the first maximum
        rows = np.arange(len(un))
        has = a[rows, c] >= 0
        if has.any():
            sel = un[has]
            flip = sel[dots[rows[has], c[has]] < 0]
            n[flip] = -n[flip]
            signs[flip] = -1
            level[sel] = r
            rounds += 1
        else:
            j = un[np.argmax(p[un, 2])]                                # un ascends: the first maximum is the smallest index
            if n[j, 2] < 0:
                n[j] = -n[j]
                signs[j] = -1
            level[j] = r
            seeds += 1
        r += 1


# ---------------------------------------------------------------- clouds (points float32, analytic outward normals float64)


def sphere(n: int = 2000, radius: float = 0.7, centre=(0.0, 0.0, 0.0)):
    p, nrm, _ = fibonacci_sphere(n, radius)
    return (p + np.asarray(centre, np.float32)).astype(np.float32), nrm.astype(np.float64)


def torus(n: int = 3000, R: float = 0.5, r: float = 0.2, seed: int = 0, noise: float = 0.0):
    """area-uniform on the torus about the z axis: the tube angle v is drawn with density (R + r cos v) by rejection"""
    rng = np.random.default_rng(seed)
    v = np.empty(0)
    while len(v) < n:
        c = rng.uniform(0, 2 * np.pi, 2 * n)
        v = np.concatenate([v, c[rng.uniform(0, R + r, 2 * n) < R + r * np.cos(c)]])
    v = v[:n]
    u = rng.uniform(0, 2 * np.pi, n)
    nrm = np.stack([np.cos(v) * np.cos(u), np.cos(v) * np.sin(u), np.sin(v)], axis=1)
    p = np.stack([(R + r * np.cos(v)) * np.cos(u), (R + r * np.cos(v)) * np.sin(u), r * np.sin(v)], axis=1)
    if noise:
        p = p + rng.normal(0, noise, p.shape)
    return p.astype(np.float32), nrm


def cube(per_face: int = 400, half: float = 0.6, seed: int = 0):
    rng = np.random.default_rng(seed)
    pts, nrm = [], []
    for axis in range(3):
        for top in (-1.0, 1.0):
            q = rng.uniform(-half, half, (per_face, 3))
            q[:, axis] = top * half
            e = np.zeros(3)
            e[axis] = top
            pts.append(q)
            nrm.append(np.tile(e, (per_face, 1)))
    return np.concatenate(pts).astype(np.float32), np.concatenate(nrm)


def two_spheres(n_each: int = 1000, radius: float = 0.3):
    a, na = sphere(n_each, radius, (-0.45, 0.0, 0.0))
    b, nb = sphere(n_each, radius, (0.45, 0.0, 0.1))
    return np.concatenate([a, b]), np.concatenate([na, nb])


def uniform_cloud(n: int, seed=None):
    """n uniform random points in [-1, 1]^3, fp32 (seed: n unless given)"""
    return np.random.default_rng(n if seed is None else seed).uniform(-1, 1, (n, 3)).astype(np.float32)


def tie_cloud(seed: int = 0):
    """300 points, every coordinate a multiple of 1/256 in [-1, 1] (every squared distance is exact in fp32 AND fp64, in any
    order of the additions): 196 random ones, a 4 x 4 x 4 lattice of pitch 1/4, 40 repeats of earlier points; shuffled"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-256, 257, (196, 3)) / 256.0
    g = np.arange(4) / 4.0 - 0.375
    b = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    ab = np.concatenate([a, b])
    p = np.concatenate([ab, ab[rng.choice(len(ab), 40, replace=False)]])
    return p[rng.permutation(len(p))].astype(np.float32)


def normal_clouds():
    """name -> (points, analytic outward normals): the clouds the normals are compared on"""
    return {"sphere": sphere(), "torus": torus(), "cube": cube()}


def orientation_clouds():
    """name -> (points, analytic outward normals, seeds the statement needs)"""
    return {"sphere": sphere() + (1,), "torus": torus() + (1,), "noisy_torus": torus(noise=0.004) + (1,),
            "two_spheres": two_spheres() + (2,)}


def angle(a, b):
    """[N] angle between the LINES along a and b (the sign of either does not count), fp64; exact for small angles"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), np.abs((a * b).sum(axis=1)))
