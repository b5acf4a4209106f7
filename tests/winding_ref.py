"""TEST INFRASTRUCTURE ONLY -- numpy statement of the generalized winding number (csrc/winding.hip):

  mesh   w(q) = 1/(4 pi) sum_f 2 atan2(a.(b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|),  a, b, c = corners - q
         (van Oosterom-Strackee); a triangle without area contributes 0
  cloud  w(q) = 1/(4 pi) sum_i a_i (p_i - q).n_i / r^3,  r^2 = max(|p_i - q|^2, a_i / (2 pi))
  areas  a_i = max(pi d_k(i)^2 / k, 1e-12),  d_k = distance to the k-th nearest other point (by index)

One place where the statement and the device differ on purpose: a query that lies exactly in a triangle's plane and inside
the triangle has a.(b x c) = 0 and a negative denominator, so the statement gives atan2(0, negative) = pi, a solid angle of
+-2 pi by the sign of the zero (w jumps by one across the triangle), while the device adds 0 for every zero numerator.  The GPU tests leave out points closer than 1e-4 to the mesh, so the two are never compared there.

`dtype=np.float64` is the statement the device is held to.  `dtype=np.float32` evaluates the SAME formulas in fp32 with the
primitives added one after the other (np.cumsum adds sequentially): a yardstick for how far fp32 rounding alone moves the
result on given inputs, not the code under test."""
from __future__ import annotations

import numpy as np

AREA_FLOOR = 1e-12


def _sequential_sum(acc, block):
    """acc [P] + block[:, 0] + block[:, 1] + ... in that order, in block's dtype"""
    return np.cumsum(np.concatenate([acc[:, None], block], axis=1), axis=1, dtype=block.dtype)[:, -1]


def _dot(x, y):
    return x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]


def solid_angles(verts, faces, points, dtype=np.float64):
    """[P, F] signed solid angles of every triangle seen from every point"""
    v = np.asarray(verts, dtype)
    f = np.asarray(faces, np.int64)
    q = np.asarray(points, dtype)[:, None, :]
    A, B, C = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n64 = np.cross(B.astype(np.float64) - A.astype(np.float64), C.astype(np.float64) - A.astype(np.float64))
    flat = (n64 == 0).all(axis=1)                                   # exact for fp32 corners: a triangle without area
    a, b, c = A[None] - q, B[None] - q, C[None] - q
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    det = _dot(a, np.cross(b, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    om = (2 * np.arctan2(det, den)).astype(dtype)
    return np.where(flat[None, :], dtype(0), om)


def mesh_winding(verts, faces, points, dtype=np.float64, chunk: int = 512):
    """[P] winding numbers; triangles are added in index order"""
    P = len(points)
    acc = np.zeros(P, dtype)
    for f0 in range(0, len(faces), chunk):
        acc = _sequential_sum(acc, solid_angles(verts, faces[f0:f0 + chunk], points, dtype))
    return (acc * dtype(1 / (4 * np.pi))).astype(dtype)


def cloud_winding(points, normals, areas, query, dtype=np.float64, chunk: int = 1024):
    p, n, a = np.asarray(points, dtype), np.asarray(normals, dtype), np.asarray(areas, dtype)
    q = np.asarray(query, dtype)[:, None, :]
    acc = np.zeros(len(query), dtype)
    for j0 in range(0, len(p), chunk):
        d = p[None, j0:j0 + chunk] - q
        aj = a[None, j0:j0 + chunk]
        r2 = np.maximum(_dot(d, d), aj * dtype(1 / (2 * np.pi)))
        acc = _sequential_sum(acc, (aj * _dot(d, n[None, j0:j0 + chunk]) / (r2 * np.sqrt(r2))).astype(dtype))
    return (acc * dtype(1 / (4 * np.pi))).astype(dtype)


def knn_sq(points, k):
    """[N, k + 1] the k + 1 smallest squared distances (fp64) of every point to the OTHER points, ascending"""
    p = np.asarray(points, np.float64)
    N = len(p)
    out = np.empty((N, k + 1))
    step = max(1, (1 << 22) // N)
    for i in range(0, N, step):
        d2 = ((p[i:i + step, None, :] - p[None]) ** 2).sum(-1)
        d2[np.arange(len(d2)), np.arange(i, i + len(d2))] = np.inf          # not itself; equal points stay, at distance 0
        out[i:i + step] = np.sort(np.partition(d2, k, axis=1)[:, :k + 1], axis=1)
    return out


def cloud_areas(points, k: int = 8):
    return np.maximum(np.pi * knn_sq(points, k)[:, k - 1] / k, AREA_FLOOR)


# ---------------------------------------------------------------- shapes


def box_quads(lo, hi, n: int = 1, skip=()):
    """The surface of the box [lo, hi] as triangles, counter-clockwise seen from outside: every face (except those in `skip`,
    numbered 0..5 = -x +x -y +y -z +z) is an n x n grid of quads, two triangles each.  (vertices float32, faces int32)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    verts, faces = [], []
    for side in range(6):
        if side in skip:
            continue
        axis, top = side // 2, side % 2
        u, w = (axis + 1) % 3, (axis + 2) % 3
        base = len(verts)
        for i in range(n + 1):
            for j in range(n + 1):
                p = np.empty(3)
                p[axis] = hi[axis] if top else lo[axis]
                p[u] = lo[u] + (hi[u] - lo[u]) * i / n
                p[w] = lo[w] + (hi[w] - lo[w]) * j / n
                verts.append(p)
        for i in range(n):
            for j in range(n):
                a, b = base + i * (n + 1) + j, base + (i + 1) * (n + 1) + j
                c, d = b + 1, a + 1
                quad = [(a, b, c), (a, c, d)]                            # (u, w, axis) is right-handed: normal +axis
                faces.extend(quad if top else [(x, z, y) for x, y, z in quad])
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)


def box_with_triangles(count: int, lo=(-0.5, -0.4, -0.3), hi=(0.4, 0.5, 0.6)):
    """`count` triangles of a subdivided box surface, in face order (an open strip unless the count closes the box):
    count = 1 is a single triangle, 12 n^2 the closed box"""
    n = 1
    while 12 * n * n < count:
        n += 1
    v, f = box_quads(lo, hi, n)
    return v, f[:count].copy()


def fibonacci_sphere(n: int, radius: float):
    """n points on the sphere, their outward unit normals and the area each stands for (4 pi r^2 / n), fp32"""
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    phi = i * np.pi * (3 - np.sqrt(5))
    s = np.sqrt(1 - z * z)
    nrm = np.stack([s * np.cos(phi), s * np.sin(phi), z], axis=1)
    return ((radius * nrm).astype(np.float32), nrm.astype(np.float32),
            np.full(n, 4 * np.pi * radius * radius / n, np.float32))
