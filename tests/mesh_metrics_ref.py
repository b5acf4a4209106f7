"""TEST INFRASTRUCTURE ONLY -- fp64 numpy statement of the distance from a point to a triangle mesh, brute force over every
triangle, with the sign of oracle.surface_cpu.mesh_occupancy (the device's +x ray parity rule).

Stated independently of the device kernel's Voronoi-region selection: the closest point of a triangle is the foot of the
perpendicular on its plane when that foot lies inside the triangle, else the nearest of the three clamped edge segments.
Also: analytic box shapes (12-triangle closed meshes and their exact signed distance) for the metrics tests.
"""
from __future__ import annotations

import numpy as np
import torch


def _seg_d2(p, a, b):
    """squared distance [P,F] from points p [P,1,3] to segments a-b [1,F,3]"""
    ab = b - a
    l2 = (ab * ab).sum(-1)
    s = np.where(l2 > 0, ((p - a) * ab).sum(-1) / np.where(l2 > 0, l2, 1.0), 0.0)
    s = np.clip(s, 0.0, 1.0)
    q = a + s[..., None] * ab
    return ((p - q) ** 2).sum(-1)


def _two_prod(a, b):
    """a * b as an unevaluated sum (product, rounding error) of two float64 (Dekker's splitting)"""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def cross_accurate(u, w):
    """u x w with every component a - b of two products rounded once, not once per product: on a thin triangle the
    products cancel, and the plain float64 cross product keeps only 1e-16 / (height / length) of the normal."""
    def dop(a, b, c, d):
        p, e = _two_prod(a, b)
        q, f = _two_prod(c, d)
        return (p - q) + (e - f)
    return np.stack([dop(u[..., 1], w[..., 2], u[..., 2], w[..., 1]), dop(u[..., 2], w[..., 0], u[..., 0], w[..., 2]),
                     dop(u[..., 0], w[..., 1], u[..., 1], w[..., 0])], axis=-1)


def point_triangle_d2(points, verts, faces):
    """[P,F] fp64 squared distances from every point to every triangle."""
    p = np.asarray(points, np.float64)[:, None, :]
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    A, B, C = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    n = cross_accurate(B - A, C - A)
    nn = (n * n).sum(-1)
    ok = nn > 0
    nsafe = np.where(ok[..., None], n, 1.0)
    t = ((p - A) * nsafe).sum(-1) / np.where(ok, nn, 1.0)
    foot = p - t[..., None] * nsafe
    # barycentric signs of the foot: inside when it is on the inner side of all three edges
    s0 = (np.cross(B - A, foot - A) * n).sum(-1)
    s1 = (np.cross(C - B, foot - B) * n).sum(-1)
    s2 = (np.cross(A - C, foot - C) * n).sum(-1)
    inside = ok & (s0 >= 0) & (s1 >= 0) & (s2 >= 0)
    plane = t * t * nn
    edges = np.minimum(np.minimum(_seg_d2(p, A, B), _seg_d2(p, B, C)), _seg_d2(p, C, A))
    return np.where(inside, np.minimum(plane, edges), edges)


def mesh_distance(verts, faces, points, chunk: int = 256):
    """(unsigned distance [P], closest triangle [P] (lowest index on ties), runner-up distance [P]) in fp64."""
    P = len(points)
    d = np.empty(P)
    idx = np.empty(P, np.int64)
    second = np.full(P, np.inf)
    for i in range(0, P, chunk):
        d2 = point_triangle_d2(points[i:i + chunk], verts, faces)
        k = d2.argmin(axis=1)
        d[i:i + chunk] = np.sqrt(d2[np.arange(len(k)), k])
        idx[i:i + chunk] = k
        if d2.shape[1] > 1:
            d2[np.arange(len(k)), k] = np.inf
            second[i:i + chunk] = np.sqrt(d2.min(axis=1))
    return d, idx, second


def occupancy(verts, faces, points) -> np.ndarray:
    """0/1 of oracle.surface_cpu.mesh_occupancy (the rule ishap_mesh_occupancy runs)."""
    from oracle import surface_cpu as S
    return S.mesh_occupancy(torch.as_tensor(np.asarray(verts, np.float32)), torch.as_tensor(np.asarray(faces, np.int64)),
                            torch.as_tensor(np.asarray(points, np.float32))).numpy()


def signed_distance(verts, faces, points):
    """fp64 distance, negative where the occupancy statement says inside."""
    d, _, _ = mesh_distance(verts, faces, points)
    return np.where(occupancy(verts, faces, points) != 0, -d, d)


def box_mesh(lo, hi):
    """closed 12-triangle mesh of the box [lo, hi] (float32 vertices, outward winding)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    corner = np.array([[(i >> k) & 1 for k in range(3)] for i in range(8)], np.float64)
    v = lo + corner * (hi - lo)
    quads = [(0, 2, 6, 4), (1, 3, 7, 5), (0, 1, 5, 4), (2, 3, 7, 6), (0, 1, 3, 2), (4, 5, 7, 6)]
    f = []
    centre = (lo + hi) / 2
    for a, b, c, d in quads:
        for tri in ((a, b, c), (a, c, d)):
            n = np.cross(v[tri[1]] - v[tri[0]], v[tri[2]] - v[tri[0]])
            if np.dot(n, v[list(tri)].mean(0) - centre) < 0:
                tri = (tri[0], tri[2], tri[1])
            f.append(tri)
    return v.astype(np.float32), np.asarray(f, np.int32)


def box_sdf(points, lo, hi):
    """exact signed distance to the box [lo, hi] (negative inside)."""
    p = np.asarray(points, np.float64)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    q = np.abs(p - (lo + hi) / 2) - (hi - lo) / 2
    outside = np.linalg.norm(np.maximum(q, 0.0), axis=1)
    inside = np.minimum(q.max(axis=1), 0.0)
    return outside + inside
