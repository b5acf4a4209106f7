"""Quadric vertex clustering restated in float64 numpy: the rule of include/ishap.h ("Mesh simplification"), operation for
operation, so that the cell partition, the integer sums, the triangle array and the vertex map of csrc/simplify.hip are compared
with ==.  No GPU, no library: numpy only.  Also the fixture the simplify tests share (fixture_volume) and the per-cluster
position bound of the quadric solve (Result.bound)."""
from typing import NamedTuple

import numpy as np

P_SCALE = 2.0 ** 32
Q_SCALE = 2.0 ** 36
GUARD = 1 << 26


class Overflow(RuntimeError):
    pass


class Result(NamedTuple):
    verts: np.ndarray          # [Vo,3] float32
    tris: np.ndarray           # [Fo,3] int32
    vertex_map: np.ndarray     # [V] int32, -1 = the vertex's cluster is not referenced
    cluster: np.ndarray        # [V] cluster of each input vertex (clusters numbered in ascending cell id)
    cells: np.ndarray          # [C] cell id of each cluster
    counts: np.ndarray         # [C] vertices per cluster
    referenced: np.ndarray     # [C] bool
    nondegenerate: int         # input triangles whose three corners lie in three clusters
    x: np.ndarray              # [C,3] float64 local representative (cell units, before the clamp for count-1 clusters: their p)
    bound: np.ndarray          # [C] float64 bound on |dx| of the quadric solve in cell units (0 for count 1 / average / tr == 0)
    sums: np.ndarray           # [C,16] int64, the row layout of csrc/simplify.h


def fixture_volume(R):
    """max(torus, sphere, slab) on linspace(-1, 1, R)^3, float64 -> float32, positive inside"""
    a = np.linspace(-1.0, 1.0, R)
    x, y, z = np.meshgrid(a, a, a, indexing="ij")
    tor = 0.18 - np.hypot(np.hypot(x, y) - 0.55, z)
    sph = 0.22 - np.sqrt((x - 0.1) ** 2 + (y + 0.05) ** 2 + (z - 0.6) ** 2)
    slab = np.minimum(np.minimum(0.7 - np.abs(x), 0.7 - np.abs(y)), 0.03 - np.abs(z + 0.8))
    return np.maximum(np.maximum(tor, sph), slab).astype(np.float32)


def default_grid(verts, cell):
    """origin = the bounding box's low corner as float64, dims = floor((max - origin) / cell) + 1 per axis"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    lo = v.min(0)
    dims = np.floor((v.max(0) - lo) / float(cell)).astype(np.int64) + 1
    return lo, np.maximum(dims, 1)


def locate(verts, lo, h, dims):
    """(cell coordinates [V,3] int64, unclamped grid coordinates q [V,3], clamped local coordinates p [V,3])"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (v - np.asarray(lo, np.float64)[None, :]) / np.float64(h)
        t = np.floor(q)
        t[np.isnan(t)] = 0.0
        t = np.minimum(np.maximum(t, 0.0), np.asarray(dims, np.float64)[None, :] - 1.0)
        c = t.astype(np.int64)
        p = q - (c.astype(np.float64) + 0.5)
        p[np.isnan(p)] = 0.0
        p = np.minimum(np.maximum(p, -0.5), 0.5)
    return c, q, p


def rotate(tri):
    """rows rotated so that the smallest entry comes first, orientation kept (rows have three distinct entries)"""
    tri = np.asarray(tri)
    k = np.argmin(tri, axis=1)
    idx = (k[:, None] + np.arange(3)[None, :]) % 3
    return np.take_along_axis(tri, idx, axis=1)


def simplify(verts, tris, lo, h, dims, contraction="quadric", regularization=1e-3):
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    V, F = verts.shape[0], tris.shape[0]
    dims = np.asarray(dims, np.int64)
    assert contraction in ("quadric", "average") and h > 0 and (dims >= 1).all() and int(dims.prod()) <= 1 << 30
    c, q, p = locate(verts, lo, h, dims)
    cell = (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]
    cells, cluster = np.unique(cell, return_inverse=True)
    cluster = cluster.reshape(-1)
    C = cells.shape[0]
    sums = np.zeros((C, 16), np.int64)
    np.add.at(sums[:, 0], cluster, 1)
    for a in range(3):
        np.add.at(sums[:, 1 + a], cluster, np.rint(p[:, a] * P_SCALE).astype(np.int64))
    first = np.full(C, V, np.int64)
    np.minimum.at(first, cluster, np.arange(V))
    sums[:, 4] = first
    valid = ((tris >= 0) & (tris < V)).all(axis=1) if F else np.zeros(0, bool)
    ncontrib = np.zeros(C, np.int64)
    guard_sum = np.zeros(C, dtype=object)         # Python integers: this sum decides the overflow error and cannot wrap itself
    if contraction == "quadric" and F:
        tv = tris[valid]
        P0, P1, P2 = q[tv[:, 0]], q[tv[:, 1]], q[tv[:, 2]]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            u, w_ = P1 - P0, P2 - P0
            Nx = u[:, 1] * w_[:, 2] - u[:, 2] * w_[:, 1]
            Ny = u[:, 2] * w_[:, 0] - u[:, 0] * w_[:, 2]
            Nz = u[:, 0] * w_[:, 1] - u[:, 1] * w_[:, 0]
            L = np.sqrt((Nx * Nx + Ny * Ny) + Nz * Nz)
            ok = (L > 0.0) & (L < np.inf)
        tv, Nx, Ny, Nz, L = tv[ok], Nx[ok], Ny[ok], Nz[ok], L[ok]
        nx, ny, nz, w = Nx / L, Ny / L, Nz / L, 0.5 * L
        big = w >= float(GUARD)
        guard = np.where(big, GUARD, np.ceil(np.where(big, 0.0, w))).astype(np.int64)
        for k in range(3):
            cl = cluster[tv[:, k]]
            pk = p[tv[:, k]]
            d = -((nx * pk[:, 0] + ny * pk[:, 1]) + nz * pk[:, 2])
            np.add.at(guard_sum, cl, guard.astype(object))
            np.add.at(ncontrib, cl[~big], 1)
            terms = ((nx, nx), (nx, ny), (nx, nz), (ny, ny), (ny, nz), (nz, nz), (nx, d), (ny, d), (nz, d), (d, d))
            for j, (f, s) in enumerate(terms):
                val = np.rint(((w * (f * s)) * Q_SCALE)[~big]).astype(np.int64)
                np.add.at(sums[:, 5 + j], cl[~big], val)
    # triangles
    ct = np.where(valid[:, None], cluster[np.clip(tris, 0, max(V - 1, 0))], -1) if F and V else np.zeros((F, 3), np.int64)
    distinct = valid & (ct[:, 0] != ct[:, 1]) & (ct[:, 1] != ct[:, 2]) & (ct[:, 0] != ct[:, 2]) if F else np.zeros(0, bool)
    nondeg = int(distinct.sum())
    keep_idx = np.nonzero(distinct)[0]
    rot = rotate(ct[keep_idx]) if nondeg else np.zeros((0, 3), np.int64)
    if nondeg:
        _, firsts = np.unique(rot, axis=0, return_index=True)       # first occurrence = lowest input index
        order = np.sort(firsts)
        rot = rot[order]
    referenced = np.zeros(C, bool)
    referenced[rot.reshape(-1)] = True
    if contraction == "quadric" and any(int(g) >= GUARD for g in guard_sum[referenced]):
        raise Overflow("a referenced cluster's sum of ceil(w) reaches 2^26: use a larger cell or contraction='average'")
    # below the guard every referenced sum fits: |entry| <= sum w 2^36 < 2^62.  An UNREFERENCED cluster may pass it (the device
    # wraps there too and never reads the row); its int64 row is then saturated here, for the record only
    sums[:, 15] = np.array([min(int(g), (1 << 62)) for g in guard_sum], np.int64)
    rank = np.cumsum(referenced) - 1
    out_tris = rank[rot].astype(np.int32).reshape(-1, 3)
    vertex_map = np.where(referenced[cluster], rank[cluster], -1).astype(np.int32)
    # representatives
    n = sums[:, 0].astype(np.float64)
    mean = sums[:, 1:4].astype(np.float64) / (n * P_SCALE)[:, None]
    x = mean.copy()
    bound = np.zeros(C)
    lam = float(regularization)
    if contraction == "quadric":
        S = sums[:, 5:15].astype(np.float64) / Q_SCALE
        tr = (S[:, 0] + S[:, 3]) + S[:, 5]
        for k in np.nonzero((tr != 0.0) & (sums[:, 0] > 1))[0]:
            A = np.array([[S[k, 0], S[k, 1], S[k, 2]], [S[k, 1], S[k, 3], S[k, 4]], [S[k, 2], S[k, 4], S[k, 5]]])
            mu = lam * tr[k]
            x[k] = np.linalg.solve(A + mu * np.eye(3), mu * mean[k] - S[k, 6:9])
            bound[k] = 4.0 * ncontrib[k] * 2.0 ** -36 * (np.abs(x[k]).sum() + 1.0) / (lam * tr[k])
    xc = np.minimum(np.maximum(x, -0.5), 0.5)
    cc = np.stack([cells // (dims[1] * dims[2]), (cells // dims[2]) % dims[1], cells % dims[2]], axis=1).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        rep = (np.asarray(lo, np.float64)[None, :] + np.float64(h) * ((cc + 0.5) + xc)).astype(np.float32)
    single = sums[:, 0] == 1
    rep[single] = verts[first[single]]
    x[single] = p[first[single]]
    return Result(rep[referenced], out_tris, vertex_map, cluster.astype(np.int64), cells, sums[:, 0].copy(), referenced, nondeg, x, bound, sums)
