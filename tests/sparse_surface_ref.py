"""numpy restatement of the sparse surface's bookkeeping (include/ishap.h, "sparse high-resolution surface"): the brick grid,
the integer seed mapping, and the host-side mesh comparisons its tests use.  No device code, no library calls."""
import numpy as np


def bricks_per_axis(R):
    return (R - 1 + 7) // 8


def brick_extent(R, b):
    """first and last fine node of brick b along an axis (its cells lie between them)"""
    return 8 * b, min(8 * b + 8, R - 1)


def seed_range(Rc, R, j):
    """(first, last) brick along an axis whose extent meets coarse cell j's, end points included -- by trying every brick:
    [8 b, min(8 b + 8, R - 1)] / (R - 1) against [j, j + 1] / (Rc - 1), compared as integers after cross-multiplying"""
    hit = [b for b in range(bricks_per_axis(R))
           if brick_extent(R, b)[0] * (Rc - 1) <= (j + 1) * (R - 1) and brick_extent(R, b)[1] * (Rc - 1) >= j * (R - 1)]
    assert hit and hit == list(range(hit[0], hit[-1] + 1))
    return hit[0], hit[-1]


def seed_map(coarse, level, R):
    """bool [nb, nb, nb]: the bricks that overlap a coarse cell whose 8 corners are not all on one side of `level`"""
    Rc, nb = coarse.shape[0], bricks_per_axis(R)
    inside = (coarse.astype(np.float32) - np.float32(level)) > 0
    n = np.zeros((Rc - 1,) * 3, np.int32)
    for c in range(8):
        dx, dy, dz = c & 1, (c >> 1) & 1, (c >> 2) & 1
        n += inside[dx:Rc - 1 + dx, dy:Rc - 1 + dy, dz:Rc - 1 + dz]
    ranges = [seed_range(Rc, R, j) for j in range(Rc - 1)]
    out = np.zeros((nb,) * 3, bool)
    for jx, jy, jz in np.argwhere((n > 0) & (n < 8)):
        (x0, x1), (y0, y1), (z0, z1) = ranges[jx], ranges[jy], ranges[jz]
        out[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = True
    return out


def brick_nodes(R, b):
    """the 9 fine node indices brick b samples along an axis (clamped to R - 1)"""
    return np.minimum(8 * b + np.arange(9), R - 1)


# ---- comparing meshes as sets --------------------------------------------------------------------------------------------
def sorted_vertex_rows(verts):
    """float32 [V,3] -> its rows as uint32 bit patterns, sorted: equal arrays <=> bitwise equal vertex multisets"""
    u = np.ascontiguousarray(verts, np.float32).view(np.uint32).reshape(-1, 3)
    return u[np.lexsort((u[:, 2], u[:, 1], u[:, 0]))]


def canonical_triangles(verts, tris):
    """every triangle as its three vertex POSITIONS (bit patterns), rotated so that the smallest position comes first (the
    cyclic order, i.e. the orientation, is kept), the rows sorted: equal arrays <=> equal triangle multisets"""
    u = np.ascontiguousarray(verts, np.float32).view(np.uint32).reshape(-1, 3)
    p = u[np.asarray(tris, np.int64).reshape(-1, 3)].astype(np.uint64)            # [F,3,3]
    if p.shape[0] == 0:
        return np.zeros((0, 9), np.uint64)
    rows = p.reshape(-1, 9)
    for shift in (1, 2):                              # the lexicographically smallest of the three rotations
        rot = np.roll(p, -shift, axis=1).reshape(-1, 9)
        ne = rot != rows
        col = np.argmax(ne, axis=1)
        at = np.arange(len(rows))
        less = ne.any(axis=1) & (rot[at, col] < rows[at, col])
        rows = np.where(less[:, None], rot, rows)
    return rows[np.lexsort(tuple(rows[:, k] for k in range(8, -1, -1)))]


def same_mesh(va, ta, vb, tb):
    a, b = sorted_vertex_rows(va), sorted_vertex_rows(vb)
    if a.shape != b.shape or not np.array_equal(a, b):
        return False
    ca, cb = canonical_triangles(va, ta), canonical_triangles(vb, tb)
    return ca.shape == cb.shape and bool(np.array_equal(ca, cb))


def vertex_components(nverts, tris):
    """label [V] of every vertex's connected component (union-find over the faces: the three vertices of a triangle are
    joined), the label being the component's smallest vertex index"""
    parent = np.arange(nverts, dtype=np.int64)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    while True:
        m = parent[t].min(axis=1)
        before = parent.copy()
        for k in range(3):
            np.minimum.at(parent, t[:, k], m)
        parent = np.minimum(parent, parent[parent])
        while True:                                   # pointer jumping
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
        if np.array_equal(parent, before):
            return parent


def vertex_bricks(verts, R):
    """for every vertex the inclusive per-axis range [lo, hi] of the bricks whose closed box [8 b, min(8 b + 8, R - 1)]^3 holds
    it (a vertex on a brick face lies in both neighbours) -> (lo [V,3], hi [V,3])"""
    nb = bricks_per_axis(R)
    v = np.asarray(verts, np.float64)
    hi = np.minimum(np.floor(v / 8).astype(np.int64), nb - 1)
    on_face = (v == np.floor(v)) & (np.floor(v) % 8 == 0) & (v > 0)
    lo = np.where(on_face, np.minimum(np.floor(v / 8).astype(np.int64) - 1, nb - 1), hi)
    return lo, hi


def in_bricks(verts, R, brick_mask):
    """bool [V]: the vertex lies in the closed box of a brick of `brick_mask` (bool [nb, nb, nb])"""
    lo, hi = vertex_bricks(verts, R)
    out = np.zeros(len(lo), bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                b = np.stack([np.where(dx, hi[:, 0], lo[:, 0]), np.where(dy, hi[:, 1], lo[:, 1]), np.where(dz, hi[:, 2], lo[:, 2])], 1)
                out |= brick_mask[b[:, 0], b[:, 1], b[:, 2]]
    return out


def select_components(verts, tris, labels, keep_labels):
    """the sub-mesh of the components in `keep_labels` -> (vertices, triangles re-indexed)"""
    keep = np.isin(labels, np.asarray(sorted(keep_labels), np.int64))
    new = np.cumsum(keep) - 1
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    tk = t[keep[t[:, 0]]]
    return np.asarray(verts)[keep], new[tk].astype(np.int32)
