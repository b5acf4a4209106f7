"""TEST INFRASTRUCTURE ONLY -- float64 statements and deterministic cases for the two device geometry queries of
csrc/surface.hip: the distance from a point to one triangle (tri_dist2) and the +x ray parity (occupancy_kernel).

* voronoi_region / closest_point: which feature of a triangle (vertex, edge, face) is nearest to a point, from the foot of
  the perpendicular and the three edge parameters.  A second statement of tests/mesh_metrics_ref.point_triangle_d2, and
  not the d1..d6 selection of the kernel.
* ambiguous_ray: the points whose +x ray passes so close to an edge or a vertex of a triangle's (y,z) projection that a
  float32 evaluation of the kernel's rule may count the crossing either way.
* occupancy64: the rule of oracle.surface_cpu.mesh_occupancy, evaluated in float64.
* case builders (float32 arrays, seeded): lone triangles by family, query points (half uniform in the box around the
  triangle, half placed at a distance < 0.05 over a chosen feature), open meshes of disjoint slivers, occupancy meshes.
* tri_dist2_f32: numpy float32 transcriptions of the kernel's arithmetic, as it was (Ericson's selection from d1..d6) and as
  it is (a frame per triangle, then a 2-D distance).  No FMA contraction: a model of the device, not the device.
"""
from __future__ import annotations

import numpy as np
import torch

from tests import mesh_metrics_ref as R

REGIONS = ("a", "b", "c", "ab", "bc", "ac", "face")
_EDGES = ((0, 1), (1, 2), (0, 2))                     # ab, bc, ac: region 3 + k
SLIVER_EPS = (1e-2, 1e-3, 1e-4, 1e-5, 1e-7)
SHIFTS = (10, 100)
NEAR = 0.05                                           # the near half of a point set lies within this of the triangle
NPTS = 4096


# ---------------------------------------------------------------- float64 statements


def closest_point(points, tri):
    """(closest point [P,3], region index [P] into REGIONS) of one triangle `tri` [3,3], in float64.

    The foot of the perpendicular is the closest point when it lies on the inner side of all three edges (face).  Otherwise
    the closest point is on the nearest clamped edge: an edge parameter of 0 or 1 names a vertex (the first of coinciding
    vertices), anything between names the edge (the longest among edges that tie, which only happens on a triangle without
    area)."""
    p = np.asarray(points, np.float64)
    v = np.asarray(tri, np.float64)
    P = len(p)
    first = [min(j for j in range(3) if np.array_equal(v[j], v[i])) for i in range(3)]
    best_d2 = np.full(P, np.inf)
    best_q = np.zeros((P, 3))
    best_r = np.zeros(P, np.int64)
    n = R.cross_accurate(v[1] - v[0], v[2] - v[0])
    nn = float(n @ n)
    order = sorted(range(3), key=lambda k: -float(((v[_EDGES[k][1]] - v[_EDGES[k][0]]) ** 2).sum()))   # longest first
    for k in order if nn > 0 else order[:1]:                 # without area the triangle is its longest edge
        i, j = _EDGES[k]
        e = v[j] - v[i]
        l2 = float(e @ e)
        s = np.clip((p - v[i]) @ e / l2, 0.0, 1.0) if l2 > 0 else np.zeros(P)
        q = v[i] + s[:, None] * e
        d2 = ((p - q) ** 2).sum(-1)
        reg = np.where(s <= 0.0, first[i], np.where(s >= 1.0, first[j], 3 + k))
        take = d2 < best_d2
        best_d2 = np.where(take, d2, best_d2)
        best_q = np.where(take[:, None], q, best_q)
        best_r = np.where(take, reg, best_r)
    if nn > 0:
        t = (p - v[0]) @ n / nn
        foot = p - t[:, None] * n
        inside = np.ones(P, bool)
        for i, j in ((0, 1), (1, 2), (2, 0)):
            inside &= np.cross(v[j] - v[i], foot - v[i]) @ n > 0
        best_q = np.where(inside[:, None], foot, best_q)
        best_r = np.where(inside, 6, best_r)
    return best_q, best_r


def voronoi_region(points, tri):
    """region names [P] (one of REGIONS) of the closest feature of `tri` to every point, in float64"""
    return np.asarray(REGIONS)[closest_point(points, tri)[1]]


def region_d2(points, tri):
    """float64 squared distance, evaluated at the closest point that voronoi_region selects"""
    q, _ = closest_point(points, tri)
    return ((np.asarray(points, np.float64) - q) ** 2).sum(-1)


def reachable_regions(tri):
    """the regions some float32 point can have: all seven with area (less an edge between neighbouring float32 numbers), the
    two ends and the long edge when collinear, one vertex when the triangle is a point"""
    v = np.asarray(tri, np.float64)
    n = R.cross_accurate(v[1] - v[0], v[2] - v[0])
    if n @ n > 0:
        # between two vertices that are neighbouring float32 numbers there is no float32 point: that edge's region is empty
        gap = [np.abs(v[j] - v[i]).max() <= 2 * np.spacing(np.float32(np.abs(v[[i, j]]).max())) for i, j in _EDGES]
        return set(REGIONS) - {REGIONS[3 + k] for k in range(3) if gap[k]}
    l2 = [float(((v[j] - v[i]) ** 2).sum()) for i, j in _EDGES]
    k = int(np.argmax(l2))
    if l2[k] == 0:
        return {"a"}
    i, j = _EDGES[k]
    first = [min(b for b in range(3) if np.array_equal(v[b], v[a])) for a in range(3)]
    return {REGIONS[first[i]], REGIONS[first[j]], REGIONS[3 + k]}


def occupancy64(verts, faces, points) -> np.ndarray:
    """oracle.surface_cpu.mesh_occupancy with every operation in float64 (the inputs are the float32 values)"""
    from oracle import surface_cpu as S
    return S.mesh_occupancy(torch.as_tensor(np.asarray(verts, np.float32)), torch.as_tensor(np.asarray(faces, np.int64)),
                            torch.as_tensor(np.asarray(points, np.float32)), dtype=torch.float64).numpy()


def ray_tolerance(verts, points) -> float:
    """4 float32 ulp of the largest |y| or |z| difference between a point and a vertex.  The kernel decides a crossing from
    q x w and u x q with q = point - vertex A in (y,z): two rounded products and their rounded difference, so the position
    of an edge as the kernel sees it is off by up to about 2 ulp of |q|; twice that is the tolerance."""
    v, p = np.asarray(verts, np.float64)[:, 1:], np.asarray(points, np.float64)[:, 1:]
    ext = max(float((p.max(0) - v.min(0)).max()), float((v.max(0) - p.min(0)).max()))
    return 4 * 2.0 ** -23 * ext


def ambiguous_ray(points, verts, faces, tol) -> np.ndarray:
    """bool [P], float64: the +x ray of the point passes within `tol` (distance in the (y,z) plane) of an edge or a vertex of
    some triangle's projection, or through a triangle whose projected area is within a factor of two of the kernel's
    edge-on rejection (1e-6): the rays occupancy_kernel documents as not counted, widened by float32 rounding."""
    p = np.asarray(points, np.float64)[:, None, 1:]
    v = np.asarray(verts, np.float64)[:, 1:]
    f = np.asarray(faces, np.int64)
    out = np.zeros(len(p), bool)
    for f0 in range(0, len(f), 512):
        T = v[f[f0:f0 + 512]]                                               # [F,3,2]
        for i, j in ((0, 1), (1, 2), (2, 0)):
            a, e = T[None, :, i], (T[:, j] - T[:, i])[None]
            l2 = (e * e).sum(-1)
            s = np.clip(((p - a) * e).sum(-1) / np.where(l2 > 0, l2, 1.0), 0.0, 1.0)
            d2 = ((p - a - s[..., None] * e) ** 2).sum(-1)
            out |= (d2 <= tol * tol).any(1)
        u, w, q = (T[:, 1] - T[:, 0])[None], (T[:, 2] - T[:, 0])[None], p - T[None, :, 0]
        D = u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]
        ratio = np.abs(D) / np.maximum(np.abs(u).sum(-1) * np.abs(w).sum(-1), 1e-300)
        unsure = (ratio > 0.5e-6) & (ratio < 2e-6)
        Ds = np.where(D != 0, D, 1.0)
        sB, sC = (q[..., 0] * w[..., 1] - q[..., 1] * w[..., 0]) / Ds, (u[..., 0] * q[..., 1] - u[..., 1] * q[..., 0]) / Ds
        out |= (unsure & (sB > 0) & (sC > 0) & (sB + sC < 1)).any(1)
    return out


# ---------------------------------------------------------------- float32 transcriptions of tri_dist2


def _seg_f32(ap, ab):
    f = np.float32
    l2 = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2]
    with np.errstate(all="ignore"):
        s = np.where(l2 > 0, np.minimum(np.maximum((ap[0] * ab[0] + ap[1] * ab[1] + ap[2] * ab[2]) / l2, f(0)), f(1)), f(0))
    s = s.astype(f)
    d = [ap[k] - s * ab[k] for k in range(3)]
    return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]


def tri_frame_f32(tri):
    """the per-triangle record of the kernel (tri_frame in csrc/surface.hip), float32 throughout: the triangle rotated so
    that its longest edge comes first, origin a, unit vectors e1 along that edge and e2 across it in the triangle's plane
    (orthogonalised against e1 twice), and the triangle in that frame: (0,0), (L,0), (cx,cy >= 0), with 1/|ac|^2, 1/|bc|^2"""
    f = np.float32
    v = np.asarray(tri, f)

    def dot(x, y):
        return f(f(f(x[0] * y[0]) + f(x[1] * y[1])) + f(x[2] * y[2]))
    l = [dot(v[j] - v[i], v[j] - v[i]) for i, j in ((0, 1), (1, 2), (2, 0))]
    if l[1] > l[0] and l[1] >= l[2]:
        v = v[[1, 2, 0]]
    elif l[2] > l[0] and l[2] > l[1]:
        v = v[[2, 0, 1]]
    a, ab, ac = v[0], v[1] - v[0], v[2] - v[0]
    zero3 = np.zeros(3, f)
    l2 = dot(ab, ab)
    if not l2 > 0:
        return dict(a=a, e1=zero3, e2=zero3, L=f(0), cx=f(0), cy=f(0), iac=f(0), ibc=f(0))
    L = f(np.sqrt(l2))
    e1 = (ab / L).astype(f)
    cx = dot(ac, e1)
    e2 = (ac - cx * e1).astype(f)
    for _ in range(3):                                   # normalise, then remove what is left along e1, twice
        n2 = dot(e2, e2)
        if not n2 > 0:
            e2 = zero3
            break
        e2 = (e2 / f(np.sqrt(n2))).astype(f)
        if _ < 2:
            e2 = (e2 - dot(e2, e1) * e1).astype(f)
    cy = dot(ac, e2)
    if cy < 0:
        e2, cy = -e2, -cy
    lac, lbc = f(f(cx * cx) + f(cy * cy)), f(f((cx - L) * (cx - L)) + f(cy * cy))
    return dict(a=a, e1=e1, e2=e2, L=L, cx=cx, cy=cy, iac=f(1) / lac if lac > 0 else f(0), ibc=f(1) / lbc if lbc > 0 else f(0))


def _frame_dist2_f32(points, tri):
    f = np.float32
    F = tri_frame_f32(tri)
    p = np.asarray(points, f)
    ap = [p[:, k] - F["a"][k] for k in range(3)]
    e1, e2, L, cx, cy = F["e1"], F["e2"], F["L"], F["cx"], F["cy"]
    x = ap[0] * e1[0] + ap[1] * e1[1] + ap[2] * e1[2]
    y = ap[0] * e2[0] + ap[1] * e2[1] + ap[2] * e2[2]
    r = [ap[k] - x * e1[k] - y * e2[k] for k in range(3)]
    z2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]
    t = np.minimum(np.maximum(x, f(0)), L)
    d0 = (x - t) * (x - t) + y * y
    t = np.minimum(np.maximum((x * cx + y * cy) * F["iac"], f(0)), f(1))
    d1 = (x - t * cx) * (x - t * cx) + (y - t * cy) * (y - t * cy)
    ux, ex = x - L, cx - L
    t = np.minimum(np.maximum((ux * ex + y * cy) * F["ibc"], f(0)), f(1))
    d2 = (ux - t * ex) * (ux - t * ex) + (y - t * cy) * (y - t * cy)
    inside = (y > 0) & (ex * y - cy * ux > 0) & (cy * x - cx * y > 0)
    return (z2 + np.where(inside, f(0), np.minimum(np.minimum(d0, d1), d2))).astype(f)


def tri_dist2_f32(points, tri, variant: str):
    """float32 squared distance [P] by the kernel's arithmetic, operation by operation in numpy float32.
    "ericson": the kernel before -- Ericson's region selection from d1..d6, the edge segments only when the result is not
    finite.  "min_edges": the minimum of that and the three clamped edge segments (too little: see the module docstring of
    tests/test_mesh_query_host.py).  "frame": the kernel now -- tri_frame_f32, then a 2-D distance in that frame."""
    if variant == "frame":
        return _frame_dist2_f32(points, tri)
    assert variant in ("ericson", "min_edges")
    fixed = variant == "min_edges"
    f = np.float32
    p = np.asarray(points, f)
    a, b, c = (np.asarray(tri, f)[i] for i in range(3))
    ab, ac, bc = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)], [c[k] - b[k] for k in range(3)]
    ap, bp, cp = ([p[:, k] - x[k] for k in range(3)] for x in (a, b, c))

    def dot(x, y):
        return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    with np.errstate(all="ignore"):
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        one, zero = np.ones_like(d1), np.zeros_like(d1)
        nv, nw, den = vb, vc, va + vb + vc
        for cond, xv, xw, xd in (
                ((va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0), d5 - d6, d4 - d3, (d5 - d6) + (d4 - d3)),
                ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
                ((d6 >= 0) & (d5 <= d6), zero, one, one),
                ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
                ((d3 >= 0) & (d4 <= d3), one, zero, one),
                ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
            nv, nw, den = np.where(cond, xv, nv), np.where(cond, xw, nw), np.where(cond, xd, den)
        r = (f(1) / den).astype(f)
        sv, sw = nv * r, nw * r
        d = [ap[k] - sv * ab[k] - sw * ac[k] for k in range(3)]
        dd = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]).astype(f)
        segs = np.minimum(np.minimum(_seg_f32(ap, ab), _seg_f32(ap, ac)), _seg_f32(bp, bc))
        if fixed:
            return np.fmin(dd, segs).astype(f)
        return np.where(dd <= f(3.0e38), dd, segs).astype(f)


# ---------------------------------------------------------------- lone triangles


def _fat(g):
    while True:
        v = g.uniform(-1, 1, (3, 3))
        l = [np.linalg.norm(v[j] - v[i]) for i, j in _EDGES]
        if np.linalg.norm(np.cross(v[1] - v[0], v[2] - v[0])) > 0.5 * max(l) ** 2 and min(l) > 0.5:
            return v


def _sliver(g, eps):
    a, b = g.uniform(-1, 1, 3), g.uniform(-1, 1, 3)
    return np.stack([a, b, a + g.uniform(0.2, 0.8) * (b - a) + eps * g.standard_normal(3)])


def _needle(g):
    a, c = g.uniform(-1, 1, 3), g.uniform(-1, 1, 3)
    u = g.standard_normal(3)
    return np.stack([a, a + 1e-6 * g.uniform(0.5, 1.0) * u / np.linalg.norm(u), c])


def _collinear(g):
    """three distinct points on one line, exactly: coordinates on a 1/256 grid, the third a dyadic step along the edge"""
    a = np.round(g.uniform(-0.5, 0.5, 3) * 256) / 256
    d = np.round(g.uniform(0.125, 0.5, 3) * 256) / 256 * g.choice([-1.0, 1.0], 3)
    s = g.choice([0.25, 0.5, 2.0, -1.0])
    v = np.stack([a, a + d, a + s * d])
    return v[g.permutation(3)]


def _point(g):
    return np.repeat(g.uniform(-1, 1, (1, 3)), 3, axis=0)


def family_names():
    base = ["fat"] + [f"sliver({e:g})" for e in SLIVER_EPS] + ["needle", "collinear", "point"]
    shifted = [f"shifted({m}):{n}" for m in SHIFTS for n in ("fat", "sliver(0.001)", "sliver(1e-05)", "needle", "collinear")]
    return base + shifted


def triangle(name: str, seed: int) -> np.ndarray:
    """float32 [3,3] triangle of a family (family_names())."""
    shift = 0.0
    if name.startswith("shifted("):
        head, name = name.split(":")
        shift = float(head[len("shifted("):-1])
    g = np.random.default_rng([seed, sum(map(ord, name))])
    if name == "fat":
        v = _fat(g)
    elif name.startswith("sliver("):
        v = _sliver(g, float(name[len("sliver("):-1]))
    else:
        v = {"needle": _needle, "collinear": _collinear, "point": _point}[name](g)
    return (v.astype(np.float32) + np.float32(shift)).astype(np.float32)


def _unit(x):
    return x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), 1e-300)


def _over_feature(g, v, region, n):
    """n float64 points at a distance < NEAR from feature `region` of the float64 triangle v, placed so that the feature is
    their closest one: along the normal over the face, in the outward half plane over an edge, in the normal cone of a
    vertex.  On a triangle without area any direction across the line serves."""
    nrm = R.cross_accurate(v[1] - v[0], v[2] - v[0])
    if not nrm @ nrm > 0:
        i, j = _EDGES[int(np.argmax([((v[j] - v[i]) ** 2).sum() for i, j in _EDGES]))]
        nrm = np.cross(v[j] - v[i], g.standard_normal(3))
    nrm = _unit(nrm)
    dist = g.uniform(0, NEAR, (n, 1))
    k = REGIONS.index(region)
    if k == 6:
        w = g.dirichlet([1.0, 1.0, 1.0], n)
        return w @ v + dist * nrm * g.choice([-1.0, 1.0], (n, 1))
    if k >= 3:
        i, j = _EDGES[k - 3]
        o = 3 - i - j
        e = v[j] - v[i]
        out = -(v[o] - v[i] - ((v[o] - v[i]) @ e) / max(e @ e, 1e-300) * e)          # in plane, away from the third vertex
        out = _unit(out) if out @ out > 0 else _unit(np.cross(e, nrm))
        phi = g.uniform(-np.pi / 2, np.pi / 2, (n, 1))
        return v[i] + g.uniform(0, 1, (n, 1)) * e + dist * (np.cos(phi) * out + np.sin(phi) * nrm)
    e1, e2 = (v[j] - v[k] for j in range(3) if j != k)
    g1 = -(e2 - (e2 @ e1) / max(e1 @ e1, 1e-300) * e1)                       # in plane, across e1, away from e2
    g2 = -(e1 - (e1 @ e2) / max(e2 @ e2, 1e-300) * e2)
    if g1 @ g1 > 0 and g2 @ g2 > 0:                                          # the cone spanned by g1, g2 and +-normal
        u = g.uniform(0, 1, (n, 1)) * _unit(g1) + g.uniform(0, 1, (n, 1)) * _unit(g2) + g.uniform(-1, 1, (n, 1)) * nrm
        return v[k] + dist * _unit(u)
    u = _unit(g.standard_normal((n, 3)))                                     # no area: the half space(s) beyond the vertex
    for e in (e1, e2):
        if e @ e > 0:
            u = np.where((u @ e > 0)[:, None], u - 2 * (u @ e)[:, None] * e / (e @ e), u)
    return v[k] + dist * u


def query_points(tri, seed: int, n: int = NPTS) -> np.ndarray:
    """float32 [n,3]: half uniform in the box [-1,1]^3 about the triangle's coordinates rounded to integers, half within
    NEAR of the triangle, shared evenly among the features that reachable_regions names."""
    v = np.asarray(tri, np.float64)
    g = np.random.default_rng([seed, 77])
    centre = np.round(v.mean(0))
    uniform = centre + g.uniform(-1, 1, (n // 2, 3))
    regs = sorted(reachable_regions(v))
    per = (n - n // 2 + len(regs) - 1) // len(regs)
    near, spare = [], []
    for r in regs:                       # eight candidates per place; those that still have feature r after rounding go first
        cand = _over_feature(g, v, r, 8 * per).astype(np.float32)
        hit = voronoi_region(cand, v) == r
        near.append(cand[hit][:per])
        spare.append(cand[~hit])
    near = np.concatenate(near + spare)[:n - n // 2]
    return np.concatenate([uniform.astype(np.float32), near])


def on_feature(seed: int, n: int = NPTS):
    """(triangle float32 [3,3], points float32 [n,3], zero bool [n]): points at the vertices, at the edge midpoints, at the
    centroid, at random places of the edges and of the face (zero: expected distance 0, or the rounding of the point to
    float32), and on the extensions of the edges beyond their ends (zero False).  Seeds 0-3: fat, 4-6: sliver(1e-3),
    7-9: fat shifted by 100."""
    tri = triangle("fat" if seed < 4 else "sliver(0.001)" if seed < 7 else "shifted(100):fat", seed)
    v = tri.astype(np.float64)
    g = np.random.default_rng([seed, 78])
    fixed = [v[0], v[1], v[2]] + [(v[i] + v[j]) / 2 for i, j in _EDGES] + [v.mean(0)]
    m = (n - len(fixed)) // 3
    k = g.integers(0, 3, m)
    i, j = np.asarray(_EDGES)[k, 0], np.asarray(_EDGES)[k, 1]
    on_edge = v[i] + g.uniform(0, 1, (m, 1)) * (v[j] - v[i])
    on_face = g.dirichlet([1.0, 1.0, 1.0], m) @ v
    rest = n - len(fixed) - 2 * m
    k = g.integers(0, 3, rest)
    i, j = np.asarray(_EDGES)[k, 0], np.asarray(_EDGES)[k, 1]
    s = g.uniform(0.01, 1.0, (rest, 1))
    beyond = np.where(g.uniform(size=(rest, 1)) < 0.5, v[i] - s * (v[j] - v[i]), v[j] + s * (v[j] - v[i]))
    pts = np.concatenate([np.stack(fixed), on_edge, on_face, beyond]).astype(np.float32)
    zero = np.arange(n) < n - rest
    return tri, pts, zero


def magnitude(*arrays) -> float:
    """max(1, largest absolute coordinate): the bound on a distance is 1e-5 times this"""
    return max(1.0, max(float(np.abs(np.asarray(a, np.float64)).max()) for a in arrays))


# ---------------------------------------------------------------- open meshes of disjoint thin triangles


def sliver_mesh(ntri: int, seed: int = 0, shift: float = 0.0, duplicate: bool = False):
    """(verts float32 [3 ntri, 3], faces int32 [ntri, 3]): disjoint slivers, one per cell of a lattice in [-1,1]^3 and listed
    in lattice order (spatially sorted), eps cycling through SLIVER_EPS.  duplicate: the last triangle is listed again at
    index 1, with vertices of its own (equal distances, so the lowest index has to win)."""
    g = np.random.default_rng([seed, ntri])
    side = int(np.ceil(ntri ** (1 / 3)))
    h = 2.0 / side
    tris = []
    for t in range(ntri):
        cell = np.array([t // (side * side), (t // side) % side, t % side], np.float64)
        lo = -1 + cell * h
        a, b = lo + g.uniform(0.1, 0.9, 3) * h, lo + g.uniform(0.1, 0.9, 3) * h
        eps = SLIVER_EPS[t % len(SLIVER_EPS)]
        c = a + g.uniform(0.2, 0.8) * (b - a) + eps * h * g.standard_normal(3)
        tris.append(np.stack([a, b, np.clip(c, lo, lo + h)]))
    if duplicate:
        tris[1] = tris[-1].copy()
    v = (np.concatenate(tris).astype(np.float32) + np.float32(shift)).astype(np.float32)
    return v, np.arange(3 * ntri, dtype=np.int32).reshape(ntri, 3)


def mesh_points(verts, n: int, seed: int = 0) -> np.ndarray:
    """float32 [n,3]: half uniform in the mesh's box grown by 0.1, half within NEAR / 4 of a random vertex"""
    v = np.asarray(verts, np.float64)
    g = np.random.default_rng([seed, n, 79])
    lo, hi = v.min(0) - 0.1, v.max(0) + 0.1
    uniform = g.uniform(lo, hi, (n // 2, 3))
    near = v[g.integers(0, len(v), n - n // 2)] + g.uniform(-NEAR / 4, NEAR / 4, (n - n // 2, 3))
    return np.concatenate([uniform, near]).astype(np.float32)


def box_with_degenerate_triangles(lo, hi):
    """R.box_mesh with the first edge a-b of its first face (a, b, c) split: at the midpoint m, which the neighbour across
    the edge does not use, so the gap is closed by the triangle (a, b, m) without area; and at s, three quarters along and
    1e-5 inside the face, which leaves the sliver (m, b, s).  Closed, consistently wound, and still exactly the box."""
    v, f = R.box_mesh(lo, hi)
    v = v.astype(np.float64)
    a, b, c = (int(x) for x in f[0])
    m = 0.5 * (v[a] + v[b])
    inward = v[c] - m
    s = 0.5 * (m + v[b]) + 1e-5 * inward / np.linalg.norm(inward)
    im, js = len(v), len(v) + 1
    faces = f[1:].tolist() + [[a, im, c], [im, js, c], [js, b, c], [im, b, js], [a, b, im]]
    return np.concatenate([v, m[None], s[None]]).astype(np.float32), np.asarray(faces, np.int32)


# ---------------------------------------------------------------- occupancy cases


def rotated_box(angle: float):
    """closed box [-0.5, 0.4] x [-0.45, 0.5] x [-0.4, 0.55] rotated by `angle` about y, then about z (float32 vertices)"""
    v, f = R.box_mesh((-0.5, -0.45, -0.4), (0.4, 0.5, 0.55))
    c, s = np.cos(angle), np.sin(angle)
    ry = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    return (v.astype(np.float64) @ ry.T @ rz.T).astype(np.float32), f


def near_tie_sphere():
    """closed marching-tetrahedra mesh (oracle.surface_cpu) of a 14^3 sphere whose radius passes 1e-4 outside the lattice
    points (+-4.5, +-0.5, +-0.5) and their permutations: vertices 1e-4 from grid corners, hence thin triangles.  Mapped to
    [-1,1]^3; float32 verts, int32 faces."""
    from oracle import surface_cpu as S
    res = 14
    ax = torch.arange(res, dtype=torch.float64) - (res - 1) / 2
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    vol = (np.sqrt(20.75) + 1e-4) - torch.sqrt(x * x + y * y + z * z)
    v, f = S.marching_tetrahedra(vol.float())
    return (v.numpy() / (res - 1) * 2 - 1).astype(np.float32), f.numpy().astype(np.int32)


def occupancy_cases():
    """name -> (verts, faces, points): the cases of the parity tests, all with random points"""
    cases = {}
    for ang in (0.3, 1e-3, 1e-5):
        v, f = rotated_box(ang)
        cases[f"box rotated {ang:g}"] = (v, f, np.random.default_rng([3, int(ang * 1e6)]).uniform(-0.9, 0.9, (4096, 3)).astype(np.float32))
    # rays through the faces that the 1e-3 box shows nearly edge-on: random points of their (y,z) projections, 1e-3 wide
    v, f = rotated_box(1e-3)
    g = np.random.default_rng(4)
    T = v[f].astype(np.float64)
    u, w = T[:, 1, 1:] - T[:, 0, 1:], T[:, 2, 1:] - T[:, 0, 1:]
    ratio = np.abs(u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]) / (np.abs(u).sum(1) * np.abs(w).sum(1))
    thin = np.flatnonzero(ratio < 1e-2)
    yz = np.concatenate([g.dirichlet([1.0, 1.0, 1.0], 1000) @ T[k][:, 1:] for k in thin])
    cases["box rotated 0.001, rays through its slivers"] = (v, f, np.concatenate([g.uniform(-0.9, 0.9, (len(yz), 1)), yz], 1).astype(np.float32))
    v, f = near_tie_sphere()
    g = np.random.default_rng(5)
    cases["near-tie sphere"] = (v, f, g.uniform(-1, 1, (2048, 3)).astype(np.float32))
    for nt in (255, 256, 257):
        for npts in (255, 256, 257):
            cases[f"sphere[:{nt}] x {npts}"] = (v, f[:nt], g.uniform(-1, 1, (npts, 3)).astype(np.float32))
    return cases
