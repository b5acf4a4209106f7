"""Host checks (no GPU) of tests/mesh_query_ref.py, the float64 oracle of the device distance and parity queries:

* the float64 statement tests/mesh_metrics_ref.point_triangle_d2 agrees with a second one (the closest point by
  voronoi_region, the distance evaluated there) on every family, to 1e-12 relative + 1e-14 absolute.  Both take the
  triangle's normal from mesh_metrics_ref.cross_accurate: with numpy's cross product they disagreed by 4e-11 relative over
  the face of a 1e-5 sliver, because the float64 normal of a thin triangle keeps only 1e-16 * length / height;
* every family's point set puts at least 50 points into every region the triangle has, so that the device test cannot pass
  by never visiting a region;
* float32 numpy transcriptions of tri_dist2: the arithmetic before this oracle existed (Ericson's selection from d1..d6)
  breaks the device test's bound on sliver(1e-3) and thinner, the arithmetic of the kernel now (a frame per triangle) holds it
  on every family.  The oracle can tell the two apart;
* the ambiguous rays of every parity case are at most 1 % of its points.

Measured here (numpy float32, no FMA contraction; 10 triangles x 4 096 points per family; |d - d64| / max(1, M), in
brackets the points over the bound of 1e-5 out of 40 960):

    family                        ericson (before)     min_edges            frame (now)
    fat                           2.2e-07 (0)          2.2e-07 (0)          3.1e-07 (0)
    sliver(0.01)                  2.0e-05 (3)          2.0e-05 (3)          3.5e-07 (0)
    sliver(0.001)                 5.5e-02 (1194)       2.2e-04 (79)         2.7e-07 (0)
    sliver(0.0001)                3.4e-01 (681)        4.7e-05 (4)          2.3e-07 (0)
    sliver(1e-05)                 4.9e-01 (189)        1.2e-06 (0)          3.1e-07 (0)
    sliver(1e-07)                 6.8e-01 (429)        2.1e-07 (0)          4.1e-07 (0)
    needle                        7.9e-02 (1204)       1.8e-07 (0)          2.3e-07 (0)
    collinear                     1.8e-07 (0)          1.6e-07 (0)          3.0e-07 (0)
    point                         1.3e-07 (0)          1.3e-07 (0)          1.3e-07 (0)
    shifted(10):fat               2.5e-08 (0)          1.8e-08 (0)          2.8e-08 (0)
    shifted(10):sliver(0.001)     3.6e-03 (843)        2.9e-05 (5)          2.8e-08 (0)
    shifted(10):sliver(1e-05)     1.0e-01 (166)        9.6e-08 (0)          2.3e-08 (0)
    shifted(10):needle            3.9e-03 (738)        1.2e-08 (0)          3.6e-08 (0)
    shifted(10):collinear         1.3e-08 (0)          1.4e-08 (0)          3.2e-08 (0)
    shifted(100):fat              2.2e-09 (0)          1.9e-09 (0)          3.5e-09 (0)
    shifted(100):sliver(0.001)    4.6e-04 (489)        3.6e-06 (0)          3.6e-09 (0)
    shifted(100):sliver(1e-05)    7.7e-03 (125)        6.4e-09 (0)          3.9e-09 (0)
    shifted(100):needle           4.6e-06 (0)          1.5e-09 (0)          2.7e-09 (0)
    shifted(100):collinear        1.3e-09 (0)          1.6e-09 (0)          3.1e-09 (0)
    on_feature, d / max(1, M)     4.8e-02              1.9e-04              1.6e-07      (bound 1e-6)

"min_edges" is the minimum of Ericson's result and the three clamped edge segments.  It repairs every wrong edge or vertex
region but not a wrong closest point inside the face of a sliver (the edges of a sliver of height h are up to h / 2 away
from a point of its face, and a query point at distance d over the face is then off by h^2 / 8d), so it is transcribed only
to record why the kernel does not use it.  Every error of "ericson" and "min_edges" is an overestimate.  The device, which
contracts products and sums into FMAs, was worse than the "ericson" column (tests/test_gpu_mesh_query.py has its figures): it
also failed on collinear triangles, which this transcription passes.

The open sliver meshes of the device test have a runner-up farther than twice the bound at 0.996 .. 1.0 of their points.
"""
import numpy as np
import pytest

from tests import mesh_metrics_ref as R
from tests import mesh_query_ref as Q

SEEDS = range(10)
ONE = np.array([[0, 1, 2]])
BOUND = 1e-5                     # times max(1, M): the bound of tests/test_gpu_mesh_query.py on a distance


def _cases(name):
    for seed in SEEDS:
        tri = Q.triangle(name, seed)
        yield seed, tri, Q.query_points(tri, seed)


def _rel_err(d2_f32, d64, m):
    d = np.sqrt(np.asarray(d2_f32, np.float64))
    assert np.isfinite(d).all()
    return np.abs(d - d64) / m


@pytest.mark.parametrize("name", Q.family_names())
def test_two_float64_statements_agree(name):
    for _, tri, pts in _cases(name):
        d2, e2 = R.point_triangle_d2(pts, tri, ONE)[:, 0], Q.region_d2(pts, tri)
        assert np.all(np.abs(d2 - e2) <= 1e-12 * d2 + 1e-14)
    if name == "fat":
        for seed in SEEDS:
            tri, pts, _ = Q.on_feature(seed)
            d2, e2 = R.point_triangle_d2(pts, tri, ONE)[:, 0], Q.region_d2(pts, tri)
            assert np.all(np.abs(d2 - e2) <= 1e-12 * d2 + 1e-14)


@pytest.mark.parametrize("name", Q.family_names())
def test_every_region_is_visited(name):
    for seed, tri, pts in _cases(name):
        assert pts.dtype == np.float32 and pts.shape == (Q.NPTS, 3) and tri.dtype == np.float32
        reach = Q.reachable_regions(tri)
        reg = Q.voronoi_region(pts, tri)
        assert set(np.unique(reg)) <= reach, (name, seed)
        for r in reach:
            assert (reg == r).sum() >= 50, (name, seed, r, int((reg == r).sum()))
        if name.endswith("point"):
            assert reach == {"a"}
        elif name.endswith("collinear"):
            assert "face" not in reach and len(reach) == 3
        elif not name.startswith("shifted"):
            assert reach == set(Q.REGIONS)
        near = np.sqrt(Q.region_d2(pts[Q.NPTS // 2:], tri))
        assert near.max() <= Q.NEAR + 1e-5 * Q.magnitude(tri)


def test_families_are_what_they_say():
    for seed in SEEDS:
        v = Q.triangle("collinear", seed).astype(np.float64)
        assert not np.any(R.cross_accurate(v[1] - v[0], v[2] - v[0])) and len({tuple(x) for x in v}) == 3
        v = Q.triangle("point", seed)
        assert np.array_equal(v[0], v[1]) and np.array_equal(v[0], v[2])
        v = Q.triangle("needle", seed).astype(np.float64)
        assert 0 < np.linalg.norm(v[1] - v[0]) <= 1.2e-6 and np.linalg.norm(v[2] - v[0]) > 1e-2
        for m in Q.SHIFTS:
            assert Q.magnitude(Q.triangle(f"shifted({m}):fat", seed)) > m - 1


@pytest.mark.parametrize("name", Q.family_names())
def test_the_kernels_arithmetic_holds_the_bound(name):
    for _, tri, pts in _cases(name):
        d64 = np.sqrt(R.point_triangle_d2(pts, tri, ONE)[:, 0])
        err = _rel_err(Q.tri_dist2_f32(pts, tri, "frame"), d64, Q.magnitude(tri, pts))
        assert err.max() <= BOUND


def test_the_kernels_arithmetic_on_features():
    for seed in SEEDS:
        tri, pts, zero = Q.on_feature(seed)
        m = Q.magnitude(tri, pts)
        d64 = np.sqrt(R.point_triangle_d2(pts, tri, ONE)[:, 0])
        d = np.sqrt(Q.tri_dist2_f32(pts, tri, "frame").astype(np.float64))
        assert zero.sum() > 2500 and (~zero).sum() > 1000
        assert d64[zero].max() <= 1e-7 * m and d64[~zero].min() > 1e-6 * m   # the reference: a rounding of 0, or not 0
        assert np.abs(d - d64).max() <= BOUND * m and d[zero].max() <= 1e-6 * m


@pytest.mark.parametrize("name", [f"sliver({e:g})" for e in Q.SLIVER_EPS[1:]] + ["needle"])
@pytest.mark.parametrize("variant", ["ericson", "min_edges"])
def test_the_oracle_sees_the_earlier_arithmetic_fail(name, variant):
    """The selection from d1..d6 breaks the bound on every sliver from 1e-3 down and on needles.  With the edge segments added
    it still breaks it on sliver(1e-3) and sliver(1e-4) (thinner slivers have no face to speak of); nothing it returns is
    below the true distance."""
    worst, over = 0.0, 0
    for _, tri, pts in _cases(name):
        d64 = np.sqrt(R.point_triangle_d2(pts, tri, ONE)[:, 0])
        m = Q.magnitude(tri, pts)
        d = np.sqrt(Q.tri_dist2_f32(pts, tri, variant).astype(np.float64))
        assert np.all(d - d64 >= -BOUND * m)
        err = np.abs(d - d64) / m
        worst, over = max(worst, float(err.max())), over + int((err > BOUND).sum())
    print(f"{name} {variant}: worst {worst:.2e}, {over} over the bound")
    if variant == "ericson" or name in ("sliver(0.001)", "sliver(0.0001)"):
        assert worst > 2 * BOUND and over >= 4
    else:
        assert worst <= BOUND


def test_box_with_degenerate_triangles_is_the_closed_box():
    v, f = Q.box_with_degenerate_triangles((-0.5,) * 3, (0.5,) * 3)
    assert f.shape == (16, 3)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = {tuple(x) for x in e.tolist()}
    assert len(directed) == len(e) and all((b, a) in directed for a, b in directed)       # closed, consistently wound
    vv = v.astype(np.float64)
    n = R.cross_accurate(vv[f[:, 1]] - vv[f[:, 0]], vv[f[:, 2]] - vv[f[:, 0]])
    area = np.linalg.norm(n, axis=1) / 2
    assert (area == 0).sum() == 1 and ((area > 0) & (area < 1e-5)).sum() == 1
    assert np.isclose((n * vv[f[:, 0]]).sum() / 6, 1.0, rtol=1e-6)                          # volume, outward
    g = np.random.default_rng(0)
    pts = g.uniform(-1.2, 1.2, (2000, 3))
    d, _, _ = R.mesh_distance(v, f, pts)
    assert np.abs(d - np.abs(R.box_sdf(pts, (-0.5,) * 3, (0.5,) * 3))).max() <= 1e-12


def test_sliver_meshes_are_disjoint_cells():
    for ntri in (2, 255, 256, 257, 1025):
        v, f = Q.sliver_mesh(ntri)
        assert v.shape == (3 * ntri, 3) and f.shape == (ntri, 3) and np.abs(v).max() <= 1.0
    v, f = Q.sliver_mesh(257, duplicate=True)
    assert np.array_equal(v[f[1]], v[f[256]]) and not np.array_equal(f[1], f[256])


@pytest.mark.parametrize("ntri", [2, 255, 256, 257, 1025])
def test_open_meshes_have_a_clear_nearest_triangle(ntri):
    """the device test compares triangle indices where the runner-up is farther than twice the bound: at least a quarter of
    the points of every case must be that clear"""
    v, f = Q.sliver_mesh(ntri)
    for npts in (255, 256, 257, 5000):
        pts = Q.mesh_points(v, npts)
        assert pts.shape == (npts, 3) and pts.dtype == np.float32
        d, _, second = R.mesh_distance(v, f, pts)
        assert (second - d > 2 * BOUND * Q.magnitude(v, pts)).mean() >= 0.25


@pytest.mark.parametrize("name", list(Q.occupancy_cases()))
def test_ambiguous_rays_are_rare(name):
    v, f, pts = Q.occupancy_cases()[name]
    assert pts.dtype == np.float32 and v.dtype == np.float32
    tol = Q.ray_tolerance(v, pts)
    assert 2.0 ** -23 < tol < 16 * 2.0 ** -23
    amb = Q.ambiguous_ray(pts, v, f, tol)
    assert amb.mean() <= 0.01
    occ = Q.occupancy64(v, f, pts)
    assert set(np.unique(occ)) <= {0.0, 1.0}
    if "[" not in name:                                   # the closed ones: a sensible share inside
        assert 0.05 < occ.mean() < 0.6
    if "slivers" in name:
        assert len(pts) == 4000


def test_ambiguous_ray_marks_edges_and_vertices():
    v = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    f = np.array([[0, 1, 2]])
    tol = 1e-6
    pts = np.array([[-1, 0.25, 0.25], [-1, 0.5, 0.5], [-1, 0.5, 0.5 + 5e-7], [-1, 0.5, 0.5 + 5e-6], [-1, 0, 0], [-1, -5e-7, 0.3],
                    [-1, 1 + 5e-7, -5e-7], [-1, 2, 2]], np.float64)
    assert Q.ambiguous_ray(pts, v, f, tol).tolist() == [False, True, True, False, True, True, True, False]
    # a projection 1e-6 as wide as long sits on the kernel's edge-on threshold: every ray through it is marked
    v2 = np.array([[0, 0, 0], [0, 1, 0], [0.5, 0.5, 5e-7]], np.float32)
    assert Q.ambiguous_ray(np.array([[-1, 0.5, 2e-7]]), v2, f, 1e-9).tolist() == [True]
