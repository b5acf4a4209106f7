"""The two device geometry queries of csrc/surface.hip against the float64 oracle of tests/mesh_query_ref.py, where a closed,
well-shaped mesh cannot show a wrong per-triangle answer (there the minimum over triangles takes a neighbour's correct
value): lone thin and degenerate triangles, open meshes of disjoint slivers at the tile tails, culling, and the ray parity
on faces nearly parallel to the ray.

Distance (metrics.mesh_distance(..., sdf=False)).  Bound: |d - d64| <= 1e-5 * max(1, M), M the largest absolute coordinate of
triangle and points; 1e-5 is the bound of test_gpu_mesh_metrics.test_signed_distance_matches_the_fp64_statement, whose
coordinates stay below 1.2.  It is not loosened for thin triangles.  Points on a feature: d <= 1e-6 * max(1, M).

Parity (mesh.mesh_occupancy, method "parity") against oracle.surface_cpu.mesh_occupancy evaluated in float64: equal
everywhere outside mesh_query_ref.ambiguous_ray at tolerance mesh_query_ref.ray_tolerance, 4 float32 ulp of the largest (y,z)
difference between a point and a vertex.  The kernel decides a crossing from two cross products of such differences, each
two rounded products and a rounded difference, which moves an edge, as the kernel sees it, by about 2 ulp of that difference;
a ray closer to an edge than that may be counted either way.  The host module caps the set at 1 % of every case.

Measured on one MI355X (10 triangles x 4 096 points per family; worst |d - d64| / max(1, M), in brackets the points over the
bound out of 40 960; "before" is the kernel that selected Ericson's Voronoi region from products of float32 dot products):

    family                        before               now
    fat                           2.5e-07 (0)          2.6e-07 (0)
    sliver(0.01)                  4.8e-05 (3)          3.9e-07 (0)
    sliver(0.001)                 4.4e-02 (1234)       2.8e-07 (0)
    sliver(0.0001)                2.5e+00 (1222)       3.5e-07 (0)
    sliver(1e-05)                 6.0e+00 (546)        3.6e-07 (0)
    sliver(1e-07)                 1.5e+02 (1247)       3.9e-07 (0)
    needle                        7.3e-02 (1208)       2.7e-07 (0)
    collinear                     1.1e+00 (1197)       3.4e-07 (0)
    point                         1.6e-07 (0)          1.6e-07 (0)
    shifted(10):fat               2.3e-08 (0)          2.9e-08 (0)
    shifted(10):sliver(0.001)     6.5e-03 (851)        2.4e-08 (0)
    shifted(10):sliver(1e-05)     8.2e+00 (481)        2.7e-08 (0)
    shifted(10):needle            2.8e-03 (742)        3.1e-08 (0)
    shifted(10):collinear         1.0e-01 (1135)       2.7e-08 (0)
    shifted(100):fat              1.9e-09 (0)          2.8e-09 (0)
    shifted(100):sliver(0.001)    4.4e-04 (476)        3.6e-09 (0)
    shifted(100):sliver(1e-05)    1.7e-01 (464)        3.4e-09 (0)
    shifted(100):needle           1.2e-05 (1)          3.0e-09 (0)
    shifted(100):collinear        1.1e-02 (1052)       3.0e-09 (0)
    on_feature: d / max(1, M)     4.3e-02              1.2e-07              (bound 1e-6)

No output was NaN or infinite, before or now; every error before was an overestimate (the most negative d - d64 was
-2.5e-7).  Now: open sliver meshes 2 .. 1 025 triangles x 255 .. 5 000 points worst 1.1e-7, every clear index equal; the doubled
triangle reported as index 1 at all 614 points nearest to it; sorted against shuffled order 0 differing bits, worst error
5.0e-8 (6.2e-8 shifted by 100, bound 1.0e-3); box with a triangle without area and a 1e-5 sliver 2.4e-7 from box_sdf.
Parity: 0 mismatches in all 14 cases, outside the ambiguous set and inside it; the set holds 0.28 % of the points aimed at the
1e-3 box's nearly edge-on faces and none of the uniform points of the other cases.  occupancy_kernel is unchanged.  The
module runs in 9 s.
"""
import numpy as np
import pytest
import torch

from tests import mesh_metrics_ref as R
from tests import mesh_query_ref as Q

pytestmark = pytest.mark.gpu

SEEDS = range(10)
ONE = np.array([[0, 1, 2]], np.int32)
BOUND = 1e-5


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def device_distance(v, f, pts):
    from ishapediting_amd.metrics import mesh_distance
    d, tri = mesh_distance(torch.from_numpy(np.ascontiguousarray(v)).to(dev()), torch.from_numpy(np.ascontiguousarray(f)).to(dev()),
                           torch.from_numpy(np.ascontiguousarray(pts)).to(dev()), sdf=False)
    return d.cpu().numpy(), tri.cpu().numpy()


# ---------------------------------------------------------------- lone triangles


@pytest.mark.parametrize("name", Q.family_names())
def test_lone_triangle_distance(name):
    worst = 0.0
    for seed in SEEDS:
        tri = Q.triangle(name, seed)
        pts = Q.query_points(tri, seed)
        d, idx = device_distance(tri, ONE, pts)
        d64 = np.sqrt(R.point_triangle_d2(pts, tri, ONE)[:, 0])
        m = Q.magnitude(tri, pts)
        err = np.abs(d.astype(np.float64) - d64) / m
        worst = max(worst, float(np.nanmax(err)))
        print(f"{name} seed {seed}: worst |d - d64| / max(1, M) = {np.nanmax(err):.3e}, non-finite {int((~np.isfinite(d)).sum())}")
        assert np.isfinite(d).all() and (d >= 0).all()
        assert np.all(idx == 0)
        assert err.max() <= BOUND, (name, seed, float(err.max()), Q.voronoi_region(pts[err.argmax()][None], tri)[0])
    print(f"{name}: worst over {len(SEEDS)} triangles {worst:.3e}")


def test_points_on_a_feature():
    worst = zworst = 0.0
    for seed in SEEDS:
        tri, pts, zero = Q.on_feature(seed)
        d, _ = device_distance(tri, ONE, pts)
        d64 = np.sqrt(R.point_triangle_d2(pts, tri, ONE)[:, 0])
        m = Q.magnitude(tri, pts)
        err = np.abs(d.astype(np.float64) - d64) / m
        worst, zworst = max(worst, float(np.nanmax(err))), max(zworst, float(np.nanmax(d[zero])) / m)
        print(f"on_feature seed {seed}: worst error {np.nanmax(err):.3e}, largest d / max(1, M) on a feature {np.nanmax(d[zero]) / m:.3e}")
        assert np.isfinite(d).all()
        assert err.max() <= BOUND
        assert d[zero].max() <= 1e-6 * m
    print(f"on_feature: worst error {worst:.3e}, worst zero {zworst:.3e}")


# ---------------------------------------------------------------- open meshes of disjoint slivers


@pytest.fixture(scope="module")
def open_mesh_refs():
    """(ntri, npts) -> (verts, faces, points, d64, argmin, runner-up), computed once"""
    out = {}
    for ntri in (2, 255, 256, 257, 1025):
        v, f = Q.sliver_mesh(ntri)
        for npts in (255, 256, 257, 5000):
            pts = Q.mesh_points(v, npts)
            out[ntri, npts] = (v, f, pts) + R.mesh_distance(v, f, pts)
    return out


@pytest.mark.parametrize("ntri", [2, 255, 256, 257, 1025])
@pytest.mark.parametrize("npts", [255, 256, 257, 5000])
def test_open_sliver_mesh_distance_and_index(open_mesh_refs, ntri, npts):
    v, f, pts, d64, ridx, second = open_mesh_refs[ntri, npts]
    d, idx = device_distance(v, f, pts)
    bound = BOUND * Q.magnitude(v, pts)
    err = np.abs(d.astype(np.float64) - d64)
    clear = second - d64 > 2 * bound
    print(f"{ntri} triangles x {npts} points: worst error {err.max():.3e} (bound {bound:.3e}), clear {clear.mean():.3f}, "
          f"index mismatches among clear {int((idx[clear] != ridx[clear]).sum())}")
    assert np.isfinite(d).all() and err.max() <= bound
    assert np.all((idx >= 0) & (idx < ntri))
    assert clear.mean() >= 0.25
    np.testing.assert_array_equal(idx[clear], ridx[clear])


def test_lowest_index_wins_an_exact_tie():
    """triangle 256 (the first of the second tile) is listed again at index 1 with vertices of its own"""
    v, f = Q.sliver_mesh(257, duplicate=True)
    g = np.random.default_rng(11)
    near = (v[f[256]].astype(np.float64)[g.integers(0, 3, 600)] + g.uniform(-0.02, 0.02, (600, 3))).astype(np.float32)
    pts = np.concatenate([Q.mesh_points(v, 1000), near])
    d, idx = device_distance(v, f, pts)
    d64, ridx, second = R.mesh_distance(v, f[:256], pts)                 # without the copy: its runner-up is another triangle
    bound = BOUND * Q.magnitude(v, pts)
    tie = (ridx == 1) & (second - d64 > 2 * bound)
    print(f"ties: {int(tie.sum())} points nearest to the doubled triangle, indices reported {np.unique(idx[tie]).tolist()}")
    assert tie.sum() >= 300
    assert np.all(idx[tie] == 1)
    assert not np.any(idx == 256)
    assert np.abs(d - d64).max() <= bound


@pytest.mark.parametrize("shift", [0.0, 100.0])
def test_culling_is_invisible(shift):
    """1 025 slivers in lattice order (tiles are compact slabs, points sorted along the same axis: tiles get skipped) and in a
    seeded shuffle (tiles span the box: none is): the same bits.  Shifted by 100, MD_ABS * (|p| + |box|) is what keeps a
    tile from being skipped on a rounded box distance."""
    v, f = Q.sliver_mesh(1025, shift=shift)
    pts = Q.mesh_points(v, 5000, seed=1)
    pts = pts[np.argsort(pts[:, 0], kind="stable")]
    perm = np.random.default_rng(12).permutation(len(f))
    d_sorted, i_sorted = device_distance(v, f, pts)
    d_shuffled, i_shuffled = device_distance(v, f[perm], pts)
    d64, _, _ = R.mesh_distance(v, f, pts)
    bound = BOUND * Q.magnitude(v, pts)
    err = np.abs(d_sorted.astype(np.float64) - d64).max()
    print(f"culling, shift {shift:g}: worst error {err:.3e} (bound {bound:.3e}), "
          f"bits differ at {int((d_sorted.view(np.int32) != d_shuffled.view(np.int32)).sum())} points")
    assert np.array_equal(d_sorted.view(np.int32), d_shuffled.view(np.int32))
    assert err <= bound
    same = perm[i_shuffled] == i_sorted                                   # the same triangle, unless two are equally near
    assert same.mean() > 0.99


def test_signed_distance_of_a_box_with_degenerate_triangles():
    from ishapediting_amd.metrics import calc_implicit_field
    lo, hi = (-0.5,) * 3, (0.5,) * 3
    v, f = Q.box_with_degenerate_triangles(lo, hi)
    g = torch.Generator().manual_seed(3)
    pts = torch.cat([torch.rand((20000, 3), generator=g) * 2.4 - 1.2, torch.rand((5000, 3), generator=g) - 0.5])
    sd = calc_implicit_field((torch.from_numpy(v).to(dev()), torch.from_numpy(f).to(dev())), pts).cpu().numpy()
    exact = R.box_sdf(pts.numpy(), lo, hi)
    print(f"box with a triangle without area and a 1e-5 sliver: worst |sd - box_sdf| = {np.abs(sd - exact).max():.3e}")
    assert np.isfinite(sd).all()
    assert float(np.abs(sd - exact).max()) <= 2e-6


# ---------------------------------------------------------------- ray parity


@pytest.fixture(scope="module")
def parity_cases():
    return Q.occupancy_cases()


@pytest.mark.parametrize("name", list(Q.occupancy_cases()))
def test_parity_occupancy_outside_the_ambiguous_rays(parity_cases, name):
    from ishapediting_amd.mesh import mesh_occupancy
    v, f, pts = parity_cases[name]
    occ = mesh_occupancy(torch.from_numpy(v).to(dev()), torch.from_numpy(f).to(dev()), torch.from_numpy(pts).to(dev()),
                         method="parity").cpu().numpy()
    ref = Q.occupancy64(v, f, pts)
    amb = Q.ambiguous_ray(pts, v, f, Q.ray_tolerance(v, pts))
    print(f"{name}: {len(f)} triangles, {len(pts)} points, ambiguous {amb.mean():.4%}, inside {ref.mean():.3f}, "
          f"mismatches outside the set {int((occ != ref)[~amb].sum())}, inside it {int((occ != ref)[amb].sum())}")
    assert amb.mean() <= 0.01
    assert set(np.unique(occ)) <= {0.0, 1.0}
    np.testing.assert_array_equal(occ[~amb], ref[~amb])
