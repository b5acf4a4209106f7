"""Generalized winding number on the device (csrc/winding.hip: ishap_mesh_winding, ishap_cloud_winding, ishap_cloud_areas,
sdf == 2 of ishap_mesh_distance) through the public functions, against the numpy statement tests/winding_ref.py and
closed forms.

Tolerance of every comparison with the fp64 statement: 4 x the largest error of the fp32 numpy evaluation of the same
formulas on the same inputs (winding_ref, dtype=np.float32), and not below 2e-6 -- fp32 rounding as measured, never what
the device gives.  Points closer than 1e-4 (fp64) to the mesh, where w jumps by one, are left out; they may be 1 % at most."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from tests import mesh_metrics_ref as R
from tests import winding_ref as W

pytestmark = pytest.mark.gpu

NEAR = 1e-4
BAND = 0.05


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def smooth_field(res, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((1, 1, 6, 6, 6), generator=g)
    return torch.nn.functional.interpolate(f, size=(res, res, res), mode="trilinear", align_corners=True)[0, 0].contiguous()


def grid_mesh(vol):
    """marching-cubes mesh of a volume, vertices mapped to [-1, 1]"""
    from ishapediting_amd.mesh import extract_surface
    res = vol.shape[0]
    v, f = extract_surface(vol.to(dev()))
    return (v / (res - 1) * 2 - 1).contiguous(), f


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def tolerance(w32, w64):
    return max(4 * float(np.abs(w32.astype(np.float64) - w64).max()), 2e-6)


def uniform_points(n, seed, half=1.2):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand((n, 3), generator=g) * 2 - 1) * half).numpy()


def over_points(fn, pts, blocks=16):
    """fn(points) -> [P] (or a tuple of [P] arrays) evaluated on `blocks` slices of the points by as many threads: every
    point's value, and the order its primitives are added in, is what one call over all points gives"""
    if len(pts) < 64 * blocks:
        return fn(pts)
    with ThreadPoolExecutor(blocks) as ex:
        parts = list(ex.map(fn, np.array_split(pts, blocks)))
    if isinstance(parts[0], tuple):
        return tuple(np.concatenate(x) for x in zip(*parts))
    return np.concatenate(parts)


def open_edges(faces):
    """number of edges that do not lie in exactly two triangles"""
    t = np.asarray(faces, np.int64)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    return int((np.unique(e, axis=0, return_counts=True)[1] != 2).sum())


def check_mesh(v, f, pts, what):
    """device w against the statement on (v, f, pts) numpy arrays; returns (device w as numpy, kept mask, tolerance)"""
    from ishapediting_amd.mesh import mesh_winding_number
    w64 = over_points(lambda q: W.mesh_winding(v, f, q, chunk=128), pts)
    tol = tolerance(over_points(lambda q: W.mesh_winding(v, f, q, np.float32, chunk=128), pts), w64)
    keep = over_points(lambda q: R.mesh_distance(v, f, q)[0], pts) >= NEAR
    w = mesh_winding_number(T(v), T(f), T(pts)).cpu().numpy()
    err = float(np.abs(w[keep] - w64[keep]).max()) if keep.any() else 0.0
    print(f"{what}: |w - fp64| max {err:.3e}, tolerance {tol:.3e}, left out {(~keep).mean():.4%}")
    assert (~keep).mean() <= 0.01
    assert err <= tol
    return w, keep, tol


@pytest.fixture(scope="module")
def closed():
    """The 28^3 smooth-field mesh, 20 000 queries in [-1.2, 1.2]^3 and everything the statement says about them.
    grid_mesh(smooth_field(28, 5)) as it comes is cut open where the surface meets the volume's faces (marching cubes emits
    nothing beyond the grid), and inside / outside by parity means nothing for a ray that leaves through such a cut; the
    volume's outer layer is therefore set to outside first, which closes the surface: every edge lies in two triangles."""
    vol = smooth_field(28, 5)
    raw_open = open_edges(grid_mesh(vol)[1].cpu().numpy())
    for axis in range(3):
        vol.select(axis, 0).fill_(-1.0)
        vol.select(axis, 27).fill_(-1.0)
    v, f = grid_mesh(vol)
    assert 1000 < f.shape[0] < 20000
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    print(f"smooth_field(28, 5): {raw_open} open edges as extracted, {open_edges(fn)} with the outer layer outside")
    assert open_edges(fn) == 0
    pts = uniform_points(20000, 1)
    w64 = over_points(lambda q: W.mesh_winding(vn, fn, q, chunk=128), pts)
    w32 = over_points(lambda q: W.mesh_winding(vn, fn, q, np.float32, chunk=128), pts)
    d64 = over_points(lambda q: R.mesh_distance(vn, fn, q)[0], pts)
    out = dict(v=v, f=f, vn=vn, fn=fn, pts=pts, w64=w64, tol=tolerance(w32, w64), d64=d64)
    return out


def test_closed_mesh_against_the_statement_and_parity(closed):
    from ishapediting_amd.mesh import mesh_occupancy, mesh_winding_number, orientation_sign
    from ishapediting_amd.metrics import calc_implicit_field, mesh_distance
    v, f, p = closed["v"], closed["f"], T(closed["pts"])
    w = mesh_winding_number(v, f, p)
    keep = closed["d64"] >= NEAR
    err = float(np.abs(w.cpu().numpy() - closed["w64"])[keep].max())
    print(f"closed mesh, {f.shape[0]} triangles: |w - fp64| max {err:.3e}, tolerance {closed['tol']:.3e}, "
          f"left out {(~keep).mean():.4%}, orientation {orientation_sign(v, f)}")
    assert (~keep).mean() <= 0.01
    assert err <= closed["tol"]
    occ_w, occ_p = mesh_occupancy(v, f, p, method="winding"), mesh_occupancy(v, f, p)
    k = T(keep)
    assert 0.05 < float(occ_p.mean()) < 0.95
    assert torch.equal(occ_w[k], occ_p[k])
    assert torch.equal(mesh_occupancy(v, f, p, method="parity"), occ_p)
    d1, t1 = mesh_distance(v, f, p, sdf=1)
    d2, t2 = mesh_distance(v, f, p, sdf=2)
    assert torch.equal(d1, d2) and torch.equal(t1, t2)
    assert torch.equal(calc_implicit_field((v, f), p, sign="winding"), d1)
    assert torch.equal(calc_implicit_field((v, f), p, sdf=False, sign="winding"), occ_w)


@pytest.mark.parametrize("nq", [5, 256, 4097])
@pytest.mark.parametrize("ntris", [1, 255, 256, 257, 1000])
def test_triangle_tiles_and_parts(ntris, nq):
    """1 .. 1000 triangles of a subdivided box surface (an open strip): across the 256-triangle LDS tile and, with few
    queries, through the part sums; repeatable, and a query's value does not depend on its position."""
    from ishapediting_amd.mesh import mesh_winding_number
    v, f = W.box_with_triangles(ntris)
    assert f.shape[0] == ntris
    pts = uniform_points(nq, 100 + ntris + nq)
    w, _, _ = check_mesh(v, f, pts, f"{ntris} triangles x {nq} queries")
    again = mesh_winding_number(T(v), T(f), T(pts))
    assert torch.equal(again, T(w))
    perm = torch.randperm(nq, generator=torch.Generator().manual_seed(7))
    shuffled = mesh_winding_number(T(v), T(f), T(pts)[perm.to(dev())].contiguous())
    assert torch.equal(shuffled, again[perm.to(dev())])


def test_more_tiles_than_parts():
    """20 000 triangles (79 tiles) x 5 queries: more tiles than the largest number of parts, so a part walks several tiles
    and the last part is shorter than the others"""
    from ishapediting_amd.mesh import mesh_winding_number
    v, f = W.box_with_triangles(20000)
    assert f.shape[0] == 20000
    pts = uniform_points(5, 31)
    w, _, _ = check_mesh(v, f, pts, "20000 triangles x 5 queries")
    assert torch.equal(mesh_winding_number(T(v), T(f), T(pts)), T(w))
    assert torch.equal(mesh_winding_number(T(v), T(f), T(pts[::-1].copy())), T(w[::-1].copy()))


def test_open_surfaces():
    from ishapediting_amd.mesh import mesh_occupancy, mesh_winding_number
    centre = np.zeros((1, 3), np.float32)
    # cube without its +z face
    v, f = W.box_quads((-0.5,) * 3, (0.5,) * 3, 3, skip=(5,))
    w, _, tol = check_mesh(v, f, centre, "cube minus a face")
    assert abs(float(w[0]) - 5 / 6) <= tol
    # a square seen from its axis
    a, h = 0.5, np.float64(np.float32(0.3))
    sq_v = np.array([[-a, -a, h], [a, -a, h], [a, a, h], [-a, a, h]], np.float32)
    sq_f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    w, _, tol = check_mesh(sq_v, sq_f, centre, "square on its axis")
    assert abs(float(w[0]) - 4 * np.arctan(a * a / (h * np.sqrt(2 * a * a + h * h))) / (4 * np.pi)) <= tol
    # every face twice: 2 w; every face reversed: -w, and the same inside with orientation="auto"
    v, f = W.box_quads((-0.5, -0.3, -0.4), (0.4, 0.5, 0.2), 2)
    pts = uniform_points(3000, 11, 1.0)
    w1, keep, tol = check_mesh(v, f, pts, "closed box")
    w2, _, _ = check_mesh(v, np.concatenate([f, f]), pts, "doubled box")
    assert float(np.abs(w2 - 2 * w1)[keep].max()) <= 2 * tol
    inside = np.all((pts > v.min(0)) & (pts < v.max(0)), axis=1)
    occ = mesh_occupancy(T(v), T(f), T(pts), method="winding")
    assert np.array_equal(occ.cpu().numpy()[keep], inside[keep].astype(np.float32))
    rev = np.ascontiguousarray(f[:, ::-1])
    assert float(np.abs(mesh_winding_number(T(v), T(rev), T(pts)).cpu().numpy() + w1)[keep].max()) <= 2 * tol
    assert torch.equal(mesh_occupancy(T(v), T(rev), T(pts), method="winding")[T(keep)], occ[T(keep)])
    assert float(mesh_occupancy(T(v), T(rev), T(pts), method="winding", orientation="ccw").sum()) == 0.0


def test_winding_keeps_the_inside_where_parity_loses_it(closed):
    """2 % of the triangles deleted: every +x ray through a hole flips its parity label, while the winding number moves by
    the holes' solid angle / 4 pi.  Truth: the closed mesh's occupancy; points farther than 0.05 from the surface."""
    from ishapediting_amd.mesh import mesh_occupancy
    v, f, p = closed["v"], closed["f"], T(closed["pts"])
    truth = mesh_occupancy(v, f, p)
    g = torch.Generator().manual_seed(2)
    nf = f.shape[0]
    kept_faces = torch.randperm(nf, generator=g)[: nf - max(1, round(0.02 * nf))].sort().values.to(dev())
    holed = f[kept_faces].contiguous()
    far = T(closed["d64"] > BAND)
    assert int(far.sum()) > 10000
    wrong_p = float((mesh_occupancy(v, holed, p) != truth)[far].float().mean())
    wrong_w = float((mesh_occupancy(v, holed, p, method="winding") != truth)[far].float().mean())
    print(f"{nf - holed.shape[0]} of {nf} triangles deleted, {int(far.sum())} points: parity wrong on {wrong_p:.4%}, "
          f"winding wrong on {wrong_w:.4%}")
    assert wrong_p > 0
    assert wrong_w < wrong_p / 4


# ---------------------------------------------------------------- oriented point clouds


@pytest.fixture(scope="module")
def sphere_cloud():
    p, n, a = W.fibonacci_sphere(4000, 0.7)
    q = uniform_points(3000, 21, 1.0)
    w64 = W.cloud_winding(p, n, a, q)
    tol = tolerance(W.cloud_winding(p, n, a, q, np.float32), w64)
    knn = W.knn_sq(p, 8)
    out = dict(p=p, n=n, a=a, q=q, w64=w64, tol=tol, knn=knn)
    return out


def signs_right(w, q, radius=0.7):
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    keep = np.abs(r - radius) > BAND
    assert keep.mean() >= 0.85
    return np.array_equal(w[keep] > 0.5, r[keep] < radius)


def check_areas(area, knn, k):
    """device areas against pi d_k^2 / k; where the k-th neighbour ties with the next or the previous one within 1e-6 (squared
    distance), either is accepted"""
    def close(d2):
        return np.abs(area - np.maximum(np.pi * d2 / k, W.AREA_FLOOR)) <= 1e-5 * np.maximum(np.pi * d2 / k, W.AREA_FLOOR)
    ok = close(knn[:, k - 1])
    ok |= (knn[:, k] - knn[:, k - 1] <= 1e-6) & close(knn[:, k])
    if k > 1:
        ok |= (knn[:, k - 1] - knn[:, k - 2] <= 1e-6) & close(knn[:, k - 2])
    assert ok.all(), (int((~ok).sum()), area[~ok][:4], (np.pi * knn[:, k - 1] / k)[~ok][:4])


def test_sphere_cloud(sphere_cloud):
    from ishapediting_amd.mesh import cloud_areas, cloud_winding_number
    c = sphere_cloud
    p, n, a, q = T(c["p"]), T(c["n"]), T(c["a"]), T(c["q"])
    w = cloud_winding_number(p, n, q, a)
    err = float(np.abs(w.cpu().numpy() - c["w64"]).max())
    print(f"sphere cloud 4000 x 3000: |w - fp64| max {err:.3e}, tolerance {c['tol']:.3e}")
    assert err <= c["tol"]
    assert signs_right(w.cpu().numpy(), c["q"])
    assert torch.equal(cloud_winding_number(p, n, q, a), w)
    est = cloud_areas(p, 8)
    check_areas(est.cpu().numpy().astype(np.float64), c["knn"], 8)
    total = float(est.double().sum()) / (4 * np.pi * 0.49)
    print(f"estimated area / sphere area: {total:.4f}")
    assert abs(total - 1) <= 0.10
    assert torch.equal(cloud_areas(p, 8), est)
    w_est = cloud_winding_number(p, n, q)
    assert torch.equal(w_est, cloud_winding_number(p, n, q, est))
    assert signs_right(w_est.cpu().numpy(), c["q"])


@pytest.mark.parametrize("k", [1, 4, 11, 16])
@pytest.mark.parametrize("npoints", [255, 256, 257, 1300])
def test_cloud_tiles_and_neighbour_counts(npoints, k):
    """point counts across the 256-sample LDS tile (1300 x 40 queries: the part sums), every template instance of the
    neighbour search, and a repeated point (a neighbour at distance 0: the area floor for k = 1)"""
    from ishapediting_amd.mesh import cloud_areas, cloud_winding_number
    p, n, a = W.fibonacci_sphere(npoints, 0.7)
    p = p.copy()
    p[npoints // 2] = p[3]
    q = uniform_points(40, npoints + k, 1.0)
    est = cloud_areas(T(p), k)
    check_areas(est.cpu().numpy().astype(np.float64), W.knn_sq(p, k), k)
    if k == 1:
        assert float(est[3]) == float(np.float32(W.AREA_FLOOR)) == float(est[npoints // 2])
    w64 = W.cloud_winding(p, n, a, q)
    tol = tolerance(W.cloud_winding(p, n, a, q, np.float32), w64)
    w = cloud_winding_number(T(p), T(n), T(q), T(a))
    assert float(np.abs(w.cpu().numpy() - w64).max()) <= tol
    assert torch.equal(cloud_winding_number(T(p), T(n), T(q), T(a)), w)
    perm = torch.randperm(40, generator=torch.Generator().manual_seed(3)).to(dev())
    assert torch.equal(cloud_winding_number(T(p), T(n), T(q)[perm].contiguous(), T(a)), w[perm])


# ---------------------------------------------------------------- the public route


def test_sample_occupancy_winding_equals_parity_on_a_closed_box():
    from ishapediting_amd.mesh import sample_occupancy
    v, f = W.box_quads((-0.6, -0.5, -0.4), (0.3, 0.5, 0.4), 1)
    out = [sample_occupancy((v, f), None, True, 20000, 0.5, device=dev(), generator=torch.Generator().manual_seed(5), **kw)
           for kw in ({}, {"occupancy": "parity"}, {"occupancy": "winding"})]
    for pts, occ in out[1:]:
        assert np.array_equal(pts, out[0][0]) and np.array_equal(occ, out[0][1])
    assert out[0][1].shape == (20000, 1) and 0.05 < out[0][1].mean() < 0.95


def test_sample_cloud_occupancy(sphere_cloud):
    from ishapediting_amd.mesh import sample_cloud_occupancy
    c = sphere_cloud
    pts, occ = sample_cloud_occupancy(c["p"], c["n"], 6000, 0.5, generator=torch.Generator().manual_seed(6), device=dev())
    assert pts.shape == (6000, 3) and occ.shape == (6000, 1) and pts.dtype == np.float32 and occ.dtype == np.float32
    assert set(np.unique(occ)) == {0.0, 1.0}
    uni = pts[:3000]
    assert np.abs(uni).max() <= 1.0 and signs_right(occ[:3000, 0], uni)
    near = np.linalg.norm(pts[3000:], axis=1)
    assert np.abs(near - 0.7).max() < 0.1                              # cloud points + N(0, 0.01)
    again = sample_cloud_occupancy(c["p"], c["n"], 6000, 0.5, generator=torch.Generator().manual_seed(6), device=dev())
    assert np.array_equal(again[0], pts) and np.array_equal(again[1], occ)


def test_sample_cloud_occupancy_keeps_given_areas_through_centring(sphere_cloud, monkeypatch):
    """a cloud three times too large and off centre: centring moves and rescales it by s, and the caller's areas are
    multiplied by s^2 -- no second neighbour search"""
    from ishapediting_amd import mesh as M
    c = sphere_cloud
    big = (3 * c["p"] + np.float32([4.0, 0.5, -0.25])).astype(np.float32)
    seen = {}
    winding = M.cloud_winding_number

    def spy(points, normals, query, areas=None):
        seen["points"], seen["areas"] = points, areas
        return winding(points, normals, query, areas)

    def no_search(*a, **k):
        raise AssertionError("cloud_areas called although areas were given")

    monkeypatch.setattr(M, "cloud_winding_number", spy)
    monkeypatch.setattr(M, "cloud_areas", no_search)
    pts, occ = M.sample_cloud_occupancy(big, c["n"], 4000, 0.5, areas=9 * c["a"], generator=torch.Generator().manual_seed(8),
                                        device=dev())
    radius = float(seen["points"].norm(dim=1).max())
    s = radius / float(np.linalg.norm(3 * c["p"].astype(np.float64), axis=1).max())
    assert 0.9 < radius <= 1.0 and s < 0.5
    want = 9 * c["a"].astype(np.float64) * s * s
    assert np.abs(seen["areas"].cpu().numpy() - want).max() <= 1e-4 * want.max()
    centre = seen["points"].double().mean(dim=0).cpu().numpy()
    r = np.linalg.norm(pts[:2000].astype(np.float64) - centre, axis=1)
    keep = np.abs(r - radius) > BAND
    assert np.array_equal(occ[:2000, 0][keep] > 0.5, r[keep] < radius)


def test_train_triplane_opt_from_a_cloud(tmp_path, sphere_cloud):
    from ishapediting_amd import synthetic
    from ishapediting_amd.drag_utils import DragStuff
    from tests.helpers import small96_args, small96_config
    c = sphere_cloud
    ds = DragStuff(dev(), args=small96_args(4, w_time=2, feat_layer=1))
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(small96_config(), 202))
    ds.load_weights(sd, synthetic.decoder_state_dict(), -np.full(96, 1.5, np.float32), np.full(96, 0.5, np.float32))
    rs = np.random.RandomState(4)
    means, stds = (0.05 * rs.randn(96)).astype(np.float32), (0.3 + 0.1 * rs.rand(96)).astype(np.float32)
    w_sentinel = torch.full((1, 96, 16, 16), 3.0, device=dev())
    mesh0_sentinel = object()
    ds.w, ds.mesh0 = w_sentinel, mesh0_sentinel
    np.savez(tmp_path / "pointcloud.npz", points=c["p"], normals=c["n"])
    lat = ds.train_triplane_opt(cloud=str(tmp_path / "pointcloud.npz"), path=str(tmp_path), stats=(means, stds), epochs=1,
                                batch_size=2000, seed=0)
    assert tuple(lat.shape) == (1, 96, 16, 16) and bool(torch.isfinite(lat).all())
    bce = ds.last_losses[:, 0].cpu()
    print(f"BCE over {len(bce)} steps: {float(bce[0]):.5f} -> {float(bce[-1]):.5f}")
    assert len(bce) == 10 and float(bce[-1]) < float(bce[0])
    assert ds.w is w_sentinel and bool((ds.w == 3.0).all()) and ds.mesh0 is mesh0_sentinel


def test_cloud_to_mesh_is_closed(sphere_cloud):
    from ishapediting_amd.mesh import cloud_to_mesh, mesh_signed_volume
    c = sphere_cloud
    res = 32
    v, t = cloud_to_mesh(T(c["p"]), T(c["n"]), res=res)
    assert t.shape[0] > 500 and v.dtype == torch.float32 and t.dtype == torch.int32
    tn = t.cpu().numpy().astype(np.int64)
    e = np.sort(np.concatenate([tn[:, [0, 1]], tn[:, [1, 2]], tn[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert (counts == 2).all()                                         # every edge in exactly two triangles
    radius = float(v.norm(dim=1).mean())
    print(f"cloud_to_mesh {res}^3: {v.shape[0]} vertices, mean radius {radius:.4f}")
    assert abs(radius - 0.7) <= 2 * (2 / (res - 1))
    assert mesh_signed_volume(v, t) > 0
