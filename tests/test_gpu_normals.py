"""Clouds without normals on the device (csrc/normals.hip: ishap_cloud_knn, ishap_cloud_normals, ishap_cloud_orient)
through the public functions of ishapediting_amd.mesh, against the numpy statement tests/normals_ref.py.

Tolerances.  Squared distances: 1e-5 relative, the bar the area test holds the same quantity to.  Normals and variation:
4 x the largest error the float32 numpy evaluation of the SAME statement shows on the same input (normals_ref, dtype=
np.float32) -- fp32 rounding as measured, never what the device gives; no floor under it was needed.  Left out: neighbour
ranks whose distance is within 1e-5 relative of the next or previous rank's (either index is right there), and points whose
eigen-gap (l1 - l0) / l2 is below 1e-3 (the eigenvector is ill-conditioned); tests/test_normals_host.py checks on the CPU
that each stays below 1 % on these inputs.  Orientation has no tolerance: signs, rounds and seeds equal the statement's."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import normals_ref as N

pytestmark = pytest.mark.gpu

BAND = 0.05


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


@functools.lru_cache(maxsize=None)
def uniform_case(n):
    """(points, the statement's 17 neighbours) -- one more than the largest k, so that the last rank has a next one"""
    p = N.uniform_cloud(n)
    return (p,) + N.knn(p, 17)


@functools.lru_cache(maxsize=None)
def orientation_cloud(name):
    return N.orientation_clouds()[name]


def device_normals(p, idx, variation=True):
    """ishap_cloud_normals on given neighbour lists (the public estimate_normals searches its own)"""
    from ishapediting_amd import _lib
    n = torch.empty_like(p)
    var = torch.empty(p.shape[0], dtype=torch.float32, device=p.device) if variation else None
    _lib.check(_lib.lib().ishap_cloud_normals(p.data_ptr(), p.shape[0], idx.data_ptr(), idx.shape[1], n.data_ptr(), _lib.ptr(var),
                                             _lib.stream_ptr(p.device)))
    return n, var


def check_unit_and_signed(n):
    n = n.astype(np.float64)
    assert np.isfinite(n).all()
    assert float(np.abs(np.linalg.norm(n, axis=1) - 1).max()) <= 1e-6
    lead = np.take_along_axis(n, np.argmax(np.abs(n), axis=1)[:, None], axis=1)
    assert (lead > 0).all()                                            # the sign rule, on the numbers the device wrote


# ---------------------------------------------------------------- 1. neighbours


@pytest.mark.parametrize("k", [1, 4, 8, 11, 16])
@pytest.mark.parametrize("n", [255, 256, 257, 1300])
def test_knn_tiles_and_k(n, k):
    """point counts across the 256-candidate LDS tile and more than one workgroup; every template instance (K = 4, 8, 16)
    both full and partly used"""
    from ishapediting_amd.mesh import cloud_knn
    p, ref_idx, ref_d2 = uniform_case(n)
    idx, d2 = cloud_knn(T(p), k)
    assert idx.shape == (n, k) and idx.dtype == torch.int32 and d2.shape == (n, k) and d2.dtype == torch.float32
    gi, gd = idx.cpu().numpy().astype(np.int64), d2.cpu().numpy().astype(np.float64)
    err = float((np.abs(gd - ref_d2[:, :k]) / ref_d2[:, :k]).max())
    sure = N.distinct_ranks(ref_d2, k)
    print(f"knn {n} x k={k}: d2 relative error max {err:.3e}; {int((~sure).sum())} of {sure.size} ranks within 1e-5 of a neighbour")
    assert err <= 1e-5
    assert 1 - sure.mean() <= 0.01
    assert np.array_equal(gi[sure], ref_idx[:, :k][sure])
    assert (gi != np.arange(n)[:, None]).all() and gi.min() >= 0 and gi.max() < n
    again = cloud_knn(T(p), k)
    assert torch.equal(again[0], idx) and torch.equal(again[1], d2)
    perm = np.random.default_rng(k).permutation(n)                     # point i of the shuffled cloud is point perm[i]
    pi, pd = cloud_knn(T(p[perm]), k)
    assert np.array_equal(pd.cpu().numpy(), d2.cpu().numpy()[perm])     # a distance does not depend on where its points stand
    back = perm[pi.cpu().numpy().astype(np.int64)]
    assert np.array_equal(back[sure[perm]], gi[perm][sure[perm]])


@pytest.mark.parametrize("k", [3, 8, 16])
def test_knn_ties_go_to_the_smaller_index(k):
    """repeated points and lattice points: many exactly equal distances, all exact in fp32 -- indices and distances EQUAL the
    statement's"""
    from ishapediting_amd.mesh import cloud_knn
    p = N.tie_cloud()
    ref_idx, ref_d2 = N.knn(p, k)
    ties = int((np.diff(ref_d2, axis=1) == 0).sum())
    assert ties > 30 * k and int((ref_d2[:, 0] == 0).sum()) == 80      # 40 repeats: both copies see the other at 0
    idx, d2 = cloud_knn(T(p), k)
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), ref_d2)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), ref_idx)


# ---------------------------------------------------------------- 2. normals


@pytest.mark.parametrize("k", [8, 16])
@pytest.mark.parametrize("name", ["sphere", "torus", "cube"])
def test_normals_against_the_statement(name, k):
    from ishapediting_amd.mesh import cloud_knn, estimate_normals
    p, outward = N.normal_clouds()[name]
    idx, _ = cloud_knn(T(p), k)
    hidx = idx.cpu().numpy()
    n64, var64, gap = N.pca_normals(p, hidx)
    n32, var32, _ = N.pca_normals(p, hidx, np.float32)
    keep = gap >= 1e-3
    assert 1 - keep.mean() <= 0.01
    tol = 4 * float(N.angle(n32, n64)[keep].max())
    vtol = 4 * float(np.abs(var32.astype(np.float64) - var64)[keep].max())
    n, var = device_normals(T(p), idx)
    gn, gv = n.cpu().numpy(), var.cpu().numpy().astype(np.float64)
    err, verr = float(N.angle(gn, n64)[keep].max()), float(np.abs(gv - var64)[keep].max())
    to_surface = float(np.degrees(N.angle(gn, outward)).mean())
    print(f"normals {name} k={k}: angle to the statement max {err:.3e} rad (tolerance {tol:.3e}), variation error max {verr:.3e} "
          f"(tolerance {vtol:.3e}), {int((~keep).sum())} points left out, mean angle to the analytic normal {to_surface:.2f} deg")
    assert err <= tol and verr <= vtol
    check_unit_and_signed(gn)
    assert (gv >= 0).all() and (gv <= 1 / 3 + 1e-6).all()
    again = device_normals(T(p), idx)
    assert torch.equal(again[0], n) and torch.equal(again[1], var)
    pub, info = estimate_normals(T(p), k, orient=False, return_info=True)       # the public call: its own search, same result
    assert torch.equal(pub, n) and torch.equal(info["variation"], var) and info["rounds"] is None and info["seeds"] is None
    assert torch.equal(device_normals(T(p), idx, variation=False)[0], n)         # variation is optional


def test_degenerate_neighbourhoods_give_unit_vectors():
    from ishapediting_amd.mesh import estimate_normals
    same = np.tile(np.float32([[0.3, -0.2, 0.7]]), (50, 1))
    t = np.linspace(-1, 1, 300)[:, None]
    line = (t * np.float64([[0.3, 0.5, -0.4]]) + 0.1).astype(np.float32)
    plane = N.uniform_cloud(500)
    plane[:, 1] = 0.25
    for cloud, k in ((same, 8), (same, 16), (line, 4), (line, 12), (plane, 10)):
        n, info = estimate_normals(T(cloud), k, orient=False, return_info=True)
        check_unit_and_signed(n.cpu().numpy())
        assert bool(torch.isfinite(info["variation"]).all()) and float(info["variation"].max()) <= 1e-6
    assert np.array_equal(n.cpu().numpy(), np.tile(np.float32([[0, 1, 0]]), (500, 1)))     # the plane y = 0.25, exactly
    n = estimate_normals(T(line), 12).cpu().numpy()                    # and orientation ends on them
    check_len = np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1).max()
    assert np.isfinite(n).all() and check_len <= 1e-6


# ---------------------------------------------------------------- 3. orientation


@pytest.mark.parametrize("k", [8, 12, 16])
@pytest.mark.parametrize("name", ["sphere", "torus", "noisy_torus", "two_spheres"])
def test_orientation(name, k):
    """The binding has no chunk parameter: rounds are enqueued 16 at a time, and every case here needs 20 to 40 rounds plus a
    seed round per component, so each crosses a chunk boundary once or twice."""
    from ishapediting_amd.mesh import cloud_knn, estimate_normals
    p, outward, seeds = orientation_cloud(name)
    tp = T(p)
    idx, _ = cloud_knn(tp, k)
    n0 = estimate_normals(tp, k, orient=False)
    n1, info = estimate_normals(tp, k, return_info=True)
    h0, h1 = n0.cpu().numpy(), n1.cpu().numpy()
    same, flipped = (h1 == h0).all(axis=1), (h1 == -h0).all(axis=1)
    assert (same | flipped).all() and not (same & flipped).any()       # each normal as it was, or negated, bit for bit
    dots = (h1.astype(np.float64) * outward).sum(axis=1)
    signs, rounds, got_seeds = N.orient(p, h0, idx.cpu().numpy())
    print(f"orientation {name} k={k}: {info['rounds']} rounds, {info['seeds']} seeds, {int((dots <= 0).sum())} normals against the "
          f"analytic one, smallest |cos| {np.abs(dots).min():.3f}, {int(flipped.sum())} flipped")
    assert int((dots <= 0).sum()) == 0
    assert np.array_equal(np.where(flipped, -1, 1), signs)
    assert (info["rounds"], info["seeds"]) == (rounds, got_seeds) and got_seeds == seeds
    again, info2 = estimate_normals(tp, k, return_info=True)
    assert torch.equal(again, n1) and (info2["rounds"], info2["seeds"]) == (rounds, got_seeds)


def test_orient_normals_takes_any_length_and_sign():
    from ishapediting_amd.mesh import orient_normals
    p, outward, _ = orientation_cloud("sphere")
    rng = np.random.default_rng(5)
    given = (outward * rng.uniform(0.1, 7.0, (len(p), 1)) * rng.choice([-1.0, 1.0], (len(p), 1))).astype(np.float32)
    n, info = orient_normals(T(p), T(given), 12, return_info=True)
    hn = n.cpu().numpy().astype(np.float64)
    assert float(np.abs(np.linalg.norm(hn, axis=1) - 1).max()) <= 1e-6
    assert ((hn * outward).sum(axis=1) > 0.999).all() and info["seeds"] == 1 and 10 <= info["rounds"] <= 60
    assert torch.equal(orient_normals(T(p), T(given)), n)


def test_bad_indices_and_small_scratch_fail_safely():
    """an index outside the cloud is read as the point itself (normals) or passed over (orientation); a scratch buffer one
    byte short fails the call before any launch"""
    from ishapediting_amd import _lib
    from ishapediting_amd.mesh import cloud_knn
    p, _, _ = orientation_cloud("sphere")
    tp = T(p)
    idx, _ = cloud_knn(tp, 8)
    bad = idx.clone()
    bad[::7, 3] = -5
    bad[::11, 6] = len(p)
    n, var = device_normals(tp, bad)
    check_unit_and_signed(n.cpu().numpy())
    L = _lib.lib()
    need = int(L.ishap_cloud_orient_scratch_bytes(len(p)))
    scratch = torch.empty(need, dtype=torch.uint8, device=dev())
    info = (C.c_int * 2)()
    before = n.clone()
    rc = L.ishap_cloud_orient(tp.data_ptr(), n.data_ptr(), bad.data_ptr(), len(p), 8, scratch.data_ptr(), need - 1, info,
                              _lib.stream_ptr(dev()))
    assert rc != 0 and b"scratch smaller" in L.ishap_last_error() and torch.equal(n, before)
    _lib.check(L.ishap_cloud_orient(tp.data_ptr(), n.data_ptr(), bad.data_ptr(), len(p), 8, scratch.data_ptr(), need, info,
                                    _lib.stream_ptr(dev())))
    signs, rounds, seeds = N.orient(p, before.cpu().numpy(), np.where((bad.cpu().numpy() < 0) | (bad.cpu().numpy() >= len(p)),
                                                                      np.arange(len(p))[:, None], bad.cpu().numpy()))
    assert (info[0], info[1]) == (rounds, seeds)                       # a point is never its own parent: it has no level yet
    assert np.array_equal(n.cpu().numpy(), before.cpu().numpy() * signs[:, None].astype(np.float32))


# ---------------------------------------------------------------- 4. the public route


def signs_right(w, q, radius=0.7):
    r = np.linalg.norm(q.astype(np.float64), axis=1)
    keep = np.abs(r - radius) > BAND
    assert keep.mean() >= 0.85
    return np.array_equal(w[keep] > 0.5, r[keep] < radius)


@pytest.fixture(scope="module")
def bare_sphere():
    p, outward, _ = N.fibonacci_sphere(4000, 0.7)
    q = (np.random.default_rng(21).uniform(-1, 1, (3000, 3))).astype(np.float32)
    return dict(p=p, n=outward, q=q)


def test_estimated_normals_give_the_winding_number_its_signs(bare_sphere):
    from ishapediting_amd.mesh import cloud_winding_number, estimate_normals
    c = bare_sphere
    n, info = estimate_normals(T(c["p"]), return_info=True)
    cos = (n.cpu().numpy().astype(np.float64) * c["n"]).sum(axis=1)
    print(f"sphere 4000, k=12: {info['rounds']} rounds, {info['seeds']} seeds, smallest cos to the radius {cos.min():.6f}")
    assert cos.min() > 0.999 and info["seeds"] == 1
    w = cloud_winding_number(T(c["p"]), n, T(c["q"]))
    assert signs_right(w.cpu().numpy(), c["q"])


def test_sample_cloud_occupancy_without_normals(bare_sphere):
    from ishapediting_amd.mesh import sample_cloud_occupancy
    c = bare_sphere
    gen = lambda: torch.Generator().manual_seed(6)                      # noqa: E731
    pts, occ = sample_cloud_occupancy(c["p"], None, 6000, 0.5, generator=gen(), device=dev())
    ref_pts, ref_occ = sample_cloud_occupancy(c["p"], c["n"], 6000, 0.5, generator=gen(), device=dev())
    assert pts.shape == (6000, 3) and occ.shape == (6000, 1) and np.array_equal(pts, ref_pts)
    keep = np.abs(np.linalg.norm(pts.astype(np.float64), axis=1) - 0.7) > BAND
    assert keep[:3000].mean() >= 0.85 and np.array_equal(occ[keep], ref_occ[keep])
    assert signs_right(occ[:3000, 0], pts[:3000])
    kw = sample_cloud_occupancy(points=c["p"], points_size=6000, uniform_ratio=0.5, generator=gen(), device=dev(), normals_k=12)
    assert np.array_equal(kw[0], pts) and np.array_equal(kw[1], occ)
    big = (3 * c["p"] + np.float32([4.0, 0.5, -0.25])).astype(np.float32)          # centred and rescaled before the estimate
    bp, bo = sample_cloud_occupancy(big, None, 4000, 0.5, generator=gen(), device=dev(), normals_k=8)
    assert 0.05 < bo.mean() < 0.95 and set(np.unique(bo)) == {0.0, 1.0}


def test_cloud_to_mesh_without_normals_is_closed(bare_sphere):
    from ishapediting_amd.mesh import cloud_to_mesh, mesh_signed_volume
    res = 32
    v, t = cloud_to_mesh(T(bare_sphere["p"]), res=res)
    assert t.shape[0] > 500 and v.dtype == torch.float32 and t.dtype == torch.int32
    tn = t.cpu().numpy().astype(np.int64)
    e = np.sort(np.concatenate([tn[:, [0, 1]], tn[:, [1, 2]], tn[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    assert (counts == 2).all()                                         # every edge in exactly two triangles
    radius = float(v.norm(dim=1).mean())
    print(f"cloud_to_mesh {res}^3 without normals: {v.shape[0]} vertices, mean radius {radius:.4f}")
    assert abs(radius - 0.7) <= 2 * (2 / (res - 1))
    assert mesh_signed_volume(v, t) > 0


def test_train_triplane_opt_from_bare_points(tmp_path, bare_sphere):
    from ishapediting_amd import synthetic
    from ishapediting_amd.drag_utils import DragStuff
    from tests.helpers import small96_args, small96_config
    ds = DragStuff(dev(), args=small96_args(4, w_time=2, feat_layer=1))
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(small96_config(), 202))
    ds.load_weights(sd, synthetic.decoder_state_dict(), -np.full(96, 1.5, np.float32), np.full(96, 0.5, np.float32))
    rs = np.random.RandomState(4)
    means, stds = (0.05 * rs.randn(96)).astype(np.float32), (0.3 + 0.1 * rs.rand(96)).astype(np.float32)
    w_sentinel = torch.full((1, 96, 16, 16), 3.0, device=dev())
    mesh0_sentinel = object()
    ds.w, ds.mesh0 = w_sentinel, mesh0_sentinel
    lat = ds.train_triplane_opt(cloud=bare_sphere["p"], path=str(tmp_path), stats=(means, stds), epochs=1, batch_size=2000, seed=0)
    assert tuple(lat.shape) == (1, 96, 16, 16) and bool(torch.isfinite(lat).all())
    bce = ds.last_losses[:, 0].cpu()
    print(f"BCE over {len(bce)} steps: {float(bce[0]):.5f} -> {float(bce[-1]):.5f}")
    assert len(bce) == 10 and float(bce[-1]) < float(bce[0])
    assert ds.w is w_sentinel and bool((ds.w == 3.0).all()) and ds.mesh0 is mesh0_sentinel
