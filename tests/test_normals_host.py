"""CPU checks of the front end for clouds without normals (csrc/normals.hip): the C ABI and the kernels' code-object
metadata, argument rejection before any device work, load_cloud's input forms, and the numpy statement the GPU tests pin to
(tests/normals_ref.py) against analytic normals (no GPU)."""
import os

import numpy as np
import pytest

from tests import normals_ref as N
from tests import winding_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000                                                          # a non-null address nothing dereferences


def test_normals_abi():
    import re
    from ishapediting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ishap.h")).read()
    for name in ("ishap_cloud_knn", "ishap_cloud_normals", "ishap_cloud_orient", "ishap_cloud_orient_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS
    L = _lib.lib()
    assert L.ishap_version() >= 14
    assert L.ishap_cloud_orient_scratch_bytes(-1) == -1 and L.ishap_cloud_orient_scratch_bytes(-(1 << 40)) == -1
    sizes = [L.ishap_cloud_orient_scratch_bytes(n) for n in (0, 1, 64, 65, 100_000)]
    assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes)
    for n, s in zip((0, 1, 64, 65, 100_000), sizes):
        assert s >= 4 * n + 16, (n, s)                                 # a level per point and the four counters
    assert L.ishap_cloud_orient_scratch_bytes(65) == sizes[3]          # a function of the count alone
    # argument checks fail before any launch, and say which call
    info = (__import__("ctypes").c_int * 2)()
    assert L.ishap_cloud_knn(None, 0, 8, None, None, None) != 0 and b"cloud_knn" in L.ishap_last_error()
    for k, n in ((0, 100), (17, 100), (8, 8)):
        assert L.ishap_cloud_knn(FAKE, n, k, FAKE, FAKE, None) != 0 and b"cloud_knn" in L.ishap_last_error()
        assert L.ishap_cloud_normals(FAKE, n, FAKE, k, FAKE, None, None) != 0 and b"cloud_normals" in L.ishap_last_error()
        assert L.ishap_cloud_orient(FAKE, FAKE, FAKE, n, k, FAKE, 1 << 20, info, None) != 0
        assert b"cloud_orient" in L.ishap_last_error()
    assert L.ishap_cloud_normals(None, 100, None, 8, None, None, None) != 0 and b"cloud_normals" in L.ishap_last_error()
    assert L.ishap_cloud_orient(None, None, None, 100, 8, None, 0, None, None) != 0 and b"cloud_orient" in L.ishap_last_error()
    need = L.ishap_cloud_orient_scratch_bytes(100)
    assert L.ishap_cloud_orient(FAKE, FAKE, FAKE, 100, 8, FAKE, need - 1, info, None) != 0
    assert b"scratch smaller" in L.ishap_last_error()


def test_normals_kernels_use_no_scratch():
    """The kernels this front end adds, by name, in the built library's code-object metadata: private segment 0 bytes
    (cloud_knn_kernel is a template: every instance)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for want, count in [("cloud_knn_kernel", 3), ("cloud_normals_kernel", 1), ("orient_round_kernel", 1),
                        ("orient_seed_kernel", 1), ("orient_init_kernel", 1)]:
        found = [n for n in ks if want in n]
        assert len(found) == count, (want, found)
        for n in found:
            assert ks[n].get(".private_segment_fixed_size", 0) == 0, (want, ks[n])


def _no_device(monkeypatch):
    from ishapediting_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", refuse)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_bad_arguments_are_rejected_before_the_library(monkeypatch):
    import torch
    from ishapediting_amd import mesh
    _no_device(monkeypatch)
    p = torch.zeros((20, 3))
    unit = torch.tensor([[0.0, 0.0, 1.0]]).repeat(20, 1)
    for fn in (mesh.cloud_knn, mesh.estimate_normals, lambda pts, k: mesh.orient_normals(pts, unit[:len(pts)], k)):
        for k in (0, 17, -3):
            with pytest.raises(ValueError, match="k must be"):
                fn(p, k)
        with pytest.raises(ValueError, match="more than 16 points"):
            fn(p[:16], 16)
        with pytest.raises(ValueError, match=r"\[N,3\]"):
            fn(torch.zeros((20, 2)), 8)
        with pytest.raises(ValueError, match=r"\[N,3\]"):
            fn(torch.zeros(60), 8)
        with pytest.raises(ValueError, match=r"\[N,3\]"):
            fn(np.zeros((20, 3), np.float32), 8)
    with pytest.raises(ValueError, match="20 points but normals"):
        mesh.orient_normals(p, unit[:19], 8)
    with pytest.raises(ValueError, match="20 points but normals"):
        mesh.orient_normals(p, None, 8)
    zero = unit.clone()
    zero[7] = 0
    with pytest.raises(ValueError, match="1 normals are zero"):
        mesh.orient_normals(p, zero, 8)
    zero[3, 1] = float("nan")
    with pytest.raises(ValueError, match="2 normals are zero"):
        mesh.orient_normals(p, zero, 8)
    with pytest.raises(ValueError, match="normals_k"):
        mesh.sample_cloud_occupancy(p, None, 100, 0.5, normals_k=17)
    with pytest.raises(ValueError, match="points_size"):
        mesh.sample_cloud_occupancy(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # good arguments get as far as the device check
        mesh.estimate_normals(p, 8)


def test_load_cloud_with_and_without_normals(tmp_path):
    import torch
    from ishapediting_amd.mesh import load_cloud
    p, n, _ = W.fibonacci_sphere(10, 1.0)
    np.savez(tmp_path / "bare.npz", points=p.astype(np.float64))
    np.savez(tmp_path / "pointcloud.npz", points=p.astype(np.float64), normals=n)
    for cloud in (p, p.astype(np.float64), torch.from_numpy(p), (p, None), [torch.from_numpy(p), None], str(tmp_path / "bare.npz"),
                  tmp_path / "bare.npz"):
        pts, nrm = load_cloud(cloud)
        assert nrm is None and pts.dtype == np.float32 and pts.shape == (10, 3) and np.array_equal(pts, p)
    # the oriented forms give what they gave before
    for cloud in (str(tmp_path / "pointcloud.npz"), (p, n), [p, n], (torch.from_numpy(p), torch.from_numpy(n)), np.stack([p, n])):
        pts, nrm = load_cloud(cloud)
        assert pts.dtype == np.float32 and nrm.dtype == np.float32 and np.array_equal(pts, p) and np.array_equal(nrm, n)
    pts, nrm = load_cloud(np.stack([p[0], n[0]]))                      # [2,3]: one point and its normal, as before
    assert np.array_equal(pts, p[:1]) and np.array_equal(nrm, n[:1])
    with pytest.raises(ValueError, match="normals"):
        load_cloud((p, n[:5]))


def test_statement_knn_order_and_ties():
    g = np.arange(4.0)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    p = np.concatenate([p, p[:3]])                                     # three repeated points
    idx, d2 = N.knn(p, 7)
    assert (np.diff(d2, axis=1) >= 0).all() and (idx != np.arange(len(p))[:, None]).all()
    assert idx[0, 0] == 64 and d2[0, 0] == 0 and idx[64, 0] == 0       # an equal point is the nearest neighbour
    tie = np.diff(d2, axis=1) == 0
    assert tie.sum() > 100 and (np.diff(idx, axis=1)[tie] > 0).all()   # equal distances: the smaller index first
    brute = np.sort(((p[:, None] - p[None]) ** 2).sum(-1) + np.diag(np.full(len(p), np.inf)), axis=1)[:, :7]
    np.testing.assert_array_equal(d2, brute)


def test_statement_normals_on_a_plane_and_sign_rule():
    rng = np.random.default_rng(0)
    e = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    uv = rng.uniform(-1, 1, (400, 2))
    p = uv @ e[:2]                                                     # fp64 points on the plane across e[2]
    idx, _ = N.knn(p, 10)
    n, var, gap = N.pca_normals(p, idx)
    assert float(N.angle(n, np.tile(e[2], (400, 1))).max()) < 1e-7 and float(var.max()) < 1e-14 and float(gap.min()) > 0.01
    lead = np.take_along_axis(n, np.argmax(np.abs(n), axis=1)[:, None], axis=1)
    assert (lead > 0).all()
    np.testing.assert_array_equal(N.signed_by_convention(np.array([[0.5, -0.5, 0.1], [-0.5, 0.5, 0.1], [0.1, -0.2, 0.2]])),
                                  [[0.5, -0.5, 0.1], [0.5, -0.5, -0.1], [-0.1, 0.2, -0.2]])
    n32 = N.pca_normals(p.astype(np.float32), idx, np.float32)[0]
    assert n32.dtype == np.float32 and float(N.angle(n32, n).max()) < 1e-5


@pytest.mark.parametrize("name", ["sphere", "torus", "noisy_torus", "two_spheres"])
def test_statement_orients_outward(name):
    """the round rule alone, in fp64, on the clouds the GPU test orients: no normal ends up against the analytic outward
    normal, and a seed per component"""
    p, outward, seeds = N.orientation_clouds()[name]
    idx, _ = N.knn(p, 12)
    n, _, gap = N.pca_normals(p, idx)
    signs, rounds, got_seeds = N.orient(p, n, idx)
    dots = ((n * signs[:, None]) * outward).sum(axis=1)
    print(f"{name}: {rounds} rounds, {got_seeds} seeds, smallest cos to the analytic normal {dots.min():.3f}")
    assert int((dots <= 0).sum()) == 0 and got_seeds == seeds and 10 <= rounds <= 60
    assert set(np.unique(signs)) <= {-1, 1}
    top = int(np.argmax(p[:, 2]))
    assert (n[top] * signs[top])[2] >= 0                                # the first seed: the topmost point, turned upward


def test_the_gpu_tests_inputs_stay_within_their_exclusion_limits():
    """what tests/test_gpu_normals.py leaves out of a comparison, counted on the CPU: ranks whose distance is within 1e-5
    (relative) of a neighbouring rank's, and points whose eigen-gap is below 1e-3 -- each at most 1 %"""
    for n in (255, 256, 257, 1300):
        _, d2 = N.knn(N.uniform_cloud(n), 17)
        for k in (1, 4, 8, 11, 16):
            assert 1 - N.distinct_ranks(d2, k).mean() <= 0.01, (n, k)
    for name, (p, _) in N.normal_clouds().items():
        for k in (8, 16):
            gap = N.pca_normals(p, N.knn(p, k)[0])[2]
            assert (gap < 1e-3).mean() <= 0.01, (name, k)
