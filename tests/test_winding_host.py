"""CPU checks of the generalized winding number (csrc/winding.hip): the numpy statement the GPU tests pin to against
closed forms, argument rejection before any device work, the C ABI and the new kernels' code-object metadata (no GPU)."""
import os

import numpy as np
import pytest

from tests import winding_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_statement_is_an_integer_around_a_closed_box():
    v, f = W.box_quads((-0.5, -0.3, -0.4), (0.4, 0.5, 0.2), 2)
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1.2, 1.2, (2000, 3)).astype(np.float32)
    w = W.mesh_winding(v, f, pts)
    assert float(np.abs(w - np.round(w)).max()) <= 1e-12
    inside = np.all((pts > v.min(0)) & (pts < v.max(0)), axis=1)
    assert inside.sum() > 50 and (~inside).sum() > 50
    np.testing.assert_array_equal(np.round(w), inside.astype(np.float64))      # +1 inside a counter-clockwise mesh


def test_statement_cube_without_a_face_is_five_sixths_at_the_centre():
    v, f = W.box_quads((-0.5,) * 3, (0.5,) * 3, 3, skip=(5,))
    assert abs(W.mesh_winding(v, f, np.zeros((1, 3), np.float32))[0] - 5 / 6) <= 1e-12


def test_statement_square_on_its_axis():
    a, h = 0.5, 0.3
    v = np.array([[-a, -a, h], [a, -a, h], [a, a, h], [-a, a, h]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)                    # counter-clockwise seen from +z: the origin is behind it
    exact = 4 * np.arctan(a * a / (np.float64(np.float32(h)) * np.sqrt(2 * a * a + np.float64(np.float32(h)) ** 2)))
    assert abs(exact - 3.3044021677) < 2e-7                           # h = 0.3 rounded to fp32
    w = W.mesh_winding(v, f, np.zeros((1, 3), np.float32))[0]
    assert abs(w - exact / (4 * np.pi)) <= 1e-12


def test_statement_reversed_triangles_negate_and_flat_triangles_vanish():
    v, f = W.box_quads((-0.5, -0.3, -0.4), (0.4, 0.5, 0.2), 2, skip=(1,))
    pts = np.random.default_rng(1).uniform(-1, 1, (300, 3)).astype(np.float32)
    w = W.mesh_winding(v, f, pts)
    np.testing.assert_allclose(W.mesh_winding(v, f[:, ::-1], pts), -w, rtol=0, atol=1e-13)
    flat = np.array([[0, 0, 1], [0, 1, 1], [0, 1, 2]], np.int32)      # repeated corners
    np.testing.assert_array_equal(W.mesh_winding(v, np.concatenate([f, flat]), pts), w)


def test_statement_cloud_areas_on_a_lattice():
    s = 0.125
    g = np.arange(9) * s
    p = np.stack(np.meshgrid(g, g, [0.0], indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    a = W.cloud_areas(p, 4).reshape(9, 9)
    np.testing.assert_allclose(a[1:-1, 1:-1], np.pi * s * s / 4, rtol=1e-12)
    assert a[0, 0] > a[1, 1]                                          # a corner has two neighbours at s only
    dup = np.concatenate([p, p[:1]])                                  # an equal point is a neighbour at distance 0
    assert W.knn_sq(dup, 4)[0, 0] == 0.0 and W.cloud_areas(dup, 1)[0] == W.AREA_FLOOR


def test_statement_cloud_winding_of_a_sphere():
    p, n, a = W.fibonacci_sphere(4000, 0.7)
    q = np.random.default_rng(2).uniform(-1, 1, (500, 3)).astype(np.float32)
    r = np.linalg.norm(q, axis=1)
    keep = np.abs(r - 0.7) > 0.05
    w = W.cloud_winding(p, n, a, q)
    np.testing.assert_array_equal(w[keep] > 0.5, r[keep] < 0.7)
    assert float(np.abs(W.cloud_winding(p, n, a, q, np.float32) - w).max()) < 1e-4


def test_fp32_yardstick_is_close_to_the_statement():
    v, f = W.box_quads((-0.5, -0.3, -0.4), (0.4, 0.5, 0.2), 6)
    pts = np.random.default_rng(3).uniform(-1.2, 1.2, (500, 3)).astype(np.float32)
    w32 = W.mesh_winding(v, f, pts, np.float32)
    assert w32.dtype == np.float32
    assert 0 < float(np.abs(w32 - W.mesh_winding(v, f, pts)).max()) < 1e-4


def _no_device(monkeypatch):
    from ishapediting_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", refuse)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_unknown_choices_are_rejected_before_the_library(monkeypatch):
    import torch
    from ishapediting_amd import mesh, metrics
    from ishapediting_amd.drag_utils import DragStuff
    _no_device(monkeypatch)
    never = object()
    z = torch.zeros((3, 3))
    zi = torch.zeros((1, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match="method"):
        mesh.mesh_occupancy(z, zi, z, method="rays")
    with pytest.raises(ValueError, match="orientation"):
        mesh.mesh_occupancy(z, zi, z, method="winding", orientation="inside-out")
    with pytest.raises(ValueError, match="occupancy"):
        mesh.sample_occupancy((z, zi), None, True, 10, 0.5, occupancy="Winding")
    with pytest.raises(ValueError, match="k must be"):
        mesh.cloud_areas(z, k=17)
    with pytest.raises(ValueError, match="sign"):
        metrics.calc_implicit_field(never, z, sign="wind")
    with pytest.raises(ValueError, match="sign"):
        metrics.calc_iou(never, never, 100, sign="")
    with pytest.raises(ValueError, match="sign"):
        metrics.calc_local_distance(never, never, z, z, 0.1, 10, sign="generalized")
    ds = DragStuff.__new__(DragStuff)                                 # no model: the check comes first
    with pytest.raises(ValueError, match="occupancy"):
        ds.train_triplane(mesh=never, occupancy="rays")
    with pytest.raises(ValueError, match="occupancy"):
        ds.train_triplane_opt(mesh=never, occupancy="rays")


def test_third_party_route_does_not_label_winding_by_parity(monkeypatch):
    """Open3D's compute_occupancy is ray parity: asking that route for winding labels is an error, not parity labels"""
    from ishapediting_amd import mesh
    _no_device(monkeypatch)
    monkeypatch.setattr(mesh, "BACKEND", "third_party")
    with pytest.raises(ValueError, match="device route"):
        mesh.sample_occupancy(object(), None, True, 10, 0.5, occupancy="winding")
    with pytest.raises(ValueError, match="device route"):
        mesh.sample_occupancy(None, "shape.obj", True, 10, 0.5, occupancy="winding")


def test_load_cloud_forms(tmp_path):
    from ishapediting_amd.mesh import load_cloud
    p, n, _ = W.fibonacci_sphere(10, 1.0)
    np.savez(tmp_path / "pointcloud.npz", points=p.astype(np.float64), normals=n)
    for got in (load_cloud(str(tmp_path / "pointcloud.npz")), load_cloud((p, n))):
        assert got[0].dtype == np.float32 and np.array_equal(got[0], p) and np.array_equal(got[1], n)
    with pytest.raises(ValueError, match="normals"):
        load_cloud((p, n[:5]))


def test_winding_abi():
    from ishapediting_amd import _lib
    L = _lib.lib()
    assert L.ishap_version() >= 12
    # size functions
    assert L.ishap_winding_scratch_bytes(-1, 5) == -1 and L.ishap_winding_scratch_bytes(5, -1) == -1
    assert L.ishap_mesh_distance_scratch_bytes_sdf(-1, 5, 2) == -1 and L.ishap_mesh_distance_scratch_bytes_sdf(5, -1, 2) == -1
    for sdf in (0, 1, -1, 3):                                         # every value but +-2 is unsigned or parity: the boxes alone
        assert L.ishap_mesh_distance_scratch_bytes_sdf(257, 1000, sdf) == L.ishap_mesh_distance_scratch_bytes(257)
    one = L.ishap_winding_scratch_bytes(256, 5)                       # one tile: no part sums
    four = L.ishap_winding_scratch_bytes(1000, 5)                     # four tiles, few queries: one part per tile
    assert 0 < one < four and four >= 4 * 5 * 4 and four % 256 == 0
    assert L.ishap_winding_scratch_bytes(1000, 5) == four            # a function of the two counts alone
    assert L.ishap_mesh_distance_scratch_bytes_sdf(1000, 5, 2) >= L.ishap_mesh_distance_scratch_bytes(1000) + four
    # argument checks fail before any launch, and say which call
    assert L.ishap_mesh_winding(None, None, 0, None, 0, None, None, 0, None) != 0
    assert b"mesh_winding" in L.ishap_last_error()
    assert L.ishap_cloud_winding(None, None, None, 0, None, 0, None, None, 0, None) != 0
    assert b"cloud_winding" in L.ishap_last_error()
    assert L.ishap_cloud_areas(None, 0, 8, None, None) != 0
    assert b"cloud_areas" in L.ishap_last_error()


def test_winding_kernels_use_no_scratch():
    """The kernels the winding number adds, by name, in the built library's code-object metadata: private segment 0 bytes
    (cloud_areas_kernel is a template: every instance)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for want, count in [("winding_mesh_kernel", 1), ("winding_cloud_kernel", 1), ("cloud_areas_kernel", 3),
                        ("winding_reduce_kernel", 1)]:
        found = [n for n in ks if want in n]
        assert len(found) == count, (want, found)
        for n in found:
            assert ks[n].get(".private_segment_fixed_size", 0) == 0, (want, ks[n])
