"""CPU checks of the device mesh metrics (meshProcess.py:7-118 on the GPU): the fp64 statement the GPU tests pin to, argument
rejection before any device work, the C ABI and the new kernels' code-object metadata (no GPU needed)."""
import os

import numpy as np
import pytest

from tests import mesh_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_statement_gives_the_exact_box_sdf():
    lo, hi = (-0.5, -0.3, -0.4), (0.4, 0.5, 0.2)
    v, f = R.box_mesh(lo, hi)
    rng = np.random.default_rng(0)
    pts = np.concatenate([rng.uniform(-1.2, 1.2, (1000, 3)), rng.uniform(lo, hi, (500, 3))]).astype(np.float32)
    exact = R.box_sdf(pts, v.min(axis=0), v.max(axis=0))               # the fp32 corners are the box
    assert (exact < 0).sum() > 100 and (exact > 0).sum() > 100          # inside and outside both covered
    np.testing.assert_allclose(R.signed_distance(v, f, pts), exact, rtol=0, atol=1e-12)
    d, idx, second = R.mesh_distance(v, f, pts)
    assert idx.min() >= 0 and idx.max() < 12 and np.all(second >= d)


def test_statement_closest_point_regions():
    """one triangle, a point in each Voronoi region: vertex, edge and face distances by hand"""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f = np.array([[0, 1, 2]], np.int32)
    pts = np.array([[-1, -1, 0], [0.5, -1, 2], [0.25, 0.25, -3], [1, 1, 0], [2, 0, 0]], np.float32)
    want = [np.sqrt(2), np.sqrt(5), 3, np.sqrt(0.5), 1]
    np.testing.assert_allclose(R.mesh_distance(v, f, pts)[0], want, rtol=0, atol=1e-12)


def _no_device(monkeypatch):
    from ishapediting_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", refuse)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_local_distance_rejects_mismatched_handles_before_device_work(monkeypatch):
    from ishapediting_amd.metrics import calc_local_distance
    _no_device(monkeypatch)
    never = object()                     # not a mesh: any attempt to read it would raise something else
    with pytest.raises(ArithmeticError, match="same shape"):
        calc_local_distance(never, never, np.zeros((2, 3), np.float32), np.zeros((3, 3), np.float32), 0.1, 100)
    with pytest.raises(ArithmeticError):
        calc_local_distance(never, never, np.zeros((1, 3)), np.zeros(3), 0.1, 100, metric="L2")


def test_local_distance_rejects_an_unknown_metric(monkeypatch):
    from ishapediting_amd.metrics import calc_local_distance
    _no_device(monkeypatch)
    never = object()
    h = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError, match="metric"):
        calc_local_distance(never, never, h, h, 0.1, 100, metric="iou")
    assert calc_local_distance(never, never, h, h, 0.1, 100, metric="CD") == 0.0     # the reference's `pass`


def test_mesh_distance_abi():
    from ishapediting_amd import _lib
    L = _lib.lib()
    assert L.ishap_version() >= 7
    assert L.ishap_mesh_distance_scratch_bytes(1) == 32
    assert L.ishap_mesh_distance_scratch_bytes(257) == 64
    assert L.ishap_mesh_distance_scratch_bytes(-1) == -1
    # argument checks fail before any launch
    assert L.ishap_mesh_distance(None, None, 0, None, 0, 1, None, None, None, 0, None) != 0
    assert b"mesh_distance" in L.ishap_last_error()
    assert L.ishap_hausdorff(None, 0, None, 0, None, None, None) != 0
    assert L.ishap_group_field_stats(None, None, 0, 0, 0, None, None) != 0


def test_mesh_metric_kernels_use_no_scratch():
    """The kernels the metrics add, by name, in the built library's code-object metadata: private segment 0 bytes."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for want in ["mesh_tile_box_kernel", "mesh_distance_kernel", "max2_kernel", "group_stats_kernel", "group_mean_kernel"]:
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        assert ks[found[0]].get(".private_segment_fixed_size", 0) == 0, (want, ks[found[0]])
