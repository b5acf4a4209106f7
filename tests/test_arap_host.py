"""CPU checks of the ARAP deformation (meshProcess.arap on the device): properties of the fp64 statement the GPU tests pin
to, argument rejection before any device work, the C ABI and the new kernels' code-object metadata (no GPU needed)."""
import os

import numpy as np
import pytest

from tests import arap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sphere_case():
    v, f = R.icosphere(2)                                   # 162 vertices
    top = np.argsort(v[:, 2])[-3:]
    bottom = np.argsort(v[:, 2])[:20]
    ids = np.concatenate([bottom, top])
    pos = np.concatenate([v[bottom], v[top] + np.array([0.15, 0.0, 0.1], np.float32)])
    return v, f, ids, pos


def test_constraints_at_rest_leave_the_mesh_at_rest():
    v, f = R.icosphere(2)
    ids = np.array([0, 5, 40, 99])
    x, E = R.arap(v, f, ids, v[ids], max_iter=5)
    assert np.abs(x - v.astype(np.float64)).max() < 1e-12
    assert E.max() <= 1e-12 * R.rest_energy_scale(v, f)


def test_statement_is_rigid_motion_equivariant():
    v, f, ids, pos = _sphere_case()
    x, E = R.arap(v, f, ids, pos, max_iter=10)
    Q, t = R.rigid(v, 3)
    vq = v.astype(np.float64) @ Q.T + t
    pq = pos.astype(np.float64) @ Q.T + t
    xq, Eq = R.arap(vq, f, ids, pq, max_iter=10)
    assert np.abs(xq - (x @ Q.T + t)).max() < 1e-9
    np.testing.assert_allclose(Eq, E, rtol=1e-9, atol=1e-12)


def test_statement_energy_does_not_increase():
    v, f, ids, pos = _sphere_case()
    _, E = R.arap(v, f, ids, pos, max_iter=30)
    assert E[0] > 10 * E[-1] > 0
    assert np.all(np.diff(E) <= 1e-12 * E[0])


def test_statement_keeps_unconstrained_components_at_rest():
    v1, f1 = R.icosphere(1)
    v2, f2 = R.grid_box((3, 3, 3), (2, 2, 2), (3, 3, 3))
    v = np.concatenate([v1, v2])
    f = np.concatenate([f1, f2 + len(v1)])
    e, w = R.edge_weights(v, f)
    role = R.roles(len(v), e, w, [0, 1])
    assert np.all(role[len(v1):] == 0) and np.all(role[2:len(v1)] == 1)
    x, _ = R.arap(v, f, [0, 1], v[[0, 1]] + 0.1, max_iter=3)
    assert np.array_equal(x[len(v1):], v2.astype(np.float64))


def test_statement_rotation_rules():
    g = np.random.default_rng(0)
    Q, _ = R.rigid(None, 1)
    C = g.normal(size=(3, 3))
    C = C @ C.T + 0.1 * np.eye(3)                           # symmetric positive definite
    S = np.stack([C @ Q.T, C, np.zeros((3, 3)), np.outer([1, 0, 0], [0, 1, 0]), -C])
    Rs = R.fit_rotations(S)
    np.testing.assert_allclose(Rs[0], Q, atol=1e-12)       # S = C Q^T gives Q back
    np.testing.assert_allclose(Rs[1], np.eye(3), atol=1e-12)
    assert np.array_equal(Rs[2], np.eye(3)) and np.array_equal(Rs[3], np.eye(3))     # rank < 2
    assert abs(np.linalg.det(Rs[4]) - 1) < 1e-12           # reflection fixed


def _no_device(monkeypatch):
    from ishapediting_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", refuse)
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_arap_rejects_bad_ids_before_device_work(monkeypatch):
    from ishapediting_amd.deform import arap, deform_as_rigid_as_possible
    _no_device(monkeypatch)
    v, f = R.icosphere(1)
    mesh = (v, f)
    hp = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError, match="both static and handle"):
        arap(mesh, [0, 1, 2], [2, 3], hp)
    with pytest.raises(ValueError, match="repeated"):
        arap(mesh, [0, 1, 1], [2, 3], hp)
    with pytest.raises(ValueError, match="repeated"):
        arap(mesh, [0, 1], [3, 3], hp)
    with pytest.raises(ValueError, match="must lie in"):
        arap(mesh, [0, len(v)], [2, 3], hp)
    with pytest.raises(ValueError, match="must lie in"):
        arap(mesh, [0, 1], [-1, 3], hp)
    with pytest.raises(ValueError, match="shape"):
        arap(mesh, [0, 1], [2, 3], np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="shape"):
        arap(mesh, [0, 1], [2, 3], np.zeros(6, np.float32))
    with pytest.raises(ValueError, match="repeated"):
        deform_as_rigid_as_possible(v, f, [4, 4], np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="must lie in"):
        deform_as_rigid_as_possible(v, f, [len(v)], np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError, match="shape"):
        deform_as_rigid_as_possible(v, f, [1, 2], np.zeros((2, 2), np.float32))


def test_arap_abi():
    from ishapediting_amd import _lib
    L = _lib.lib()
    assert L.ishap_version() >= 8
    assert L.ishap_arap_scratch_bytes(100, 196, 3) > 0
    assert L.ishap_arap_scratch_bytes(-1, 1, 1) == -1
    # argument checks fail before any launch
    assert L.ishap_arap(None, 0, None, 0, None, None, 0, 50, 1e-8, 0, None, None, None, None, 0, None) != 0
    assert b"arap" in L.ishap_last_error()
    assert L.ishap_nearest_vertices(None, 0, None, 0, None, None) != 0
    assert b"nearest_vertices" in L.ishap_last_error()


def test_arap_kernels_use_no_scratch():
    """The kernels ishap_arap launches (deform.hip's and the shared scan.hip's), by name, in the built library's code-object metadata: private segment 0 bytes."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    names = ["arap_check_tris_kernel", "arap_check_cons_kernel", "scan_blocks_kernel", "scan_totals_kernel",
             "scan_add_kernel", "corner_degree_kernel", "arap_vt_fill_kernel", "arap_rows_kernel", "arap_weights_kernel",
             "arap_label_init_kernel", "arap_label_sweep_kernel", "arap_label_jump_kernel", "arap_mark_kernel",
             "arap_roles_kernel", "arap_targets_kernel", "arap_local_kernel", "arap_energy_kernel", "arap_rhs_kernel",
             "arap_cg_init_kernel", "arap_cg_spmv_kernel", "arap_cg_alpha_kernel", "arap_cg_update_kernel",
             "arap_cg_beta_kernel", "arap_cg_record_kernel", "arap_output_kernel", "nearest_vertex_kernel"]
    for want in names:
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        assert ks[found[0]].get(".private_segment_fixed_size", 0) == 0, (want, ks[found[0]])
