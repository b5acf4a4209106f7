"""Volume constraints without a GPU: the float64 reference (tests/constrain_ref.py) against what the project already trusts
(tests/decoder_ref.py), the reference gather list's own properties, the argument checks of constraints.py that need no device,
the ABI, and the code-object metadata of the new kernels (csrc/constrain.hip)."""
import os
import sys

import numpy as np
import pytest
import torch

from tests import constrain_ref as R
from tests import decoder_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(S=8, n=33, seed=5):
    _, net = D.synthetic_net()
    rs = np.random.RandomState(seed)
    planes = D.make_planes(S, D.AMP_BWD, S)
    coords = rs.uniform(-1.05, 1.05, (n, 3)).astype(np.float32)
    gt = (rs.rand(n) < 0.5).astype(np.float32)
    return net, planes, coords, gt


def test_unit_weights_are_the_unweighted_reference_exactly():
    net, planes, coords, gt = _case()
    a = D.points_loss_grad(net, planes, coords, gt)
    b = R.weighted_loss_grad(net, planes, coords, gt, np.ones(len(coords)))
    assert a.loss == b.loss and a.bce_abs_mean == b.bce_abs_mean
    for k in ("dplanes", "logits", "A", "A1", "Aw", "cnt"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_weights_scale_each_point_and_a_zero_weight_removes_it():
    net, planes, coords, gt = _case()
    n = len(coords)
    w = np.random.RandomState(6).uniform(0.5, 3.0, n)
    w[::5] = 0.0
    full = R.weighted_loss_grad(net, planes, coords, gt, w)
    keep = w > 0
    less = R.weighted_loss_grad(net, planes, coords[keep], gt[keep], w[keep])
    assert abs(full.loss - less.loss) <= 1e-15 * (1 + abs(full.loss))
    assert np.abs(full.dplanes - less.dplanes).max() <= 1e-15 * (np.abs(full.dplanes).max() + 1e-300)
    # by hand: sum_j w_j d bce_j
    per = [D.points_loss_grad(net, planes, coords[j:j + 1], gt[j:j + 1]) for j in range(n)]
    want = sum(w[j] * per[j].dplanes for j in range(n)) / w.sum()
    assert np.abs(full.dplanes - want).max() <= 1e-13 * np.abs(want).max()
    assert abs(full.loss - sum(w[j] * per[j].loss for j in range(n)) / w.sum()) <= 1e-13


@pytest.mark.parametrize("S", [2, 8, 16])
def test_reference_gather_list(S):
    rs = np.random.RandomState(S)
    coords = np.concatenate([D.mixed_coords(12, S, 3)[:72], np.repeat(rs.uniform(-1, 1, (1, 3)), 20, 0)]).astype(np.float32)
    row_start, entry, entry_w = R.gather_list(coords, S)
    t = D.taps(coords, S, np.float32)
    assert row_start[0] == 0 and row_start[-1] == len(entry) == len(entry_w) == int((t.tex >= 0).sum())
    assert (np.diff(row_start) >= 0).all()
    seen = set()
    for row in range(3 * S * S):
        e = entry[row_start[row]:row_start[row + 1]]
        assert (np.diff(e) > 0).all(), "entries ascend strictly within a row"
        p = row // (S * S)
        for k, key in zip(range(row_start[row], row_start[row + 1]), e):
            j, q = key >> 2, key & 3
            assert t.tex[j, p, q] == row
            assert entry_w[k].view(np.uint32) == np.float32(t.w[j, p, q]).view(np.uint32)
            seen.add((j, p, q))
    assert len(seen) == len(entry), "each in-range tap once"


def test_builder_argument_checks():
    from ishapediting_amd import constraints as K
    from ishapediting_amd.regions import Box, Voxels
    box = Box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="no region"):
        K.check_builder_args(None, None, [], 32, 100, (1, 1, 1))
    for bad in ((1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, float("inf"), 1.0), (1.0, 1.0), 3.0):
        with pytest.raises(ValueError, match="weights"):
            K.check_builder_args(box, None, None, 32, 100, bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError, match="max_points"):
            K.check_builder_args(box, None, None, 32, bad, (1, 1, 1))
    for bad in (1, 2000, 7.5):
        with pytest.raises(ValueError, match="D must"):
            K.check_builder_args(box, None, None, bad, 100, (1, 1, 1))
    with pytest.raises(ValueError, match="Voxels grid of size 8"):
        K.check_builder_args(None, Voxels(torch.ones(8, 8, 8, dtype=torch.bool)), None, 16, 100, (1, 1, 1))
    with pytest.raises(ValueError, match="a region is"):
        K.check_builder_args([box, "chair"], None, None, 32, 100, (1, 1, 1))
    roles, Dd, mp, w = K.check_builder_args(box, [box, box], None, 32, 100, (1, 2, 0))
    assert [len(r) for r in roles] == [1, 2, 0] and (Dd, mp, w) == (32, 100, (1.0, 2.0, 0.0))
    with pytest.raises(ValueError, match="points must be"):
        K.VolumeConstraints(torch.zeros(0, 3), torch.zeros(0), torch.zeros(0))
    with pytest.raises(ValueError, match="targets and weights"):
        K.VolumeConstraints(torch.zeros(4, 3), torch.zeros(3), torch.zeros(4))
    assert K.VolumeConstraints(torch.zeros(4, 3), torch.zeros(4), torch.ones(4)).M == 4


def test_mask_points_order_and_stride():
    from ishapediting_amd import constraints as K
    m = torch.zeros(5, 5, 5, dtype=torch.bool)
    m[1, 2, 3] = m[0, 4, 4] = m[4, 0, 0] = m[1, 2, 4] = m[3, 3, 3] = True
    p = K.mask_points(m, 100).numpy()
    want = np.array([[0, 4, 4], [1, 2, 3], [1, 2, 4], [3, 3, 3], [4, 0, 0]], np.float64) * 2 / 4 - 1
    assert np.array_equal(p, want.astype(np.float32))
    assert np.array_equal(K.mask_points(m, 2).numpy(), want[::3].astype(np.float32))      # ceil(5 / 2) = 3: every third
    assert np.array_equal(K.mask_points(m, 5).numpy(), want.astype(np.float32))


def test_abi_and_symbols():
    from ishapediting_amd import _lib
    L = _lib.lib()
    assert L.ishap_version() >= 24
    for name in ("ishap_constraint_setup", "ishap_constraint_setup_scratch_bytes", "ishap_constraint_loss_grad"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    # sizes are checked before anything else
    assert L.ishap_constraint_setup_scratch_bytes(0, 16) == -1 and L.ishap_constraint_setup_scratch_bytes((1 << 20) + 1, 16) == -1
    assert L.ishap_constraint_setup_scratch_bytes(5, 1) == -1 and L.ishap_constraint_setup_scratch_bytes(5, 1025) == -1
    assert L.ishap_constraint_setup_scratch_bytes(1, 2) > 0 and L.ishap_constraint_setup_scratch_bytes(1 << 20, 1024) > 0
    assert L.ishap_constraint_setup(None, 4, 16, None, None, None, None, 0, None) != 0
    assert L.ishap_constraint_setup(None, 0, 16, None, None, None, None, 0, None) != 0


def test_constraint_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for name in ("constraint_point_kernel", "constraint_gather_kernel", "constraint_count_kernel", "constraint_fill_kernel",
                 "constraint_rank_kernel", "constraint_cursor_kernel"):
        mine = [n for n in ks if name in n]
        assert len(mine) == 1, (name, mine)
        k = ks[mine[0]]
        assert k.get(".private_segment_fixed_size", 0) == 0, (mine[0], k.get(".private_segment_fixed_size"))
        assert k.get(".vgpr_spill_count", 0) == 0, (mine[0], k.get(".vgpr_spill_count"))


def test_the_pools_of_the_gpu_cases_stay_under_the_filters_cap():
    for S in (8, 16):
        assert D.survivor_pool(S).rejected <= 0.10, (S, D.survivor_pool(S).rejected)
