"""CPU checks of direct triplane fitting (drag_utils.py:473-550, train_triplane_opt): the C ABI, the kernels' resources,
the host-side batch schedule and statistics lookup, and the test-side statement of the step against golden G17."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import triplane_opt_ref as R  # noqa: E402
from triplane_opt_ref import G17_GRAD1_SPREAD, G17_TOTAL_LOSS_SPREAD  # noqa: E402

NEW_SYMBOLS = ("ishap_triplane_fit_loss_grad", "ishap_triplane_reg_adam_step", "ishap_triplane_reg_values")


def test_fit_abi_declared_and_exported():
    from ishapediting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ishap.h")).read()
    declared = set(re.findall(r"\b(ishap_[a-z0-9_]+)\s*\(", hdr))
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SYMBOLS
        assert getattr(L, name) is not None
    assert L.ishap_version() >= 6
    m = re.search(r"#define ISHAP_TRIPLANE_REG_WS (\d+)", hdr)
    from ishapediting_amd.triplane_decoder import REG_WS
    assert m and int(m.group(1)) == REG_WS


def test_fit_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    names = [n for n in ks if any(k in n for k in ("triplane_fit_kernel", "triplane_reg_partials_kernel",
                                                    "triplane_reg_adam_kernel"))]
    assert len(names) == 3, names
    for n in names:
        assert ks[n].get(".private_segment_fixed_size", 0) == 0, (n, ks[n].get(".private_segment_fixed_size"))


def test_batch_schedule():
    from ishapediting_amd.triplane_decoder import batch_schedule
    full = batch_schedule(200000, 40000)
    assert full == [(i * 40000, 40000) for i in range(5)]
    part = batch_schedule(210000, 40000)
    assert len(part) == 6 and part[-1] == (200000, 10000) and sum(c for _, c in part) == 210000
    assert batch_schedule(20000, 4000) == [(i * 4000, 4000) for i in range(5)]
    assert batch_schedule(100, 40000) == [(0, 100)]
    with pytest.raises(ValueError):
        batch_schedule(0, 40000)


def test_stats_lookup_and_error(tmp_path):
    from ishapediting_amd.drag_utils import load_triplane_stats
    m, s = np.arange(96, dtype=np.float64), np.ones(96)
    got = load_triplane_stats((m, s), None)
    assert got[0].dtype == np.float32 and np.array_equal(got[0], m.astype(np.float32))
    np.save(tmp_path / "means.npy", m.reshape(1, 96, 1, 1))
    np.save(tmp_path / "stds.npy", s)
    got = load_triplane_stats(None, str(tmp_path))
    assert np.array_equal(got[0], m.astype(np.float32)) and np.array_equal(got[1], s.astype(np.float32))
    # explicit stats win over the directory
    got = load_triplane_stats((m + 1, s), str(tmp_path))
    assert got[0][0] == 1
    for d in (None, str(tmp_path / "missing")):
        with pytest.raises(FileNotFoundError, match="means.npy and stds.npy"):
            load_triplane_stats(None, d)
    os.remove(tmp_path / "stds.npy")
    with pytest.raises(FileNotFoundError, match="stats=\\(means, stds\\)"):
        load_triplane_stats(None, str(tmp_path))
    with pytest.raises(ValueError, match="96 values"):
        load_triplane_stats((np.zeros(3), np.zeros(3)))


def test_statement_agrees_with_the_fixture(gold):
    """The test-side statement (the oracle of tests/test_gpu_triplane_opt.py) against golden G17, made by the reference's
    own MultiTriplane / l2reg / tvreg and torch.optim.Adam: fp32 reproduces it, fp64 lies within the measured spreads."""
    g = gold("g17_triplane_opt")
    net, p0, coords, gt = R.fixture_inputs(g)
    batches = R.fixture_batches(g)
    fix = g["parts"]
    l32, t32, _, g32 = R.run_fit(net, p0, coords, gt, batches, torch.float32)
    np.testing.assert_allclose(l32.double().numpy(), fix[:, :4], rtol=1e-6)
    np.testing.assert_allclose(t32.double().numpy(), fix[:, 4], rtol=1e-6)
    assert float((g32 - torch.from_numpy(g["grad1"])).norm() / torch.from_numpy(g["grad1"]).norm()) < 1e-5
    l64, t64, p64, g64 = R.run_fit(net, p0, coords, gt, batches, torch.float64)
    np.testing.assert_allclose(l64[0].numpy(), fix[0, :4], rtol=1e-5)
    assert np.abs(t64.numpy() - fix[:, 4]).max() <= G17_TOTAL_LOSS_SPREAD * 1.01
    grad_rel = float((g64 - torch.from_numpy(g["grad1"]).double()).norm() / g64.norm())
    assert grad_rel <= G17_GRAD1_SPREAD * 1.01
