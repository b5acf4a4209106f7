"""The references of tests/edt_ref.py against each other and against scipy, the properties of the morphology and of the feather
built on them, and what the built library must hold for the distance transform (csrc/edt.hip): no GPU needed."""
import os
import sys

import numpy as np
import pytest

from tests import edt_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so")


@pytest.mark.parametrize("shape", E.SMALL_SHAPES + [(5, 9, 12)], ids=str)
def test_brute_equals_separable_on_the_small_cases(shape):
    for name, grid in E.seed_sets(shape).items():
        for invert in (False, True):
            for axes in ((7,) if shape != (5, 9, 12) else range(1, 8)):
                a, b = E.edt_brute(grid, axes, invert), E.edt_separable(grid, axes, invert)
                assert np.array_equal(a, b), (shape, name, invert, axes)
    assert int(E.edt_separable(np.zeros(shape, np.uint8)).min()) == E.INF


def test_scipy_brute_and_separable_agree_at_33():
    import scipy.ndimage as ndi
    rng = np.random.default_rng(33)
    grid = rng.random((33, 33, 33)) < 0.01
    sep = E.edt_separable(grid)
    assert np.array_equal(sep, E.edt_brute(grid))
    sci = np.rint(ndi.distance_transform_edt(~grid) ** 2).astype(np.int64)       # scipy: distance to the nearest ZERO
    assert np.array_equal(sep, sci)
    assert np.array_equal(E.edt_separable(grid, invert=True), np.rint(ndi.distance_transform_edt(grid) ** 2).astype(np.int64))


def _blob(D=21, seed=5):
    rng = np.random.default_rng(seed)
    ax = np.arange(D)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    m = (x - 9) ** 2 + (y - 10) ** 2 + (z - 8) ** 2 <= 36
    m |= (abs(x - 16) <= 2) & (abs(y - 10) <= 1) & (abs(z - 8) <= 1)             # a spur
    m[9, 10, 8] = False                                                        # a hole
    return m | (rng.random((D, D, D)) < 0.002)


@pytest.mark.parametrize("r", [0, 1, 1.5, 2, 3.7])
def test_grow_and_shrink_are_dual_and_open_close_bracket_the_region(r):
    m = _blob()
    assert np.array_equal(E.shrink(m, r), ~E.grow(~m, r))
    assert np.array_equal(E.grow(m, r), ~E.shrink(~m, r))
    o, c = E.open_(m, r), E.close_(m, r)
    assert not (o & ~m).any() and not (m & ~c).any()
    assert np.array_equal(E.shell(m, r, r), E.grow(m, r) & ~E.shrink(m, r))
    if r == 0:
        assert np.array_equal(o, m) and np.array_equal(c, m)
    full = np.ones((7, 7, 7), bool)
    assert E.shrink(full, r).all()                                             # the walls of the cube do not erode


def _marks(W=24):
    m = np.zeros((3, W, W), np.uint8)
    m[0, 4:10, 5:12] |= 1
    m[0, 8:15, 9:20] |= 2                      # overlaps keep
    m[1, 2:5, 2:5] |= 2                        # plane 1: free only; plane 2: nothing at all
    return m


@pytest.mark.parametrize("weights", [(4.0, 0.0), (0.5, 2.5), (1.0, 1.0)])
def test_feather_is_the_hard_map_up_to_one_texel_and_stays_within_the_weights(weights):
    kw, fw = weights
    m = _marks()
    hard = E.hard_ref(m, kw, fw)
    for falloff in (0.5, 1.0):
        assert np.array_equal(E.feather_ref(m, kw, fw, falloff).view(np.uint32), hard.view(np.uint32))
    lo, hi = min(1.0, kw, fw), max(1.0, kw, fw)
    for falloff in (2.5, 8.0, 64.0):
        w = E.feather_ref(m, kw, fw, falloff)
        assert w.dtype == np.float32 and float(w.min()) >= lo and float(w.max()) <= hi
        assert np.array_equal(w[m & 1 != 0], hard[m & 1 != 0])                  # the keep shadow itself keeps its weight
        assert (w[2] == 1.0).all()                                             # a plane without shadows
        if kw != 1.0 or fw != 1.0:
            assert not np.array_equal(w, hard)
    assert len(E.falloff_table(64.0)) == 4096 and E.falloff_table(0.3).tolist() == [1.0]


def test_neck_reference_cuts_two_blocks_apart():
    D = 24
    sel = np.zeros((D, D, D), bool)
    sel[2:10, 4:12, 4:12] = True
    sel[14:22, 4:12, 4:12] = True
    sel[10:14, 7:9, 7:9] = True                                                # the neck, 2 voxels wide
    assert len(np.unique(E.components6(sel))) == 2                              # one piece (and the outside)
    got = E.neck(sel, (5, 8, 8), 2)
    # the picked block's core (its inner 4^3) grown back by 2: nothing of the other block, and of the neck no more than the
    # 2 voxels next to the picked block
    assert got is not None and got[4:8, 6:10, 6:10].all() and not got[12:].any() and not (got & ~sel).any()
    assert E.neck(sel, (12, 7, 7), 2) is None


# ------------------------------------------------------------------------------------------------ the built library
def test_library_exports_the_transform():
    import ctypes as C
    from ishapediting_amd import _lib, build
    assert "edt.hip" in build.SOURCES
    for name in ("ishap_edt", "ishap_edt_scratch_bytes", "ishap_region_plane_marks", "ishap_region_plane_feather",
                 "ishap_region_plane_feather_scratch_bytes"):
        assert name in _lib.SYMBOLS
    lib = C.CDLL(LIB)
    for name in ("ishap_edt", "ishap_edt_scratch_bytes"):
        assert hasattr(lib, name)
    lib.ishap_version.restype = C.c_int
    assert lib.ishap_version() >= 23
    sb = lib.ishap_edt_scratch_bytes
    sb.restype, sb.argtypes = C.c_longlong, [C.c_int] * 4
    assert sb(256, 256, 256, 7) >= 4 * 256 ** 3 and sb(1, 1, 70, 4) > 0
    assert sb(4, 4, 4, 0) == -1 and sb(4, 4, 4, 8) == -1 and sb(0, 4, 4, 7) == -1 and sb(1025, 4, 4, 1) == -1
    assert sb(2048, 4, 4, 6) > 0                                               # a batch axis may be longer than 1024
    assert sb(2048, 1024, 1024, 6) == -1                                       # 2^31 voxels


def test_edt_and_feather_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(LIB)
    mine = [n for n in ks if "edt_" in n or "region_feather_kernel" in n or "region_compose_marks_kernel" in n]
    for want in ("edt_col_kernel", "edt_row_kernel", "region_feather_kernel", "region_compose_marks_kernel"):
        assert any(want in n for n in mine), (want, mine)
    for n in mine:
        k = ks[n]
        assert k.get(".private_segment_fixed_size", 0) == 0, (n, k.get(".private_segment_fixed_size"))
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (n, k)
