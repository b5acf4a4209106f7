"""Part edits without a GPU: the numpy reference of csrc/parts.hip against definitions (tests/parts_ref.py), regions.Rigid and the
host half of plan_part_edit, and the ABI of the new entry points.  tests/test_gpu_parts.py holds the device to this reference
byte for byte; the half-integer margins asserted here are what lets it do so for general rotations with no tolerance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import parts_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ farthest-point reference
def _fps_cases():
    rng = np.random.default_rng(5)
    yield "scattered", 12, P.candidates(P.scattered_mask(12, 150, 1)), 17
    yield "L", 16, P.candidates(P.l_volume(16) > 0), 9
    yield "cube", 9, P.candidates(P.cube_mask(9, 2, 7)), 12
    yield "cross", 9, P.candidates(P.cross_mask(9, 3)), 19
    yield "line", 8, np.stack([np.arange(8), np.full(8, 3), np.full(8, 3)], axis=1), 8
    yield "few", 10, rng.integers(0, 10, size=(1, 3)), 3


@pytest.mark.parametrize("case", list(_fps_cases()), ids=lambda c: c[0])
def test_incremental_picks_are_the_definitional_picks(case):
    _, D, coords, n = case
    coords = coords[np.argsort(P._lin(coords, D))]
    for start in (None, (0, 0, 0), (D - 1, D // 2, 1), tuple(int(v) for v in coords[len(coords) // 2])):
        a, b = P.fps_ref(coords, D, n, start), P.fps_brute(coords, D, n, start)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == len(coords), (case[0], start)
        m = min(n, len(coords))
        assert len({tuple(p) for p in a[0][:m]}) == m                     # no voxel is picked twice while r < M
        assert (a[0][m:] == -1).all() and (a[1][m:] == 0).all() and a[1][0] == 0
        for k in range(2, m + 1):                                         # the squared distance at pick k - 1 is the spacing of the first k
            assert a[1][k - 1] == P.min_pairwise_dist2(a[0][:k]), (case[0], start, k)
        assert (np.diff(a[1][1:m]) <= 0).all()                            # and it never grows


def test_first_pick_rules():
    D = 11
    coords = P.candidates(P.cube_mask(D, 3, 8))
    # no start: farthest from the centre of the bounding box -- the eight corners tie, the lowest index wins
    assert P.fps_ref(coords, D, 1)[0][0].tolist() == [3, 3, 3]
    # a start in the part is picked itself; one outside picks the nearest voxel, ties to the lowest index
    assert P.fps_ref(coords, D, 1, (5, 6, 4))[0][0].tolist() == [5, 6, 4]
    assert P.fps_ref(coords, D, 1, (0, 5, 5))[0][0].tolist() == [3, 5, 5]
    assert P.fps_ref(coords, D, 1, (10, 10, 10))[0][0].tolist() == [7, 7, 7]


def test_ties_go_to_the_lowest_index():
    """A full cube: the eight corners tie for the first pick, the opposite corner is alone for the second; for the third,
    min(|v|^2, |v - (4, 4, 4)|^2) is largest where both are equal (a + b + c = 6) and a^2 + b^2 + c^2 is: the six permutations
    of (0, 2, 4), value 20 -> the lowest index, (0, 2, 4).  A symmetric cross: the six arm tips tie for the first pick."""
    D = 5
    coords = P.candidates(P.cube_mask(D, 0, 5))
    picks, d2, M = P.fps_ref(coords, D, 3)
    assert M == 125 and picks.tolist() == [[0, 0, 0], [4, 4, 4], [0, 2, 4]] and d2.tolist() == [0, 48, 20]
    mind = np.minimum((coords ** 2).sum(1), ((coords - 4) ** 2).sum(1))
    assert mind.max() == 20 and int((mind == 20).sum()) == 6               # the tie is real
    D = 9
    picks, d2, M = P.fps_ref(P.candidates(P.cross_mask(D, 3)), D, 7)
    assert M == 19 and picks[0].tolist() == [1, 4, 4] and picks[1].tolist() == [7, 4, 4] and d2[1] == 36
    assert picks[2].tolist() == [4, 1, 4] and d2[2] == 18                  # four tips tie at 18: (4, 1, 4) has the lowest index
    assert sorted(map(tuple, picks[:6].tolist())) == sorted([(1, 4, 4), (7, 4, 4), (4, 1, 4), (4, 7, 4), (4, 4, 1), (4, 4, 7)])


# ------------------------------------------------------------------------------------------------ select
def test_select_reference_rules():
    D = 16
    vol = P.l_volume(D)
    c = P.centres(D)
    # a box whose faces pass through voxel centres: both faces are in
    box = ("box", (c[2], c[3], c[4]), (c[9], c[5], c[11]))
    got = P.select_ref(vol, 0.0, [box])
    want = np.zeros((D, D, D), bool)
    want[2:10, 3:6, 4:12] = True
    assert np.array_equal(got != 0, want & (vol > 0)) and got.any()
    # level: nothing is above 1, everything above -2
    assert not P.select_ref(vol, 1.0, [box]).any()
    assert np.array_equal(P.select_ref(vol, -2.0, [box]) != 0, want)
    # a grid is ORed in, and the volume still gates it
    grid = np.zeros((D, D, D), np.uint8)
    grid[:, :, 0:8] = 1
    assert np.array_equal(P.select_ref(vol, 0.0, [], grid) != 0, (grid != 0) & (vol > 0))
    u = P.select_ref(vol, 0.0, [box, ("sphere", (0.4, -0.4, 0.0), 0.3)], grid)
    assert np.array_equal(u, P.select_ref(vol, 0.0, [box]) | P.select_ref(vol, 0.0, [("sphere", (0.4, -0.4, 0.0), 0.3)]) | P.select_ref(vol, 0.0, [], grid))


# ------------------------------------------------------------------------------------------------ transform
def _shape(D):
    return (P.l_volume(D) > 0).astype(np.uint8)


@pytest.mark.parametrize("D", [16, 17])
def test_transform_identity_quarter_turns_and_shifts(D):
    m = _shape(D)
    eye, zero = np.eye(3), (0.0, 0.0, 0.0)
    assert np.array_equal(P.transform_ref(m, eye, zero, zero), m)
    assert np.array_equal(P.transform_ref(m, eye, (0.3, -0.2, 0.1), zero), m)          # a pivot alone moves nothing
    for k in (1, 2, 3):
        R = P.rotation_ref((0, 0, 1), 90.0 * k)
        assert set(np.unique(R).tolist()) <= {-1.0, 0.0, 1.0}
        assert np.array_equal(P.transform_ref(m, R, zero, zero), np.rot90(m, k, axes=(0, 1))), (D, k)
    assert np.array_equal(P.transform_ref(m, P.rotation_ref((2, 0, 0), 90.0), zero, zero), np.rot90(m, 1, axes=(1, 2)))
    # whole voxels: a shift; what leaves the cube is cut off and nothing wraps round
    h = 2.0 / (D - 1)
    got = P.transform_ref(m, eye, zero, (3 * h, 0.0, -2 * h))
    want = np.zeros_like(m)
    want[3:, :, :D - 2] = m[:D - 3, :, 2:]
    assert np.array_equal(got, want)
    far = P.transform_ref(m, eye, zero, (0.0, 9 * h, 0.0))
    want = np.zeros_like(m)
    want[:, 9:, :] = m[:, :D - 9, :]
    assert np.array_equal(far, want) and 0 < far.sum() < m.sum()
    assert not P.transform_ref(m, eye, zero, (0.0, 0.0, 2.5)).any()


@pytest.mark.parametrize("D", P.SIZES)
@pytest.mark.parametrize("k", range(len(P.GENERAL)))
def test_general_transforms_stay_clear_of_half_integers(D, k):
    """The device and numpy may differ in the last bit of nothing here -- the operation order is the same -- but the margin is
    what makes the byte-for-byte comparison of the GPU test robust: no source index is within 1e-9 of a rounding tie."""
    axis, deg, pivot, t = P.GENERAL[k]
    R = P.rotation_ref(axis, deg)
    assert P.half_integer_margin(D, R, pivot, t) > 1e-9
    moved = P.transform_ref(_shape(D), R, pivot, t)
    n0, n1 = int(_shape(D).sum()), int(moved.sum())
    assert n1 > 0 and abs(n1 - n0) <= 0.2 * n0                           # a rigid motion inside the cube keeps the volume, roughly


# ------------------------------------------------------------------------------------------------ Rigid, the plan
def test_rigid_matrix_apply_and_refusals():
    from ishapediting_amd.regions import Rigid
    assert np.array_equal(Rigid().matrix, np.eye(3)) and Rigid().matrix.dtype == np.float64
    for axis in ((1, 0, 0), (0, -3, 0), (0, 0, 0.5)):
        for k in range(-4, 9):
            R = Rigid(rotation=(axis, 90.0 * k)).matrix
            assert set(np.unique(R).tolist()) <= {-1.0, 0.0, 1.0} and not np.signbit(R[R == 0]).any(), (axis, k)
            assert np.array_equal(R, P.rotation_ref(axis, 90.0 * k))
    for axis, deg, pivot, t in P.GENERAL:
        g = Rigid(rotation=(axis, deg), pivot=pivot, translation=t)
        assert np.array_equal(g.matrix, P.rotation_ref(axis, deg))
        assert np.abs(g.matrix.T @ g.matrix - np.eye(3)).max() < 1e-15 and np.linalg.det(g.matrix) > 0
        pts = np.random.default_rng(2).uniform(-1, 1, (50, 3)).astype(np.float32)
        out = g.apply(pts)
        assert out.dtype == np.float64 and np.array_equal(out, P.apply_ref(g.matrix, pivot, t, pts))
        assert np.allclose(out, (pts.astype(np.float64) - pivot) @ g.matrix.T + pivot + t, atol=1e-14)
        assert np.array_equal(Rigid(rotation=g.matrix, pivot=pivot, translation=t).apply(pts), out)      # a matrix is taken as it is
        assert np.allclose(g.apply(np.asarray(pivot)), np.asarray(pivot) + t, atol=1e-16)               # the pivot only translates
    R = P.rotation_ref((1, 2, 3), 40.0)
    with pytest.raises(ValueError, match="not a rotation"):
        Rigid(rotation=1.001 * R)                                          # scaled
    with pytest.raises(ValueError, match="not a rotation"):
        Rigid(rotation=R @ np.diag([1.0, 1.0, -1.0]))                      # reflected
    with pytest.raises(ValueError, match="not a rotation"):
        Rigid(rotation=R + np.array([[0, 1e-6, 0], [0, 0, 0], [0, 0, 0]]))
    with pytest.raises(ValueError):
        Rigid(rotation=np.eye(4))
    with pytest.raises(ValueError, match="zero vector"):
        Rigid(rotation=((0, 0, 0), 30))
    with pytest.raises(ValueError):
        Rigid(pivot=(0, 0))
    with pytest.raises(Exception):
        Rigid().pivot = (1, 1, 1)                                          # frozen


def test_plan_refuses_targets_outside_the_cube_and_too_many_handles():
    from ishapediting_amd.regions import Rigid, handle_targets
    D = 16
    mask = _shape(D)
    M = int(mask.sum())
    g = Rigid(rotation=((0, 0, 1), 30.0), pivot=(-0.4, -0.4, 0.0), translation=(0.05, 0.0, 0.0))
    src, tgt, moved, spacing = P.plan_ref(mask, g.matrix, g.pivot, g.translation, 8)
    assert src.dtype == tgt.dtype == np.float32 and moved.any() and spacing > 0
    assert np.array_equal(handle_targets(src, g).view(np.uint32), tgt.view(np.uint32))          # the product's host half, bit for bit
    assert (mask[tuple(np.rint((src.astype(np.float64) + 1) * (D - 1) / 2).astype(int).T)] == 1).all()
    with pytest.raises(ValueError, match=f"{M + 1} handles asked of a part of {M} voxels"):
        P.plan_ref(mask, g.matrix, g.pivot, g.translation, M + 1)
    out = Rigid(translation=(0.0, 0.5, 0.0))
    with pytest.raises(ValueError, match="outside"):
        P.plan_ref(mask, out.matrix, out.pivot, out.translation, 8)
    with pytest.raises(ValueError, match=r"handle \d+ at .* outside \[-1, 1\]\^3"):
        handle_targets(src, out)
    with pytest.raises(ValueError, match="Rigid"):
        from ishapediting_amd.regions import plan_part_edit
        plan_part_edit(None, "not a rigid")


# ------------------------------------------------------------------------------------------------ ABI, no GPU needed
NEW = ("ishap_region_select", "ishap_region_handles_scratch_bytes", "ishap_region_handles", "ishap_region_transform")
FAKE = C.c_void_p(0x1000)


def test_header_bindings_and_library_agree():
    from ishapediting_amd import _lib
    L = _lib.lib()
    assert L.ishap_version() >= 19
    header = open(os.path.join(ROOT, "include", "ishap.h")).read()
    for name in NEW:
        decl = re.search(r"^(?:int|long long) " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SYMBOLS[name][1]), name          # as many parameters as the binding passes
        assert hasattr(L, name)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from ishapediting_amd import _lib
    L = _lib.lib()
    assert L.ishap_region_handles_scratch_bytes(1, 4) == -1 and L.ishap_region_handles_scratch_bytes(1025, 4) == -1
    assert L.ishap_region_handles_scratch_bytes(64, 0) == -1 and L.ishap_region_handles_scratch_bytes(64, 4097) == -1
    for D, n in ((2, 1), (64, 16), (256, 4096), (1024, 16)):
        assert L.ishap_region_handles_scratch_bytes(D, n) >= 8 * D ** 3 + 8 * n
    big = 1 << 40
    bad = (C.c_int * 3)(0, 64, 0)
    assert L.ishap_region_select(FAKE, 1, 0.0, None, 0, FAKE, FAKE, FAKE, None) == -2                   # D < 2
    assert L.ishap_region_select(FAKE, 1025, 0.0, None, 0, FAKE, FAKE, FAKE, None) == -2
    assert L.ishap_region_select(FAKE, 16, float("nan"), None, 0, FAKE, FAKE, FAKE, None) == -2
    assert L.ishap_region_select(FAKE, 16, 0.0, None, 2, FAKE, FAKE, FAKE, None) == -2                  # primitives counted but absent
    assert L.ishap_region_select(None, 16, 0.0, None, 0, FAKE, FAKE, FAKE, None) == -2
    assert L.ishap_region_select(FAKE, 16, 0.0, None, 0, FAKE, FAKE, None, None) == -2
    assert L.ishap_region_handles(FAKE, 64, 0, None, FAKE, FAKE, FAKE, FAKE, big, None) == -2           # n < 1
    assert L.ishap_region_handles(FAKE, 64, 4097, None, FAKE, FAKE, FAKE, FAKE, big, None) == -2
    assert L.ishap_region_handles(FAKE, 1025, 4, None, FAKE, FAKE, FAKE, FAKE, big, None) == -2
    assert L.ishap_region_handles(FAKE, 64, 4, bad, FAKE, FAKE, FAKE, FAKE, big, None) == -2            # a start outside the grid
    assert L.ishap_region_handles(FAKE, 64, 4, None, FAKE, FAKE, FAKE, FAKE, 1024, None) == -2          # scratch too small
    assert L.ishap_region_handles(FAKE, 64, 4, None, FAKE, FAKE, FAKE, C.c_void_p(0x1008), big, None) == -2
    assert L.ishap_region_handles(FAKE, 64, 4, None, None, FAKE, FAKE, FAKE, big, None) == -2
    assert b"region handles" in L.ishap_last_error()
    ok = (C.c_double * 15)(1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0)
    nan = (C.c_double * 15)(1, 0, 0, 0, float("nan"), 0, 0, 0, 1, 0, 0, 0, 0, 0, 0)
    assert L.ishap_region_transform(FAKE, 1, ok, C.c_void_p(0x2000), FAKE, None) == -2
    assert L.ishap_region_transform(FAKE, 16, nan, C.c_void_p(0x2000), FAKE, None) == -2
    assert L.ishap_region_transform(FAKE, 16, ok, FAKE, FAKE, None) == -2                               # in place
    assert L.ishap_region_transform(FAKE, 16, None, C.c_void_p(0x2000), FAKE, None) == -2
