"""The exact distance transform on the device (csrc/edt.hip) and what is built on it, against tests/edt_ref.py: squared
distances equal as integers at every voxel, the feathered weight map bitwise the float64 formula, the morphology and the neck cut
byte for byte, and margin / region_falloff through DragStuff on the tiny model.  There is no tolerance anywhere in this file."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest
import torch

from ishapediting_amd import _lib
from tests import edt_ref as E

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def edt_dev(grid, axes=7, invert=0):
    """ishap_edt itself on a uint8 [n0, n1, n2] array -> int32 device tensor"""
    g = T(np.ascontiguousarray(grid, np.uint8)).to(dev())
    n0, n1, n2 = g.shape
    L = _lib.lib()
    nbytes = int(L.ishap_edt_scratch_bytes(n0, n1, n2, axes))
    assert nbytes > 0
    out = torch.empty((n0, n1, n2), dtype=torch.int32, device=dev())
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev())
    _lib.check(L.ishap_edt(g.data_ptr(), n0, n1, n2, axes, invert, out.data_ptr(), scratch.data_ptr(), nbytes, _lib.stream_ptr(dev())))
    return out


def _check(grid, axes, invert, what):
    got = edt_dev(grid, axes, invert).cpu().numpy()
    want = E.edt_separable(grid, axes, bool(invert))
    assert got.dtype == np.int32 and np.array_equal(got, want), (what, axes, invert, np.argwhere(got != want)[:8].tolist())


# ------------------------------------------------------------------------------------------------ 1. the transform
@pytest.mark.parametrize("shape", E.SHAPES, ids=str)
def test_dist2_equals_the_reference_at_every_voxel(shape):
    for name, grid in E.seed_sets(shape).items():
        for invert in (0, 1):
            _check(grid, 7, invert, (shape, name))


@pytest.mark.parametrize("axes", [1, 2, 4, 3, 5, 6])
def test_every_single_axis_and_every_pair(axes):
    for name, grid in E.seed_sets((17, 33, 65)).items():
        for invert in (0, 1):
            _check(grid, axes, invert, name)


def test_three_plane_maps_with_one_empty_slice():
    rng = np.random.default_rng(6)
    grid = (rng.random((3, 33, 33)) < 0.02).astype(np.uint8)
    grid[1] = 0
    got = edt_dev(grid, 6).cpu().numpy()
    assert np.array_equal(got, E.edt_separable(grid, 6)) and (got[1] == E.INF).all() and got[0].max() < E.INF
    _check(grid, 6, 1, "planes inverted")
    for name, g in E.seed_sets((3, 33, 33)).items():
        _check(g, 6, 0, name)


@pytest.mark.parametrize("shape", [(1, 1, 1024), (1, 1024, 1), (1024, 1, 1), (130, 130, 130)], ids=str)
def test_long_range_against_the_closed_form(shape):
    grid = np.zeros(shape, np.uint8)
    grid[0, 0, 0] = 1
    i, j, k = np.meshgrid(*(np.arange(n, dtype=np.int64) for n in shape), indexing="ij")
    got = edt_dev(grid).cpu().numpy()
    assert np.array_equal(got, i * i + j * j + k * k)
    if shape[0] == 130:                                                  # the far corner too: the search runs the other way
        grid[0, 0, 0], grid[-1, -1, -1] = 0, 1
        assert np.array_equal(edt_dev(grid).cpu().numpy(), (129 - i) ** 2 + (129 - j) ** 2 + (129 - k) ** 2)


def test_the_workload_size_once():
    D = 256
    rng = np.random.default_rng(256)
    seeds = rng.integers(0, D, size=(8, 3))
    grid = torch.zeros((D, D, D), dtype=torch.uint8)
    for s in seeds:
        grid[tuple(int(v) for v in s)] = 1
    got = edt_dev(grid.numpy())
    ax = torch.arange(D, device=dev(), dtype=torch.int32)
    want = torch.full((D, D, D), E.INF, dtype=torch.int32, device=dev())
    for s in seeds:                                                      # min over seeds, the definition (integer torch ops)
        sx, sy, sz = (int(v) for v in s)
        want = torch.minimum(want, ((ax - sx) ** 2)[:, None, None] + ((ax - sy) ** 2)[None, :, None] + ((ax - sz) ** 2)[None, None, :])
    assert torch.equal(got, want)
    assert np.array_equal(got[::37, ::41, ::43].cpu().numpy(),           # and in numpy on a sub-lattice
                          np.min([sum((np.arange(D)[::st].reshape([-1 if a == b else 1 for b in range(3)]) - int(s[a])) ** 2
                                      for a, st in enumerate((37, 41, 43))) for s in seeds], axis=0))


def test_two_runs_and_another_stream_give_the_same_bits():
    grid = E.seed_sets((17, 33, 65))["rand1"]
    a, b = edt_dev(grid), edt_dev(grid)
    assert torch.equal(a, b)
    side = torch.cuda.Stream(device=dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        c = edt_dev(grid, 7, 1)
        d = edt_dev(grid)
    side.synchronize()
    assert torch.equal(d, a) and torch.equal(c, edt_dev(grid, 7, 1))


def test_bad_arguments_launch_nothing():
    L = _lib.lib()
    g = torch.zeros((4, 4, 4), dtype=torch.uint8, device=dev())
    out = torch.full((4, 4, 4), -7, dtype=torch.int32, device=dev())
    scratch = torch.empty(1024, dtype=torch.uint8, device=dev())
    s = _lib.stream_ptr(dev())
    bad = [(g.data_ptr(), 4, 4, 4, 0, 0, out.data_ptr(), scratch.data_ptr(), 1024), (g.data_ptr(), 4, 4, 4, 8, 0, out.data_ptr(), scratch.data_ptr(), 1024),
           (g.data_ptr(), 4, 4, 4, 7, 2, out.data_ptr(), scratch.data_ptr(), 1024), (None, 4, 4, 4, 7, 0, out.data_ptr(), scratch.data_ptr(), 1024),
           (g.data_ptr(), 4, 4, 4, 7, 0, None, scratch.data_ptr(), 1024), (g.data_ptr(), 4, 4, 4, 7, 0, out.data_ptr(), None, 1024),
           (g.data_ptr(), 4, 4, 4, 7, 0, out.data_ptr(), scratch.data_ptr(), 255), (g.data_ptr(), 0, 4, 4, 7, 0, out.data_ptr(), scratch.data_ptr(), 1024),
           (g.data_ptr(), 1025, 1, 1, 1, 0, out.data_ptr(), scratch.data_ptr(), 1024), (out.data_ptr() + 8, 4, 4, 4, 7, 0, out.data_ptr(), scratch.data_ptr(), 1024)]
    for args in bad:
        assert L.ishap_edt(*args, s) != 0, args
    torch.cuda.synchronize()
    assert bool((out == -7).all())
    assert int(L.ishap_edt_scratch_bytes(4, 4, 4, 0)) == -1


# ------------------------------------------------------------------------------------------------ 2. the Python layer
def test_distance_transform_shapes_and_axes():
    from ishapediting_amd.volume import distance_transform
    rng = np.random.default_rng(2)
    m3 = rng.random((5, 9, 12)) < 0.05
    assert np.array_equal(distance_transform(T(m3).to(dev())).cpu().numpy(), E.edt_separable(m3))
    assert np.array_equal(distance_transform(T(m3).to(dev()), axes=(1, 2)).cpu().numpy(), E.edt_separable(m3, 6))
    assert np.array_equal(distance_transform(T(m3).to(dev()), axes=(0, -1), invert=True).cpu().numpy(), E.edt_separable(m3, 5, True))
    m2 = rng.random((9, 70)) < 0.05
    assert np.array_equal(distance_transform(T(m2.astype(np.uint8)).to(dev())).cpu().numpy(), E.edt_separable(m2[None], 6)[0])
    m1 = rng.random(70) < 0.05
    got = distance_transform(T(m1).to(dev()))
    assert got.shape == (70,) and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), E.edt_separable(m1[None, None], 4)[0, 0])
    with pytest.raises(ValueError):
        distance_transform(T(m1).to(dev()), axes=(1,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distance_transform(T(m1))                                        # not on the device


def _ball(D=33, cavity=False):
    ax = np.arange(D) - D // 2
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    r2 = x * x + y * y + z * z
    v = (10.5 ** 2 - r2).astype(np.float32)
    if cavity:
        v = np.where(r2 < 4.2 ** 2, np.float32(-1.0), v)
    return v


@pytest.mark.parametrize("case", ["ball", "cavity", "outside", "inside"])
def test_signed_distance_equals_the_float64_reference(case):
    from ishapediting_amd.volume import signed_distance
    vol = {"ball": _ball(), "cavity": _ball(cavity=True), "outside": np.full((33, 33, 33), -1.0, np.float32),
           "inside": np.full((33, 33, 33), 1.0, np.float32)}[case]
    got = signed_distance(T(vol).to(dev())).cpu().numpy()
    want = E.signed_distance(vol - np.float32(0.0) > 0)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if case == "outside":
        assert np.isposinf(got).all()
    elif case == "inside":
        assert np.isneginf(got).all()
    else:
        assert got[16, 16, 16 if case == "ball" else 26] < 0 and got[0, 0, 0] > 0          # negative inside
        level = signed_distance(T(vol).to(dev()), level=50.0).cpu().numpy()
        assert np.array_equal(level.view(np.uint32), E.signed_distance(vol - np.float32(50.0) > 0).view(np.uint32))


@lru_cache(maxsize=None)
def _region33():
    D = 33
    ax = np.arange(D)
    x, y, z = np.meshgrid(ax, ax, ax, indexing="ij")
    m = (x - 14) ** 2 + (y - 16) ** 2 + (z - 15) ** 2 <= 64
    m |= (abs(x - 26) <= 3) & (abs(y - 16) <= 1) & (abs(z - 15) <= 1)             # a spur thinner than some radii
    m[13:16, 15:18, 14:17] = False                                              # a hole
    m[0:3, 0:4, 0:2] = True                                                     # a piece in the corner of the cube
    return m


@pytest.mark.parametrize("r", [0, 1, 1.5, 2, 3.7])
def test_morphology_equals_the_reference_byte_for_byte(r):
    from ishapediting_amd import regions as Rg
    m = _region33()
    reg = Rg.Voxels(T(m).to(dev()))
    for fn, ref in ((Rg.grow, E.grow), (Rg.shrink, E.shrink), (Rg.open_region, E.open_), (Rg.close_region, E.close_)):
        got = fn(reg, r)
        assert isinstance(got, Rg.Voxels) and np.array_equal(got.mask.cpu().numpy(), ref(m, r)), (fn.__name__, r)
        if r == 0:
            assert got is reg                                                   # the region itself, nothing launched
    for inner, outer in ((r, 2), (1, r)):
        assert np.array_equal(Rg.shell(reg, inner, outer).mask.cpu().numpy(), E.shell(m, inner, outer)), (inner, outer)
    with pytest.raises(ValueError):
        Rg.grow(reg, -1)


def test_select_part_cuts_at_a_neck():
    """Two 10^3 blocks joined by a neck 2 voxels wide, D = 48.  neck = 0: the pick's piece is both blocks and the neck.
    neck = 2: the picked block (opened by 2: its corners are rounded) and of the neck no more than the 2 voxels next to it."""
    from ishapediting_amd.regions import Box, select_part
    D = 48
    sel = np.zeros((D, D, D), bool)
    sel[6:16, 18:28, 18:28] = True
    sel[26:36, 18:28, 18:28] = True
    sel[16:26, 22:24, 22:24] = True
    vol = T(np.where(sel, 1.0, -1.0).astype(np.float32)).to(dev())
    c = lambda i: 2.0 * i / (D - 1) - 1.0                                       # noqa: E731
    whole = Box((-1, -1, -1), (1, 1, 1))
    pick = (c(10), c(22), c(22))
    both = select_part(vol, whole, point=pick).mask.cpu().numpy()
    assert np.array_equal(both, sel) and both[26:36].any()                      # neck = 0: everything connected to the pick
    got = select_part(vol, whole, point=pick, neck=2).mask.cpu().numpy()
    want = E.neck(sel, (10, 22, 22), 2)
    assert want is not None and np.array_equal(got, want)
    assert got[8:14, 20:26, 20:26].all() and not got[18:].any() and not (got & ~sel).any()
    other = select_part(vol, whole, point=(c(30), c(22), c(22)), neck=2).mask.cpu().numpy()
    assert np.array_equal(other, E.neck(sel, (30, 22, 22), 2)) and not other[:24].any() and other[28:34, 20:26, 20:26].all()
    with pytest.raises(ValueError, match="thinner than"):
        select_part(vol, whole, point=(c(21), c(22), c(22)), neck=2)            # a pick on the neck itself
    with pytest.raises(ValueError, match="needs a point"):
        select_part(vol, whole, neck=2)


# ------------------------------------------------------------------------------------------------ 3. the feathered map
def _feather_regions(W):
    """keep and free shadows that overlap on planes 0 and 2; with `free` alone one plane pair stays as it is"""
    from ishapediting_amd.regions import Box, Sphere
    keep = [Box((-0.6, -0.5, -0.2), (0.1, 0.2, 0.3))]
    free = [Sphere((0.2, 0.1, 0.0), 0.35), Box((0.5, 0.6, -0.9), (0.8, 0.9, -0.7))]
    return keep, free


@pytest.mark.parametrize("falloff", [0.5, 1, 2.5, 8, 64])
@pytest.mark.parametrize("W", [33, 128])
def test_feathered_map_equals_the_float64_formula_bitwise(W, falloff):
    from ishapediting_amd.regions import plane_marks, plane_weights
    keep, free = _feather_regions(W)
    for k, f, dilate, kw, fw in ((keep, free, 0, 4.0, 0.0), (keep, None, 1, 2.5, 0.0), (None, free, 0, 4.0, 0.25)):       # one shadow empty
        marks = plane_marks(keep=k, free=f, W=W, dilate=dilate, device=dev()).cpu().numpy()
        got = plane_weights(keep=k, free=f, W=W, keep_weight=kw, free_weight=fw, dilate=dilate, device=dev(), falloff=falloff)
        assert got.dtype == torch.float32 and got.shape == (3, W, W)
        want = E.feather_ref(marks, kw, fw, falloff)
        got = got.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (W, falloff, np.argwhere(got != want)[:8].tolist())
        hard = plane_weights(keep=k, free=f, W=W, keep_weight=kw, free_weight=fw, dilate=dilate, device=dev()).cpu().numpy()
        assert np.array_equal(hard, E.hard_ref(marks, kw, fw))
        assert np.array_equal(got, hard) == (falloff <= 1)


@pytest.mark.parametrize("W", [33, 128])
def test_falloff_zero_is_todays_map_and_the_marks_are_the_hard_maps_marks(W):
    from ishapediting_amd.regions import Voxels, plane_marks, plane_weights
    keep, free = _feather_regions(W)
    D = 2 * W
    grid = np.zeros((D, D, D), bool)
    grid[D // 3:D // 2, D // 4:D // 2, D // 5:D // 3] = True
    free = free + [Voxels(T(grid))]
    for dilate in (0, 2):
        today = plane_weights(keep=keep, free=free, W=W, dilate=dilate, device=dev())
        assert torch.equal(plane_weights(keep=keep, free=free, W=W, dilate=dilate, device=dev(), falloff=0.0), today)
        # the marks, recomputed from hard maps: each region alone shows its whole shadow
        k_only = plane_weights(keep=keep, W=W, dilate=dilate, device=dev()) == 4.0
        f_only = plane_weights(free=free, W=W, dilate=dilate, device=dev()) == 0.0
        marks = plane_marks(keep=keep, free=free, W=W, dilate=dilate, device=dev())
        assert marks.dtype == torch.uint8 and torch.equal(marks, k_only.to(torch.uint8) | (f_only.to(torch.uint8) << 1))
        assert np.array_equal(today.cpu().numpy(), E.hard_ref(marks.cpu().numpy(), 4.0, 0.0))
    with pytest.raises(ValueError, match="falloff"):
        plane_weights(keep=keep, W=W, device=dev(), falloff=65)
    with pytest.raises(ValueError, match="empty shadow"):
        plane_weights(keep=keep, free=[Voxels(torch.zeros(D, D, D, dtype=torch.bool))], W=W, device=dev(), falloff=3)


# ------------------------------------------------------------------------------------------------ 4. through the edit, tiny model
def test_margin_and_falloff_through_training_on_the_tiny_model(gold):
    from ishapediting_amd.regions import grow, plane_weights
    from tests.test_gpu_parts import _finish, _part_and_motion, _same
    from tests.test_gpu_regions import _box, _tiny
    ds, g, dn, w_time = _tiny(gold)
    _, width = ds.model.tap_shape(ds.args.feat_layer)
    part, rigid = _part_and_motion()
    # margin
    base = _finish(ds, ds.training_part(part, rigid, handles=4, scale=50.0, cof=0.4))
    free0 = ds.part_plan.free
    assert _same(_finish(ds, ds.training_part(part, rigid, handles=4, scale=50.0, cof=0.4, margin=0)), base)
    assert ds.part_plan.free[0] is part and ds.part_plan.free[1] is ds.part_plan.moved
    grown = _finish(ds, ds.training_part(part, rigid, handles=4, scale=50.0, cof=0.4, margin=3))
    plan = ds.part_plan
    assert not torch.equal(grown[0], base[0])
    assert torch.equal(plan.moved.mask, free0[1].mask)                          # `moved` stays the ungrown region
    assert int(plan.free[0].mask.sum()) > int(part.mask.sum()) and torch.equal(plan.free[1].mask, grow(plan.moved, 3).mask)
    by_hand = _finish(ds, ds.training(plan.sources, plan.targets, scale=50.0, cof=0.4, free=[grow(part, 3), grow(plan.moved, 3)]))
    assert _same(grown, by_hand)
    # region_falloff
    plain = _finish(ds, ds.training(g["drag_sources"], g["drag_targets"], scale=50.0, cof=0.4, keep=[_box()]))
    assert _same(_finish(ds, ds.training(g["drag_sources"], g["drag_targets"], scale=50.0, cof=0.4, keep=[_box()], region_falloff=0)), plain)
    soft = _finish(ds, ds.training(g["drag_sources"], g["drag_targets"], scale=50.0, cof=0.4, keep=[_box()], region_falloff=4))
    assert not torch.equal(soft[0], plain[0])
    wmap = plane_weights(keep=[_box()], W=width, device=dev(), falloff=4)
    assert 1.0 < float(wmap[(wmap > 1.0) & (wmap < 4.0)].min()) and torch.equal(ds._dk.weights.reshape(-1), wmap.reshape(-1))
    assert _same(_finish(ds, ds.training(g["drag_sources"], g["drag_targets"], scale=50.0, cof=0.4, weights=wmap)), soft)
    # both through training_part
    both = _finish(ds, ds.training_part(part, rigid, handles=4, scale=50.0, cof=0.4, margin=3, region_falloff=4))
    assert not torch.equal(both[0], grown[0])
    wfree = plane_weights(free=ds.part_plan.free, W=width, device=dev(), falloff=4)
    assert _same(_finish(ds, ds.training(plan.sources, plan.targets, scale=50.0, cof=0.4, weights=wfree)), both)
    assert int(_lib.lib().ishap_device_status()) == 0


def test_a_feathered_edit_beside_a_plain_one_in_one_batch(gold):
    """The batched-drag criterion (tests/test_gpu_parts.py): at every step each edit's loss has the bits of a solo loss call,
    set up for that edit alone, on its slice of the step's tap."""
    from ishapediting_amd import drag_utils
    from ishapediting_amd.regions import plane_weights
    from tests.test_gpu_regions import _box, _tiny
    ds, g, dn, w_time = _tiny(gold, max_edits=2)
    ds.step_noise = lambda i: dn[w_time - 1 - i].repeat(2, 1, 1, 1)
    ch, width = ds.model.tap_shape(ds.args.feat_layer)
    src, tgt = g["drag_sources"], g["drag_targets"]
    solos = []
    for wmap in (plane_weights(keep=[_box()], W=width, device=dev(), falloff=4), None):
        dk = drag_utils.DragKernels(dev(), W=width, ld=ch, chmap=drag_utils.feat_channel_map(ch), r=ds.r1, voxel=ds.voxel_size, loss_type="l2")
        dk.setup(src, tgt, 0.4, weights=wmap)
        solos.append(dk)
    seen, inner = [], drag_utils.BatchDragKernels.loss_cotangent_ptr

    def spy(self, edit_ptr, orig_ptr, orig_stride=0, loss_out=None):
        assert orig_stride == 0
        solo = [dk.loss_grad_ptr(edit_ptr + 2 * e * width * width * ch, orig_ptr)[1].clone() for e, dk in enumerate(solos)]
        out = inner(self, edit_ptr, orig_ptr, orig_stride=orig_stride, loss_out=loss_out)
        seen.append((torch.cat(solo), loss_out.clone()))
        return out
    drag_utils.BatchDragKernels.loss_cotangent_ptr = spy
    try:
        list(ds.training_batch([src, src], [tgt, tgt], scale=50.0, cof=0.4, keep=[[_box()], None], region_falloff=[4, 0]))
    finally:
        drag_utils.BatchDragKernels.loss_cotangent_ptr = inner
    torch.cuda.synchronize()
    assert len(seen) == w_time
    for step, (solo, batch) in enumerate(seen):
        assert torch.equal(solo, batch), (step, solo.tolist(), batch.tolist())
    assert not torch.equal(seen[-1][1][0], seen[-1][1][1])                      # the feathered map is in use
    with pytest.raises(ValueError, match="region_falloff"):
        list(ds.training_batch([src, src], [tgt, tgt], scale=50.0, cof=0.4, keep=[[_box()], None], region_falloff=[4, 0, 0]))
    assert int(_lib.lib().ishap_device_status()) == 0
