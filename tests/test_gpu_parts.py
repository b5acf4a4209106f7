"""Part edits on the device (csrc/parts.hip, regions.select_part / sample_handles / transform_region / plan_part_edit,
DragStuff.training_part) against tests/parts_ref.py.  Everything is integers or float64 in one stated operation order, so every
comparison is exact: masks byte for byte, picks and squared distances equal, no tolerance anywhere.  For the general rotations
tests/test_parts_host.py asserts that no source index lies within 1e-9 of a rounding tie.  Volumes are analytic."""
import numpy as np
import pytest
import torch

from ishapediting_amd import _lib
from tests import parts_ref as P

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _vox(mask):
    from ishapediting_amd.regions import Voxels
    return Voxels(T(np.ascontiguousarray(mask)).to(dev()) != 0)


def _product(prims):
    from ishapediting_amd.regions import Box, Sphere
    return [Box(p[1], p[2]) if p[0] == "box" else Sphere(p[1], p[2]) for p in prims]


def _bytes(v):
    return v.mask.to(torch.uint8).cpu().numpy()


# ------------------------------------------------------------------------------------------------ (a) select
def _ball_volume(D):
    c = P.centres(D)
    x, y, z = c[:, None, None], c[None, :, None], c[None, None, :]
    return (0.7 - np.sqrt(x * x + y * y + z * z)).astype(np.float32)


@pytest.mark.parametrize("D", P.SIZES)
def test_select_is_the_reference_byte_for_byte(D):
    from ishapediting_amd.regions import select_part
    c = P.centres(D)
    box = ("box", (c[1], c[2], c[D // 4]), (c[D - 3], c[D // 2], c[D - 2]))          # every face passes through voxel centres
    sphere = ("sphere", (0.3, -0.35, 0.05), 0.45)
    grid = np.zeros((D, D, D), np.uint8)
    grid[: D // 3, :, D // 2:] = 1
    grid[D - 1, D - 1, D - 1] = 1
    for vol, levels in ((P.l_volume(D), (0.0, 0.5, -1.5)), (_ball_volume(D), (0.0, 0.13, -0.2))):
        v = T(vol).to(dev())
        for level in levels:
            for prims, g in (([box], None), ([sphere], None), ([], grid), ([box, sphere], grid), ([sphere, box], None)):
                want = P.select_ref(vol, level, prims, g)
                within = _product(prims) + ([_vox(g)] if g is not None else [])
                if not want.any():
                    with pytest.raises(ValueError, match="selection is empty"):
                        select_part(v, within, level=level)
                    continue
                got = select_part(v, within, level=level)
                assert got.mask.device.type == "cuda" and got.mask.dtype == torch.bool
                assert np.array_equal(_bytes(got), want), (D, level, prims, np.argwhere(_bytes(got) != want)[:6].tolist())
    # the box's inclusive faces are really in play: the reference differs when the box shrinks by a hair
    vol = np.ones((D, D, D), np.float32)
    full = P.select_ref(vol, 0.0, [box])
    shrunk = ("box", tuple(np.nextafter(box[1], 2.0)), tuple(np.nextafter(box[2], -2.0)))
    assert P.select_ref(vol, 0.0, [shrunk]).sum() < full.sum()
    assert np.array_equal(_bytes(select_part(T(vol).to(dev()), _product([box]))), full)
    assert np.array_equal(_bytes(select_part(T(vol).to(dev()), _product([shrunk]))), P.select_ref(vol, 0.0, [shrunk]))


def test_select_with_a_point_keeps_one_connected_piece():
    from ishapediting_amd.regions import Box, select_part
    D = 33
    vol = P.two_blobs_volume(D)
    v = T(vol).to(dev())
    everything = Box((-1, -1, -1), (1, 1, 1))
    c = P.centres(D)
    left, right = (vol > 0) & (c[:, None, None] < 0), (vol > 0) & (c[:, None, None] > 0)
    assert left.any() and right.any()
    assert np.array_equal(_bytes(select_part(v, everything)), (vol > 0).astype(np.uint8))
    assert np.array_equal(_bytes(select_part(v, everything, point=(-0.5, 0.1, 0.0))) != 0, left)
    assert np.array_equal(_bytes(select_part(v, everything, point=(0.6, -0.2, 0.3), connectivity=26)) != 0, right)
    with pytest.raises(ValueError, match="not in the selection"):
        select_part(v, everything, point=(0.0, 0.0, 0.0))
    # a region that cuts a blob in two: the point picks the half it lies in
    half = Box((-1, 0.05, -1), (1, 1, 1))
    both = P.select_ref(vol, 0.0, [("box", half.lo, half.hi)]) != 0
    assert np.array_equal(_bytes(select_part(v, half, point=(0.5, 0.3, 0.0))) != 0, both & right)
    with pytest.raises(ValueError, match="not in the selection"):
        select_part(v, half, point=(0.5, -0.3, 0.0))                   # in the shape, outside the region
    with pytest.raises(ValueError, match="selection is empty"):
        select_part(v, Box((-0.1, -0.1, -0.1), (0.1, 0.1, 0.1)))


# ------------------------------------------------------------------------------------------------ (b) handles
def _raw(mask, n, start=None):
    """the kernels' own output on the host: (picks int64 [n, 3], dist2 int64 [n], M)"""
    from ishapediting_amd.regions import handle_voxels
    picks, tail = handle_voxels(mask if not isinstance(mask, np.ndarray) else _vox(mask), n, start)
    t = tail.cpu().numpy()
    return picks.cpu().numpy().astype(np.int64), t[:n].view(np.uint32).astype(np.int64), int(t[n])


def _check_handles(mask, D, n, start=None):
    want = P.fps_ref(P.candidates(mask), D, n, start)
    got = _raw(mask, n, start)
    assert got[2] == want[2], (got[2], want[2])
    assert np.array_equal(got[0], want[0]), (D, n, start, got[0][:5].tolist(), want[0][:5].tolist())
    assert np.array_equal(got[1], want[1]), (D, n, start, got[1][:5].tolist(), want[1][:5].tolist())
    return got


@pytest.mark.parametrize("M", [1, 2047, 2048, 2049])
def test_handles_either_side_of_a_scan_block(M):
    D = 16
    for mask in (P.first_voxels_mask(D, M), P.scattered_mask(D, M, M)):
        for n in (1, 2, 17):
            for start in (None, (15, 0, 9), tuple(int(v) for v in P.candidates(mask)[M // 2])):
                got = _check_handles(mask, D, n, start)
                assert (got[0][min(n, M):] == -1).all()               # rounds beyond M
    if M in (1, 2049):
        _check_handles(P.first_voxels_mask(D, M), D, M)               # n = M: every voxel is picked once
        _check_handles(P.first_voxels_mask(D, M), D, M + 1)           # and the round after writes (-1, -1, -1)


def test_handles_across_many_workgroups():
    D, M = 64, 40000
    mask = P.scattered_mask(D, M, 7)
    for n, start in ((17, None), (17, (0, 63, 31)), (2, None)):
        assert _check_handles(mask, D, n, start)[2] == M
    solid = (P.l_volume(D) > 0).astype(np.uint8)
    assert _check_handles(solid, D, 17)[2] == int(solid.sum())


def test_handles_ties_go_to_the_lowest_index():
    for D, mask in ((9, P.cube_mask(9, 0, 9)), (9, P.cube_mask(9, 2, 7)), (9, P.cross_mask(9, 3)), (33, P.cross_mask(33, 12))):
        M = int(mask.sum())
        for n in (1, 2, 17, M if M <= 100 else 64):
            _check_handles(mask, D, n)
            _check_handles(mask, D, n, (D // 2, D // 2, D // 2))       # the centre: every symmetric voxel ties
            _check_handles(mask, D, n, (0, D - 1, 0))                  # outside the part


def test_handles_far_corner_of_the_largest_grid():
    """D = 1024: linear indices just below 2^30 in the low half of the key.  The mask is 1 GiB of zeros with a handful of set
    voxels at its far end, made and kept on the device."""
    from ishapediting_amd.regions import Voxels
    D = 1024
    coords = np.array([[1023, 1023, 1023], [1023, 1023, 1000], [1023, 1000, 1023], [1000, 1023, 1023], [1023, 1022, 1023],
                       [1011, 1011, 1011], [1000, 1000, 1000]], np.int64)
    coords = coords[np.argsort(P._lin(coords, D))]
    mask = torch.zeros((D, D, D), dtype=torch.bool, device=dev())
    mask[tuple(T(coords).to(dev()).T)] = True
    part = Voxels(mask)
    for n, start in ((7, None), (8, (1023, 1023, 1023)), (3, (0, 0, 0))):
        want, got = P.fps_ref(coords, D, n, start), _raw(part, n, start)
        assert got[2] == want[2] == 7 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, start, got, want)
    del part, mask
    torch.cuda.empty_cache()


def test_sample_handles_points_spacing_repeat_and_refusal():
    from ishapediting_amd.regions import sample_handles
    D = 33
    mask = (P.l_volume(D) > 0).astype(np.uint8)
    part = _vox(mask)
    for n, start, start_vox in ((16, None, None), (5, (0.9, 0.9, 0.9), (31, 31, 31)), (1, None, None)):
        picks, d2, _ = P.fps_ref(P.candidates(mask), D, n, start_vox)
        h = sample_handles(part, n, start=start)
        assert h.points.device.type == "cuda" and h.points.dtype == torch.float32 and h.voxels.dtype == torch.int32
        assert np.array_equal(h.voxels.cpu().numpy(), picks)
        assert np.array_equal(h.points.cpu().numpy().view(np.uint32), P.handle_points(picks, D).view(np.uint32))
        assert h.spacing == float(np.sqrt(float(d2[n - 1])) * 2.0 / (D - 1))
        if n > 1:
            assert d2[n - 1] == P.min_pairwise_dist2(picks)
        again = sample_handles(part, n, start=start)
        assert torch.equal(again.voxels, h.voxels) and torch.equal(again.points, h.points) and again.spacing == h.spacing
    small = _vox(P.first_voxels_mask(16, 40))
    with pytest.raises(ValueError, match="41 handles asked of a part of 40 voxels"):
        sample_handles(small, 41)
    assert sample_handles(small, 40).voxels.shape == (40, 3)
    with pytest.raises(ValueError, match="1..4096"):
        sample_handles(small, 0)
    with pytest.raises(ValueError, match="outside"):
        sample_handles(small, 2, start=(1.5, 0.0, 0.0))


# ------------------------------------------------------------------------------------------------ (c) transform
@pytest.mark.parametrize("D", P.SIZES)
def test_transform_is_the_reference_byte_for_byte(D):
    from ishapediting_amd.regions import Rigid, transform_region
    mask = (P.l_volume(D) > 0).astype(np.uint8)
    part = _vox(mask)
    h = 2.0 / (D - 1)
    cases = [Rigid(), Rigid(pivot=(0.3, -0.2, 0.1))]
    cases += [Rigid(rotation=(axis, 90.0 * k)) for axis in ((0, 0, 1), (1, 0, 0), (0, -1, 0)) for k in (1, 2, 3)]
    cases += [Rigid(translation=(3 * h, 0.0, -2 * h)), Rigid(translation=(0.0, (D // 2) * h, 0.0))]      # the second leaves the cube in part
    cases += [Rigid(rotation=(axis, deg), pivot=pivot, translation=t) for axis, deg, pivot, t in P.GENERAL]
    for k, g in enumerate(cases):
        want = P.transform_ref(mask, g.matrix, g.pivot, g.translation)
        got = _bytes(transform_region(part, g))
        assert want.any() and np.array_equal(got, want), (D, k, np.argwhere(got != want)[:6].tolist())
    assert np.array_equal(_bytes(transform_region(part, cases[0])), mask)
    assert np.array_equal(_bytes(transform_region(part, cases[2])), np.rot90(mask, 1, axes=(0, 1)))
    cut = _bytes(transform_region(part, cases[12]))
    assert 0 < cut.sum() < mask.sum()
    with pytest.raises(ValueError, match="moved region is empty"):
        transform_region(part, Rigid(translation=(0.0, 0.0, 2.5)))


def test_plan_part_edit_is_the_reference_plan():
    from ishapediting_amd.regions import Rigid, plan_part_edit
    D = 33
    mask = (P.l_volume(D) > 0).astype(np.uint8)
    part = _vox(mask)
    g = Rigid(rotation=((0, 0, 1), 25.0), pivot=(-0.4, -0.4, 0.0), translation=(0.03, 0.0, 0.02))
    for n, start, sv in ((16, None, None), (6, (-0.4, 0.7, 0.0), (10, 27, 16))):
        src, tgt, moved, spacing = P.plan_ref(mask, g.matrix, g.pivot, g.translation, n, sv)
        plan = plan_part_edit(part, g, handles=n, start=start)
        assert plan.sources.dtype == plan.targets.dtype == np.float32
        assert np.array_equal(plan.sources.view(np.uint32), src.view(np.uint32)) and np.array_equal(plan.targets.view(np.uint32), tgt.view(np.uint32))
        assert plan.spacing == spacing and plan.free[0] is part and plan.free[1] is plan.moved
        assert np.array_equal(_bytes(plan.moved), moved)
    with pytest.raises(ValueError, match=r"handle \d+ at .* outside \[-1, 1\]\^3"):
        plan_part_edit(part, Rigid(translation=(0.0, 0.5, 0.0)))
    with pytest.raises(ValueError, match="handles asked of a part of"):
        plan_part_edit(_vox(P.first_voxels_mask(16, 10)), Rigid(), handles=11)


# ------------------------------------------------------------------------------------------------ end to end, tiny model
def _part_and_motion():
    """A box-shaped part on a 32^3 grid (the tiny model's tap is 16 wide: D >= W) and a motion that keeps it in the cube"""
    from ishapediting_amd.regions import Rigid
    D = 32
    c = P.centres(D)
    x, y, z = c[:, None, None], c[None, :, None], c[None, None, :]
    mask = ((x >= -0.7) & (x <= -0.1) & (y >= -0.6) & (y <= 0.2) & (z >= -0.3) & (z <= 0.3)).astype(np.uint8)
    return _vox(mask), Rigid(rotation=((0, 0, 1), 20.0), pivot=(-0.4, -0.6, 0.0), translation=(0.05, 0.0, 0.03))


def _finish(ds, gen):
    prog = list(gen)
    torch.cuda.synchronize()
    assert len(prog) == len(ds.last_losses) > 0
    return ds.tri_feat.clone(), [l.clone() for l in ds.last_losses]


def _same(a, b):
    return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_training_part_is_training_with_the_plan(gold):
    """The tiny model's latent has 6 channels, which the triplane decoder cannot take, so `_tiny` stubs the decode: the final
    latent (of which a volume is a pure function) and every step's loss are what is compared, bit for bit."""
    from tests.test_gpu_regions import _tiny
    ds, g, dn, w_time = _tiny(gold)
    part, rigid = _part_and_motion()
    _, width = ds.model.tap_shape(ds.args.feat_layer)
    assert part.D >= width
    planned = _finish(ds, ds.training_part(part, rigid, handles=4, scale=50.0, cof=0.4))
    plan = ds.part_plan
    assert plan.sources.shape == plan.targets.shape == (4, 3) and plan.free[0] is part and plan.spacing > 0
    assert ds._dk.weights is not None and float(ds._dk.weights.min()) == 0.0 and float(ds._dk.weights.max()) == 1.0
    by_hand = _finish(ds, ds.training(sources=plan.sources, targets=plan.targets, scale=50.0, cof=0.4, free=plan.free))
    assert _same(planned, by_hand)
    assert _same(_finish(ds, ds.training_part(part, rigid, handles=4, scale=50.0, cof=0.4)), planned)        # repeatable
    plain = _finish(ds, ds.training(plan.sources, plan.targets, scale=50.0, cof=0.4))
    assert not torch.equal(plain[0], planned[0]) and not torch.equal(plain[1][-1], planned[1][-1])           # the free regions count
    # keep passes through; handles and start change the plan
    kept = _finish(ds, ds.training_part(part, rigid, handles=4, scale=50.0, cof=0.4, keep=[_box_far()]))
    assert not torch.equal(kept[0], planned[0])
    other = _finish(ds, ds.training_part(part, rigid, handles=5, start=(-0.4, -0.2, 0.0), scale=50.0, cof=0.4))
    assert ds.part_plan.sources.shape == (5, 3) and not torch.equal(other[0], planned[0])
    with pytest.raises(ValueError, match="cof"):
        list(ds.training_part(part, rigid, handles=4, scale=50.0, cof=0.0))
    assert int(_lib.lib().ishap_device_status()) == 0


def _box_far():
    from ishapediting_amd.regions import Box
    return Box((0.4, 0.4, 0.4), (0.9, 0.9, 0.9))


def test_a_planned_edit_beside_a_plain_one_in_one_batch(gold):
    """training_batch takes the plan's arrays and regions per edit.  At EVERY step of the loop each edit's loss has the bits of
    the solo loss call (a DragKernels set up for that edit alone: the plan's handles and free regions for the planned one, no
    map for the plain one) on that edit's slice of the step's tap and guidance.
    What is NOT compared is the batch's loss sequence against a separate solo loop, or against a batch with another neighbour:
    the UNet's forward and backward at batch 2 differ from batch 1 in the last bits and the batch shares one fp16 loss scale
    (tests/test_gpu_batched_drag.py, LOOP_BOUND), so two loops see different taps from the second step on -- measured here:
    step 0 equal bit for bit, then -2.879305 against -2.879113 (planned) and -11.395764 against -11.393325 (plain, last step)."""
    from ishapediting_amd import drag_utils
    from ishapediting_amd.regions import plan_part_edit, plane_weights
    from tests.test_gpu_regions import _tiny
    ds, g, dn, w_time = _tiny(gold, max_edits=2)
    ds.step_noise = lambda i: dn[w_time - 1 - i].repeat(2, 1, 1, 1)
    part, rigid = _part_and_motion()
    plan = plan_part_edit(part, rigid, handles=4)
    ch, width = ds.model.tap_shape(ds.args.feat_layer)
    edits = [(plan.sources, plan.targets, plane_weights(free=plan.free, W=width, device=dev())), (g["drag_sources"], g["drag_targets"], None)]
    solos = []
    for src, tgt, wmap in edits:
        dk = drag_utils.DragKernels(dev(), W=width, ld=ch, chmap=drag_utils.feat_channel_map(ch), r=ds.r1, voxel=ds.voxel_size, loss_type="l2")
        dk.setup(src, tgt, 0.4, weights=wmap)
        solos.append(dk)
    seen, inner = [], drag_utils.BatchDragKernels.loss_cotangent_ptr

    def spy(self, edit_ptr, orig_ptr, orig_stride=0, loss_out=None):
        assert orig_stride == 0                                                 # variants of one shape share the guidance tap
        solo = [dk.loss_grad_ptr(edit_ptr + 2 * e * width * width * ch, orig_ptr)[1].clone() for e, dk in enumerate(solos)]
        out = inner(self, edit_ptr, orig_ptr, orig_stride=orig_stride, loss_out=loss_out)
        seen.append((torch.cat(solo), loss_out.clone()))
        return out

    def run(sources, targets, free):
        list(ds.training_batch(sources, targets, scale=50.0, cof=0.4, free=free))
        torch.cuda.synchronize()
        return ds.tri_feat_batch.clone(), torch.stack(ds.last_losses).clone()
    drag_utils.BatchDragKernels.loss_cotangent_ptr = spy
    try:
        mixed, mixed_losses = run([plan.sources, g["drag_sources"]], [plan.targets, g["drag_targets"]], [plan.free, None])
    finally:
        drag_utils.BatchDragKernels.loss_cotangent_ptr = inner
    assert len(seen) == w_time and mixed_losses.shape == (w_time, 2)
    for step, (solo, batch) in enumerate(seen):
        print(f"step {step}: solo {solo.tolist()} batch {batch.tolist()}")
        assert torch.equal(solo, batch), (step, solo.tolist(), batch.tolist())
    assert float(ds._dk_batch.weights[0].min()) == 0.0 and float(ds._dk_batch.weights[1].min()) == 1.0       # only edit 0 has regions
    assert bool(torch.isfinite(mixed).all()) and not torch.equal(mixed[0], mixed[1])
    again, again_losses = run([plan.sources, g["drag_sources"]], [plan.targets, g["drag_targets"]], [plan.free, None])
    assert torch.equal(again, mixed) and torch.equal(again_losses, mixed_losses)                              # repeatable
    assert int(_lib.lib().ishap_device_status()) == 0
