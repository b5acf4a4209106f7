"""Region-constrained drag edits, the part that needs no GPU: the conditions the inputs of tests/test_gpu_regions.py must meet,
the weighted oracles against the unweighted ones of tests/drag_ref.py, the numpy shadows, the argument validation of
ishapediting_amd.regions and of the new keywords of the drag calls, and the ctypes structs against the header."""
import ctypes as C
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ishapediting_amd import _lib, regions
from ishapediting_amd import drag_utils as du
from tests import drag_ref as R
from tests import regions_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("name", G.CASES)
def test_weight_maps_meet_their_conditions(name):
    c = R.make_case(name)
    w = G.weight_map(name)
    assert w.shape == (3, c.W, c.W) and w.dtype == np.float32 and set(np.unique(w)) <= set(G.WEIGHT_VALUES)
    assert not np.array_equal(w[0], w[1]) and not np.array_equal(w[1], w[2]) and not np.array_equal(w[0], w[2])
    untouched = np.stack([m.numpy() for m in G.oracle(name, "l2").setup.masks])
    assert (untouched & (w == 0)).any(), "an untouched texel at weight 0"
    assert (untouched & (w > 1)).any(), "an untouched texel held harder"
    assert (~untouched & (w != 1)).any(), "non-unit weights on touched texels"


@pytest.mark.parametrize("combo", G.COMBOS, ids=lambda c: f"{c[0]}-{c[1]}")
def test_weights_on_touched_texels_have_no_effect_and_the_others_do(combo):
    name, lt = combo
    c = R.make_case(name)
    w = G.weight_map(name)
    untouched = np.stack([m.numpy() for m in G.oracle(name, lt).setup.masks])
    res = G.oracle(name, lt)
    other = np.where(untouched, w, np.float32(7.0)).astype(np.float32)          # another value on every touched texel
    again = G.drag_loss_grad64_weighted(*G._args(name, lt, other))
    assert again.loss == res.loss and torch.equal(again.grad, res.grad)
    plain = R.oracle(name, lt, G.COF)
    assert plain.loss != res.loss and not torch.equal(plain.grad, res.grad)
    z = G.structural_zero(name)
    for key in ("unmapped", "touched", "freed"):
        # case A's lattices overlap so far that every touched texel lies under a target footprint; every other case has all three
        assert z[key].any() or (name, key) == ("A", "touched"), (name, key)
        assert bool((res.grad[torch.from_numpy(z[key])] == 0).all()), (name, key)
    assert not z["freed"][:, :].all() and bool((plain.grad[torch.from_numpy(z["freed"])] != 0).any())     # freed: zero only with the map


@pytest.mark.parametrize("name", ["A", "H"])
@pytest.mark.parametrize("lt", ["l2", "l1"])
@pytest.mark.parametrize("cof", [0.0, 0.4])
def test_weighted_oracles_with_ones_are_the_unweighted_ones(name, lt, cof):
    c = R.make_case(name)
    ones = np.ones((3, c.W, c.W), np.float32)
    a = (c.edit, c.orig, c.chmap, c.sources, c.targets, c.r, c.voxel, c.W, cof, lt)
    r64, w64 = R.drag_loss_grad64(*a), G.drag_loss_grad64_weighted(*a, ones)
    assert w64.loss == r64.loss and torch.equal(w64.grad, r64.grad) and w64.nmask == r64.nmask and torch.equal(w64.d, r64.d)
    (l32, g32), (lw, gw) = R.drag_loss_grad32(*a), G.drag_loss_grad32_weighted(*a, ones)
    assert lw == l32 and torch.equal(gw, g32)


@pytest.mark.parametrize("name", [c for c, lt in G.COMBOS if lt == "l1"])
def test_l1_cases_exclude_few_elements(name):
    c = R.make_case(name)
    res = G.oracle(name, "l1")
    amb = R.l1_ambiguous_elements(res, c.edit, c.orig, c.chmap, c.W)
    nonzero = int((res.grad != 0).sum())
    assert nonzero > 0 and int((amb & (res.grad != 0)).sum()) <= R.L1_EXCLUDED_CAP * nonzero


# ------------------------------------------------------------------------------------------------ shadows
def test_voxel_rasterisation_of_a_texel_aligned_box_gives_the_boxs_shadow():
    """D = 2 W - 1: every second voxel sits on a texel centre.  The voxels of the box [t3, t9] x [t2, t5] x [t6, t12] (texel
    centres, +- a quarter voxel) rasterised as a grid give the shadow of the box."""
    W = 16
    D = 2 * W - 1
    t, x = G.texel_centres(W), np.linspace(-1, 1, D)
    q = 0.25 * (x[1] - x[0])
    lo, hi = np.array([t[3], t[2], t[6]]) - q, np.array([t[9], t[5], t[12]]) + q
    gx, gy, gz = np.meshgrid(x, x, x, indexing="ij")
    grid = (gx >= lo[0]) & (gx <= hi[0]) & (gy >= lo[1]) & (gy <= hi[1]) & (gz >= lo[2]) & (gz <= hi[2])
    box = G.shadow_ref([("box", lo, hi)], W)
    assert box[0].sum() == 7 * 4 and box[1].sum() == 4 * 7 and box[2].sum() == 7 * 7
    assert box[0][2:6, 3:10].all() and box[1][6:13, 2:6].all() and box[2][6:13, 3:10].all()      # [row, col]
    # a voxel midway between two texel centres goes to one of them: shrink the grid to the on-centre voxels' hull first
    assert np.array_equal(G.shadow_ref([("voxels", grid)], W), box)


def test_keep_overrides_free_and_dilation_clips_at_the_border():
    W = 16
    keep, free = [("box", (-0.5, -0.5, -0.5), (0.1, 0.1, 0.1))], [("box", (-0.1, -0.1, -0.1), (0.6, 0.6, 0.6))]
    w = G.plane_weights_ref(keep, free, W, 4.0, 0.25)
    sk, sf = G.shadow_ref(keep, W), G.shadow_ref(free, W)
    assert (sk & sf).any() and (w[sk] == 4.0).all() and (w[sf & ~sk] == 0.25).all() and (w[~sk & ~sf] == 1.0).all()
    corner = [("box", (-1.01, -1.01, -1.01), (-0.99, -0.99, -0.99))]               # the texel (0, 0) of every plane
    s = G.shadow_ref(corner, W)
    assert s.sum() == 3 and s[:, 0, 0].all()
    d2 = G.dilate_ref(s, 2)
    assert d2.sum() == 3 * 9 and d2[:, :3, :3].all()                                # clipped: 3 x 3, not 5 x 5
    far = G.dilate_ref(G.shadow_ref([("box", (0.99, 0.99, 0.99), (1.5, 1.5, 1.5))], W), 1)
    assert far.sum() == 3 * 4 and far[:, -2:, -2:].all()


def test_an_empty_shadow_raises():
    W = 16
    thin = [("box", (0.01, 0.01, 0.01), (0.03, 0.03, 0.03))]                        # inside one texel cell on every axis
    assert not G.shadow_ref(thin, W).any()
    with pytest.raises(ValueError, match="empty shadow"):
        G.plane_weights_ref(thin, None, W)
    with pytest.raises(ValueError, match="empty shadow"):
        G.plane_weights_ref(None, [("sphere", (3.0, 3.0, 3.0), 0.5)], W)            # outside the cube
    flat = [("box", (0.01, -0.5, -0.5), (0.03, 0.5, 0.5))]                          # thin along x only: a shadow on plane yz
    s = G.shadow_ref(flat, W)
    assert not s[0].any() and s[1].any() and not s[2].any()
    G.plane_weights_ref(flat, None, W)


@pytest.mark.parametrize("size", G.MAP_SIZES, ids=lambda s: f"D{s[0]}-W{s[1]}")
def test_device_map_cases_meet_their_conditions(size):
    D, W = size
    keep, free = G.map_regions(D, "both")
    assert G.boundary_distance(keep, W) >= G.BOUNDARY_MARGIN and G.boundary_distance(free, W) >= G.BOUNDARY_MARGIN
    box, cell = keep[0], keep[1]
    assert min(box[1]) < -1 and max(box[2]) > 1 and G.shadow_ref([box], W).any()                  # sticks out, still has a shadow
    assert not G.shadow_ref([cell], W).any()                                                       # wholly inside one texel cell
    ball, thin = free[0], free[1]
    assert ball[1][0] + ball[2] > 1 and G.shadow_ref([ball], W).any()
    s = G.shadow_ref([thin], W)
    assert s[1].any() and not s[0].any() and not s[2].any()                                        # thinner than a texel along x only
    kg, fg = keep[2][1], free[2][1]
    assert kg.sum() == 8 + D and fg.sum() == 2 * D and all(kg[i, j, k] for i in (0, -1) for j in (0, -1) for k in (0, -1))
    sk, sf = G.shadow_ref(keep, W), G.shadow_ref(free, W)
    assert (sk & sf).any() and (sf & ~sk).any()                                                    # keep overrides free somewhere
    assert sk[:, 0, 0].all() and sk[:, -1, -1].all()                                               # the corners of every plane
    w = G.plane_weights_ref(keep, free, W, 2.5, 0.5, 2)
    assert set(np.unique(w)) == {0.5, 1.0, 2.5}


# ------------------------------------------------------------------------------------------------ argument validation
def test_region_classes_validate():
    with pytest.raises(ValueError):
        regions.Box((0, 0, 0), (1, -1, 1))
    with pytest.raises(ValueError):
        regions.Box((0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        regions.Sphere((0, 0, 0), -0.1)
    with pytest.raises(ValueError):
        regions.Sphere((0, 0, float("nan")), 0.1)
    with pytest.raises(ValueError):
        regions.Voxels(torch.zeros(4, 4, 5, dtype=torch.bool))
    v = regions.Voxels(np.ones((4, 4, 4), np.uint8))
    assert v.D == 4 and v.mask.dtype == torch.bool
    b = regions.Box([-1, -1, -1], np.ones(3))
    assert b.lo == (-1.0, -1.0, -1.0) and b.hi == (1.0, 1.0, 1.0)


def test_plane_weights_validates_before_it_touches_the_device():
    box = regions.Box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="D = 8 < W = 16"):
        regions.plane_weights(keep=[regions.Voxels(torch.ones(8, 8, 8, dtype=torch.bool))], W=16)
    with pytest.raises(ValueError, match="W"):
        regions.plane_weights(keep=[box], W=1)
    with pytest.raises(ValueError, match="W"):
        regions.plane_weights(keep=[box])
    with pytest.raises(ValueError, match="keep_weight"):
        regions.plane_weights(keep=[box], W=16, keep_weight=float("inf"))
    with pytest.raises(ValueError, match="free_weight"):
        regions.plane_weights(free=[box], W=16, free_weight=-1.0)
    with pytest.raises(ValueError, match="dilate"):
        regions.plane_weights(keep=[box], W=16, dilate=-1)
    with pytest.raises(ValueError, match="a region is"):
        regions.plane_weights(keep=[(0, 0, 0)], W=16)


def test_the_abi_refuses_bad_arguments_without_a_launch():
    """ishap_region_plane_weights returns an error code for D < W, W < 2, a negative dilate, non-finite or negative weights (the
    checks come before any pointer is used, so this runs without a GPU)."""
    L = _lib.lib()
    call = lambda D, W, dil, kw, fw, grid=1: L.ishap_region_plane_weights(None, 0, grid or None, None, D, W, dil, kw, fw, 64, None,   # noqa: E731
                                                                           64, 1 << 20, None)
    assert call(8, 16, 0, 4.0, 0.0) != 0 and b"D" in L.ishap_last_error()
    assert call(16, 1, 0, 4.0, 0.0) != 0
    assert call(16, 16, -1, 4.0, 0.0) != 0 and b"dilate" in L.ishap_last_error()
    assert call(16, 16, 0, float("nan"), 0.0) != 0
    assert call(16, 16, 0, float("inf"), 0.0) != 0
    assert call(16, 16, 0, 4.0, -0.5) != 0 and b"weight" in L.ishap_last_error()
    assert L.ishap_region_plane_weights_scratch_bytes(1) < 0 and L.ishap_region_plane_weights_scratch_bytes(64) >= 3 * 64 * 64


def test_drag_keywords_validate():
    W = 16
    ones = np.ones((3, W, W), np.float32)
    box = regions.Box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    stub = SimpleNamespace(device=torch.device("cpu"))
    rw = lambda **k: du.DragStuff._region_weights(stub, W, k.pop("cof", 0.2), k.pop("keep", None), k.pop("free", None), 4.0, 0.0,   # noqa: E731
                                                  0, k.pop("weights", None))
    assert rw() is None
    assert torch.equal(rw(weights=ones), torch.ones(3, W, W))
    for cof in (0.0, -1.0):                                          # regions with no preservation term
        with pytest.raises(ValueError, match="cof"):
            rw(cof=cof, keep=[box])
        with pytest.raises(ValueError, match="cof"):
            rw(cof=cof, weights=ones)
    with pytest.raises(ValueError, match="not both"):
        rw(weights=ones, keep=[box])
    with pytest.raises(ValueError, match="not both"):
        rw(weights=ones, free=box)
    with pytest.raises(ValueError, match=r"\[3, 16, 16\]"):
        rw(weights=np.ones((3, 8, 8), np.float32))
    with pytest.raises(ValueError, match="finite"):
        rw(weights=-ones)
    # the kernels objects: checked before any device call
    with pytest.raises(ValueError, match="cof"):
        du.DragKernels.setup(SimpleNamespace(W=W), None, None, 0.0, weights=ones)
    # a list of the wrong length, in training_batch's keywords and in BatchDragKernels.setup
    with pytest.raises(ValueError, match="3 entries for 2 edits"):
        du.per_edit_region([None, [box], None], 2, "keep")
    assert du.per_edit_region(None, 2, "keep") == [None, None] and du.per_edit_region(box, 2, "keep") == [box, box]
    assert du.per_edit_region([None, [box]], 2, "keep") == [None, [box]]
    with pytest.raises(ValueError, match="2 values for 3 edits"):
        du.per_edit_any([0, 1], 3, "region_dilate")


def test_training_signatures_carry_the_region_keywords():
    import inspect
    for fn in (du.DragStuff.training, du.DragStuff.training_batch):
        p = inspect.signature(fn).parameters
        assert [p[k].default for k in ("keep", "free", "keep_weight", "free_weight", "region_dilate", "weights")] == \
            [None, None, 4.0, 0.0, 0, None]
        assert p["cof"].default == 0.2 and p["scale"].default == 600
    assert inspect.signature(du.DragKernels.setup).parameters["weights"].default is None
    assert inspect.signature(du.BatchDragKernels.setup).parameters["weights"].default is None


def test_marker_box_is_twelve_closed_outward_prisms():
    from ishapediting_amd.render import edit_parts, marker_box
    v, t = marker_box((-0.5, -0.2, 0.0), (0.5, 0.3, 0.4))
    assert v.shape == (96, 3) and t.shape == (144, 3) and v.dtype == np.float32 and t.dtype == np.int32
    for k in range(12):
        vv, tt = v[8 * k:8 * k + 8].astype(np.float64), t[12 * k:12 * k + 12] - 8 * k
        assert tt.min() == 0 and tt.max() == 7
        assert sum(np.dot(vv[a], np.cross(vv[b], vv[c])) for a, b, c in tt) > 0            # positive volume: outward, closed
    assert abs(v[:, 0].min() + 0.506) < 1e-6 and abs(v[:, 2].max() - 0.406) < 1e-6
    parts = edit_parts((np.zeros((3, 3), np.float32), np.zeros((1, 3), np.int32)), [[0, 0, 0]], [[0, 0.1, 0]], boxes=[(v, t)])
    assert len(parts) == 5 and parts[-1][0][0] is v


# ------------------------------------------------------------------------------------------------ the structs
def test_ctypes_structs_have_the_headers_sizes(tmp_path):
    """A host program that includes include/ishap.h prints the sizes and the offsets of the new fields."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc")
                if c and shutil.which(c)), None)
    assert cxx, "no C++ compiler found"
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "ishap.h"\nint main() { std::printf("%zu %zu %zu %zu\\n", '
                   "sizeof(ishap_drag_batch_args), sizeof(ishap_region_prim), "
                   "offsetof(ishap_drag_batch_args, weights), offsetof(ishap_drag_batch_args, weights_stride)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(_lib.DragBatchArgsC), C.sizeof(_lib.RegionPrimC), _lib.DragBatchArgsC.weights.offset,
                   _lib.DragBatchArgsC.weights_stride.offset]
    # the new fields come last: a positional construction that stops before them means "no weights"
    assert [f[0] for f in _lib.DragBatchArgsC._fields_[-2:]] == ["weights", "weights_stride"]
    assert _lib.DragBatchArgsC(1, 16, 64, 20).weights is None
    assert _lib.lib().ishap_version() >= 17
