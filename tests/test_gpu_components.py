"""GPU tests of the volume connected-components pass (csrc/components.hip, ishapediting_amd/volume.py) against the numpy
statement (tests/components_ref.py): exact equality everywhere, no tolerance.  The boxes surround the kernel's 4 x 8 x 32
tile: one voxel, a box inside one tile row but one voxel over along z, a box of 3 x 2 x 3 ragged tiles, 64^3 (16 x 8 x 2
tiles, a 128-block root scan), and a sparse 130 x 128 x 128 (1040 blocks: the scan of the block sums carries)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import components_ref as R

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def T(a):
    return torch.from_numpy(np.array(a)).to(dev())            # a copy: the cases are read-only arrays


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


PARAMS = [pytest.param(shape, name, conn, id=f"{'x'.join(map(str, shape))}-{name}-{conn}")
          for shape in R.boxes() for name, conns in R.CASES for conn in conns]


@pytest.mark.parametrize("shape,name,connectivity", PARAMS)
def test_labels_and_table_equal_the_statement(shape, name, connectivity):
    from ishapediting_amd.volume import label_volume, volume_components
    vol, level = R.case(name, shape)
    v = T(vol)
    for phase_name, phase in (("inside", 1), ("outside", 0)):
        want = R.case_labels(name, shape, phase, connectivity)
        got = label_volume(v, level, phase_name, connectivity)
        assert got.dtype == torch.int32 and tuple(got.shape) == shape
        bad = int((got.cpu().numpy() != want).sum())
        print(f"{name} {shape} c{connectivity} {phase_name}: {int((want >= 0).sum())} voxels, "
              f"{len(np.unique(want[want >= 0]))} components, {bad} labels differ")
        assert bad == 0
        comps = volume_components(v, level, phase_name, connectivity)
        tab = R.table(want)
        assert len(comps) == len(tab)
        assert comps.roots.dtype == comps.voxels.dtype == comps.bbox.dtype == comps.border.dtype == torch.int32
        np.testing.assert_array_equal(comps.roots.cpu().numpy(), tab[:, 0])
        np.testing.assert_array_equal(comps.voxels.cpu().numpy(), tab[:, 1])
        np.testing.assert_array_equal(comps.bbox.cpu().numpy().reshape(-1, 6), tab[:, 2:8])
        np.testing.assert_array_equal(comps.border.cpu().numpy(), tab[:, 8])
        assert torch.equal(comps.labels, got)                          # a second run gives the same bits
        again = volume_components(v, level, phase_name, connectivity)
        for f in ("roots", "voxels", "bbox", "border", "labels"):
            assert torch.equal(getattr(again, f), getattr(comps, f)), f


def sparse_1040_blocks():
    """(130, 128, 128): the root scan has 1040 blocks of 2048 voxels, so the workgroup that scans the block sums takes a second
    pass of 1024 with a carry.  A few small pieces: in the first block, ending block 1023 (flat index 2048 * 1024 - 1),
    starting block 1024, across x = 127 / 128 (a root in block 1023 with voxels past it), in blocks 1024 and 1039, at the very
    end, and two voxels that touch at a corner (one component under connectivity 26, two under 6)."""
    vol = -np.ones((130, 128, 128), np.float32)
    vol[0:3, 2:5, 5:8] = 1.0
    vol[64, 64, 64] = vol[65, 65, 65] = 2.0
    vol[127:129, 120:122, 60:62] = 1.0
    vol[127, 127, 127] = vol[128, 0, 0] = 3.0
    vol[128, 10:12, 10:12] = 1.0
    vol[129, 120, 5] = 0.5
    vol[129, 126:128, 126:128] = 1.0
    return vol


@pytest.mark.parametrize("connectivity", [6, 26])
def test_the_table_past_1024_scan_blocks_equals_the_statement(connectivity):
    """The inside phase only: the outside is one component rooted at voxel 0, which no carry reaches, and costs the numpy
    statement seconds."""
    from ishapediting_amd.volume import label_volume, volume_components
    vol = sparse_1040_blocks()
    v = T(vol)
    want = R.label(vol, 0.0, 1, connectivity)
    tab = R.table(want)
    assert len(tab) == (8 if connectivity == 26 else 9)
    assert {261, 2048 * 1024 - 1, 2048 * 1024, vol.size - 130} <= set(tab[:, 0].tolist())
    assert (tab[:, 0] // 2048 < 1024).sum() >= 4 and (tab[:, 0] // 2048 >= 1024).sum() >= 4
    got = label_volume(v, 0.0, "inside", connectivity)
    assert int((got.cpu().numpy() != want).sum()) == 0
    comps = volume_components(v, 0.0, "inside", connectivity)
    assert len(comps) == len(tab)
    np.testing.assert_array_equal(comps.roots.cpu().numpy(), tab[:, 0])
    np.testing.assert_array_equal(comps.voxels.cpu().numpy(), tab[:, 1])
    np.testing.assert_array_equal(comps.bbox.cpu().numpy().reshape(-1, 6), tab[:, 2:8])
    np.testing.assert_array_equal(comps.border.cpu().numpy(), tab[:, 8])
    assert torch.equal(comps.labels, got)
    again = volume_components(v, 0.0, "inside", connectivity)
    for f in ("roots", "voxels", "bbox", "border", "labels"):
        assert torch.equal(getattr(again, f), getattr(comps, f)), f


def test_component_counts_of_the_constructed_cases():
    from ishapediting_amd.volume import volume_components
    shape = (64, 64, 64)
    n = 64 ** 3
    for name, conn, want in (("serpentine", 6, 1), ("path", 6, 1), ("combs", 6, 2), ("combs", 26, 1), ("checkerboard", 6, n // 2),
                             ("checkerboard", 26, 1), ("all_inside", 6, 1), ("all_outside", 26, 0)):
        comps = volume_components(T(R.case(name, shape)[0]), 0.0, "inside", conn)
        assert len(comps) == want, (name, conn, len(comps))
        assert int(comps.voxels.sum()) == int((R.case(name, shape)[0] > 0).sum())
    one = volume_components(T(R.case("serpentine", shape)[0]), 0.0, "inside", 6)
    assert one.roots.tolist() == [0] and one.bbox.tolist() == [[0, 63, 0, 62, 0, 63]] and one.border.tolist() == [1]


def test_non_contiguous_and_other_dtypes_are_accepted():
    from ishapediting_amd.volume import label_volume
    vol, _ = R.case("bernoulli31", (9, 9, 95))
    base = T(np.ascontiguousarray(vol.transpose(2, 0, 1)))
    got = label_volume(base.permute(1, 2, 0).to(torch.float64), 0.0, "inside", 6)
    np.testing.assert_array_equal(got.cpu().numpy(), R.case_labels("bernoulli31", (9, 9, 95), 1, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        label_volume(torch.from_numpy(vol.copy()))


# ---------------------------------------------------------------------------------------------------- clean_volume
CLEAN = [dict(keep="largest"), dict(keep=2), dict(keep=4), dict(keep=None, min_voxels=10), dict(keep=None, min_fraction=0.2),
         dict(keep="largest", fill_cavities=True), dict(keep=None, fill_cavities=True), dict(keep="largest", connectivity=26),
         dict(keep=3, min_voxels=10, fill_cavities=True, connectivity=26)]


@pytest.mark.parametrize("kw", CLEAN, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_clean_volume_equals_the_statement(kw):
    from ishapediting_amd.volume import clean_volume
    vol = R.scene40()
    want, want_info = R.clean(vol, 0.0, **kw)
    v = T(vol)
    before = v.clone()
    got, info = clean_volume(v, 0.0, return_info=True, **kw)
    print(kw, info)
    assert info == want_info
    assert torch.equal(v, before) and got.data_ptr() != v.data_ptr()   # a new volume
    assert (bits(got) == want.view(np.uint32)).all()                   # flipped voxels included, bit for bit
    untouched = want.view(np.uint32) == vol.view(np.uint32)
    assert (bits(got)[untouched] == vol.view(np.uint32)[untouched]).all()
    assert ((got > 0).cpu().numpy() == (want > 0)).all()
    assert torch.equal(clean_volume(v, 0.0, **kw), got)


def test_clean_volume_leaves_empty_and_single_component_volumes_alone():
    from ishapediting_amd.volume import clean_volume
    for name in ("all_outside", "all_inside", "serpentine"):
        vol, _ = R.case(name, (9, 9, 95))
        out, info = clean_volume(T(vol), return_info=True)
        assert (bits(out) == vol.view(np.uint32)).all() and info["removed"] == 0 and info["removed_voxels"] == 0
        assert info["components"] == (0 if name == "all_outside" else 1)
    vol, level = R.case("level", (9, 9, 95))                           # a non-zero level, values exactly at it, cavities
    want, want_info = R.clean(vol, level, keep=3, fill_cavities=True, connectivity=6)
    got, info = clean_volume(T(vol), level, keep=3, fill_cavities=True, return_info=True)
    assert info == want_info and info["cavities"] > 0 and (bits(got) == want.view(np.uint32)).all()
    vol, _ = R.case("nans", (9, 9, 95))                                # NaN voxels keep their bits wherever they are
    want, want_info = R.clean(vol, 0.0, keep="largest", fill_cavities=True, connectivity=6)
    got, info = clean_volume(T(vol), keep="largest", fill_cavities=True, connectivity=6, return_info=True)
    assert info == want_info and info["cavities"] > 0 and (bits(got) == want.view(np.uint32)).all()
    assert np.isnan(vol).sum() == np.isnan(want).sum() > 0


def _flip(vol_in, vol_out, labels, level, roots):
    from ishapediting_amd import _lib
    L = _lib.lib()
    nx, ny, nz = vol_in.shape
    scratch = torch.empty(int(L.ishap_volume_components_scratch_bytes(vol_in.numel())), dtype=torch.uint8, device=vol_in.device)
    _lib.check(L.ishap_volume_flip(vol_in.data_ptr(), vol_out.data_ptr(), labels.data_ptr(), nx, ny, nz, ctypes.c_float(level),
                                   roots.data_ptr(), roots.numel(), scratch.data_ptr(), _lib.stream_ptr(vol_in.device)))
    torch.cuda.synchronize()
    return vol_out


def test_flip_in_place_equals_out_of_place():
    from ishapediting_amd.volume import label_volume
    for name, phase, pname in (("level", 0, "outside"), ("nans", 1, "inside"), ("bernoulli31", 0, "outside")):
        vol, level = R.case(name, (9, 9, 95))
        lab = R.case_labels(name, (9, 9, 95), phase, 6)
        roots = np.unique(lab[lab >= 0])[::2].astype(np.int32)         # every second component, plus ids that name nothing
        listed = np.concatenate([roots[::-1], np.array([-1, lab.size, lab.size + 7], np.int32)])
        want = R.flip(vol, lab, level, roots)
        v, labels = T(vol), label_volume(T(vol), level, pname, 6)
        out = _flip(v, torch.full_like(v, 7.0), labels, level, T(listed))
        assert (bits(out) == want.view(np.uint32)).all() and (bits(v) == vol.view(np.uint32)).all()
        inplace = v.clone()
        _flip(inplace, inplace, labels, level, T(listed))
        assert (bits(inplace) == bits(out)).all()
        changed = R.phase_mask(want, level, 1) != R.phase_mask(vol, level, 1)
        assert (changed == (np.isin(lab, roots) & ~np.isnan(vol))).all()    # the mask differs exactly on the listed components
        same = _flip(v, torch.empty_like(v), labels, level, T(np.zeros(0, np.int32)))
        assert (bits(same) == vol.view(np.uint32)).all()               # an empty list copies


def _triangle_rows(volume):
    from ishapediting_amd.mesh import extract_surface
    v, t = extract_surface(volume, 0.0)
    rows = v[t.long()].reshape(-1, 9).cpu().numpy()
    return rows[np.lexsort(rows.T[::-1])]


def test_the_kept_surface_is_the_surface_it_was():
    """Connectivity 26: no marching-cubes cell holds both a kept and a removed inside voxel, so the triangles of the original
    are, as a multiset of coordinate rows, those of the cleaned volume plus those of the volume with only the KEPT components
    flipped away."""
    from ishapediting_amd.volume import clean_volume, volume_components
    vol = T(R.scene40())
    cleaned, info = clean_volume(vol, keep="largest", connectivity=26, return_info=True)
    comps = volume_components(vol, 0.0, "inside", 26)
    kept = comps.roots[comps.voxels == comps.voxels.max()][:1]
    rest = _flip(vol, torch.empty_like(vol), comps.labels, 0.0, kept)
    a, b, c = _triangle_rows(vol), _triangle_rows(cleaned), _triangle_rows(rest)
    print(f"triangles: original {len(a)}, cleaned {len(b)}, removed parts {len(c)}; removed {info}")
    assert len(b) > 1000 and len(c) > 100 and len(a) == len(b) + len(c)
    both = np.concatenate([b, c])
    both = both[np.lexsort(both.T[::-1])]
    assert (a.view(np.uint32) == both.view(np.uint32)).all()


# ---------------------------------------------------------------------------------------------------- hook-up
def test_clean_none_is_todays_mesh_and_clean_gives_one_component():
    from ishapediting_amd.mesh import OccupancyMesh, volume_to_mesh
    from ishapediting_amd.volume import volume_components
    vol = T(R.scene40())
    plain, same = volume_to_mesh(vol, 40), volume_to_mesh(vol, 40, clean=None)
    assert same.volume is vol and plain.volume is vol
    assert torch.equal(plain.vertices, same.vertices) and torch.equal(plain.triangles, same.triangles)
    assert R.mesh_components(plain.triangles.cpu().numpy(), plain.vertices.shape[0]) == 6   # the outsides of the 5 pieces and the cavity wall
    # the largest piece is the ball WITH its cavity: keeping it alone leaves two shells (outside and cavity wall), and one
    # once the cavity is filled as well
    largest = volume_to_mesh(vol, 40, clean={"keep": "largest"})
    assert len(volume_components(largest.volume)) == 1
    assert R.mesh_components(largest.triangles.cpu().numpy(), largest.vertices.shape[0]) == 2
    filled = OccupancyMesh(vol, 40, 10, clean={"keep": "largest", "fill_cavities": True})
    assert len(volume_components(filled.volume)) == 1 and len(volume_components(filled.volume, phase="outside")) == 1
    assert R.mesh_components(filled.triangles.cpu().numpy(), filled.vertices.shape[0]) == 1
    assert filled.counts() == (filled.vertices.shape[0], filled.triangles.shape[0])
    want, _ = R.clean(R.scene40(), keep="largest", fill_cavities=True)
    assert (bits(filled.volume) == want.view(np.uint32)).all()


def test_dragstuff_clean_attribute():
    from ishapediting_amd import synthetic
    from ishapediting_amd.drag_utils import DragStuff
    from ishapediting_amd.volume import volume_components
    from tests.helpers import small96_args, small96_config
    ds = DragStuff(dev(), args=small96_args(4, w_time=2, feat_layer=1))
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(small96_config(), 202))
    ds.load_weights(sd, synthetic.decoder_state_dict(), -np.full(96, 1.5, np.float32), np.full(96, 0.5, np.float32))
    assert ds.clean is None
    feat = torch.randn((2, 96, 16, 16), generator=torch.Generator().manual_seed(5)).to(dev())
    raw = ds.get_mesh(tri_feat=feat[:1])
    pieces = len(volume_components(raw.volume))
    print(f"decoded 32^3 volume: {pieces} inside components, {int((raw.volume > 0).sum())} inside voxels")
    assert pieces > 1 and ds.volume is raw.volume
    ds.clean = {"keep": "largest"}
    mesh = ds.get_mesh(tri_feat=feat[:1])
    assert len(volume_components(mesh.volume)) == 1 and ds.volume is mesh.volume
    want, _ = R.clean(raw.volume.cpu().numpy(), keep="largest")
    assert (bits(mesh.volume) == want.view(np.uint32)).all()
    meshes = ds.get_meshes(feat, t=0)
    assert len(meshes) == 2 and all(len(volume_components(m.volume)) == 1 for m in meshes)
    assert torch.equal(meshes[0].volume, mesh.volume)
