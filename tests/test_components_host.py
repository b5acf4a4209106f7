"""CPU checks of the volume connected-components pass (csrc/components.hip, ishapediting_amd/volume.py): the numpy statement
the GPU tests compare with (tests/components_ref.py) against a brute-force flood fill and, where it is installed, against
scipy.ndimage.label; the C ABI in the header, the binding and the built library; argument rejection without a GPU."""
import os
import re

import numpy as np
import pytest

from tests import components_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000                                                          # a non-null address nothing dereferences
NAMES = ("ishap_volume_label", "ishap_volume_components_count", "ishap_volume_components_emit",
         "ishap_volume_components_scratch_bytes", "ishap_volume_flip")


def _random_volumes():
    rng = np.random.default_rng(7)
    for p in (0.15, 0.31, 0.5, 0.8):
        vol = np.where(rng.random((5, 6, 7)) < p, 1.0, -1.0).astype(np.float32) * rng.uniform(0.1, 1, (5, 6, 7)).astype(np.float32)
        vol[rng.random(vol.shape) < 0.03] = np.nan
        yield vol


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("phase", [1, 0])
def test_statement_equals_flood_fill(connectivity, phase):
    for vol in _random_volumes():
        for level in (0.0, 0.25):
            a = R.label(vol, level, phase, connectivity)
            b = R.flood_fill_label(vol, level, phase, connectivity)
            np.testing.assert_array_equal(a, b)
            assert a.dtype == np.int32 and ((a >= 0) == R.phase_mask(vol, level, phase)).all()
            roots = np.unique(a[a >= 0])
            assert (a.reshape(-1)[roots] == roots).all()               # a root is labelled with itself: the lowest index


@pytest.mark.parametrize("connectivity", [6, 26])
def test_statement_partition_equals_scipy(connectivity):
    ndimage = pytest.importorskip("scipy.ndimage")
    structure = ndimage.generate_binary_structure(3, 1 if connectivity == 6 else 3)
    vols = list(_random_volumes()) + [R.case("bernoulli31", (9, 9, 95))[0], R.case("combs", (9, 9, 95))[0]]
    for vol in vols:
        for phase in (1, 0):
            mask = R.phase_mask(vol, 0.0, phase)
            theirs, count = ndimage.label(mask, structure=structure)
            ours = R.label(vol, 0.0, phase, connectivity)
            assert ((theirs > 0) == (ours >= 0)).all()
            pairs = np.unique(np.stack([theirs[mask], ours[mask]], axis=1), axis=0)
            assert len(pairs) == count == len(np.unique(ours[mask]))   # a bijection between the two sets of names


def test_statement_table_flip_and_rule():
    vol = R.scene40()
    lab = R.label(vol, 0.0, 1, 6)
    tab = R.table(lab)
    assert len(tab) == 5 and (np.diff(tab[:, 0]) > 0).all() and tab[:, 1].sum() == (vol > 0).sum()
    slab, small = tab[0], tab[tab[:, 1] == 8]
    assert slab[0] == 0 and slab[1] == 2 * 40 * 40 and list(slab[2:8]) == [0, 1, 0, 39, 0, 39] and slab[8] == 1
    assert len(small) == 2 and list(small[0][2:8]) == [36, 37, 5, 6, 5, 6] and small[:, 8].sum() == 0
    np.testing.assert_array_equal(R.select(tab[:, 1], "largest"), tab[:, 1] == tab[:, 1].max())
    four = R.select(tab[:, 1], 4)
    assert four.sum() == 4 and not four[np.nonzero(tab[:, 1] == 8)[0][1]]          # the tie goes to the lower root
    assert R.select(tab[:, 1], None, min_voxels=10).sum() == 3 and R.select(tab[:, 1], None, min_fraction=0.2).sum() == 2
    out, info = R.clean(vol, keep="largest", fill_cavities=True)
    assert info["components"] == 5 and info["removed"] == 4 and info["cavities"] == 1
    assert len(R.table(R.label(out, 0.0, 1, 6))) == 1 and len(R.table(R.label(out, 0.0, 0, 6))) == 1
    assert out[20, 20, 24] == np.nextafter(np.float32(0), np.float32(1)) and out[20, 20, 24] > 0
    kept = lab == tab[np.argmax(tab[:, 1]), 0]
    assert (out[kept].view(np.uint32) == vol[kept].view(np.uint32)).all()
    nan = np.array([[[np.nan, 1.0, -2.0]]], np.float32)
    f = R.flip(nan, np.zeros((1, 1, 3), np.int32), 0.5, [0])
    assert np.isnan(f[0, 0, 0]) and f[0, 0, 1] == 0.0 and f[0, 0, 2] == 3.0
    assert R.mesh_components([[0, 1, 2], [2, 3, 4], [5, 6, 7]], 9) == 2


def test_case_generators():
    for shape in R.boxes()[1:]:
        n = int(np.prod(shape))
        s = R.serpentine_mask(shape)
        assert abs(s.sum() / n - 0.5) < 0.1 and len(R.table(R.label(R.case("serpentine", shape)[0], 0.0, 1, 6))) == 1
        path = R.case_labels("path", shape, 1, 6)
        assert len(np.unique(path[path >= 0])) == 1
        for conn, want in ((6, 2), (26, 1)):
            assert len(R.table(R.case_labels("combs", shape, 1, conn))) == want
        assert len(R.table(R.case_labels("checkerboard", shape, 1, 6))) == (n + 1) // 2
        assert len(R.table(R.case_labels("checkerboard", shape, 1, 26))) == 1
    vol, level = R.case("level", (9, 9, 95))
    assert level == 0.37 and (vol == np.float32(0.37)).sum() > 100 and not R.phase_mask(vol, level, 1)[vol == np.float32(0.37)].any()
    assert np.isnan(R.case("nans", (9, 9, 95))[0]).sum() > 100


def test_components_abi():
    from ishapediting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ishap.h")).read()
    assert "connected components of a volume (ABI 16)" in hdr
    src = open(os.path.join(ROOT, "ishapediting_amd", "csrc", "components.hip")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SYMBOLS
        assert re.search(r'extern "C" (int|long long) %s\(' % name, src), name
    L = _lib.lib()                                                     # raises if the built library lacks a declared symbol
    assert L.ishap_version() >= 16
    from ishapediting_amd import build
    assert "components.hip" in build.SOURCES
    tx, ty, tz = R.TILE
    assert re.search(r"CC_TX = %d, CC_TY = %d, CC_TZ = %d\b" % (tx, ty, tz), src)   # the boxes of the GPU tests surround this tile


def test_components_kernels_use_no_scratch_memory():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for want in ("cc_tile_kernel", "cc_seam_kernel", "cc_flatten_kernel", "cc_count_kernel", "scan_totals_kernel", "cc_rows_kernel",
                 "cc_accum_kernel", "cc_mark_kernel", "cc_flip_kernel"):
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        assert ks[found[0]].get(".private_segment_fixed_size", 0) == 0, (want, ks[found[0]])


def test_bad_arguments_fail_without_a_gpu():
    from ishapediting_amd import _lib
    L = _lib.lib()
    for nx, ny, nz in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (2048, 1024, 1024), (1 << 30, 1 << 30, 8)):
        assert L.ishap_volume_label(FAKE, nx, ny, nz, 0.0, 1, 6, FAKE, None) == -2 and b"volume" in L.ishap_last_error()
        assert L.ishap_volume_components_count(FAKE, nx, ny, nz, FAKE, FAKE, None) == -2
        assert L.ishap_volume_components_emit(FAKE, nx, ny, nz, FAKE, FAKE, None) == -2
        assert L.ishap_volume_flip(FAKE, FAKE, FAKE, nx, ny, nz, 0.0, FAKE, 1, FAKE, None) == -2
    for conn in (0, 4, 8, 18, 27, -6):
        assert L.ishap_volume_label(FAKE, 4, 4, 4, 0.0, 1, conn, FAKE, None) == -2 and b"connectivity" in L.ishap_last_error()
    assert L.ishap_volume_label(FAKE, 4, 4, 4, 0.0, 2, 6, FAKE, None) == -2 and b"phase" in L.ishap_last_error()
    assert L.ishap_volume_label(None, 4, 4, 4, 0.0, 1, 6, FAKE, None) == -2
    assert L.ishap_volume_flip(FAKE, FAKE, FAKE, 4, 4, 4, 0.0, None, 3, FAKE, None) == -2
    for n in (0, -5, 1 << 31):
        assert L.ishap_volume_components_scratch_bytes(n) == -1
    sizes = [L.ishap_volume_components_scratch_bytes(n) for n in (1, 2048, 2049, 64 ** 3, 256 ** 3)]
    assert sizes == sorted(sizes) and all(s % 256 == 0 and s >= 4 * n for s, n in zip(sizes, (1, 2048, 2049, 64 ** 3, 256 ** 3)))


def test_python_arguments_are_checked_before_the_library(monkeypatch):
    import torch
    from ishapediting_amd import _lib, volume

    def refuse(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "lib", refuse)
    v = torch.zeros((3, 4, 5))
    for fn in (volume.label_volume, volume.volume_components):
        with pytest.raises(ValueError, match="connectivity"):
            fn(v, connectivity=18)
        with pytest.raises(ValueError, match="phase"):
            fn(v, phase="both")
        with pytest.raises(ValueError, match="3-D"):
            fn(torch.zeros((4, 5)))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        volume.clean_volume(v)
    with pytest.raises(ValueError, match="keep"):
        volume.select_components(torch.tensor([3, 2]), keep="smallest")
    # the selection rule in torch equals the statement's
    rng = np.random.default_rng(3)
    for _ in range(20):
        vox = rng.integers(1, 6, size=int(rng.integers(0, 9)))
        for keep in ("largest", None, 0, 1, 2, 5):
            for mv, mf in ((0, 0.0), (3, 0.0), (0, 0.75), (2, 1.0)):
                got = volume.select_components(torch.from_numpy(vox), keep, mv, mf).numpy()
                np.testing.assert_array_equal(got, R.select(vox, keep, mv, mf))
    assert volume.Components.__len__ and volume.PHASES == {"outside": 0, "inside": 1}
