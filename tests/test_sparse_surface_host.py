"""The sparse high-resolution surface without a GPU: the ABI (version, symbols, prototypes, refusals that launch nothing), the
integer seed mapping against its numpy restatement (tests/sparse_surface_ref.py), and the code-object metadata of the new
kernels through tools/kernel_meta.py (no private segment, no spills; the brick decode within the dense decode's registers)."""
import ctypes as C
import os
import sys

import pytest

from tests import sparse_surface_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x1000          # a non-NULL address no call may touch: every call below must be refused before it launches
NEW = {
    "ishap_sparse_bricks_per_axis": (C.c_int, 1),
    "ishap_sparse_seed_range": (C.c_int, 5),
    "ishap_sparse_seed_volume": (C.c_int, 6),
    "ishap_sparse_compact_scratch_bytes": (C.c_longlong, 1),
    "ishap_sparse_compact": (C.c_int, 11),
    "ishap_triplane_decode_bricks": (C.c_int, 9),
    "ishap_sparse_reach_bytes": (C.c_longlong, 1),
    "ishap_sparse_grow": (C.c_int, 10),
    "ishap_sparse_surface_scratch_bytes": (C.c_longlong, 2),
    "ishap_sparse_surface_count": (C.c_int, 11),
    "ishap_sparse_surface_emit": (C.c_int, 12),
}
KERNELS = ("sparse_seed_kernel", "sparse_flag_kernel", "sparse_scatter_kernel", "sparse_grow_kernel", "sparse_count_kernel",
           "sparse_emit_vertices_kernel", "sparse_emit_triangles_kernel", "triplane_decode_bricks_kernel")


def lib():
    from ishapediting_amd import _lib
    return _lib


def err():
    m = lib().lib().ishap_last_error()
    return m.decode() if m else ""


def test_abi_and_prototypes():
    L = lib().lib()
    assert L.ishap_version() >= 25
    header = open(os.path.join(ROOT, "include", "ishap.h")).read()
    for name, (res, nargs) in NEW.items():
        assert name in lib().SYMBOLS, name
        got_res, got_args = lib().SYMBOLS[name]
        assert got_res is res and len(got_args) == nargs, (name, got_res, len(got_args))
        assert getattr(L, name).restype is res
        assert f"{name}(" in header, f"{name} is not declared in include/ishap.h"


def test_sizes():
    L = lib().lib()
    for res in (9, 30, 33, 41, 1024, 2048):
        assert L.ishap_sparse_bricks_per_axis(res) == R.bricks_per_axis(res)
    assert L.ishap_sparse_bricks_per_axis(2048) == 256 and L.ishap_sparse_bricks_per_axis(33) == 4
    for res in (8, 0, -1, 2049):
        assert L.ishap_sparse_bricks_per_axis(res) == -1
        assert L.ishap_sparse_compact_scratch_bytes(res) == -1
        assert L.ishap_sparse_surface_scratch_bytes(res, 10) == -1
    assert L.ishap_sparse_surface_scratch_bytes(33, -1) == -1 and L.ishap_sparse_reach_bytes(-1) == -1
    assert L.ishap_sparse_compact_scratch_bytes(2048) >= 4 * 256 ** 3
    assert L.ishap_sparse_reach_bytes(3) >= 3 * 729
    assert L.ishap_sparse_surface_scratch_bytes(1024, 1000) >= 1000 * (729 * 2 + 12)


def test_refusals_launch_nothing():
    """R < 9, R > 2048 and a NULL argument: error code -2 with the requirement named; the arguments are a fake address, so a call
    that got as far as a launch (or a host write) would not return"""
    L = lib().lib()
    w = lib().DecoderWeightsC(*([FAKE] * 7))
    i0, i1 = C.c_int(-7), C.c_int(-7)
    for res in (8, 2049):
        assert L.ishap_sparse_seed_volume(FAKE, 12, 0.0, res, FAKE, None) == -2 and "9 <= R <= 2048" in err()
        assert L.ishap_sparse_compact(FAKE, res, 0, 0, FAKE, FAKE, 8, FAKE, FAKE, 1 << 30, None) == -2 and "9 <= R <= 2048" in err()
        assert L.ishap_triplane_decode_bricks(FAKE, 8, C.byref(w), FAKE, res, FAKE, 1, FAKE, None) == -2 and "res" in err()
        assert L.ishap_sparse_grow(FAKE, FAKE, 1, res, 0.0, FAKE, FAKE, FAKE, FAKE, None) == -2 and "9 <= R <= 2048" in err()
        assert L.ishap_sparse_surface_count(FAKE, FAKE, 1, res, 0.0, FAKE, FAKE, FAKE, 1 << 30, FAKE, None) == -2
        assert L.ishap_sparse_surface_emit(FAKE, FAKE, 1, res, 0.0, FAKE, FAKE, FAKE, 1 << 30, FAKE, FAKE, None) == -2
        assert L.ishap_sparse_seed_range(12, res, 0, C.byref(i0), C.byref(i1)) == -2 and (i0.value, i1.value) == (-7, -7)
    big = 1 << 30
    null_calls = [
        lambda: L.ishap_sparse_seed_volume(None, 12, 0.0, 41, FAKE, None),
        lambda: L.ishap_sparse_seed_volume(FAKE, 12, 0.0, 41, None, None),
        lambda: L.ishap_sparse_compact(None, 41, 0, 0, FAKE, FAKE, 8, FAKE, FAKE, big, None),
        lambda: L.ishap_sparse_compact(FAKE, 41, 0, 0, None, FAKE, 8, FAKE, FAKE, big, None),
        lambda: L.ishap_sparse_compact(FAKE, 41, 0, 0, FAKE, None, 8, FAKE, FAKE, big, None),
        lambda: L.ishap_sparse_compact(FAKE, 41, 0, 0, FAKE, FAKE, 8, None, FAKE, big, None),
        lambda: L.ishap_sparse_compact(FAKE, 41, 0, 0, FAKE, FAKE, 8, FAKE, None, big, None),
        lambda: L.ishap_triplane_decode_bricks(None, 8, C.byref(w), FAKE, 41, FAKE, 1, FAKE, None),
        lambda: L.ishap_triplane_decode_bricks(FAKE, 8, None, FAKE, 41, FAKE, 1, FAKE, None),
        lambda: L.ishap_triplane_decode_bricks(FAKE, 8, C.byref(w), None, 41, FAKE, 1, FAKE, None),
        lambda: L.ishap_triplane_decode_bricks(FAKE, 8, C.byref(w), FAKE, 41, None, 1, FAKE, None),
        lambda: L.ishap_triplane_decode_bricks(FAKE, 8, C.byref(w), FAKE, 41, FAKE, 1, None, None),
        lambda: L.ishap_sparse_grow(None, FAKE, 1, 41, 0.0, FAKE, FAKE, FAKE, FAKE, None),
        lambda: L.ishap_sparse_grow(FAKE, None, 1, 41, 0.0, FAKE, FAKE, FAKE, FAKE, None),
        lambda: L.ishap_sparse_grow(FAKE, FAKE, 1, 41, 0.0, None, FAKE, FAKE, FAKE, None),
        lambda: L.ishap_sparse_grow(FAKE, FAKE, 1, 41, 0.0, FAKE, None, FAKE, FAKE, None),
        lambda: L.ishap_sparse_grow(FAKE, FAKE, 1, 41, 0.0, FAKE, FAKE, None, FAKE, None),
        lambda: L.ishap_sparse_grow(FAKE, FAKE, 1, 41, 0.0, FAKE, FAKE, FAKE, None, None),
        lambda: L.ishap_sparse_surface_count(None, FAKE, 1, 41, 0.0, FAKE, FAKE, FAKE, big, FAKE, None),
        lambda: L.ishap_sparse_surface_count(FAKE, FAKE, 1, 41, 0.0, FAKE, FAKE, None, big, FAKE, None),
        lambda: L.ishap_sparse_surface_count(FAKE, FAKE, 1, 41, 0.0, FAKE, FAKE, FAKE, big, None, None),
        lambda: L.ishap_sparse_surface_emit(FAKE, FAKE, 1, 41, 0.0, FAKE, FAKE, FAKE, big, None, FAKE, None),
        lambda: L.ishap_sparse_surface_emit(FAKE, FAKE, 1, 41, 0.0, FAKE, FAKE, FAKE, big, FAKE, None, None),
        lambda: L.ishap_sparse_seed_range(12, 41, 0, None, C.byref(i1)),
    ]
    # a coarse volume too coarse for the fine grid (one thread stores its cell's whole brick box): R - 1 <= 64 (Rc - 1)
    assert L.ishap_sparse_seed_volume(FAKE, 2, 0.0, 66, FAKE, None) == -2 and "64 (Rc - 1)" in err()
    assert L.ishap_sparse_seed_volume(FAKE, 32, 0.0, 2048, FAKE, None) == -2 and "64 (Rc - 1)" in err()
    for k, call in enumerate(null_calls):
        assert call() == -2, k
        assert "null" in err().lower(), (k, err())
    # sizes of the brick lists and the scratch
    assert L.ishap_triplane_decode_bricks(FAKE, 8, C.byref(w), FAKE, 41, FAKE, 0, FAKE, None) == -2
    assert L.ishap_sparse_grow(FAKE, FAKE, 0, 41, 0.0, FAKE, FAKE, FAKE, FAKE, None) == -2
    assert L.ishap_sparse_surface_count(FAKE, FAKE, 4, 41, 0.0, FAKE, FAKE, FAKE, 16, FAKE, None) == -2 and "scratch" in err()
    assert L.ishap_sparse_compact(FAKE, 41, 3, 0, FAKE, FAKE, 8, FAKE, FAKE, big, None) == -2 and "mode" in err()
    assert L.ishap_sparse_compact(FAKE, 41, 0, 0, FAKE, FAKE, 8, FAKE, FAKE, 16, None) == -2 and "scratch" in err()


@pytest.mark.parametrize("Rc,res", [(12, 41), (16, 30), (256, 1024)])
def test_seed_mapping(Rc, res):
    """the bricks a coarse cell marks, per axis: the library's integer arithmetic against trying every brick, for the first, a
    middle and the last coarse cell (and, cheap enough, every other one)"""
    L = lib().lib()
    nb = R.bricks_per_axis(res)
    first, last = C.c_int(), C.c_int()
    for j in sorted({0, (Rc - 1) // 2, Rc - 2} | set(range(Rc - 1))):
        assert L.ishap_sparse_seed_range(Rc, res, j, C.byref(first), C.byref(last)) == 0
        assert (first.value, last.value) == R.seed_range(Rc, res, j), (Rc, res, j)
        assert 0 <= first.value <= last.value <= nb - 1
    assert L.ishap_sparse_seed_range(Rc, res, 0, C.byref(first), C.byref(last)) == 0 and first.value == 0
    assert L.ishap_sparse_seed_range(Rc, res, Rc - 2, C.byref(first), C.byref(last)) == 0 and last.value == nb - 1
    for j in (-1, Rc - 1):
        assert L.ishap_sparse_seed_range(Rc, res, j, C.byref(first), C.byref(last)) == -2


def test_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for name in KERNELS:
        mine = [n for n in ks if name in n]
        assert len(mine) == 1, (name, mine)
        k = ks[mine[0]]
        assert k.get(".private_segment_fixed_size", 0) == 0, (mine[0], k.get(".private_segment_fixed_size"))
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (mine[0], k)
        if name.startswith("sparse_"):
            assert k.get(".vgpr_count", 0) <= 64, (mine[0], k.get(".vgpr_count"))      # streaming kernels: full occupancy
    dense = [k for n, k in ks.items() if "triplane_decode_kernel" in n]
    brick = [k for n, k in ks.items() if "triplane_decode_bricks_kernel" in n]
    assert len(dense) == 1 and len(brick) == 1
    assert brick[0][".vgpr_count"] <= dense[0][".vgpr_count"], (brick[0][".vgpr_count"], dense[0][".vgpr_count"])
    assert brick[0].get(".agpr_count", 0) <= dense[0].get(".agpr_count", 0)


def test_command_line_options():
    """generate.py --mesh_resolution and tools/headless_edit.py --mesh-resolution parse to an int, None when absent"""
    from ishapediting_amd import generate
    assert generate.build_parser().parse_args(["--mesh_resolution", "1024"]).mesh_resolution == 1024
    assert generate.build_parser().parse_args([]).mesh_resolution is None
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import headless_edit
    assert headless_edit.build_parser().parse_args(["--mesh-resolution", "512"]).mesh_resolution == 512
    assert headless_edit.build_parser().parse_args([]).mesh_resolution is None
