"""Every scratch-size entry of the C ABI, pinned: the twenty ishap_*_scratch_bytes functions and ishap_sparse_reach_bytes.  No GPU needed.

The numbers were recorded from a build of the commit BEFORE the scratch layouts moved to the shared carver (csrc/common.h, Carve),
not computed from the code under test: a layout change that moves a size, or a refusal that stops answering -1 (0 for GroupNorm),
fails here.  Per entry: the smallest valid arguments, a set where no buffer is a multiple of 256 bytes, product sizes, and arguments
outside the accepted range.  ishap_surface_scratch_bytes refuses nothing (ishap_surface_count checks res): its values at res 1, 0
and -1 are pinned as they are.  A list among the arguments is an int[3] (the cluster grid of the simplifier), None a null pointer."""
import ctypes as C

import pytest

from ishapediting_amd import _lib

TABLE = {
    "ishap_group_norm32_scratch_bytes": [
        ((1, 1, 32), 26112),
        ((3, 289, 96), 415744),
        ((1, 16384, 192), 7195904),
        ((8, 4096, 512), 51052800),
        ((0, 64, 64), 0),
        ((1, 64, 16), 0),
        ((1, 0, 32), 0),
    ],
    "ishap_drag_batch_scratch_bytes": [
        ((1, 2, 1), 1280),
        ((3, 17, 96), 669696),
        ((1, 128, 96), 12633088),
        ((8, 128, 96), 101057536),
        ((32, 256, 32), 543163392),
        ((0, 128, 96), -1),
        ((1, 1, 96), -1),
        ((1, 128, 0), -1),
    ],
    "ishap_drag_track_scratch_bytes": [
        ((1, 1, 0, 0, 1), 16),
        ((3, 7, 3, 1, 33), 4128),
        ((8, 64, 8, 4, 96), 1331712),
        ((32, 32, 4, 2, 96), 62208),
        ((0, 1, 2, 1, 32), -1),
        ((2, 1, 2, 1, 32), -1),
        ((1, 1, 9, 1, 32), -1),
        ((1, 1, 2, 5, 32), -1),
        ((1, 1, 2, 1, 0), -1),
        ((33, 40, 2, 1, 32), -1),
    ],
    "ishap_region_plane_weights_scratch_bytes": [
        ((2,), 256),
        ((33,), 3328),
        ((128,), 49152),
        ((4096,), 50331648),
        ((1,), -1),
        ((4097,), -1),
        ((-3,), -1),
    ],
    "ishap_region_plane_feather_scratch_bytes": [
        ((2,), 1280),
        ((33,), 46592),
        ((128,), 688128),
        ((1024,), 44040192),
        ((1,), -1),
        ((1025,), -1),
    ],
    "ishap_edt_scratch_bytes": [
        ((1, 1, 1, 1), 256),
        ((3, 33, 33, 6), 13312),
        ((5, 7, 9, 7), 1280),
        ((3, 128, 128, 6), 196608),
        ((128, 128, 128, 7), 8388608),
        ((64, 64, 64, 4), 256),
        ((0, 4, 4, 7), -1),
        ((4, 4, 4, 0), -1),
        ((4, 4, 4, 8), -1),
        ((1025, 4, 4, 1), -1),
        ((2048, 1024, 1024, 6), -1),
    ],
    "ishap_region_handles_scratch_bytes": [
        ((2, 1), 1536),
        ((9, 3), 7168),
        ((33, 17), 290816),
        ((128, 64), 16909312),
        ((256, 4096), 135300096),
        ((1, 4), -1),
        ((1025, 4), -1),
        ((64, 0), -1),
        ((64, 4097), -1),
    ],
    "ishap_constraint_setup_scratch_bytes": [
        ((1, 2), 1024),
        ((7, 3), 1536),
        ((1000, 33), 109824),
        ((65536, 128), 6488320),
        ((1048576, 1024), 113252608),
        ((0, 64), -1),
        ((1048577, 64), -1),
        ((16, 1), -1),
        ((16, 1025), -1),
    ],
    "ishap_surface_scratch_bytes": [
        ((2,), 312),
        ((9,), 4638),
        ((17,), 29758),
        ((128,), 12591360),
        ((256,), 100729088),
        ((1024,), 6446645504),
        ((1,), 270),
        ((0,), 256),
        ((-1,), 250),
    ],
    "ishap_mesh_smooth_scratch_bytes": [
        ((0, 0), 512),
        ((1, 1), 1536),
        ((257, 511), 19712),
        ((100000, 200000), 7200768),
        ((3000000, 6000000), 216006144),
        ((-1, 4), -1),
        ((4, -1), -1),
    ],
    "ishap_mesh_distance_scratch_bytes": [
        ((0,), 0),
        ((1,), 32),
        ((257,), 64),
        ((511,), 64),
        ((200000,), 25024),
        ((6000000,), 750016),
        ((-1,), -1),
    ],
    "ishap_mesh_distance_scratch_bytes_sdf": [
        ((1, 1, 0), 32),
        ((1, 1, 2), 512),
        ((257, 100, 2), 1536),
        ((257, 100, -2), 1536),
        ((257, 100, 1), 64),
        ((511, 1000, 2), 8704),
        ((200000, 262144, 2), 25344),
        ((6000000, 2097152, -2), 750336),
        ((0, 5, 2), 256),
        ((5, 0, 2), 512),
        ((-1, 5, 2), -1),
        ((5, -1, 0), -1),
    ],
    "ishap_winding_scratch_bytes": [
        ((1, 1), 256),
        ((0, 0), 256),
        ((257, 100), 1280),
        ((511, 1000), 8448),
        ((200000, 262144), 256),
        ((6000000, 2097152), 256),
        ((-1, 1), -1),
        ((1, -1), -1),
    ],
    "ishap_cloud_orient_scratch_bytes": [
        ((0,), 256),
        ((1,), 512),
        ((257,), 1536),
        ((64,), 512),
        ((100000,), 400384),
        ((16777216,), 67109120),
        ((-1,), -1),
    ],
    "ishap_volume_components_scratch_bytes": [
        ((1,), 512),
        ((729,), 3328),
        ((4913,), 19968),
        ((2097152,), 8392704),
        ((16777216,), 67141632),
        ((2147483647,), 8594128896),
        ((0,), -1),
        ((-5,), -1),
        ((2147483648,), -1),
    ],
    "ishap_arap_scratch_bytes": [
        ((0, 0, 0), 1024),
        ((1, 1, 0), 5632),
        ((257, 511, 3), 124416),
        ((257, 511, 0), 124416),
        ((100000, 200000, 40), 46829568),
        ((3000000, 6000000, 1000), 1404850432),
        ((-1, 1, 0), -1),
        ((1, -1, 0), -1),
        ((1, 1, -1), -1),
    ],
    "ishap_render_scratch_bytes": [
        ((0, 0, 1, 1), 32),
        ((10, 20, 150, 117), 140896),
        ((7, 3, 33, 1), 448),
        ((100000, 200000, 1024, 1024), 13188624),
        ((3000000, 6000000, 16384, 16384), 2291483664),
        ((-1, 0, 4, 4), -1),
        ((0, 0, 0, 4), -1),
        ((0, 0, 4, 16385), -1),
        ((0, 2147483648, 4, 4), -1),
    ],
    "ishap_sparse_compact_scratch_bytes": [
        ((9,), 512),
        ((10,), 512),
        ((65,), 2304),
        ((200,), 62976),
        ((512,), 1049344),
        ((2048,), 67141888),
        ((8,), -1),
        ((2049,), -1),
    ],
    "ishap_sparse_surface_scratch_bytes": [
        ((9, 0), 256),
        ((9, 1), 2560),
        ((65, 7), 11520),
        ((200, 1001), 1486080),
        ((512, 30000), 44520448),
        ((2048, 2097152), 3112177920),
        ((8, 4), -1),
        ((2049, 4), -1),
        ((64, -1), -1),
        ((64, 2097153), -1),
    ],
    "ishap_mesh_simplify_scratch_bytes": [
        ((0, 0, [1, 1, 1]), 2048),
        ((1, 1, [1, 1, 1]), 2560),
        ((257, 511, [3, 5, 7]), 22784),
        ((257, 511, [33, 17, 9]), 44032),
        ((100000, 200000, [64, 64, 64]), 16564224),
        ((3000000, 6000000, [256, 256, 256]), 503315968),
        ((1000, 2000, [1024, 1024, 1024]), 268662528),
        ((-1, 1, [4, 4, 4]), -1),
        ((1, -1, [4, 4, 4]), -1),
        ((2147483648, 1, [4, 4, 4]), -1),
        ((10, 20, [0, 4, 4]), -1),
        ((10, 20, [1024, 1024, 1025]), -1),
        ((10, 20, None), -1),
    ],
    "ishap_sparse_reach_bytes": [
        ((0,), 0),
        ((1,), 736),
        ((7,), 5152),
        ((4096,), 3014656),
        ((2097152,), 1543503872),
        ((-1,), -1),
    ],
}


def test_table_covers_every_entry():
    names = [n for n in _lib.SYMBOLS if n.endswith("_scratch_bytes") or n.endswith("_scratch_bytes_sdf")] + ["ishap_sparse_reach_bytes"]
    assert len(names) == 21 and sorted(names) == sorted(TABLE)
    for name, rows in TABLE.items():
        assert len(rows) >= 4, name
        assert any(v > 0 for _, v in rows), name


@pytest.mark.parametrize("name", sorted(TABLE))
def test_scratch_bytes_pinned(name):
    fn = getattr(_lib.lib(), name)
    for args, want in TABLE[name]:
        a = [(C.c_int * 3)(*x) if isinstance(x, list) else x for x in args]
        assert fn(*a) == want, (name, args)
