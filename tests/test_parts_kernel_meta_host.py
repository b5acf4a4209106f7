"""Code-object metadata of the part-edit kernels (csrc/parts.hip) through tools/kernel_meta.py, no GPU needed: none may have a
private segment.  They are a few dozen registers each; scratch would mean an array (the bounding box's six extremes, the rigid
motion's fifteen doubles) was indexed in a way the compiler could not resolve and went to memory."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("region_select_kernel", "region_transform_kernel", "parts_count_kernel", "parts_compact_kernel", "parts_bbox_kernel",
           "parts_first_kernel", "parts_round_kernel", "parts_emit_kernel")


def test_part_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for name in KERNELS:
        mine = [n for n in ks if name in n]
        assert len(mine) == 1, (name, mine)
        k = ks[mine[0]]
        assert k.get(".private_segment_fixed_size", 0) == 0, (mine[0], k.get(".private_segment_fixed_size"))
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, (mine[0], k)
        assert k.get(".vgpr_count", 0) <= 64, (mine[0], k.get(".vgpr_count"))          # full occupancy: these are streaming kernels
