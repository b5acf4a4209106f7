"""Code-object metadata of the closed-loop retarget kernel (csrc/retarget.hip) through tools/kernel_meta.py, no GPU needed.
It has no private segment: its few arrays (a goal's three floats) are indexed by constants.  Its static LDS is the reduction
scratch alone, two ints per wave of the 1024-thread workgroup; the bitmaps are dynamic LDS, 3*W*W bytes chosen at launch, and
whatever else were static would come off the 64 KB the widest tap needs."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS = 1024                          # csrc/retarget.h RETARGET_THREADS
REDUCTION_SCRATCH = 2 * (THREADS // 64) * 4


def test_retarget_kernel_uses_no_scratch_and_no_static_lds_beyond_the_reduction():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    mine = [n for n in ks if "drag_retarget_kernel" in n]
    assert len(mine) == 1, mine
    k = ks[mine[0]]
    assert k.get(".private_segment_fixed_size", 0) == 0, k.get(".private_segment_fixed_size")
    assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, k
    assert k.get(".group_segment_fixed_size", 0) <= REDUCTION_SCRATCH, k.get(".group_segment_fixed_size")
    assert k.get(".max_flat_workgroup_size", 0) == THREADS
    assert k.get(".vgpr_count", 0) <= 128, k.get(".vgpr_count")         # 16 waves on four SIMDs of 512 VGPRs: 4 waves x 128
