"""Code-object metadata of the decoder's field kernels (csrc/decode_field.hip, the MLP in csrc/decode_mlp.h) through tools/kernel_meta.py, no GPU needed:
both must keep everything in registers.  They hold the state of a forward AND a backward of a 32-point tile; a private segment
would mean that part of it went to scratch memory."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_field_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for name in ("triplane_field_kernel", "triplane_project_kernel"):
        mine = [n for n in ks if name in n]
        assert len(mine) == 1, (name, mine)
        k = ks[mine[0]]
        assert k.get(".private_segment_fixed_size", 0) == 0, (mine[0], k.get(".private_segment_fixed_size"))
        assert k.get(".vgpr_spill_count", 0) == 0, (mine[0], k.get(".vgpr_spill_count"))
