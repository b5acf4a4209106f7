"""CPU checks of batched drag edits: handle packing, per-edit arguments, rejection messages, and the new kernels' code-object
metadata (no GPU needed)."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pack_handles_builds_csr_offsets():
    from ishapediting_amd.drag_utils import pack_handles
    a = np.array([[0.1, 0.2, 0.3]], np.float32)
    b = torch.tensor([[0.4, 0.5, 0.6], [0.7, 0.8, 0.9], [-0.1, -0.2, -0.3]])
    c = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    src, tgt, offs = pack_handles([a, b, c], [a + 1, b + 1, np.asarray(c) + 1])
    assert offs == [0, 1, 4, 6]
    assert src.dtype == torch.float32 and tuple(src.shape) == (6, 3) and src.is_contiguous()
    assert torch.equal(src[1:4], b) and torch.equal(tgt[4:6], torch.tensor(c) + 1)
    np.testing.assert_array_equal(src[0].numpy(), a[0])


def test_pack_handles_rejects_mismatched_counts():
    from ishapediting_amd.drag_utils import pack_handles
    a = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError, match="2 source sets but 1 target sets"):
        pack_handles([a, a], [a])
    with pytest.raises(ValueError, match="edit 1: 2 sources and 1 targets"):
        pack_handles([a, a], [a, a[:1]])
    with pytest.raises(ValueError, match="edit 0: 0 sources"):
        pack_handles([a[:0]], [a[:0]])
    with pytest.raises(ValueError, match="no edits"):
        pack_handles([], [])


def test_scale_and_cof_broadcast_per_edit():
    from ishapediting_amd.drag_utils import per_edit
    assert per_edit(600, 3, "scale") == [600.0] * 3
    assert per_edit(0.2, 2, "cof") == [0.2, 0.2]
    assert per_edit([0, 50, 100], 3, "scale") == [0.0, 50.0, 100.0]
    assert per_edit(np.array([1.5, 2.5]), 2, "scale") == [1.5, 2.5]
    assert per_edit(torch.tensor(3.0), 2, "cof") == [3.0, 3.0]
    with pytest.raises(ValueError, match="scale: 2 values for 3 edits"):
        per_edit([1.0, 2.0], 3, "scale")
    with pytest.raises(ValueError, match="cof: 4 values for 3 edits"):
        per_edit((0.1, 0.2, 0.3, 0.4), 3, "cof")


def _unbuilt_dragstuff(max_edits):
    """A DragStuff without its model context (no GPU here): training_batch validates its request before any device work."""
    from ishapediting_amd.drag_utils import DragStuff
    ds = DragStuff.__new__(DragStuff)
    ds.max_edits = max_edits
    return ds


def test_training_batch_rejects_more_edits_than_max_edits():
    h = np.zeros((1, 3), np.float32)
    ds = _unbuilt_dragstuff(2)
    with pytest.raises(ValueError, match="3 edits requested but this DragStuff was built for max_edits=2"):
        next(ds.training_batch([h] * 3, [h] * 3))
    with pytest.raises(ValueError, match="3 source sets but 2 target sets"):
        next(ds.training_batch([h] * 3, [h] * 2))
    with pytest.raises(ValueError, match="scale: 3 values for 2 edits"):
        next(ds.training_batch([h] * 2, [h] * 2, scale=[1.0, 2.0, 3.0]))
    from ishapediting_amd.drag_utils import check_edit_count
    check_edit_count(2, 2)
    with pytest.raises(ValueError, match="no edits"):
        check_edit_count(0, 2)


def test_batch_scratch_size_and_version():
    from ishapediting_amd import _lib
    L = _lib.lib()
    assert L.ishap_version() >= 4
    one = L.ishap_drag_batch_scratch_bytes(1, 64, 512)
    four = L.ishap_drag_batch_scratch_bytes(4, 64, 512)
    assert one >= 64 * 64 * 512 * 8 + 16 + 4 + 3 * 64 * 64 + 3 * 512
    assert four >= 4 * 64 * 64 * 512 * 8 and four > 3 * one
    assert L.ishap_drag_batch_scratch_bytes(0, 64, 512) < 0


def test_batched_drag_kernels_use_no_scratch():
    """The kernels the batched edit adds, by name, in the built library's code-object metadata: private segment 0 bytes."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    names = ["drag_batch_touch_kernel", "drag_batch_count_kernel", "drag_batch_terms_kernel", "drag_batch_gather_kernel",
             "drag_batch_finish_kernel", "drag_batch_scale_kernel", "ddpm_step_kernelILb1E"]
    for want in names:
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        assert ks[found[0]].get(".private_segment_fixed_size", 0) == 0, (want, ks[found[0]])
