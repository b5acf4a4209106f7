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


# ------------------------------------------------------------------------------------------------ the shared guided loop
class _TailModel:
    """What p_sample_guidance needs of a model up to `between`: a forward with a tap, and the planned tail's two calls."""

    def __init__(self, run_tail_error=None):
        self.calls, self.run_tail_error = [], run_tail_error

    def tap_ptr(self):
        return 0

    def __call__(self, x, ts, feat_layer=-1, **kw):
        self.calls.append(("forward", kw.get("overlap_tail", False)))
        return torch.zeros(x.shape[0], 2 * x.shape[1], *x.shape[2:]), None

    def run_tail(self):
        self.calls.append("run_tail")
        if self.run_tail_error is not None:
            raise self.run_tail_error

    def join_tail(self):
        self.calls.append("join_tail")


def test_failing_run_tail_neither_skips_join_tail_nor_hides_what_between_raised():
    from ishapediting_amd.gaussian_diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(timestep_respacing="10")
    x = torch.zeros(1, 6, 4, 4)

    def between():
        raise ValueError("the loss failed")

    second = RuntimeError("ishap error -3")
    m = _TailModel(run_tail_error=second)
    with pytest.raises(ValueError, match="the loss failed") as ei:
        d.p_sample_guidance(m, x, 3, feat_layer=1, keep_for_backward=True, between=between, overlap=True)
    assert m.calls == [("forward", True), "run_tail", "join_tail"]
    assert ei.value.__cause__ is second                  # the second failure is chained, not lost
    # a tail that closes cleanly: the same exception, nothing chained
    m = _TailModel()
    with pytest.raises(ValueError, match="the loss failed") as ei:
        d.p_sample_guidance(m, x, 3, feat_layer=1, keep_for_backward=True, between=between, overlap=True)
    assert m.calls == [("forward", True), "run_tail", "join_tail"] and ei.value.__cause__ is None
    # the plain sequence plans no tail and closes none
    m = _TailModel()
    with pytest.raises(ValueError, match="the loss failed"):
        d.p_sample_guidance(m, x, 3, feat_layer=1, keep_for_backward=True, between=between, overlap=False)
    assert m.calls == [("forward", False)]


class _LoopModel:
    def tap_shape(self, feat_layer):
        return 16, 4                   # channels, width

    def tap_ptr(self):
        return 1000

    def backward_input(self, cot, scale2):
        return "grad"


class _LoopDiffusion:
    def __init__(self, log):
        self.log = log

    def prepare(self, model, indices):
        self.log.append(("prepare", list(indices)))

    def p_sample_guidance(self, model, x, t, **kw):
        self.log.append(("step", t, kw))
        if kw.get("between") is not None:
            assert kw["between"]() == "grad"
        return {"guided": x + 1, "sample": x + 1}


def _loop_dragstuff(monkeypatch, log):
    """A DragStuff without its model context; the two kernels classes replaced by recorders of the calls the loop makes."""
    from argparse import Namespace
    from ishapediting_amd import drag_utils as du

    def recorder(batched):
        class Kernels:
            def __init__(self, device, *a, **kw):
                log.append(("kernels", batched, a[0] if batched else None, kw["W"], kw["ld"], kw["r"], kw["loss_type"]))

            def setup(self, sources, targets, cof):
                log.append(("setup", batched, cof))

            def loss_cotangent_ptr(self, edit_ptr, orig_ptr, orig_stride=0, loss_out=None):
                log.append(("loss", batched, edit_ptr, orig_stride, tuple(loss_out.shape)))
                return "cot", "scale2"
        return Kernels
    monkeypatch.setattr(du, "DragKernels", recorder(False))
    monkeypatch.setattr(du, "BatchDragKernels", recorder(True))
    ds = du.DragStuff.__new__(du.DragStuff)
    ds.args = Namespace(num_samples=1, w_time=3, feat_layer=2, loss_type="l2", clip_denoised=True)
    ds.device, ds.max_edits = torch.device("cpu"), 2
    ds.model, ds.diffusion = _LoopModel(), _LoopDiffusion(log)
    ds.r1, ds.voxel_size, ds.step_noise = 2, 0.25, None
    ds.overlap_tail = True                           # whatever ISHAP_OVERLAP_TAIL / ISHAP_FUSED_UPDATE say in this environment
    monkeypatch.setattr(du, "_FUSED_UPDATE", True)
    ds.w, ds.w_batch = torch.zeros(1, 6, 4, 4), None
    ds.feature_guidance = [torch.zeros(16, 16, dtype=torch.float16) for _ in range(3)]
    ds.get_mesh = lambda tri_feat=None, img=None, t=0: log.append(("get_mesh", float(img.mean()), t))
    ds.get_meshes = lambda img, t=0: log.append(("get_meshes", float(img.mean()), t))
    loops, bodies = [], []
    inner, body = du.DragStuff._guided_loop, du.DragStuff._edits
    monkeypatch.setattr(du.DragStuff, "_guided_loop", lambda self, *a: (loops.append(1), inner(self, *a))[1])
    monkeypatch.setattr(du.DragStuff, "_edits", lambda self, *a, **kw: (bodies.append(1), body(self, *a, **kw))[1])
    return ds, loops, bodies


def test_training_and_training_batch_drive_one_guided_loop(monkeypatch):
    """Both entry points run the one edit body, DragStuff._edits, and through it DragStuff._guided_loop; for K = 1 the steps they
    issue differ in the guidance scale (a float against a device tensor) and in nothing else -- same keyword set, same loss
    slot, same progress values."""
    h = np.array([[0.1, 0.2, 0.3]], np.float32)
    runs = {}
    for name in ("training", "training_batch"):
        log = []
        ds, loops, bodies = _loop_dragstuff(monkeypatch, log)
        args = (h, h + 0.1) if name == "training" else ([h], [h + 0.1])
        prog = list(getattr(ds, name)(*args, scale=50, cof=0.4))
        assert loops == [1] and bodies == [1], name
        assert prog == [0.0, 0.5, 1.0] and len(ds.last_losses) == 3 and all(l.shape == (1,) for l in ds.last_losses)
        runs[name] = log
    solo, batch = runs["training"], runs["training_batch"]
    assert [e[0] for e in solo] == ["kernels", "setup", "prepare"] + ["step", "loss"] * 3 + ["get_mesh"]
    assert [e[0] for e in batch] == ["kernels", "setup", "prepare"] + ["step", "loss"] * 3 + ["get_meshes"]
    assert solo[0] == ("kernels", False, None, 4, 16, 2, "l2") and batch[0] == ("kernels", True, 1, 4, 16, 2, "l2")
    assert solo[1] == ("setup", False, 0.4) and batch[1] == ("setup", True, [0.4])
    assert solo[2] == batch[2] == ("prepare", [0, 1, 2])
    for a, b in zip(solo[3:-1], batch[3:-1]):
        if a[0] == "loss":                 # tap pointer, orig_stride 0 (one shape: shared guidance), a one-float loss slot
            assert a[2:] == b[2:] == (1000, 0, (1,))
            continue
        assert a[1] == b[1] and set(a[2]) == set(b[2])
        ka, kb = dict(a[2]), dict(b[2])
        assert isinstance(ka.pop("guided_scale"), float) and torch.equal(kb.pop("guided_scale"), torch.tensor([50.0]))
        assert callable(ka.pop("between")) and callable(kb.pop("between"))
        assert ka == kb == dict(feat_layer=2, keep_for_backward=True, want_inter_feat=False, noise=None, overlap=True,
                                want_noise=False)
    assert solo[-1] == ("get_mesh", 3.0, 0) and batch[-1] == ("get_meshes", 3.0, 0)
