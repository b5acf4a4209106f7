"""CPU checks of the first-step reuse of DragStuff.training(): which edits call the model in their first guided step, what
invalidates the snapshot, the switch, the fall-back while a restore is unavailable, and the tail after a failing step.  The
model is a stub that counts its calls; the diffusion is the real one with the step arithmetic (a device kernel) replaced."""
from argparse import Namespace

import numpy as np
import pytest
import torch

W_TIME = 40
H = np.array([[0.1, 0.2, 0.3]], np.float32)


class _Model:
    """What the guided loop and p_sample_guidance use of UNetModel, with the library's snapshot rules."""

    def __init__(self):
        self.forwards = []            # (timestep, overlap_tail) of every model call
        self.saves = self.restores = 0
        self.snap = False
        self.available = True         # False: the per-launch profile is recording
        self.pending = False          # a planned tail that has not been joined

    def tap_shape(self, feat_layer):
        return 16, 4

    def tap_ptr(self):
        return 1000

    def backward_input(self, cot, scale2):
        return torch.zeros(1, 6, 4, 4)

    def __call__(self, x, ts, feat_layer=-1, keep_for_backward=False, want_inter_feat=True, overlap_tail=False):
        self.forwards.append((int(ts[0]), overlap_tail))
        self.pending = overlap_tail
        return torch.full((x.shape[0], 2 * x.shape[1], *x.shape[2:]), float(len(self.forwards))), None

    def run_tail(self):
        pass

    def join_tail(self):
        self.pending = False

    def load_state_dict(self, sd, strict=True):
        self.snap = False

    def convert_to_fp16(self):
        self.snap = False

    def eval(self):
        return self

    def has_snapshot(self):
        return self.snap

    def snapshot_save(self):
        if not self.available:
            return False
        self.pending = False
        self.snap = True
        self.saves += 1
        return True

    def snapshot_restore(self):
        if not self.snap:
            raise RuntimeError("no valid snapshot")
        if not self.available:
            return False
        self.pending = False
        self.restores += 1
        return True


def _dragstuff(monkeypatch, reuse=True, overlap=True):
    from ishapediting_amd import drag_utils as du
    from ishapediting_amd.gaussian_diffusion import create_gaussian_diffusion

    class Kernels:
        def __init__(self, device, *a, **kw):
            pass

        def setup(self, sources, targets, cof):
            pass

        def loss_cotangent_ptr(self, edit_ptr, orig_ptr, orig_stride=0, loss_out=None):
            return "cot", "scale2"
    monkeypatch.setattr(du, "DragKernels", Kernels)
    monkeypatch.setattr(du, "_FUSED_UPDATE", True)
    monkeypatch.setattr(du, "_FIRST_STEP_REUSE", reuse)
    ds = du.DragStuff.__new__(du.DragStuff)
    ds.args = Namespace(num_samples=1, w_time=W_TIME, feat_layer=2, loss_type="l2", clip_denoised=True, use_fp16=True, num_steps=50)
    ds.device, ds.max_edits = torch.device("cpu"), 1
    ds.model = _Model()
    ds.diffusion = create_gaussian_diffusion(timestep_respacing="50")
    ds.used = []                      # the model output every step kernel was given
    ds.diffusion._step = lambda x, mo, *a, **kw: (ds.used.append(float(mo.flatten()[0])), {"guided": x + 1})[1]
    ds.r1, ds.voxel_size, ds.step_noise = 2, 0.25, None
    ds.overlap_tail = overlap
    ds.w, ds.w_batch = torch.zeros(1, 6, 4, 4), None
    ds.feature_guidance = [torch.zeros(16, 16, dtype=torch.float16) for _ in range(W_TIME)]
    ds.get_mesh = lambda tri_feat=None, img=None, t=0: None
    return ds


def _edit(ds):
    """One training() call: (model calls it made, timestep of the first one, the model output its first step kernel used)."""
    n0, u0 = len(ds.model.forwards), len(ds.used)
    prog = list(ds.training(H, H + 0.1, scale=50, cof=0.4))
    assert len(prog) == W_TIME and len(ds.used) - u0 == W_TIME
    calls = ds.model.forwards[n0:]
    return len(calls), calls[0][0], ds.used[u0]


def test_second_edit_restores_the_first_step_and_calls_the_model_39_times(monkeypatch):
    ds = _dragstuff(monkeypatch)
    t_first = ds.diffusion.timestep_map[W_TIME - 1]
    t_second = ds.diffusion.timestep_map[W_TIME - 2]
    assert _edit(ds) == (W_TIME, t_first, 1.0)                 # the first edit runs every forward and saves after the first
    assert (ds.model.saves, ds.model.restores) == (1, 0)
    for k in range(2):                                         # later edits: no model call in the first iteration, 39 afterwards,
        assert _edit(ds) == (W_TIME - 1, t_second, 1.0)        # and the step kernel gets the kept output of the very first call
        assert (ds.model.saves, ds.model.restores) == (1, 1 + k)
    assert not ds.model.pending


def test_switch_off_runs_40_forwards_and_takes_no_snapshot(monkeypatch):
    ds = _dragstuff(monkeypatch, reuse=False)
    for _ in range(2):
        assert _edit(ds)[0] == W_TIME
    assert (ds.model.saves, ds.model.restores) == (0, 0) and ds._first_step is None


def _new_w(ds):
    ds.w = torch.ones(1, 6, 4, 4)


def _in_place(ds):
    ds.w.add_(1.0)


def _stub_sampling(ds):
    """update_latent_params' denoising loop without a model: `each` sees the steps w_time .. 0."""
    ds._denoise = lambda img, t, each=None, **kw: ([each(i, img) for i in range(ds.args.w_time, -1, -1)], img)[1]
    ds.model.copy_tap = lambda k, K=None: torch.zeros(1, 16, 16, dtype=torch.float16)


def _update_latent_params(ds):
    _stub_sampling(ds)
    ds.feature_guidance = []
    ds.update_latent_params(img=torch.zeros(1, 6, 4, 4))


def _update_latent_params_batch(ds):
    _stub_sampling(ds)
    ds.update_latent_params_batch(torch.zeros(1, 6, 4, 4))


def _latent_inversion(ds):
    ds.diffusion.ddpm_inversion = lambda *a, **kw: {"latent": torch.zeros(1, 6, 4, 4), "sample": torch.zeros(1, 6, 4, 4),
                                                    "variance": [], "variance_noise": []}
    ds.variance, ds.variance_noise = [], []
    ds.latent_inversion(torch.zeros(1, 6, 4, 4))
    ds.feature_guidance = [torch.zeros(16, 16, dtype=torch.float16) for _ in range(W_TIME)]


def _clear_params(ds):
    ds.noise, ds.variance, ds.variance_noise = [], [], []
    ds.clear_params()
    ds.w = torch.zeros(1, 6, 4, 4)
    ds.feature_guidance = [torch.zeros(16, 16, dtype=torch.float16) for _ in range(W_TIME)]


def _load_weights(ds):
    ds.decoder = Namespace(net=Namespace(load_state_dict=lambda sd: None), eval=lambda: None)
    ds.load_weights({}, {})


def _update_model_params(ds, tmp):
    import os
    os.makedirs(tmp / "ddpm_x")
    os.makedirs(tmp / "statistics" / "s")
    torch.save({}, tmp / "ddpm_x" / "ema_0.pt")
    torch.save({}, tmp / "decoder.pt")
    ds.args.explicit_normalization = False
    ds.decoder = Namespace(net=Namespace(load_state_dict=lambda sd: None), eval=lambda: None)
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        ds.update_model_params(str(tmp))
    finally:
        os.chdir(cwd)


def _feat_layer(ds):
    ds.args.feat_layer = 1


def _overlap(ds):
    ds.overlap_tail = False


def _timestep_map(ds):
    ds.diffusion.timestep_map = [t + 1 for t in ds.diffusion.timestep_map]


@pytest.mark.parametrize("event", [_new_w, _in_place, _update_latent_params, _update_latent_params_batch, _latent_inversion,
                                   _clear_params, _load_weights, _update_model_params, _feat_layer, _overlap, _timestep_map],
                         ids=lambda f: f.__name__.strip("_"))
def test_every_change_of_the_shape_state_forces_a_fresh_forward(monkeypatch, tmp_path, event):
    ds = _dragstuff(monkeypatch)
    assert _edit(ds)[0] == W_TIME and _edit(ds)[0] == W_TIME - 1
    if event is _update_model_params:
        event(ds, tmp_path)
    else:
        event(ds)
    saves = ds.model.saves
    n, _, used = _edit(ds)
    assert n == W_TIME and used == float(len(ds.model.forwards) - W_TIME + 1)      # its own first forward's output
    assert ds.model.saves == saves + 1
    assert _edit(ds)[0] == W_TIME - 1                                                # and the new snapshot serves the next edit


def test_w_time_is_part_of_the_key(monkeypatch):
    ds = _dragstuff(monkeypatch)
    assert _edit(ds)[0] == W_TIME
    key = ds._first_step["key"]
    ds.args.w_time = W_TIME - 1
    assert ds._first_step_key(True) != key


def test_restore_unavailable_falls_back_to_the_forward_and_keeps_the_snapshot(monkeypatch):
    ds = _dragstuff(monkeypatch)
    assert _edit(ds)[0] == W_TIME
    kept = ds._first_step
    ds.model.available = False                                 # the per-launch profile records: all 40 forwards run and count
    n, _, used = _edit(ds)
    assert n == W_TIME and used == float(W_TIME + 1)
    assert ds._first_step is kept and (ds.model.saves, ds.model.restores) == (1, 0)
    ds.model.available = True
    assert _edit(ds) == (W_TIME - 1, ds.diffusion.timestep_map[W_TIME - 2], 1.0)


def test_model_without_snapshot_calls_runs_the_plain_loop(monkeypatch):
    ds = _dragstuff(monkeypatch)

    class Plain:
        forwards = []

        def __getattr__(self, name):
            if name.startswith("snapshot") or name == "has_snapshot":
                raise AttributeError(name)
            return getattr(inner, name)

        def __call__(self, *a, **kw):
            return inner(*a, **kw)
    inner = ds.model
    ds.model = Plain()
    for _ in range(2):
        n0 = len(inner.forwards)
        list(ds.training(H, H + 0.1, scale=50, cof=0.4))
        assert len(inner.forwards) - n0 == W_TIME


def test_exception_in_between_on_a_reused_step_leaves_no_tail_pending(monkeypatch):
    ds = _dragstuff(monkeypatch)
    assert _edit(ds)[0] == W_TIME
    n0 = len(ds.model.forwards)
    ds.model.backward_input = lambda cot, scale2: (_ for _ in ()).throw(ValueError("the backward failed"))
    with pytest.raises(ValueError, match="the backward failed"):
        list(ds.training(H, H + 0.1, scale=50, cof=0.4))
    assert len(ds.model.forwards) == n0 and ds.model.restores == 1           # the failing step was the reused one: no model call,
    assert not ds.model.pending                                                # nothing planned, nothing left to join
    # p_sample_guidance itself: a kept model output plans no tail whatever `overlap` says, and closes none
    from ishapediting_amd.gaussian_diffusion import create_gaussian_diffusion
    d = create_gaussian_diffusion(timestep_respacing="10")
    x = torch.zeros(1, 6, 4, 4)
    m = _Model()
    m.run_tail = lambda: pytest.fail("no tail was planned")

    def between():
        raise ValueError("the loss failed")
    with pytest.raises(ValueError, match="the loss failed") as ei:
        d.p_sample_guidance(m, x, 3, feat_layer=1, keep_for_backward=True, between=between, overlap=True,
                            model_output=torch.zeros(1, 12, 4, 4))
    assert m.forwards == [] and not m.pending and ei.value.__cause__ is None


def test_abi_has_the_snapshot_calls():
    from ishapediting_amd import _lib
    L = _lib.lib()
    assert L.ishap_version() >= 15
    assert L.ishap_unet_snapshot_bytes(None) == 0
    for name in ("ishap_unet_snapshot_save", "ishap_unet_snapshot_restore", "ishap_unet_snapshot_drop"):
        assert getattr(L, name)(None, *([None] if name != "ishap_unet_snapshot_drop" else [])) != 0     # null context: an error
