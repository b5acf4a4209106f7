"""Snapshot and restore of a kept forward (ishap_unet_snapshot_*) and its use by DragStuff.training(): the first guided step of
every edit of a loaded shape has the same input, timestep and weights, so its forward is run once and put back afterwards.
Everything here is compared bit for bit: a restore puts bytes back, and the kernels that read them are deterministic."""
import ctypes as C
from argparse import Namespace

import numpy as np
import pytest
import torch

from ishapediting_amd import _lib, synthetic
from ishapediting_amd.unet_spec import UNetConfig, tiny_config

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def wide64_config():
    """64^2 .. 8^2 maps, 32 .. 128 channels: the 64^2 level takes the full-map GroupNorm route and unsliced convolutions, the
    levels below the group-local route and (16^2, 8^2) K-sliced convolutions whose slices the next GroupNorm adds up."""
    return UNetConfig(image_size=64, in_channels=6, model_channels=32, out_channels=12, num_res_blocks=1,
                      attention_resolutions="8", channel_mult=(1, 2, 3, 4), num_head_channels=32)


def _gn_route(H, ch):
    r = C.c_int()
    _lib.check(_lib.lib().ishap_group_norm32_plan(1, H, H, ch, 0, 0, 0, 1, 0, 0, 0, C.byref(r), None, None, None, None, None, None,
                                                  None, None, 0))
    return r.value


def _conv_ksplit(H, ch, pending):
    ks, slot, kern = C.c_int(), C.c_int(), C.create_string_buffer(256)
    _lib.check(_lib.lib().ishap_igemm_plan(H * H, ch, ch, 9, 0, H, H, 1, int(pending), 0, C.byref(ks), C.byref(slot), kern, len(kern)))
    return ks.value


def test_wide64_config_has_both_groupnorm_routes_and_both_convolution_launch_kinds():
    """What case (b) below relies on, through the planning calls (nothing is launched): the ResBlock convolutions c -> c on the
    four levels, each feeding the GroupNorm of its level."""
    cfg = wide64_config()
    levels = [(cfg.image_size >> i, cfg.model_channels * m) for i, m in enumerate(cfg.channel_mult)]
    routes = [_gn_route(H, ch) for H, ch in levels]
    local = [r in (2, 3) for r in routes]
    assert any(local) and any(r in (1, 4) for r in routes), routes
    splits = [_conv_ksplit(H, ch, loc) for (H, ch), loc in zip(levels, local)]        # a group-local consumer adds the slices up
    assert any(k == 1 for k in splits) and any(k > 1 for k in splits), splits


def _inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, cfg.in_channels, cfg.image_size, cfg.image_size, generator=g).to(dev())


def _forward(m, x, t, feat_layer, overlap):
    out, _ = m(x, torch.tensor([float(t)]), feat_layer=feat_layer, keep_for_backward=True, want_inter_feat=False,
               overlap_tail=overlap)
    return out


def _close(m, overlap):
    if overlap:
        m.run_tail()
        m.join_tail()


def _snapshot_sequence(cfg, seed, feat_layer, overlap):
    from ishapediting_amd.unet import UNetModel
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(cfg, seed))
    m = UNetModel(cfg, dev())
    m.load_state_dict(sd)
    assert not m.has_snapshot() and m.snapshot_bytes() == 0
    with pytest.raises(RuntimeError, match="no valid snapshot"):
        m.snapshot_restore()
    ch, sz = m.tap_shape(feat_layer)
    g = torch.Generator().manual_seed(seed + 1)
    cot = (torch.randn(1, sz * sz, ch, generator=g) * 0.05).half().to(dev())
    x0 = _inputs(cfg, seed + 2)
    # 1. forward with keep, backward with a fixed cotangent (beside the planned tail when overlapping)
    out1 = _forward(m, x0, 37, feat_layer, overlap)
    g1 = m.backward_input(cot).clone()
    _close(m, overlap)
    tap1 = m.copy_tap(feat_layer).clone()
    out1 = out1.clone()
    # 2. save
    ws0 = m.workspace_bytes()
    assert m.snapshot_save() and m.has_snapshot()
    assert m.snapshot_bytes() > tap1.numel() * 2 and m.workspace_bytes() == ws0 + m.snapshot_bytes()
    # 3. two forwards on other inputs and timesteps overwrite the arena (the second one leaves its tail to the restore's join)
    for k, t in ((3, 911), (4, 5)):
        _forward(m, _inputs(cfg, seed + k), t, feat_layer, overlap)
        m.backward_input(cot)
        if k == 3:
            _close(m, overlap)
    assert not torch.equal(m.copy_tap(feat_layer), tap1)
    # 4. / 5. restore: the backward and the tap are the first forward's
    assert m.snapshot_restore()
    assert torch.equal(m.copy_tap(feat_layer), tap1)
    g2 = m.backward_input(cot).clone()
    assert torch.equal(g1, g2)
    assert torch.equal(m.backward_input(cot), g1)               # a second backward on the restored state
    # 6. a second restore (after another forward in between)
    _forward(m, _inputs(cfg, seed + 5), 500, feat_layer, overlap)
    _close(m, overlap)
    assert m.snapshot_restore()
    assert torch.equal(m.backward_input(cot), g1) and torch.equal(m.copy_tap(feat_layer), tap1)
    if overlap:            # the snapshot of a forward with a planned tail ends at the tap
        with pytest.raises(RuntimeError, match="up to the tap only"):
            m.backward_from_output(torch.zeros_like(out1))
    else:                  # the whole forward was kept: the full-depth backward runs on the restored state
        cot_out = torch.zeros_like(out1)
        cot_out[:, :, ::7, ::5] = 1e-3
        ga = m.backward_from_output(cot_out).clone()
        _forward(m, x0, 37, feat_layer, overlap)
        assert torch.equal(m.backward_from_output(cot_out), ga)
        assert m.snapshot_restore()
    assert int(_lib.lib().ishap_device_status()) == 0
    # 7. a weight load invalidates the snapshot: restore fails and launches nothing (the resident tap stays the last forward's)
    m.load_state_dict(sd)
    assert not m.has_snapshot()
    _forward(m, _inputs(cfg, seed + 6), 250, feat_layer, overlap)
    _close(m, overlap)
    tap_b = m.copy_tap(feat_layer).clone()
    with pytest.raises(RuntimeError, match="no valid snapshot"):
        m.snapshot_restore()
    assert torch.equal(m.copy_tap(feat_layer), tap_b)
    assert torch.equal(m.backward_input(cot), m.backward_input(cot))          # and the kept forward is still differentiable
    # a forward of another tap invalidates it too; convert_to_fp16 drops the buffers
    assert m.snapshot_save() and m.has_snapshot()
    _forward(m, x0, 37, feat_layer - 1, False)
    assert not m.has_snapshot()
    with pytest.raises(RuntimeError, match="no valid snapshot"):
        m.snapshot_restore()
    _forward(m, x0, 37, feat_layer, False)
    assert m.snapshot_save() and m.snapshot_bytes() > 0
    m.convert_to_fp16()
    assert not m.has_snapshot() and m.snapshot_bytes() == 0
    torch.cuda.synchronize()
    assert int(_lib.lib().ishap_device_status()) == 0


@pytest.mark.parametrize("overlap", [False, True])
def test_snapshot_restore_tiny_net(overlap):
    """(a) the 16x16 net of the golden fixtures: plain, up and down ResBlocks, attention, the 1x1 skip, concatenation."""
    _snapshot_sequence(tiny_config(1), 211, feat_layer=2, overlap=overlap)


@pytest.mark.parametrize("overlap", [False, True])
def test_snapshot_restore_64x64_net(overlap):
    """(b) both GroupNorm routes and sliced as well as unsliced convolutions below the tap (output block 6 of 8, on the 64^2 map)."""
    _snapshot_sequence(wide64_config(), 223, feat_layer=6, overlap=overlap)


def test_snapshot_unavailable_while_the_profile_records():
    from ishapediting_amd.unet import UNetModel
    cfg = tiny_config(1)
    m = UNetModel(cfg, dev())
    m.load_state_dict(synthetic.round_torso_to_fp16(synthetic.unet_state_dict(cfg, 211)))
    _forward(m, _inputs(cfg, 1), 37, 2, False)
    assert m.snapshot_save()
    L = _lib.lib()
    L.ishap_profile_begin()
    try:
        assert m.snapshot_restore() is False and m.snapshot_save() is False
    finally:
        out = (C.c_double * 39)()
        L.ishap_profile_end(out, 13)
    assert m.has_snapshot() and m.snapshot_restore() is True


# ------------------------------------------------------------------------------------------------ (c) the drag loop
def _tiny(gold):
    """The tiny DragStuff of tests/test_gpu_batched_drag.py.  Its 6-channel latent is no triplane, so `volume` is the decoder's
    volume of the latent tiled to 96 channels: a deterministic function of the edit's result, decoded on the device."""
    from ishapediting_amd.drag_utils import DragStuff
    from ishapediting_amd.triplane_decoder import decode_volume
    g = gold("g8_g9_tiny_loops")
    Tn, w_time, feat_layer, r1, B = g["meta"].tolist()
    args = Namespace(clip_denoised=True, num_samples=1, batch_size=1, use_ddim=False, num_steps=Tn, image_size=16,
                     num_channels=32, num_res_blocks=1, num_heads=4, num_heads_upsample=-1, num_head_channels=32,
                     attention_resolutions="8", channel_mult="1,2", dropout=0.1, class_cond=False, shape_resolution=32,
                     use_checkpoint=False, use_scale_shift_norm=True, resblock_updown=True, use_fp16=True,
                     use_new_attention_order=False, in_out_channels=6, learn_sigma=True, diffusion_steps=1000,
                     noise_schedule="linear", timestep_respacing=str(Tn), w_time=w_time, feat_layer=feat_layer,
                     loss_type="l2", use_kl=False, predict_xstart=False, rescale_timesteps=False,
                     rescale_learned_sigmas=False, explicit_normalization=False)
    ds = DragStuff(dev(), args=args)
    ds.model.load_state_dict(synthetic.round_torso_to_fp16(synthetic.unet_state_dict(tiny_config(1), 101)))
    ds.decoder.net.load_state_dict(synthetic.decoder_state_dict(4321))
    ds.set_offset1(r1)
    ds.voxel_size = 2.0 / 32

    def get_mesh(tri_feat=None, img=None, t=0):
        if tri_feat is None:
            tri_feat = ds._denoise(img, t)
        ds.tri_feat = tri_feat
        ds.volume = decode_volume(ds.decoder, tri_feat.repeat(1, 16, 1, 1).contiguous(), 1.0, 0.0, 32)
    ds.get_mesh = get_mesh
    return ds, g, (Tn, w_time)


SRC1 = np.array([[-0.3, 0.2, -0.1], [0.35, -0.25, 0.4]], np.float32)
TGT1 = np.array([[-0.1, 0.3, -0.2], [0.3, -0.05, 0.25]], np.float32)


def _two_edits(gold, monkeypatch, reuse, overlap):
    from ishapediting_amd import drag_utils as du
    monkeypatch.setattr(du, "_FIRST_STEP_REUSE", reuse)
    ds, g, (Tn, w_time) = _tiny(gold)
    ds.overlap_tail = overlap
    ns, dn = T(g["loop_noise_sampling"]).to(dev()), T(g["drag_noise"]).to(dev())
    ds.step_noise = lambda i: ns[Tn - 1 - i]
    ds.update_latent_params(img=g["loop_latent0"])
    ds.step_noise = lambda i: dn[w_time - 1 - i]
    res = []
    for src, tgt in ((g["drag_sources"], g["drag_targets"]), (SRC1, TGT1), (g["drag_sources"], g["drag_targets"])):
        prog = list(ds.training(src, tgt, scale=50.0, cof=0.4))
        torch.cuda.synchronize()
        assert len(prog) == w_time and len(ds.last_losses) == w_time
        res.append((ds.tri_feat.clone(), [l.clone() for l in ds.last_losses], ds.volume.clone()))
    assert (ds._first_step is not None) == reuse and (ds.model.snapshot_bytes() > 0) == reuse
    assert int(_lib.lib().ishap_device_status()) == 0
    return res


@pytest.mark.parametrize("overlap", [True, False])
def test_edits_with_the_first_step_reused_equal_edits_without(gold, monkeypatch, overlap):
    """Two edits with different handles, then the first one again: with reuse the second and third restore the snapshot the first
    took.  tri_feat, every loss and the decoded volume are bitwise those of the run that calls the model in every step."""
    on = _two_edits(gold, monkeypatch, True, overlap)
    off = _two_edits(gold, monkeypatch, False, overlap)
    for e, ((tf_a, ls_a, vol_a), (tf_b, ls_b, vol_b)) in enumerate(zip(on, off)):
        assert torch.equal(tf_a, tf_b), e
        assert len(ls_a) == len(ls_b) and all(torch.equal(a, b) for a, b in zip(ls_a, ls_b)), e
        assert torch.equal(vol_a, vol_b), e
    assert not torch.equal(on[0][0], on[1][0])                                    # other handles: another result
    assert torch.equal(on[0][0], on[2][0]) and torch.equal(on[0][2], on[2][2])    # the same edit again (injected noise): the same


def test_in_place_edit_of_w_and_a_new_shape_take_a_new_snapshot(gold, monkeypatch):
    from ishapediting_amd import drag_utils as du
    monkeypatch.setattr(du, "_FIRST_STEP_REUSE", True)
    ds, g, (Tn, w_time) = _tiny(gold)
    ns, dn = T(g["loop_noise_sampling"]).to(dev()), T(g["drag_noise"]).to(dev())
    ds.step_noise = lambda i: ns[Tn - 1 - i]
    ds.update_latent_params(img=g["loop_latent0"])
    ds.step_noise = lambda i: dn[w_time - 1 - i]
    run = lambda: (list(ds.training(SRC1, TGT1, scale=50.0, cof=0.4)), ds.tri_feat.clone())[1]      # noqa: E731
    a = run()
    kept = ds._first_step
    assert torch.equal(run(), a) and ds._first_step is kept                       # reused
    ds.w.mul_(0.5)                                                                # in place: the tensor's version moves on
    b = run()
    assert ds._first_step is not kept and not torch.equal(a, b)
    monkeypatch.setattr(du, "_FIRST_STEP_REUSE", False)
    assert torch.equal(run(), b)                                                  # what the plain loop gives from the edited w
