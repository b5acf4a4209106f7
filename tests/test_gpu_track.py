"""The handle tracker on the device (csrc/track.hip) against the float64 oracle of tests/track_ref.py, the tie rule, repeatability,
batching, the argument checks, and tracking inside training() / training_batch() on the tiny model.

The bound on every entry of the distance volume is DESIGN.md 5.2l's (n + 8) 2^-24 M, M = sum(|shift| + |patch|) of that candidate in
float64 and n the length of the kernel's longest addition chain (track_ref.chain_length, from the summation order of
track_corr_kernel / track_argmin_kernel):
    n = ceil(P / nsub)   a lane adds its share of the P = (2 rp + 1)^2 patch terms of its channel in order (nsub = 64 / chunk width)
      + 6                butterfly levels over the 64 lanes of the wave
      + nchunk           the chunk sums of a plane map, in order
      + 2                the three planes
e.g. the real shape (R 4, rp 2, Cc 170, 64-channel chunks): n = 25 + 6 + 3 + 2 = 36.  None of it is tuned to what the device gives.
"""
from argparse import Namespace

import numpy as np
import pytest
import torch

from ishapediting_amd import _lib, synthetic
from ishapediting_amd.unet_spec import tiny_config
from tests import track_ref as K

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _tracker(c):
    from ishapediting_amd.drag_utils import HandleTracker
    return HandleTracker(dev(), c.W, c.ld, c.chmap, c.voxel, radius=c.R, patch=c.rp)


_RUNS = {}


def _device(name):
    """The case's batched call, run once per session and shared: one Track per edit, on the CPU."""
    if name not in _RUNS:
        c = K.make_case(name)
        out = _tracker(c).track_batch(c.edits.to(dev()), c.origs.to(dev()), c.sources, offsets=c.K_in, want_volume=True)
        torch.cuda.synchronize()
        _RUNS[name] = [type(t)(*(v.cpu() for v in t)) for t in out]
    return _RUNS[name]


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("name", K.CASES)
def test_distance_volume_within_the_chain_bound(name):
    c, o, d = K.make_case(name), K.oracle(name), _device(name)
    n = K.chain_length(c.R, c.rp, c.Cc)          # n: see the module docstring; 36 at the real shape
    for e in range(c.E):
        err = (d[e].volume.double() - o[e].D).abs()
        tol = (n + 8) * 2.0 ** -24 * o[e].M
        worst = float((err / tol.clamp_min(1e-300)).max())
        print(f"{name} edit {e}: n = {n}, max err / tol = {worst:.3f}, max err = {float(err.max()):.3e}")
        assert bool((err <= tol).all()), (name, e, worst)


@pytest.mark.parametrize("name", K.CASES)
def test_outputs_are_the_oracles_winner_and_the_volumes_own_entries(name):
    c, o, d = K.make_case(name), K.oracle(name), _device(name)
    centre = ((c.R * c.side) + c.R) * c.side + c.R
    for e in range(c.E):
        assert d[e].offsets.dtype == torch.int32 and d[e].positions.dtype == torch.float32
        assert np.array_equal(d[e].offsets.numpy(), c.K_in[e] + o[e].winner), (name, e)          # every handle, tie handles included
        idx = torch.from_numpy(o[e].index).long()[:, None]
        assert torch.equal(d[e].dist, d[e].volume.gather(1, idx)[:, 0])                         # bitwise
        assert torch.equal(d[e].dist0, d[e].volume[:, centre])
        want = K.lattice32(c.sources[e], c.voxel, d[e].offsets.numpy())
        assert np.array_equal(d[e].positions.numpy(), want)


def test_without_the_volume_the_outputs_are_the_same():
    c, d = K.make_case("B"), _device("B")
    t = _tracker(c).track(c.edits[0].to(dev()), c.origs[0].to(dev()), c.sources[0], offsets=c.K_in[0])
    assert t.volume is None
    assert torch.equal(t.offsets.cpu(), d[0].offsets) and torch.equal(t.dist.cpu(), d[0].dist) and torch.equal(t.dist0.cpu(), d[0].dist0)


# ------------------------------------------------------------------------------------------------ 2. ties
def test_ties():
    a = K.make_case("A")
    tr, src = _tracker(a), a.sources[0]
    zero = torch.zeros_like(a.edits[0]).to(dev())
    t = tr.track(zero, zero, src, want_volume=True)
    assert not t.offsets.any() and not t.volume.any() and not t.dist.any()               # all-zero taps: every D is 0, k* = 0
    same = a.origs[0].to(dev())
    t = tr.track(same, same.clone(), src)
    assert not t.offsets.any() and torch.equal(t.dist.cpu(), torch.zeros(len(src))) and torch.equal(t.dist0, t.dist)
    r = K.roll_case()
    rt = _tracker(r)
    t = rt.track(r.edit.to(dev()), r.orig.to(dev()), r.sources)
    assert tuple(t.offsets[0].tolist()) == r.k and float(t.dist[0]) == 0.0 and float(t.dist0[0]) > 1.0
    t = rt.track(r.edit.to(dev()), r.orig.to(dev()), r.sources, offsets=np.array([r.k], np.int32))      # found: it stays
    assert tuple(t.offsets[0].tolist()) == r.k and float(t.dist[0]) == 0.0 == float(t.dist0[0])


# ------------------------------------------------------------------------------------------------ 3. repeatability and batching
@pytest.mark.parametrize("name", ("B", "P16"))
def test_two_runs_are_equal(name):
    c, d = K.make_case(name), _device(name)
    again = _tracker(c).track_batch(c.edits.to(dev()), c.origs.to(dev()), c.sources, offsets=c.K_in, want_volume=True)
    for x, y in zip(again, d):
        assert all(torch.equal(u.cpu(), v) for u, v in zip(x, y))


@pytest.mark.parametrize("name", ("L", "Ls"))
def test_each_edit_of_a_batch_is_its_solo_run(name):
    c, d = K.make_case(name), _device(name)
    tr = _tracker(c)
    for e in range(c.E):
        o = c.origs[e if c.origs.shape[0] > 1 else 0]
        solo = tr.track(c.edits[e].to(dev()), o.to(dev()), c.sources[e], offsets=c.K_in[e], want_volume=True)
        assert all(torch.equal(u.cpu(), v) for u, v in zip(solo, d[e])), (name, e)


def test_radius_zero_returns_k_in():
    c = K.make_case("C")
    k_in = np.array([[3, -1, 0], [0, 0, 0], [-7, 2, 5]], np.int32)
    t = _tracker(c).track(c.edits[0].to(dev()), c.origs[0].to(dev()), c.sources[0], offsets=k_in, want_volume=True)
    assert np.array_equal(t.offsets.cpu().numpy(), k_in) and t.volume.shape == (3, 1) and torch.equal(t.dist, t.dist0)
    assert torch.equal(t.dist, t.volume[:, 0])


# ------------------------------------------------------------------------------------------------ 4. arguments
def test_invalid_arguments_raise_before_any_launch():
    from ishapediting_amd.drag_utils import HandleTracker
    c = K.make_case("A")
    for kw in ({"radius": 9}, {"radius": -1}, {"patch": 5}, {"patch": -1}):
        with pytest.raises(ValueError, match="radius"):
            HandleTracker(dev(), c.W, c.ld, c.chmap, c.voxel, **kw)
    with pytest.raises(ValueError, match="chmap"):
        HandleTracker(dev(), c.W, c.ld, c.chmap + c.ld, c.voxel)
    tr = _tracker(c)
    with pytest.raises(ValueError, match="edits"):
        tr.setup([c.sources[0][:1]] * 33)
    # the C call itself: outputs prefilled, nothing may be written
    L = _lib.lib()
    edit, orig = c.edits[0].to(dev()), c.origs[0].to(dev())
    src = T(c.sources[0]).to(dev())
    chmap = T(c.chmap).to(dev())
    B = len(c.sources[0])
    k_in = torch.zeros(B, 3, dtype=torch.int32, device=dev())
    k_out = torch.full((B, 3), 77, dtype=torch.int32, device=dev())
    dist, dist0 = torch.full((B,), -1.0, device=dev()), torch.full((B,), -1.0, device=dev())
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
    import ctypes as C

    def call(E, offs, Rs, rp, nbytes=scratch.numel()):
        return L.ishap_drag_track(edit.data_ptr(), orig.data_ptr(), 0, c.W, c.ld, c.Cc, chmap.data_ptr(), src.data_ptr(),
                                  (C.c_int * len(offs))(*offs), E, c.voxel, Rs, rp, k_in.data_ptr(), k_out.data_ptr(), dist.data_ptr(),
                                  dist0.data_ptr(), None, scratch.data_ptr(), nbytes, _lib.stream_ptr(dev()))
    for E, offs, Rs, rp in ((1, [0, B], 9, 1), (1, [0, B], -1, 1), (1, [0, B], 2, 5), (1, [0, B], 2, -1), (0, [0, B], 2, 1),
                            (33, list(range(34)), 2, 1), (2, [0, B, B], 2, 1), (1, [1, B], 2, 1)):
        assert call(E, offs, Rs, rp) != 0 and L.ishap_last_error()
    assert call(1, [0, B], 2, 1, nbytes=16) != 0 and b"scratch" in L.ishap_last_error()
    torch.cuda.synchronize()
    assert bool((k_out == 77).all()) and bool((dist == -1).all()) and bool((dist0 == -1).all())
    assert call(1, [0, B], 2, 1) == 0
    torch.cuda.synchronize()
    assert torch.equal(k_out.cpu(), _device("A")[0].offsets)


# ------------------------------------------------------------------------------------------------ 5. end to end, tiny model
def _tiny(gold, max_edits=1):
    """The tiny DragStuff of tests/test_gpu_regions.py (built for `max_edits`); get_mesh keeps the final latent only."""
    from ishapediting_amd.drag_utils import DragStuff
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
    ds = DragStuff(dev(), args=args, max_edits=max_edits)
    ds.model.load_state_dict(synthetic.round_torso_to_fp16(synthetic.unet_state_dict(tiny_config(1), 101)))
    ds.set_offset1(r1)
    ds.voxel_size = 2.0 / 32

    def get_mesh(tri_feat=None, img=None, t=0):
        if tri_feat is None:
            tri_feat = ds._denoise(img, t)
        ds.tri_feat = tri_feat
    ds.get_mesh = get_mesh
    ns, dn = T(g["loop_noise_sampling"]).to(dev()), T(g["drag_noise"]).to(dev())
    ds.step_noise = lambda i: ns[Tn - 1 - i]
    ds.update_latent_params(img=g["loop_latent0"])
    ds.step_noise = lambda i: dn[w_time - 1 - i]
    return ds, g, dn, w_time


def _check_track(tr, w_time, B, Rs, every=1):
    rows = (w_time + every - 1) // every
    assert tr["steps"] == list(range(0, w_time, every))
    assert tr["offsets"].shape == (rows, B, 3) and tr["offsets"].dtype == torch.int32
    assert tr["positions"].shape == (rows, B, 3) and tr["dist"].shape == (rows, B) == tr["dist0"].shape
    offs = tr["offsets"].cpu()
    assert not offs[0].any()                                              # the first tracked step: nothing has moved yet
    assert int((offs[1:] - offs[:-1]).abs().max()) <= Rs if rows > 1 else True
    assert bool(torch.isfinite(tr["dist"]).all()) and bool((tr["dist"] <= tr["dist0"]).all())


def test_training_with_tracking_on_the_tiny_model(gold):
    from ishapediting_amd.drag_utils import TRACK_DEFAULTS
    ds, g, dn, w_time = _tiny(gold)
    src, tgt = g["drag_sources"], g["drag_targets"]
    B = len(src)

    def run(**kw):
        prog = list(ds.training(src, tgt, scale=50.0, cof=0.4, **kw))
        torch.cuda.synchronize()
        assert len(prog) == len(ds.last_losses)
        return ds.tri_feat.clone(), torch.stack([l.clone() for l in ds.last_losses])
    with pytest.raises(RuntimeError, match="no tracked edit"):
        ds.handle_error()
    plain = run()
    assert ds.last_track is None
    # the first step's tap is bitwise the recorded guidance tap (same latent, same timestep, same weights)
    assert ds.model.snapshot_restore()
    ch, width = ds.model.tap_shape(ds.args.feat_layer)
    assert torch.equal(ds.model.copy_tap(ds.args.feat_layer)[0], ds.feature_guidance[0])
    tracked = run(track=True)
    assert torch.equal(tracked[0], plain[0]) and torch.equal(tracked[1], plain[1])       # tracking changes nothing of the edit
    tr = ds.last_track
    _check_track(tr, w_time, B, TRACK_DEFAULTS["radius"])
    assert not tr["dist"][0].any() and not tr["dist0"][0].any()                          # ... so its distance is exactly 0
    he = ds.handle_error()
    s_, t_ = T(np.asarray(src, np.float32)).to(dev()), T(np.asarray(tgt, np.float32)).to(dev())
    pos = tr["positions"][-1]
    assert np.array_equal(pos.cpu().numpy(), K.lattice32(np.asarray(src, np.float32), ds.voxel_size, tr["offsets"][-1].cpu().numpy()))
    assert torch.equal(he["error"], (pos - t_).norm(dim=-1) / ds.voxel_size)
    assert torch.allclose(he["fraction"], ((pos - s_) * (t_ - s_)).sum(-1) / ((t_ - s_) ** 2).sum(-1))
    # the options: a smaller search every second step -- and still the same edit
    sparse = run(track={"radius": 2, "patch": 1, "every": 2})
    assert torch.equal(sparse[0], plain[0])
    _check_track(ds.last_track, w_time, B, 2, every=2)
    with pytest.raises(ValueError, match="radius"):
        list(ds.training(src, tgt, scale=50.0, cof=0.4, track={"radius": 9}))
    with pytest.raises(ValueError, match="unknown"):
        list(ds.training(src, tgt, scale=50.0, cof=0.4, track={"radios": 2}))
    assert int(_lib.lib().ishap_device_status()) == 0


def test_training_batch_yields_the_same_two_tracks(gold):
    ds, g, dn, w_time = _tiny(gold, max_edits=2)
    src, tgt = g["drag_sources"], g["drag_targets"]
    list(ds.training(src, tgt, scale=50.0, cof=0.4, track=True))
    torch.cuda.synchronize()
    solo, solo_err = ds.last_track, ds.handle_error()
    ds.step_noise = lambda i: dn[w_time - 1 - i].repeat(2, 1, 1, 1)
    list(ds.training_batch([src] * 2, [tgt] * 2, scale=50.0, cof=0.4, track=True))
    torch.cuda.synchronize()
    assert isinstance(ds.last_track, list) and len(ds.last_track) == 2
    errs = ds.handle_error()
    for k in range(2):
        tr = ds.last_track[k]
        _check_track(tr, w_time, len(src), 4)
        assert tr["steps"] == solo["steps"]
        # where the handles went is the solo edit's, exactly: the tracks are integers
        assert torch.equal(tr["offsets"], solo["offsets"]) and torch.equal(tr["positions"], solo["positions"]), k
        assert torch.equal(errs[k]["error"], solo_err["error"]) and torch.equal(errs[k]["fraction"], solo_err["fraction"])
        # the distances are sums over the taps of a batch-2 forward, which are the solo taps within fp16 rounding and not bit for bit
        # (tests/test_gpu_batched_drag.py): the first step, where nothing has run yet, is exact, the later ones close, and the two
        # identical edits of the batch agree bit for bit.  rtol: a tap element moves by a few fp16 roundings (2^-11 each) and D is a
        # sum of |differences| of such elements with M / D of a few units: 2e-3, four roundings' worth
        assert not tr["dist"][0].any() and not tr["dist0"][0].any()
        for key in ("dist", "dist0"):
            assert torch.allclose(tr[key], solo[key], rtol=2e-3, atol=0), (k, key)
            assert torch.equal(tr[key], ds.last_track[0][key]), (k, key)
    assert int(_lib.lib().ishap_device_status()) == 0
