"""The closed-loop retarget on the device (csrc/retarget.hip) against the float64 statement of tests/retarget_ref.py, against the
setup kernels it stands in for, and inside training() / training_batch() on the tiny model.

Tolerances.  arrived and done are exact: no case has a distance within 1e-9 of its step or arrive (asserted on the host,
tests/test_retarget_ref_host.py, and again here).  A goal on the d <= step branch is the target's bits.  The other goals and
`remaining` come out of a double chain of a dozen IEEE operations (subtract, divide, multiply and add without contraction, one
square root), each correctly rounded on the device as in NumPy, then ONE rounding to float.  The bound reasoned beforehand was 1 float32 ulp, for
a double that might differ by a few 2^-53 and sit on a float rounding boundary; the device turned out to give the oracle's
bits at every handle of every case and every recorded row of the tiny model's edits (0 ulp throughout), as a chain of correctly
rounded operations in one order must, so the tests assert equality.
"""
import ctypes as C
from argparse import Namespace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ishapediting_amd import _lib, synthetic
from ishapediting_amd.unet_spec import tiny_config
from tests import drag_ref as R
from tests import retarget_ref as Q

pytestmark = pytest.mark.gpu
T = torch.from_numpy
INF = float("inf")
COF = 0.3


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _solo_kernels(c, e, targets=None, cof=COF):
    from ishapediting_amd.drag_utils import DragKernels
    dk = DragKernels(dev(), c.W, c.ld, c.chmap, c.r, c.voxel)
    dk.setup(c.sources[e], c.targets[e] if targets is None else targets, cof)
    return dk


def _batch_kernels(c, targets=None, cof=COF):
    from ishapediting_amd.drag_utils import BatchDragKernels
    dk = BatchDragKernels(dev(), c.E, c.W, c.ld, c.chmap, c.r, c.voxel)
    dk.setup(c.sources, c.targets if targets is None else targets, cof)
    return dk


def _state(dk):
    """(touched [E, 3*W*W], nmask [E], gfx, acc, chan_weight) of a solo or batched kernels object, cloned."""
    if hasattr(dk, "scratch"):
        p = dk.scratch_parts()
        return tuple(p[k].clone() for k in ("touched", "nmask", "gfx", "acc", "chan_weight"))
    return dk.touched[None].clone(), dk.nmask.clone(), dk.gfx.clone(), dk.acc.clone(), dk.chan_weight.clone()


def _retarget(dk, K, step, arrive):
    before = _state(dk)
    out = dk.retarget(np.concatenate(K) if isinstance(K, list) else K, step, arrive)
    torch.cuda.synchronize()
    after = _state(dk)
    goals, remaining, arrived, done = (t.cpu().clone() for t in out)
    return dict(goals=goals, remaining=remaining, arrived=arrived, done=done, touched=after[0].cpu(), nmask=after[1].cpu(),
                scratch_same=all(torch.equal(x, y) for x, y in zip(before[2:], after[2:])))


_RUNS = {}


def _device(name):
    """The case's batched call and the solo call of each of its edits, run once per session and shared."""
    if name not in _RUNS:
        c = Q.make_case(name)
        batch = _retarget(_batch_kernels(c), c.K, c.step, c.arrive)
        solo = [_retarget(_solo_kernels(c, e), c.K[e], c.step, c.arrive) for e in range(c.E)]
        _RUNS[name] = dict(batch=batch, solo=solo)
    return _RUNS[name]


def _edit_of(run, c, e):
    a, b = c.offsets[e], c.offsets[e + 1]
    return dict(goals=run["goals"][a:b], remaining=run["remaining"][a:b], arrived=run["arrived"][a:b], done=run["done"][e],
                touched=run["touched"][e], nmask=run["nmask"][e])


def _check_reaim(tag, got_goals, got_remaining, o, targets):
    """Goals and remaining of one edit against the oracle `o`: the same bits (module docstring); the distance is printed first."""
    goals, rem = np.asarray(got_goals, np.float32), np.asarray(got_remaining, np.float32)
    tgt = np.asarray(targets, np.float32)
    assert np.array_equal(goals[o.hold].view(np.uint32), tgt[o.hold].view(np.uint32)), tag      # a bit copy
    ug = Q.ulps32(goals[~o.hold], o.goals[~o.hold]) if (~o.hold).any() else np.zeros(1, np.int64)
    ur = Q.ulps32(rem, o.remaining)
    print(f"{tag}: goals off the hold branch max {int(ug.max())} ulp, remaining max {int(ur.max())} ulp")
    assert int(ug.max()) == 0 and int(ur.max()) == 0, (tag, ug, ur)
    assert np.array_equal(goals.view(np.uint32), o.goals.view(np.uint32)) and np.array_equal(rem.view(np.uint32), o.remaining.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 1. against the oracle
@pytest.mark.parametrize("name", Q.CASES)
def test_goals_remaining_arrived_done_against_the_oracle(name):
    c, orc, d = Q.make_case(name), Q.oracle(name), _device(name)
    for e, o in enumerate(orc):
        assert all(x == 0.0 or (abs(x - c.step) > Q.MARGIN and abs(x - c.arrive) > Q.MARGIN) for x in o.d)
        for form, got in (("batch", _edit_of(d["batch"], c, e)), ("solo", _edit_of(d["solo"][e], SimpleNamespace(offsets=[0, len(o.d)]), 0))):
            _check_reaim(f"{name} edit {e} {form}", got["goals"].numpy(), got["remaining"].numpy(), o, c.targets[e])
            assert got["arrived"].dtype == torch.int32 and np.array_equal(got["arrived"].numpy() != 0, o.arrived), (name, e, form)
            assert set(got["arrived"].tolist()) <= {0, 1} and int(got["done"]) == int(o.done), (name, e, form)


# ------------------------------------------------------------------------------------------------ 2. touched and nmask
@pytest.mark.parametrize("name", Q.CASES)
def test_touched_and_nmask_are_those_of_a_setup_with_the_goals(name):
    c, orc, d = Q.make_case(name), Q.oracle(name), _device(name)
    # the reference is the setup kernels (not the code under test) on a second buffer set, given targets = the goals read back
    goals = [_edit_of(d["batch"], c, e)["goals"].numpy() for e in range(c.E)]
    ref_t, ref_n = (t.cpu() for t in _state(_batch_kernels(c, targets=goals))[:2])
    assert torch.equal(d["batch"]["touched"], ref_t) and torch.equal(d["batch"]["nmask"], ref_n), name
    for e in range(c.E):
        g = d["solo"][e]["goals"].numpy()
        st, sn = (t.cpu() for t in _state(_solo_kernels(c, e, targets=g))[:2])
        assert torch.equal(d["solo"][e]["touched"], st) and torch.equal(d["solo"][e]["nmask"], sn), (name, e)
        # the host builder, from first principles, on the device's own goals -- which test 1 holds to the oracle's bits, so this
        # is oracle(name)[e].touched
        ht, hn = Q.touched_sets(c.sources[e], g, c.r, c.voxel, c.W)
        assert np.array_equal(d["solo"][e]["touched"][0].numpy().reshape(3, c.W, c.W), ht) and int(d["solo"][e]["nmask"][0]) == hn
        bt = _edit_of(d["batch"], c, e)
        hb, hbn = Q.touched_sets(c.sources[e], goals[e], c.r, c.voxel, c.W)
        assert np.array_equal(bt["touched"].numpy().reshape(3, c.W, c.W), hb) and int(bt["nmask"]) == hbn
        assert np.array_equal(ht, orc[e].touched) and hn == orc[e].nmask


# ------------------------------------------------------------------------------------------------ 3. the loss after a retarget
@pytest.mark.parametrize("name", Q.CASES)
def test_scratch_buffers_are_not_touched(name):
    d = _device(name)
    assert d["batch"]["scratch_same"] and all(s["scratch_same"] for s in d["solo"])       # gfx, acc, chan_weight: bitwise


@pytest.mark.parametrize("name", Q.LOSS_CASES)
def test_a_loss_call_after_a_retarget_is_that_of_a_fresh_setup_with_the_goals(name):
    c = Q.make_case(name)
    edits, origs = c.edits.to(dev()), c.origs.to(dev())
    stride = c.W * c.W * c.ld
    dk = _batch_kernels(c)
    goals = dk.retarget(np.concatenate(c.K), c.step, c.arrive)[0].cpu().numpy().copy()
    g1, l1 = (t.clone() for t in dk.loss_grad_ptr(edits.data_ptr(), origs.data_ptr(), stride))
    fresh = _batch_kernels(c, targets=[goals[a:b] for a, b in zip(c.offsets[:-1], c.offsets[1:])])
    g2, l2 = fresh.loss_grad_ptr(edits.data_ptr(), origs.data_ptr(), stride)
    torch.cuda.synchronize()
    assert torch.equal(g1, g2) and torch.equal(l1, l2) and bool(torch.isfinite(l1).all()) and bool(g1.any()), name
    for e in range(c.E):
        sk = _solo_kernels(c, e)
        sg = sk.retarget(c.K[e], c.step, c.arrive)[0].cpu().numpy().copy()
        a1, b1 = (t.clone() for t in sk.loss_grad(edits[e], origs[e]))
        a2, b2 = _solo_kernels(c, e, targets=sg).loss_grad(edits[e], origs[e])
        torch.cuda.synchronize()
        assert torch.equal(a1, a2) and torch.equal(b1, b2), (name, e)
        assert torch.equal(a1, g1[e]) and torch.equal(b1[0], l1[e]), (name, e)                   # and the batch's edit e
        # the final targets stay beside the goals, and setup() puts the aim back on them
        assert np.array_equal(sk.targets.cpu().numpy(), np.asarray(c.targets[e], np.float32))
        sk.setup(c.sources[e], c.targets[e], COF)
        a3, b3 = sk.loss_grad(edits[e], origs[e])
        a4, b4 = _solo_kernels(c, e).loss_grad(edits[e], origs[e])
        torch.cuda.synchronize()
        assert torch.equal(a3, a4) and torch.equal(b3, b4), (name, e)


# ------------------------------------------------------------------------------------------------ 4. batching, repeatability
def test_each_edit_of_batch_L_is_its_solo_run_and_two_runs_are_equal():
    c, d = Q.make_case("L"), _device("L")
    for e in range(c.E):
        b, s = _edit_of(d["batch"], c, e), d["solo"][e]
        assert torch.equal(b["goals"], s["goals"]) and torch.equal(b["remaining"], s["remaining"]), e
        assert torch.equal(b["arrived"], s["arrived"]) and int(b["done"]) == int(s["done"][0]), e
        assert torch.equal(b["touched"], s["touched"][0]) and int(b["nmask"]) == int(s["nmask"][0]), e
    again = _retarget(_batch_kernels(c), c.K, c.step, c.arrive)
    assert all(torch.equal(again[k], d["batch"][k]) for k in ("goals", "remaining", "arrived", "done", "touched", "nmask"))
    # a second retarget on the same object, from other offsets and back: nothing of the first one is left in the bitmaps
    dk = _batch_kernels(c)
    _retarget(dk, [k + 2 for k in c.K], 0.75, c.arrive)
    back = _retarget(dk, c.K, c.step, c.arrive)
    assert all(torch.equal(back[k], d["batch"][k]) for k in ("goals", "remaining", "arrived", "done", "touched", "nmask"))
    # one lead and one arrival radius per edit: each edit is the solo run with its own
    steps, arrives = [0.5, INF, 2.5], [0.0, 3.0, INF]
    each = _retarget(_batch_kernels(c), c.K, steps, arrives)
    for e in range(c.E):
        s, b = _retarget(_solo_kernels(c, e), c.K[e], steps[e], arrives[e]), _edit_of(each, c, e)
        assert torch.equal(b["goals"], s["goals"]) and torch.equal(b["arrived"], s["arrived"]) and int(b["done"]) == int(s["done"][0])
        assert torch.equal(b["touched"], s["touched"][0]) and int(b["nmask"]) == int(s["nmask"][0]), e
        o = Q.reaim64(c.sources[e], c.targets[e], c.K[e], c.voxel, steps[e], arrives[e])
        assert np.array_equal(b["arrived"].numpy() != 0, o.arrived) and int(b["done"]) == int(o.done)


# ------------------------------------------------------------------------------------------------ 5. arguments
def test_invalid_arguments_error_before_any_launch():
    from ishapediting_amd.drag_utils import DragKernels
    L = _lib.lib()
    c = Q.make_case("A")
    B = len(c.sources[0])
    sp = _lib.stream_ptr(dev())

    def sentinels():
        return (torch.full((B, 3), 7.0, device=dev()), torch.full((B,), -1.0, device=dev()),
                torch.full((B,), 77, dtype=torch.int32, device=dev()), torch.full((c.E,), 77, dtype=torch.int32, device=dev()))

    def untouched(goals, rem, arr, done):
        return bool((goals == 7.0).all()) and bool((rem == -1.0).all()) and bool((arr == 77).all()) and bool((done == 77).all())

    for form in ("solo", "batch"):
        dk = _solo_kernels(c, 0) if form == "solo" else _batch_kernels(c)
        fn = L.ishap_drag_batch_retarget               # one edit: the same entry with E = 1
        K = torch.zeros(B, 3, dtype=torch.int32, device=dev())
        goals, rem, arr, done = sentinels()
        before = _state(dk)

        def call(step, arrive, final=dk.targets, k=K, outs=None):
            g, r_, a_, d_ = outs or (goals, rem, arr, done)
            dk._aim_ptr = g.data_ptr()                 # the struct's `targets`: the goals buffer the call writes
            args = dk._args()
            return fn(C.byref(args), _lib.ptr(final), _lib.ptr(k), step, arrive, _lib.ptr(r_), _lib.ptr(a_), _lib.ptr(d_), sp)
        for step, arrive, word in ((0.0, 1.0, b"step"), (-2.0, 1.0, b"step"), (float("nan"), 1.0, b"step"), (1.0, -0.5, b"arrive"),
                                   (1.0, float("nan"), b"arrive")):
            assert call(step, arrive) != 0 and word in L.ishap_last_error(), (form, step, arrive, L.ishap_last_error())
        assert call(1.0, 1.0, final=None) != 0 and b"null" in L.ishap_last_error()
        assert call(1.0, 1.0, k=None) != 0 and b"null" in L.ishap_last_error()
        assert call(1.0, 1.0, outs=(goals, None, arr, done)) != 0 and b"null" in L.ishap_last_error()
        assert call(1.0, 1.0, outs=(goals, rem, arr, None)) != 0 and b"null" in L.ishap_last_error()
        assert call(1.0, 1.0, final=goals) != 0                               # the goals buffer may not be the final targets
        torch.cuda.synchronize()
        assert untouched(goals, rem, arr, done), form
        assert all(torch.equal(x, y) for x, y in zip(before, _state(dk))), form
        # the Python call reports the same errors and leaves the aim where it was
        dk._aim_ptr = None
        with pytest.raises(RuntimeError, match="step"):
            dk.retarget(K, 0.0, 1.0)
        assert dk._targets_ptr() == dk.targets.data_ptr()
        with pytest.raises(ValueError, match="K must be"):
            dk.retarget(K[:1], 1.0, 1.0)
        # ... and the valid call then runs
        assert call(c.step, c.arrive) == 0
        torch.cuda.synchronize()
        want = _device("A")["solo"][0] if form == "solo" else _device("A")["batch"]
        assert torch.equal(goals.cpu(), want["goals"]) and torch.equal(rem.cpu(), want["remaining"])
        assert torch.equal(arr.cpu(), want["arrived"]) and torch.equal(done.cpu(), want["done"])
    # W = 148: 3 * 148 * 148 = 65712 bytes of bitmaps do not fit 65536
    wide = DragKernels(dev(), 148, 8, R._arange_map(2), 1, 2 / 148)
    wide.setup(c.sources[0], c.targets[0], 0.0)
    before = _state(wide)
    with pytest.raises(RuntimeError, match="65536"):
        wide.retarget(torch.zeros(B, 3, dtype=torch.int32), 1.0, 1.0)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, _state(wide)))
    assert int(L.ishap_device_status()) == 0


# ------------------------------------------------------------------------------------------------ 6. end to end, tiny model
def _tiny(gold, max_edits=1):
    """The tiny DragStuff of tests/test_gpu_track.py (built for `max_edits`); get_mesh keeps the final latent only."""
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


def _check_recorded_goals(tr, src, tgt, voxel, step, arrive):
    """goals[r] / remaining[r] / arrived[r] of a track are reaim64 of offsets[r - 1] (zeros for r = 0)."""
    offs = tr["offsets"].cpu().numpy()
    rows = len(tr["steps"])
    assert tr["goals"].shape == (rows, len(src), 3) and tr["remaining"].shape == (rows, len(src)) == tr["arrived"].shape
    for r in range(rows):
        K = np.zeros_like(offs[0]) if r == 0 else offs[r - 1]
        o = Q.reaim64(src, tgt, K, voxel, step, arrive)
        _check_reaim(f"row {r}", tr["goals"][r].cpu().numpy(), tr["remaining"][r].cpu().numpy(), o, tgt)
        near = (np.abs(o.d - step) <= Q.MARGIN) | (np.abs(o.d - arrive) <= Q.MARGIN)
        assert np.array_equal(tr["arrived"][r].cpu().numpy()[~near], o.arrived[~near])
    last = Q.reaim64(src, tgt, offs[-1], voxel, step, arrive)
    assert np.array_equal(tr["remaining_after"].cpu().numpy(), last.remaining)


def test_closed_loop_on_the_tiny_model(gold):
    ds, g, dn, w_time = _tiny(gold)
    src, tgt = np.asarray(g["drag_sources"], np.float32), np.asarray(g["drag_targets"], np.float32)
    assert w_time >= 3                      # (d) stops before guided step 2

    def run(stop_after=None, **kw):
        n = 0
        for _ in ds.training(src, tgt, scale=50.0, cof=0.4, **kw):
            n += 1
            if stop_after is not None and n == stop_after:
                ds.train_flag = False
        torch.cuda.synchronize()
        assert n == len(ds.last_losses)
        return ds.tri_feat.clone(), torch.stack([l.clone() for l in ds.last_losses])

    plain = run()
    tracked = run(track=True)
    track_only = ds.last_track
    assert "goals" not in track_only
    # (a) an infinite lead is the open-loop edit, bit for bit, and its track is the tracked edit's
    inf = run(closed_loop={"step": INF})
    assert torch.equal(inf[0], plain[0]) and torch.equal(inf[1], plain[1]) and torch.equal(tracked[0], plain[0])
    tr = ds.last_track
    assert tr["steps"] == track_only["steps"] and ds.last_stop is None
    for key in ("offsets", "positions", "dist", "dist0"):
        assert torch.equal(tr[key], track_only[key]), key
    assert np.array_equal(tr["goals"].cpu().numpy().view(np.uint32), np.broadcast_to(tgt, tr["goals"].shape).copy().view(np.uint32))
    he = ds.handle_error()
    assert torch.equal(he["error"], (tr["positions"][-1] - T(tgt).to(dev())).norm(dim=-1) / ds.voxel_size)      # unchanged
    # (b) a lead of one voxel
    d0 = Q.reaim64(src, tgt, np.zeros((len(src), 3), np.int32), ds.voxel_size, 1.0, 1.0).d
    assert (d0 > 1.0 + Q.MARGIN).any()                                                   # some handle's move is longer than that
    one = run(closed_loop={"step": 1.0})
    tr1 = ds.last_track
    assert bool(torch.isfinite(one[1]).all()) and tr1["steps"] == list(range(w_time))
    _check_recorded_goals(tr1, src, tgt, ds.voxel_size, 1.0, 1.0)
    far = d0 > 1.0 + Q.MARGIN
    assert bool((tr1["goals"][0].cpu()[T(far)] != T(tgt)[T(far)]).any(dim=-1).all())       # step 0 already aims short of them
    assert not torch.equal(one[1], plain[1])
    again = run(closed_loop={"step": 1.0})
    assert torch.equal(again[0], one[0]) and torch.equal(again[1], one[1])
    for key in ("offsets", "dist", "dist0", "goals", "remaining", "arrived", "remaining_after"):
        assert torch.equal(ds.last_track[key], tr1[key]), key
    # (d) stop: everything has "arrived" at arrive = inf, and the host sees step 0's flag before step 2
    stopped = run(closed_loop={"step": 1.0, "arrive": INF, "stop": True, "lag": 2})
    assert len(ds.last_losses) == 2 and ds.last_stop == 2 and ds.last_track["steps"] == [0, 1]
    by_hand = run(stop_after=2, closed_loop={"step": 1.0, "arrive": INF})
    assert len(ds.last_losses) == 2 and ds.last_stop is None
    assert torch.equal(stopped[0], by_hand[0]) and torch.equal(stopped[1], by_hand[1])
    assert not torch.equal(stopped[0], one[0])
    # (e) a stop that never fires changes nothing
    never = run(closed_loop={"step": 1.0, "arrive": 0.0, "stop": True})
    ref = run(closed_loop={"step": 1.0, "arrive": 0.0})
    assert ds.last_stop is None and len(never[1]) == w_time
    assert torch.equal(never[0], ref[0]) and torch.equal(never[1], ref[1]) and torch.equal(never[0], one[0])
    # options are refused before anything runs
    for bad, word in (({"step": 0.0}, "step"), ({"arrive": -1.0}, "arrive"), ({"lead": 1.0}, "unknown"), ({"lag": 0}, "lag")):
        with pytest.raises(ValueError, match=word):
            list(ds.training(src, tgt, scale=50.0, cof=0.4, closed_loop=bad))
    with pytest.raises(ValueError, match="track"):
        list(ds.training(src, tgt, scale=50.0, cof=0.4, closed_loop=True, track=False))
    after = run()
    assert torch.equal(after[0], plain[0]) and torch.equal(after[1], plain[1])            # and the plain edit is what it was
    assert int(_lib.lib().ishap_device_status()) == 0


def test_closed_loop_batch_of_two_identical_edits(gold):
    ds, g, dn, w_time = _tiny(gold, max_edits=2)
    src, tgt = np.asarray(g["drag_sources"], np.float32), np.asarray(g["drag_targets"], np.float32)
    list(ds.training(src, tgt, scale=50.0, cof=0.4, closed_loop={"step": 1.0}))
    torch.cuda.synchronize()
    solo = ds.last_track
    ds.step_noise = lambda i: dn[w_time - 1 - i].repeat(2, 1, 1, 1)
    list(ds.training_batch([src] * 2, [tgt] * 2, scale=50.0, cof=0.4, closed_loop={"step": 1.0}))
    torch.cuda.synchronize()
    a, b = ds.last_track
    for key in ("offsets", "positions", "dist", "dist0", "goals", "remaining", "arrived", "remaining_after"):
        assert torch.equal(a[key], b[key]), key
    assert torch.equal(ds.tri_feat_batch[0], ds.tri_feat_batch[1]) and bool(torch.isfinite(ds.tri_feat_batch).all())
    assert torch.equal(a["goals"][0], solo["goals"][0]) and torch.equal(a["remaining"][0], solo["remaining"][0])
    for k, tr in enumerate(ds.last_track):
        _check_recorded_goals(tr, src, tgt, ds.voxel_size, 1.0, 1.0)
    assert len(ds.handle_error()) == 2
    # one lead per edit: edit 0 open loop, edit 1 closed
    list(ds.training_batch([src] * 2, [tgt] * 2, scale=50.0, cof=0.4, closed_loop=[{"step": INF}, {"step": 1.0}]))
    torch.cuda.synchronize()
    p, q = ds.last_track
    assert np.array_equal(p["goals"].cpu().numpy(), np.broadcast_to(tgt, p["goals"].shape))
    assert torch.equal(q["goals"][0], solo["goals"][0]) and (p["step"], q["step"]) == (INF, 1.0)
    assert int(_lib.lib().ishap_device_status()) == 0
