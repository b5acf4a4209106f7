"""Volume constraints on the GPU (csrc/constrain.hip, ishapediting_amd/constraints.py, DragStuff.training's volume_keep / carve /
fill): the gather list against its numpy statement, the loss and its gradient against float64 (tests/constrain_ref.py on
tests/decoder_ref.py's bounds), repeatability, the logits against ishap_triplane_field_grad's bit for bit, the unweighted call
against ishap_triplane_points_loss_grad, an ascent on planes alone, and the guided loop on the small 96-channel model.

Shapes follow LOSS_CASES of tests/test_gpu_decoder_oracle.py: S = 8 and 16, the survivor pools of the kink filter.  Point counts
1, 31, 32, 33 (the tile's tail on both sides) and 32 * 4 * 3 + 5 = 389 (three workgroups of four waves and a tail).

Zero weights.  "Removing a zero-weight point changes no bit" holds for dplanes wherever the point stands (its products are +-0
and the other entries of a row keep their order) and for the logits of the others.  The loss is a sum of per-TILE partials, so
its bits are the same only while the other points keep their tiles: that is asserted with the zero-weight points at the end.
"""
import ctypes as C
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import constrain_ref as R
from tests import decoder_ref as D
from tests.test_gpu_decoder_oracle import (CANARY_BITS, NCANARY, L, Weights, _w3_scaled, check_forward, check_gradient, dev, guarded,
                                           put, read)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def guarded_int(n):
    host = torch.full((n + NCANARY,), -7, dtype=torch.int32)
    host[n:] = CANARY_BITS
    return host.to(dev())


def read_int(buf, n, tag):
    host = buf.cpu()
    assert bool((host[n:] == CANARY_BITS).all()), f"{tag}: a canary changed"
    return host[:n].numpy().copy()


def setup_list(coords, S):
    """ishap_constraint_setup on guarded buffers -> (row_start, entry, entry_w as numpy, the device tensors)"""
    M = len(coords)
    lib = L().lib()
    c_d = put(coords)
    nbytes = int(lib.ishap_constraint_setup_scratch_bytes(M, S))
    assert nbytes > 0
    scratch = torch.empty(nbytes + NCANARY, dtype=torch.uint8, device=dev())
    scratch[nbytes:] = 0x5A
    rs, en, ew = guarded_int(3 * S * S + 1), guarded_int(12 * M), guarded(12 * M)
    L().check(lib.ishap_constraint_setup(c_d.data_ptr(), M, S, rs.data_ptr(), en.data_ptr(), ew.data_ptr(), scratch.data_ptr(), nbytes,
                                         L().stream_ptr(dev())))
    torch.cuda.synchronize()
    assert bool((scratch[nbytes:] == 0x5A).all()), "setup wrote behind its scratch"
    row_start = read_int(rs, 3 * S * S + 1, "row_start")
    n = int(row_start[-1])
    assert 0 <= n <= 12 * M
    entry = read_int(en, 12 * M, "entry")
    host_w = ew.cpu()
    assert bool((host_w[12 * M:].view(torch.int32) == CANARY_BITS).all()), "entry_w: a canary changed"
    return row_start, entry[:n], host_w[:n].numpy().copy(), SimpleNamespace(coords=c_d, row_start=rs, entry=en, entry_w=ew)


def loss_grad(w, planes_d, S, lst, M, gt, pw, want_logits=True):
    """one ishap_constraint_loss_grad on NaN-guarded outputs -> (dplanes [3,S,S,32], loss, logits)"""
    lib = L().lib()
    gt_d, pw_d = put(gt), put(pw)
    wsum = float(np.asarray(pw, np.float64).sum())
    dfeat, partials = guarded(M * 32), guarded((M + 31) // 32)
    dpl, loss, logits = guarded(3 * S * S * 32), guarded(1), guarded(M)
    L().check(lib.ishap_constraint_loss_grad(planes_d.data_ptr(), S, C.byref(w.c), lst.coords.data_ptr(), gt_d.data_ptr(), pw_d.data_ptr(),
                                             M, wsum, lst.row_start.data_ptr(), lst.entry.data_ptr(), lst.entry_w.data_ptr(),
                                             dfeat.data_ptr(), partials.data_ptr(), dpl.data_ptr(), loss.data_ptr(),
                                             logits.data_ptr() if want_logits else None, L().stream_ptr(dev())))
    torch.cuda.synchronize()
    read(dfeat, M * 32, "dfeat"), read(partials, (M + 31) // 32, "partials")
    return (read(dpl, 3 * S * S * 32, "dplanes").reshape(3, S, S, 32), float(read(loss, 1, "loss")[0]),
            read(logits, M, "logits") if want_logits else None)


# ------------------------------------------------------------------------------------------------ 1. the gather list
def _list_coords(name):
    S = 2 if name.endswith("S2") else 16
    rs = np.random.RandomState(31)
    if name.startswith("m1"):
        c = rs.uniform(-1, 1, (1, 3))
    elif name.startswith("m33"):
        c = rs.uniform(-1.05, 1.05, (33, 3))
    elif name == "shared":
        c = np.concatenate([np.repeat(rs.uniform(-1, 1, (1, 3)), 512, 0), rs.uniform(-1, 1, (512, 3))])
    elif name == "faces":
        c = D.coords_family("faces", 200, S, rs)
        assert all(((np.abs(c) == 1).sum(axis=1) == k).any() for k in (1, 2, 3))
    elif name == "allout":
        c = D.coords_family("beyond", 64, S, rs)
    elif name == "mixed":
        c = D.mixed_coords(40, S, 9)[:240]                    # every family but "far"
    else:
        raise KeyError(name)
    return np.asarray(c, np.float32), S


@pytest.mark.parametrize("name", ["m1", "m1-S2", "m33", "m33-S2", "shared", "faces", "allout", "mixed"])
def test_gather_list_is_the_numpy_statement_and_repeats(name):
    coords, S = _list_coords(name)
    want = R.gather_list(coords, S)
    runs = [setup_list(coords, S)[:3] for _ in range(2)]
    for got in runs:
        assert np.array_equal(got[0], want[0]), "row_start"
        assert np.array_equal(got[1], want[1]), "entry"
        assert np.array_equal(bits(got[2]), bits(want[2])), "entry_w"
    if name == "allout":
        assert (runs[0][0] == 0).all() and len(runs[0][1]) == 0
    print(f"{name}: S {S}, {len(coords)} points, {len(want[1])} entries, longest row {int(np.diff(want[0]).max())}")


# ------------------------------------------------------------------------------------------------ 2.-5. loss and gradient
GRAD_CASES = ([dict(name=f"n{n}", S=16, n=n) for n in (1, 31, 32, 33, 32 * 4 * 3 + 5)] +
              [dict(name="shared", S=16, kind="shared"), dict(name="border", S=8, kind="border"), dict(name="allout", S=16, kind="allout"),
               dict(name="zeros", S=8, n=33, zeros=True)] +
              [dict(name=f"sat{t}-gt{g}", S=8, n=33, sat=t, gt=g) for t in (50, 100) for g in ("0", "1", "mixed")])


@lru_cache(maxsize=None)
def _grad_case(name):
    c = next(c for c in GRAD_CASES if c["name"] == name)
    sd, net = D.synthetic_net()
    S = c["S"]
    pool = D.survivor_pool(S)
    assert pool.rejected <= 0.10, pool.rejected
    planes, kind = pool.planes, c.get("kind")
    if kind == "shared":
        coords = np.concatenate([np.repeat(pool.coords[:1], 512, 0), pool.coords[1:513]])
    elif kind == "border":
        coords = D.filtered(net, planes, D.coords_family("faces", 200, S, np.random.RandomState(70)))
        assert len(coords) > 150 and sum((np.abs(coords) == 1).sum(axis=1) == 3) > 5
    elif kind == "allout":
        coords = D.coords_family("beyond", 64, S, np.random.RandomState(71))
    else:
        coords = np.resize(pool.coords, (c["n"], 3))
    n = len(coords)
    rs = np.random.RandomState(72)
    gt = {"0": np.zeros(n), "1": np.ones(n)}.get(c.get("gt"), (rs.rand(n) < 0.5) * 1.0).astype(np.float32)
    pw = rs.uniform(0.25, 4.0, n).astype(np.float32)
    if c.get("zeros"):
        pw[[0, 5, 6, 17, 31, 32]] = 0.0
    if "sat" in c:
        sd = _w3_scaled(sd, net, planes, coords, c["sat"])
        net = D.net64(sd)
        z = D.forward(net, planes, coords).logit
        assert z.min() <= -0.9 * c["sat"] and z.max() >= 0.9 * c["sat"], (z.min(), z.max())
        if c["gt"] == "mixed":
            gt[np.argsort(z)[[0, 1, -2, -1]]] = [0, 1, 0, 1]
    ref = R.weighted_loss_grad(net, planes, coords, gt, pw)
    g32 = [R.weighted_loss_grad(D.permuted_net(net, s), planes, coords, gt, pw, dtype=torch.float32).dplanes for s in range(D.REL_RUNS)]
    rel = D.measured_rel(g32, ref) if (ref.A > 0).any() else 0.0
    return SimpleNamespace(sd=sd, net=net, S=S, planes=planes, coords=coords, gt=gt, pw=pw, ref=ref, rel=rel)


def field_logits(w, planes_d, S, coords):
    n = len(coords)
    c_d = put(coords)
    logits, grad = guarded(n), guarded(3 * n)
    L().check(L().lib().ishap_triplane_field_grad(planes_d.data_ptr(), S, C.byref(w.c), c_d.data_ptr(), n, logits.data_ptr(),
                                                  grad.data_ptr(), L().stream_ptr(dev())))
    torch.cuda.synchronize()
    return read(logits, n, "field logits")


@pytest.mark.parametrize("name", [c["name"] for c in GRAD_CASES])
def test_loss_and_gradient_against_float64(name):
    c = _grad_case(name)
    n, S = len(c.coords), c.S
    w = Weights(c.sd)
    planes_d = put(c.planes)
    lst = setup_list(c.coords, S)[3]
    got, got_loss, got_logits = loss_grad(w, planes_d, S, lst, n, c.gt, c.pw)
    # 3. a second call: the same bits; without the optional logits too
    again = loss_grad(w, planes_d, S, lst, n, c.gt, c.pw)
    assert np.array_equal(bits(got), bits(again[0])) and bits(got_loss) == bits(again[1]) and np.array_equal(bits(got_logits), bits(again[2]))
    nolog = loss_grad(w, planes_d, S, lst, n, c.gt, c.pw, want_logits=False)
    assert np.array_equal(bits(got), bits(nolog[0])) and bits(got_loss) == bits(nolog[1])
    # 4. the logits are ishap_triplane_field_grad's, bit for bit
    assert np.array_equal(bits(got_logits), bits(field_logits(w, planes_d, S, c.coords))), "logits differ from the field kernel's"
    check_forward(name, got_logits, c.net, c.planes, c.coords)
    lb = 2.0 ** -20 * (1 + c.ref.bce_abs_mean)
    print(f"{name}: loss64 {c.ref.loss:.6e} |dev - 64| {abs(got_loss - c.ref.loss):.2e} bound {lb:.2e}; max |logit| {np.abs(c.ref.logits).max():.1f}")
    assert abs(got_loss - c.ref.loss) <= lb, (name, got_loss, c.ref.loss, lb)
    untouched = ~D.touched_texels(c.coords, S).reshape(3, S, S)
    assert (got[untouched] == 0.0).all(), f"{name}: {int((got[untouched] != 0).sum())} element(s) no tap reaches are not 0.0"
    if name == "allout":
        assert (got == 0.0).all() and untouched.all() and np.isfinite(got_loss)
        return
    check_gradient(name, got, c.ref, c.rel)
    if name == "zeros":
        keep = c.pw > 0
        cl = setup_list(c.coords[keep], S)[3]
        less = loss_grad(w, planes_d, S, cl, int(keep.sum()), c.gt[keep], c.pw[keep])
        assert np.array_equal(bits(got), bits(less[0])), "removing the zero-weight points changed dplanes"
        assert np.array_equal(bits(got_logits[keep]), bits(less[2]))
        assert abs(less[1] - c.ref.loss) <= lb
        # the zero-weight points at the end: the others keep their tiles, so the loss keeps its bits as well
        order = np.concatenate([np.nonzero(keep)[0], np.nonzero(~keep)[0]])
        tl = setup_list(c.coords[order], S)[3]
        tail = loss_grad(w, planes_d, S, tl, n, c.gt[order], c.pw[order])
        assert np.array_equal(bits(tail[0]), bits(less[0])) and bits(tail[1]) == bits(less[1])


def test_unit_weights_agree_with_points_loss_grad():
    """5. w = 1: the same loss as ishap_triplane_points_loss_grad; each kernel is within its bound of the float64 gradient, so
    they agree within the sum of the two."""
    c = _grad_case("n389")
    n, S = len(c.coords), c.S
    ones = np.ones(n, np.float32)
    ref = D.points_loss_grad(c.net, c.planes, c.coords, c.gt)
    g32 = [D.points_loss_grad(D.permuted_net(c.net, s), c.planes, c.coords, c.gt, dtype=torch.float32).dplanes for s in range(D.REL_RUNS)]
    bound = D.backward_bound(ref, D.measured_rel(g32, ref))
    w = Weights(c.sd)
    planes_d, coords_d, gt_d = put(c.planes), put(c.coords), put(c.gt)
    mine = loss_grad(w, planes_d, S, setup_list(c.coords, S)[3], n, c.gt, ones)
    dpl, loss, logits = guarded(c.planes.size), guarded(1), guarded(n)
    L().check(L().lib().ishap_triplane_points_loss_grad(planes_d.data_ptr(), S, C.byref(w.c), w.w1t.data_ptr(), w.w2t.data_ptr(),
                                                        coords_d.data_ptr(), gt_d.data_ptr(), n, dpl.data_ptr(), loss.data_ptr(),
                                                        logits.data_ptr(), L().stream_ptr(dev())))
    torch.cuda.synchronize()
    theirs = read(dpl, c.planes.size, "dplanes").reshape(c.planes.shape)
    err = np.abs(mine[0].astype(np.float64) - theirs)
    print(f"unit weights: max |constraint - points_loss_grad| {err.max():.2e}, worst / (2 bound) {(err / np.maximum(2 * bound, 1e-300))[bound > 0].max():.3f}")
    assert (err <= 2 * bound).all()
    lb = 2.0 ** -20 * (1 + ref.bce_abs_mean)
    assert abs(mine[1] - float(read(loss, 1, "loss")[0])) <= 2 * lb
    assert (np.abs(mine[0].astype(np.float64) - ref.dplanes) <= bound).all()


# ------------------------------------------------------------------------------------------------ 6. ascent on planes alone
ASCENT_STEPS, ASCENT_D = 20, 12
CARVE_BOX, FILL_BOX = ((-0.8, -0.8, -0.8), (-0.3, -0.3, -0.3)), ((0.2, 0.2, 0.2), (0.75, 0.75, 0.75))


def _box_points(box, Dg):
    ax = 2.0 * np.arange(Dg) / (Dg - 1) - 1.0
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    m = ((g >= np.asarray(box[0])) & (g <= np.asarray(box[1]))).all(axis=1)
    return g[m].astype(np.float32)


@lru_cache(maxsize=None)
def _ascent_reference():
    """float64 ascent planes += lr dplanes from make_planes(16, AMP_BWD, 16); lr: the largest of a decade ladder at which L_vol rises
    at every one of the steps (chosen here, on the CPU, from the reference alone)"""
    _, net = D.synthetic_net()
    carve, fill = _box_points(CARVE_BOX, ASCENT_D), _box_points(FILL_BOX, ASCENT_D)
    coords = np.concatenate([carve, fill])
    gt = np.concatenate([np.zeros(len(carve)), np.ones(len(fill))]).astype(np.float32)
    pw = np.ones(len(coords), np.float32)
    p0 = D.make_planes(16, D.AMP_BWD, 16)
    for lr in (30.0, 10.0, 3.0, 1.0, 0.3, 0.1, 0.03):
        p, losses, means = p0.astype(np.float64), [], []
        for _ in range(ASCENT_STEPS + 1):
            r = R.weighted_loss_grad(net, p, coords, gt, pw)
            losses.append(r.loss)
            means.append(r.bce_abs_mean)
            p = p + lr * r.dplanes
        if (np.diff(losses) > 0).all():
            return SimpleNamespace(lr=lr, coords=coords, gt=gt, pw=pw, planes=p0, losses=np.array(losses), means=np.array(means),
                                   carve=carve, fill=fill)
    raise AssertionError("no step length of the ladder gives a monotone ascent")


def test_ascent_on_planes_alone():
    from ishapediting_amd import constraints as K
    from ishapediting_amd import synthetic
    from ishapediting_amd.regions import Box
    from ishapediting_amd.triplane_decoder import MultiTriplane
    a = _ascent_reference()
    dec = MultiTriplane(1, device=dev())
    dec.net.load_state_dict(synthetic.decoder_state_dict())
    cons = K.volume_constraints(carve=Box(*CARVE_BOX), fill=Box(*FILL_BOX), D=ASCENT_D, device=dev())
    # the builder's points are the reference's: carve first, then fill, ascending linear index
    assert np.array_equal(cons.points.cpu().numpy(), a.coords) and np.array_equal(cons.targets.cpu().numpy(), a.gt)
    assert np.array_equal(cons.weights.cpu().numpy(), a.pw)
    st = dec.constraint_setup(cons.points, cons.targets, cons.weights, 16)
    planes = put(a.planes)
    losses = torch.zeros(ASCENT_STEPS + 1, device=dev())
    for k in range(ASCENT_STEPS + 1):
        _, dpl, _ = dec.constraint_loss_grad(planes, st, loss=losses[k:k + 1])
        planes = planes + float(a.lr) * dpl
    got = losses.cpu().numpy().astype(np.float64)
    lb = 2.0 ** -20 * (1 + a.means)
    print(f"ascent: lr {a.lr}, {len(a.coords)} points, L_vol64 {a.losses[0]:.6f} -> {a.losses[-1]:.6f}, device {got[0]:.6f} -> {got[-1]:.6f}, "
          f"max |dev - 64| / bound {(np.abs(got - a.losses) / lb).max():.3f}")
    assert got[-1] > got[0]
    assert (np.abs(got - a.losses) <= lb).all(), (np.abs(got - a.losses) / lb)


# ------------------------------------------------------------------------------------------------ 7.-10. the guided loop
SCALE, COF = 50.0, 0.4
SRC, TGT = np.array([[0.1, 0.0, -0.1], [-0.3, 0.2, 0.1]], np.float32), np.array([[0.25, 0.1, -0.1], [-0.3, 0.35, 0.2]], np.float32)
CARVE, FILL = ((-0.6, -0.6, -0.6), (-0.1, -0.2, -0.1)), ((0.1, 0.1, 0.0), (0.6, 0.5, 0.6))


@pytest.fixture(scope="module")
def shape():
    """DragStuff on helpers.small96_config() with a loaded shape; get_mesh keeps the latent the loop hands over (loop_img), the
    final latent (tri_feat) and the decoded 32^3 volume, and builds no mesh."""
    from ishapediting_amd import synthetic
    from ishapediting_amd.drag_utils import DragStuff
    from ishapediting_amd.triplane_decoder import decode_volume
    from tests.helpers import small96_args, small96_config
    Tn, w_time = 4, 2
    ds = DragStuff(dev(), args=small96_args(Tn, w_time=w_time, feat_layer=1))
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(small96_config(), 202))
    ds.load_weights(sd, synthetic.decoder_state_dict(), -np.full(96, 1.5, np.float32), np.full(96, 0.5, np.float32))
    ds.set_offset1(2)
    ds.voxel_size = 2.0 / 32

    def get_mesh(tri_feat=None, img=None, t=0):
        ds.loop_img = None if img is None else img.clone()
        if tri_feat is None:
            tri_feat = ds._denoise(img, t)
        ds.tri_feat = tri_feat
        ds.volume = decode_volume(ds.decoder, tri_feat, ds.range, ds.middle, 32)
    ds.get_mesh = get_mesh
    g = torch.Generator().manual_seed(5)
    noise = torch.randn((Tn, 1, 96, 16, 16), generator=g).to(dev())
    ds.step_noise = lambda i: noise[i]
    ds.update_latent_params(img=torch.randn((1, 96, 16, 16), generator=g))
    assert ds.tri_feat0 is not None and tuple(ds.tri_feat0.shape) == (1, 96, 16, 16)
    return ds


def _run(ds, stop_after=None, **kw):
    n = 0
    for _ in ds.training(SRC, TGT, scale=SCALE, cof=COF, **kw):
        n += 1
        if stop_after is not None and n == stop_after:
            ds.train_flag = False
    torch.cuda.synchronize()
    return SimpleNamespace(latent=ds.tri_feat.clone(), loop_img=ds.loop_img.clone(), volume=ds.volume.clone(),
                           losses=torch.stack([l.clone() for l in ds.last_losses]),
                           vol_losses=[l.clone() for l in ds.last_volume_losses])


def _same(a, b):
    return torch.equal(a.latent, b.latent) and torch.equal(a.losses, b.losses) and torch.equal(a.volume, b.volume)


def test_one_guided_step_is_its_public_pieces(shape):
    """7. the latent after one constrained step equals, bit for bit, the one assembled from fresh forwards of the same (x, t):
    backward_input alone, the reconstruct-style chain alone with the new loss, ishap_axpby, the guided update."""
    from ishapediting_amd import constraints as K
    from ishapediting_amd import _lib
    from ishapediting_amd.drag_utils import DragKernels, feat_channel_map
    from ishapediting_amd.regions import Box
    from ishapediting_amd.triplane_decoder import prepare_planes
    ds = shape
    vs = 20.0
    run = _run(ds, stop_after=1, carve=Box(*CARVE), fill=Box(*FILL), volume_scale=vs, volume_res=32, volume_points=4096)
    assert len(run.vol_losses) == 1 and len(run.losses) == 1
    d, model, lib = ds.diffusion, ds.model, _lib.lib()
    i = ds.args.w_time - 1
    x = ds.w.clone()
    noise = ds.step_noise(i)
    ch, width = model.tap_shape(ds.args.feat_layer)
    S = ds.args.image_size
    stream = lambda: _lib.stream_ptr(dev())      # noqa: E731
    # (a) the drag gradient: backward_input alone
    dk = DragKernels(dev(), W=width, ld=ch, chmap=feat_channel_map(ch), r=ds.r1, voxel=ds.voxel_size, loss_type=ds.args.loss_type)
    dk.setup(torch.tensor(SRC, device=dev()), torch.tensor(TGT, device=dev()), COF)
    slot = torch.zeros(1, device=dev())
    kept = {}

    def drag():
        cot, scale2 = dk.loss_cotangent_ptr(model.tap_ptr(), ds.feature_guidance[0].data_ptr(), orig_stride=0, loss_out=slot)
        return model.backward_input(cot, scale2)
    d.prepare(model, range(ds.args.w_time))
    d.p_sample_guidance(model, x, i, feat_layer=ds.args.feat_layer, keep_for_backward=True, want_inter_feat=False, noise=noise,
                        between=lambda: kept.setdefault("drag", drag()), overlap=False, after_tail=lambda mo: kept.update(mo=mo.clone()))
    # (b) the volume gradient: a fresh forward, then the chain of DragStuff.reconstruct with the new loss
    outs = d.p_sample_guidance(model, x, i, feat_layer=ds.args.feat_layer, keep_for_backward=True, want_inter_feat=False, noise=noise)
    cons = K.volume_constraints(carve=Box(*CARVE), fill=Box(*FILL), D=32, max_points=4096, device=dev())
    st = ds.decoder.constraint_setup(cons.points, cons.targets, cons.weights, S)
    planes = prepare_planes(outs["pred_xstart"], ds.range, ds.middle)
    lvol, dplanes, _ = ds.decoder.constraint_loss_grad(planes, st)
    g_direct, cot = torch.empty_like(x), torch.empty((1, 192, S, S), device=dev())
    cot16 = torch.empty((1, 192, S, S), dtype=torch.float16, device=dev())
    bits_, scale2 = torch.zeros(1, dtype=torch.int32, device=dev()), torch.ones(2, device=dev())
    sr, srm1 = float(np.float32(d.sqrt_recip_alphas_cumprod[i])), float(np.float32(d.sqrt_recipm1_alphas_cumprod[i]))
    rng = ds.range.reshape(-1).contiguous()
    _lib.check(lib.ishap_x0_grad_to_cotangent(dplanes.data_ptr(), rng.data_ptr(), x.data_ptr(), outs["model_output"].data_ptr(), sr, srm1,
                                              1, S, g_direct.data_ptr(), cot.data_ptr(), stream()))
    _lib.check(lib.ishap_grad_to_scaled_f16(cot.data_ptr(), cot16.data_ptr(), bits_.data_ptr(), scale2.data_ptr(), cot.numel(), stream()))
    dx = model.backward_from_output(cot16, scale2)
    gvol, grad = torch.empty_like(dx), torch.empty_like(dx)
    _lib.check(lib.ishap_axpby(dx.data_ptr(), g_direct.data_ptr(), 1.0, 1.0, dx.numel(), gvol.data_ptr(), stream()))
    # (c) the mix and (d) the guided update
    _lib.check(lib.ishap_axpby(kept["drag"].data_ptr(), gvol.data_ptr(), 1.0, vs / SCALE, dx.numel(), grad.data_ptr(), stream()))
    want = torch.empty_like(x)
    _lib.check(lib.ishap_guided_update(outs["sample"].data_ptr(), outs["variance"].data_ptr(), grad.data_ptr(), SCALE, None, x.numel(),
                                       want.data_ptr(), stream()))
    fused = d.p_sample_guidance(model, x, i, noise=noise, model_output=kept["mo"], between=lambda: grad, guided_scale=SCALE,
                                want_noise=False)["guided"]
    torch.cuda.synchronize()
    assert float(gvol.abs().max()) > 0 and bool(torch.isfinite(want).all())
    assert torch.equal(run.vol_losses[0].reshape(1), lvol) and torch.equal(run.losses[0].reshape(-1), slot)
    assert torch.equal(fused, want), "the fused step and the two-launch update disagree"
    assert torch.equal(run.loop_img, want), f"max |loop - assembled| {float((run.loop_img - want).abs().max()):.3e}"
    plain = _run(ds, stop_after=1)
    assert not torch.equal(plain.loop_img, run.loop_img)


def test_off_is_off_and_the_snapshot_survives(shape):
    """8. no constraint, and volume_scale = 0, are the plain edit bit for bit; a plain edit after a constrained one restores the
    first-step snapshot."""
    from ishapediting_amd.regions import Box
    ds = shape
    plain = _run(ds)
    assert plain.vol_losses == [] and ds._first_step is not None and ds.model.has_snapshot()
    assert _same(_run(ds, volume_keep=None, carve=None, fill=None), plain)
    assert _same(_run(ds, carve=Box(*CARVE), fill=Box(*FILL), volume_scale=0, volume_res=32), plain)
    first = ds._first_step
    cons = _run(ds, carve=Box(*CARVE), fill=Box(*FILL), volume_keep=Box((-0.9, -0.9, -0.9), (0.9, 0.9, 0.9)), volume_res=32,
                volume_points=2048)
    assert len(cons.vol_losses) == ds.args.w_time and all(bool(torch.isfinite(v)) for v in cons.vol_losses)
    assert not torch.equal(cons.latent, plain.latent)
    assert ds._first_step is first and ds.model.has_snapshot()
    restored = []
    orig = ds.model.snapshot_restore
    ds.model.snapshot_restore = lambda: restored.append(orig()) or restored[-1]
    try:
        after = _run(ds)
    finally:
        ds.model.snapshot_restore = orig
    assert restored == [True] and _same(after, plain)
    # twice the same constrained edit: the same bits
    again = _run(ds, carve=Box(*CARVE), fill=Box(*FILL), volume_keep=Box((-0.9, -0.9, -0.9), (0.9, 0.9, 0.9)), volume_res=32,
                 volume_points=2048)
    assert _same(again, cons) and all(torch.equal(a, b) for a, b in zip(again.vol_losses, cons.vol_losses))


def test_argument_checks_of_the_edit(shape):
    from ishapediting_amd.regions import Box
    ds = shape
    box = Box(*CARVE)
    with pytest.raises(ValueError, match="scale = 0"):
        list(ds.training(SRC, TGT, scale=0.0, cof=COF, carve=box, volume_scale=5.0, volume_res=32))
    with pytest.raises(ValueError, match="carve and fill overlap"):
        list(ds.training(SRC, TGT, scale=SCALE, cof=COF, carve=box, fill=box, volume_res=32))
    with pytest.raises(ValueError, match="fill rasterises to no voxel at D = 32"):
        list(ds.training(SRC, TGT, scale=SCALE, cof=COF, fill=Box((0.01, 0.01, 0.01), (0.02, 0.02, 0.02)), volume_res=32))
    with pytest.raises(ValueError, match="max_points"):
        list(ds.training(SRC, TGT, scale=SCALE, cof=COF, carve=box, volume_points=0))
    with pytest.raises(NotImplementedError, match="training_batch"):
        list(ds.training_batch([SRC], [TGT], scale=SCALE, cof=COF, carve=box))


def test_builder_on_the_device():
    """keep targets from the reference logits; carve and fill override keep; the stride of max_points"""
    from ishapediting_amd import constraints as K
    from ishapediting_amd.regions import Box, Sphere, Voxels
    Dg = 16
    keep, carve = Box((-1, -1, -1), (0.0, 1, 1)), Sphere((0.0, 0.0, 0.0), 0.4)
    fn = lambda p: p[:, 1]      # noqa: E731  "inside" where y > 0
    c = K.volume_constraints(keep=keep, carve=carve, reference_logits_fn=fn, D=Dg, max_points=100000, weights=(2.0, 3.0, 1.0), device=dev())
    ax = 2.0 * np.arange(Dg) / (Dg - 1) - 1.0
    g = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), axis=-1).reshape(-1, 3)
    in_c = (g ** 2).sum(axis=1) <= 0.4 ** 2
    in_k = (g[:, 0] <= 0.0) & ~in_c
    want = np.concatenate([g[in_k], g[in_c]]).astype(np.float32)
    assert np.array_equal(c.points.cpu().numpy(), want)
    assert np.array_equal(c.targets.cpu().numpy(), np.concatenate([g[in_k][:, 1] > 0, np.zeros(in_c.sum(), bool)]).astype(np.float32))
    assert np.array_equal(c.weights.cpu().numpy(), np.concatenate([np.full(in_k.sum(), 2.0), np.full(in_c.sum(), 3.0)]).astype(np.float32))
    few = K.volume_constraints(carve=carve, D=Dg, max_points=10, device=dev())
    step = -(-int(in_c.sum()) // 10)
    assert np.array_equal(few.points.cpu().numpy(), g[in_c][::step].astype(np.float32)) and few.M <= 10
    grid = torch.zeros(Dg, Dg, Dg, dtype=torch.bool)
    grid[3, 4, 5] = grid[10, 2, 2] = True
    v = K.volume_constraints(fill=[Voxels(grid)], D=Dg, device=dev())
    assert np.array_equal(v.points.cpu().numpy(), (np.array([[3, 4, 5], [10, 2, 2]]) * 2.0 / (Dg - 1) - 1.0).astype(np.float32))
    assert np.array_equal(v.targets.cpu().numpy(), np.ones(2, np.float32))
    with pytest.raises(ValueError, match="keep needs reference_logits_fn"):
        K.volume_constraints(keep=keep, D=Dg, device=dev())
    with pytest.raises(ValueError, match="carve rasterises to no voxel at D = 16"):
        K.volume_constraints(carve=Sphere((0.03, 0.03, 0.03), 0.01), D=Dg, device=dev())
    with pytest.raises(ValueError, match="overlap"):
        K.volume_constraints(carve=carve, fill=Box((-0.1, -0.1, -0.1), (0.1, 0.1, 0.1)), D=Dg, device=dev())


def test_constraints_with_tracking_and_the_closed_loop(shape):
    """9. track and closed_loop are orthogonal to the constraints"""
    from ishapediting_amd.regions import Box
    ds = shape
    ds.last_track = None
    run = _run(ds, carve=Box(*CARVE), fill=Box(*FILL), volume_res=32, volume_points=2048, track=True, closed_loop=True)
    assert len(run.vol_losses) == ds.args.w_time == len(run.losses)
    tr = ds.last_track
    assert tr is not None and len(tr["steps"]) == ds.args.w_time and "goals" in tr and bool(torch.isfinite(tr["positions"]).all())
    assert bool(torch.isfinite(run.latent).all())


def test_training_part_solid_passes_moved_and_left(shape):
    """10. solid=True: fill is exactly the plan's moved part, carve exactly part & ~moved"""
    from ishapediting_amd.regions import Rigid, Voxels
    ds = shape
    m = torch.zeros(32, 32, 32, dtype=torch.bool, device=dev())
    m[8:14, 10:16, 12:18] = True
    part = Voxels(m)
    seen = {}
    orig = ds.training

    def spy(*a, **kw):
        seen.update(kw)
        return orig(*a, **kw)
    ds.training = spy
    try:
        for _ in ds.training_part(part, Rigid(translation=(4 * 2.0 / 31, 0.0, 0.0)), handles=4, scale=SCALE, cof=COF, solid=True,
                                  volume_points=512):
            pass
    finally:
        ds.training = orig
    torch.cuda.synchronize()
    moved = ds.part_plan.moved.mask
    assert seen["fill"] is ds.part_plan.moved and torch.equal(seen["carve"].mask, m & ~moved) and seen["volume_res"] == 32
    assert int((m & ~moved).sum()) > 0 and int(moved.sum()) == int(m.sum())
    assert len(ds.last_volume_losses) == ds.args.w_time
    seen.clear()
    ds.training = spy
    try:
        list(ds.training_part(part, Rigid(translation=(4 * 2.0 / 31, 0.0, 0.0)), handles=4, scale=SCALE, cof=COF))
    finally:
        ds.training = orig
    assert "fill" not in seen and "carve" not in seen and ds.last_volume_losses == []
