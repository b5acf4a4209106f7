"""Direct triplane fitting on the GPU (drag_utils.py:473-550, train_triplane_opt): the fit kernel's loss and gradient, the
regulariser + Adam kernels, a ten-step trajectory against golden G17 and the public call end to end.  The oracle is the
test-side statement tests/triplane_opt_ref.py (held to G17 by tests/test_triplane_opt_host.py).  No test compares whole
fitted planes element by element: float atomics and Adam's sign-like first steps make their last bits run-dependent."""
import os
import sys
import time

import numpy as np
import pytest
import torch

from ishapediting_amd import synthetic
from tests.helpers import small96_args, small96_config

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triplane_opt_ref as R  # noqa: E402
from triplane_opt_ref import G17_DISPLACEMENT_SPREAD, G17_GRAD1_SPREAD, G17_TOTAL_LOSS_SPREAD  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda", 0)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-300))


def decoder(net):
    from ishapediting_amd.triplane_decoder import MultiTriplane
    d = MultiTriplane(1, device=dev())
    d.net.load_state_dict({k: torch.as_tensor(np.asarray(v)) for k, v in net.items()})
    return d


def to_cl(p):
    """[3,32,S,S] -> channels-last [3,S,S,32] on the device"""
    return torch.as_tensor(np.asarray(p)).float().permute(0, 2, 3, 1).contiguous().to(dev())


def to_nchw(p):
    return p.detach().permute(0, 3, 1, 2).contiguous().cpu()


def reg_grad64(p):
    """d (0.001 l2reg + 0.01 tvreg) / d planes in fp64"""
    p = torch.as_tensor(np.asarray(p)).double().clone().requires_grad_(True)
    (R.L2_W * R.l2reg(p) + R.TV_W * R.tvreg(p)).backward()
    return p.grad


def grad64(net, p, coords, gt, idx, r, noise, terms):
    """fp64 autograd of the selected data / pair terms: (bce, mse, d(bce * terms[0] + 0.3 mse * terms[1])/d planes)"""
    n = R.net_as(net, torch.float64)
    p = torch.as_tensor(np.asarray(p)).double().clone().requires_grad_(True)
    bce, mse = R.data_pair_terms(n, p, torch.as_tensor(coords).double(), torch.as_tensor(gt).double(), idx,
                                 torch.as_tensor(r).double(), torch.as_tensor(noise).double())
    (terms[0] * bce + terms[1] * R.PAIR_W * mse).backward()
    return float(bce.detach()), float(mse.detach()), p.grad


def empty3():
    return torch.empty((0, 3), dtype=torch.float32)


def test_step1_parity_with_the_fixture(gold):
    """Step 1 of golden G17 (the reference's own MultiTriplane, fp32): loss parts within 1e-5 relative; the gradient
    (kernel's data + pair part, plus the regulariser part in fp64) within 4x the measured fp32/fp64 spread of the step-1
    gradient; the data term alone within 1e-3 of fp64 autograd."""
    from ishapediting_amd.triplane_decoder import reg_values
    g = gold("g17_triplane_opt")
    net, p0, coords, gt = R.fixture_inputs(g)
    idx, r, noise = R.fixture_batches(g)[0]
    dec = decoder(net)
    planes = to_cl(p0)
    parts, dpl = dec.fit_loss_grad(planes, torch.from_numpy(coords), torch.from_numpy(gt), torch.from_numpy(idx),
                                   torch.from_numpy(r), torch.from_numpy(noise))
    reg = reg_values(planes)
    got = torch.cat([parts, reg]).cpu().double().numpy()
    np.testing.assert_allclose(got, g["parts"][0, :4], rtol=1e-5)
    total = to_nchw(dpl).double() + reg_grad64(p0)
    e = rel(total, torch.from_numpy(g["grad1"]))
    assert e <= 4 * G17_GRAD1_SPREAD, e
    _, d_only = dec.fit_loss_grad(planes, torch.from_numpy(coords), torch.from_numpy(gt), torch.from_numpy(idx), empty3(),
                                  empty3())
    bce64, _, gd = grad64(net, p0, coords, gt, idx, r, noise, (1.0, 0.0))
    assert rel(to_nchw(d_only), gd) <= 1e-3, rel(to_nchw(d_only), gd)


def test_fit_loss_grad_vs_fp64_autograd_full_size():
    """S = 128, 40 000 data points of both classes, 40 000 pairs, some on the cube's faces so that r + delta leaves it.
    Loss parts within 1e-4 abs + 1e-4 rel of fp64 autograd; the data, pair and combined gradients within 4x the relative
    L2 spread between fp32 and fp64 runs of the same autograd statement (data: at least 1e-3)."""
    g = torch.Generator().manual_seed(5)
    S, N = 128, 40000
    net = {k: v.numpy() for k, v in synthetic.decoder_state_dict(4321).items()}
    p = (torch.randn(3, 32, S, S, generator=g) * 0.4 + 0.05).numpy()
    coords = (torch.rand(N, 3, generator=g) * 2 - 1).numpy()
    gt = (np.linalg.norm(coords, axis=1) < 0.8).astype(np.float32)
    assert 0.2 < gt.mean() < 0.8
    idx = torch.randperm(N, generator=g)[: N - 123].numpy().astype(np.int64)      # a partial last tile
    r = torch.rand(N, 3, generator=g) * 2 - 1
    r[:2000, 0] = torch.where(r[:2000, 0] > 0, 1.0, -1.0)                           # on a face: the partner leaves the cube
    r = r.numpy()
    noise = torch.randn(N, 3, generator=g).numpy()
    assert (np.abs(r + noise * 0.01) > 1).any(axis=1).sum() > 500
    dec = decoder(net)
    planes = to_cl(p)
    T = torch.from_numpy
    parts, dpl = dec.fit_loss_grad(planes, T(coords), T(gt), T(idx), T(r), T(noise))
    bce, mse, gboth = grad64(net, p, coords, gt, idx, r, noise, (1.0, 1.0))
    np.testing.assert_allclose(parts.cpu().double().numpy(), [bce, mse], rtol=1e-4, atol=1e-4)
    _, d_data = dec.fit_loss_grad(planes, T(coords), T(gt), T(idx), empty3(), empty3())
    empty_i = torch.empty(0, dtype=torch.int32)
    pp, d_pair = dec.fit_loss_grad(planes, T(coords), T(gt), empty_i, T(r), T(noise))
    assert float(pp[0]) == 0.0
    _, _, gdata = grad64(net, p, coords, gt, idx, r, noise, (1.0, 0.0))
    gpair = gboth - gdata
    # the spreads between fp32 and fp64 runs of the same autograd statement, measured here on the CPU: ~8e-3 for the data
    # term at these inputs, more for the pair term (its z_r - z_r+delta cancels), so a fixed 1e-3 bar would fail fp32 itself
    n32 = R.net_as(net, torch.float32)
    spread = []
    for terms in ((1.0, 0.0), (0.0, 1.0)):
        p32 = torch.as_tensor(p).clone().requires_grad_(True)
        bce32, mse32 = R.data_pair_terms(n32, p32, T(coords), T(gt), idx, T(r), T(noise))
        (terms[0] * bce32 + terms[1] * R.PAIR_W * mse32).backward()
        spread.append(rel(p32.grad, gdata if terms[0] else gpair))
    e_data, e_pair, e_all = rel(to_nchw(d_data), gdata), rel(to_nchw(d_pair), gpair), rel(to_nchw(dpl), gboth)
    print(f"fp32/fp64 spread data {spread[0]:.2e} pair {spread[1]:.2e}; kernel data {e_data:.2e} pair {e_pair:.2e} "
          f"both {e_all:.2e}")
    assert e_data <= max(4 * spread[0], 1e-3), (e_data, spread)
    assert e_pair <= 4 * spread[1], (e_pair, spread)
    assert e_all <= 4 * max(spread), (e_all, spread)


def test_reg_adam_vs_torch_adam_fp64():
    """The regulariser + Adam launches against torch.optim.Adam in fp64 on the same injected gradient, at t = 1 and at
    t = 50 (bias corrections); planes, m, v and the regulariser values within 1e-6 relative; two launches on the same
    inputs are bitwise equal."""
    from ishapediting_amd.triplane_decoder import TriplaneAdam
    g = torch.Generator().manual_seed(9)
    S = 32
    p0 = torch.randn(3, 32, S, S, generator=g) * 0.3 + 0.1
    inj = torch.randn(3, 32, S, S, generator=g) * 1e-3
    m0 = torch.randn(3, 32, S, S, generator=g) * 1e-4
    v0 = torch.rand(3, 32, S, S, generator=g) * 1e-7
    for t0 in (0, 49):
        outs = []
        for _ in range(2):
            opt = TriplaneAdam(to_cl(p0), lr=1e-3)
            if t0:
                opt.m.copy_(to_cl(m0))
                opt.v.copy_(to_cl(v0))
                opt.step_count.fill_(t0)
            opt.dplanes.copy_(to_cl(inj))
            regp = torch.zeros(2, device=dev())
            opt.step(regp)
            outs.append((opt.planes.clone(), opt.m.clone(), opt.v.clone(), regp.clone()))
            assert int(opt.step_count) == t0 + 1 and not bool(opt.dplanes.any())
        for a, b in zip(outs[0], outs[1]):
            assert torch.equal(a, b)
        # fp64 reference
        p = p0.double().clone().requires_grad_(True)
        reg = R.L2_W * R.l2reg(p) + R.TV_W * R.tvreg(p)
        reg.backward()
        p.grad += inj.double()
        ref = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
        if t0:
            ref.state[p] = {"step": torch.tensor(float(t0)), "exp_avg": m0.double().clone(), "exp_avg_sq": v0.double().clone()}
        ref.step()
        st = ref.state[p]
        # planes and m element by element; v as a whole: where the injected and the regulariser gradients cancel, the fp32
        # gradient's relative error (and v's, twice it) reaches 1e-5 on single elements
        for got, want, elementwise in ((outs[0][0], p.detach(), True), (outs[0][1], st["exp_avg"], True),
                                       (outs[0][2], st["exp_avg_sq"], False)):
            gt_ = to_nchw(got).double()
            assert rel(gt_, want) <= 1e-6, rel(gt_, want)
            if elementwise:
                np.testing.assert_allclose(gt_.numpy(), want.numpy(), rtol=1e-6, atol=1e-6 * float(want.abs().max()))
        with torch.no_grad():
            regs = [float(R.l2reg(p0.double())), float(R.tvreg(p0.double()))]
        np.testing.assert_allclose(outs[0][3].cpu().double().numpy(), regs, rtol=1e-6)


def test_ten_step_trajectory_vs_the_fixture(gold):
    """Golden G17's ten injected steps through fit_triplanes: per-step total loss within 4x the measured fp32/fp64 spread
    of the reference's losses; the planes' displacement from init within 4x the measured spread of the fp64 run's."""
    from ishapediting_amd.triplane_decoder import fit_triplanes, planes_to_latent, total_loss
    g = gold("g17_triplane_opt")
    net, p0, coords, gt = R.fixture_inputs(g)
    batches = R.fixture_batches(g)
    dec = decoder(net)
    S = p0.shape[-1]
    T = torch.from_numpy

    def batch_fn(k):
        idx, r, noise = batches[k]
        return T(idx), T(r), T(noise)
    planes, losses = fit_triplanes(dec, T(coords), T(gt), T(p0).reshape(1, 96, S, S), epochs=10, batch_size=coords.shape[0],
                                   batch_fn=batch_fn)
    tot = total_loss(losses).cpu().double().numpy()
    assert losses.shape == (10, 4)
    dl = np.abs(tot - g["parts"][:, 4])
    assert dl.max() <= 4 * G17_TOTAL_LOSS_SPREAD, dl
    _, _, p64, _ = R.run_fit(net, p0, coords, gt, batches, torch.float64)
    disp = planes_to_latent(planes).cpu().double().reshape(3, 32, S, S) - T(p0).double()
    e = rel(disp, p64 - T(p0).double())
    assert e <= 4 * G17_DISPLACEMENT_SPREAD, e


def test_train_triplane_opt_end_to_end(tmp_path):
    """The public call on a sphere mesh (small config, S = 16, 20 000 points, batch 4 000, 20 epochs, injected batches):
    files, returned latent, falling loss, 32^3 occupancy against the fp64 fit of the same batches (at least 99 %, or
    within twice the disagreement of the fp32 fit where that is larger), the round trip
    through train_triplane(tri_feat_path=...), and the drag state left alone."""
    from ishapediting_amd import mesh as mesh_backend
    from ishapediting_amd.drag_utils import DragStuff
    from ishapediting_amd.triplane_decoder import planes_to_latent, total_loss
    from oracle import ref_cpu as O
    ax = torch.arange(32, dtype=torch.float32, device=dev()) - 15.5
    sph = 11.0 - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    v, f = mesh_backend.extract_surface(sph)
    verts = v / 31 * 2 - 1
    args = small96_args(4, w_time=2, feat_layer=1)
    ds = DragStuff(dev(), args=args)
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(small96_config(), 202))
    dec_sd = synthetic.decoder_state_dict()
    lower, upper = -np.full(96, 1.5, np.float32), np.full(96, 0.5, np.float32)
    ds.load_weights(sd, dec_sd, lower, upper)
    rs = np.random.RandomState(4)
    means, stds = (0.05 * rs.randn(96)).astype(np.float32), (0.3 + 0.1 * rs.rand(96)).astype(np.float32)
    seed, S, P, B, E = 11, 16, 20000, 4000, 20
    # the batches the fit gets, and the samples / init it will draw from `seed` (to run the same fit in fp64)
    pts, occ = mesh_backend.sample_occupancy((verts, f), None, True, P, 0.5, device=dev(),
                                             generator=torch.Generator().manual_seed(seed))
    pts, occ = (np.asarray(a.cpu() if torch.is_tensor(a) else a, dtype=np.float32) for a in (pts, occ))
    occ = occ.reshape(-1)
    assert 0.1 < occ.mean() < 0.9
    gb = torch.Generator().manual_seed(99)
    batches = []
    for _ in range(E):
        perm = torch.randperm(P, generator=gb)
        for s in range(0, P, B):
            batches.append((perm[s:s + B].numpy(), (torch.rand(B, 3, generator=gb) * 2 - 1).numpy(),
                            torch.randn(B, 3, generator=gb).numpy()))
    gi = torch.Generator(device=dev()).manual_seed(seed)
    init = (torch.randn((1, 96, S, S), generator=gi, device=dev()) * torch.from_numpy(stds).to(dev()).reshape(1, 96, 1, 1)
            + torch.from_numpy(means).to(dev()).reshape(1, 96, 1, 1)).cpu()
    w_sentinel = torch.full((1, 96, S, S), 3.0, device=dev())
    mesh0_sentinel = object()
    ds.w, ds.mesh0 = w_sentinel, mesh0_sentinel
    T = torch.from_numpy
    t0 = time.perf_counter()
    lat = ds.train_triplane_opt(mesh=(verts, f), path=str(tmp_path), stats=(means, stds), epochs=E, batch_size=B, seed=seed,
                                batch_fn=lambda k: tuple(T(a) for a in batches[k]))
    torch.cuda.synchronize()
    print(f"train_triplane_opt S={S} {len(batches)} steps: {time.perf_counter() - t0:.3f} s")
    # files and return value
    tri = np.load(tmp_path / "tri_feat_opt.npy")
    assert tri.shape == (1, 96, S, S) and (tmp_path / "mesh_opt.obj").exists()
    planes = torch.cat([e.reshape(32, S, S) for e in ds.decoder.embeddings]).reshape(1, 96, S, S)
    rng, mid = (upper - lower) / 2, (upper + lower) / 2
    want = (planes.cpu() - T(mid).reshape(1, 96, 1, 1)) / T(rng).reshape(1, 96, 1, 1)
    assert torch.allclose(lat.cpu(), want, rtol=1e-6, atol=1e-6) and np.array_equal(tri, lat.cpu().numpy())
    # loss
    assert tuple(ds.last_losses.shape) == (len(batches), 4)
    tot = total_loss(ds.last_losses).cpu()
    assert float(tot[-5:].mean()) < float(tot[0]), tot
    # the same fit in fp64
    _, t64, p64, _ = R.run_fit(dec_sd, init.reshape(3, 32, S, S).numpy(), pts, occ, batches, torch.float64)
    assert float(t64[-5:].mean()) < float(t64[0])
    vol_ref = O.decode_volume(dec_sd, p64.float().reshape(1, 96, S, S), 1.0, 0.0, 32)
    agree = float(((ds.volume.cpu() > 0) == (vol_ref > 0)).double().mean())
    # the fp32 run of the same statement, for the spread: the synthetic decoder leaves ~2.5 % of this grid within 0.01 of the
    # zero level, and 100 Adam steps move fp32 and fp64 fits apart there (measured on the CPU: 97.3 % agreement)
    _, _, p32, _ = R.run_fit(dec_sd, init.reshape(3, 32, S, S).numpy(), pts, occ, batches, torch.float32)
    vol32 = O.decode_volume(dec_sd, p32.reshape(1, 96, S, S), 1.0, 0.0, 32)
    spread = 1 - float(((vol32 > 0) == (vol_ref > 0)).double().mean())
    print(f"occupancy agreement with the fp64 fit: {agree:.5f} (fp32 statement: {1 - spread:.5f})")
    assert 1 - agree <= max(0.01, 2 * spread), (agree, spread)
    # drag state untouched
    assert ds.w is w_sentinel and bool((ds.w == 3.0).all()) and ds.mesh0 is mesh0_sentinel
    # round trip
    ds.train_triplane(tri_feat_path=str(tmp_path / "tri_feat_opt.npy"))
    assert tuple(ds.w.shape) == (1, 96, S, S) and bool(torch.isfinite(ds.w).all()) and ds.mesh0 is not None


def test_full_size_fit():
    """S = 128, 200 000 points, 20 epochs x 5 batches of 40 000 (the reference's defaults) with a seeded generator: every
    output finite, the loss falls.  Prints the fit time."""
    from ishapediting_amd.triplane_decoder import MultiTriplane, fit_triplanes, total_loss
    dec = MultiTriplane(1, device=dev())
    dec.net.load_state_dict(synthetic.decoder_state_dict(4321))
    g = torch.Generator(device=dev()).manual_seed(3)
    P = 200000
    uni = torch.rand((P // 2, 3), generator=g, device=dev()) * 2 - 1
    d = torch.randn((P // 2, 3), generator=g, device=dev())
    surf = 0.6 * d / d.norm(dim=1, keepdim=True) + 0.01 * torch.randn((P // 2, 3), generator=g, device=dev())
    pts = torch.cat([uni, surf])
    occ = (pts.norm(dim=1) < 0.6).float()
    init = torch.randn((1, 96, 128, 128), generator=g, device=dev()) * 0.3
    fit_triplanes(dec, pts, occ, init, epochs=1, batch_size=40000, generator=g)     # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    planes, losses = fit_triplanes(dec, pts, occ, init, epochs=20, batch_size=40000, generator=g)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"full-size fit: {dt * 1e3:.1f} ms for {losses.shape[0]} steps ({dt * 1e3 / losses.shape[0]:.3f} ms/step)")
    assert losses.shape == (100, 4)
    assert bool(torch.isfinite(planes).all()) and bool(torch.isfinite(losses).all())
    tot = total_loss(losses).cpu()
    assert float(tot[-5:].mean()) < float(tot[0]), tot
