"""CPU checks around the triplane decoder oracle (no GPU): tests/decoder_ref.py against what the project already trusts
(oracle/ref_cpu.py, golden g6_decoder, tests/triplane_opt_ref.py, torch autograd of the clamp chain); the forward bound passes the
float64 result with the kernel's rounding points applied and rejects every listed mutation; the backward bound rejects its
mutations; the share of candidates the kink filter drops; the hi/lo split's range as a rerunnable simulation; and the argument
checks of the decoder calls, which fail before any device work.

Measured here (synthetic weights, planes 0.05 * randn, S = 16, 4153 points):
  forward bound      median 2.2e-4 at s = 1 (2.4e-4 .. 3.4e-4 for s = 2^+-2 .. 2^+-4); the honest result sits at 0.03 of it.
  rejection factors  (largest error / bound over the points)   w_lo dropped 1.46, x_lo dropped 1.32, lo parts flushed 1.40
                     (their error is 4e-4 at the worst point); b1 missing 820; every other forward mutation above 3000.
                     Backward: one of 512 contributions lost 2.8, border column weights 1.6e5, 1 / 64 for 1 / 33 88,
                     partner's sign 85.
  kink filter        single points: 3.7 % (S = 2), 4.6 % (S = 8), 4.4 % (S = 16) of 1100 candidates dropped;
                     pairs (both points must pass): 6.3 % (S = 2), 7.0 % (S = 16) of 256.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from tests import decoder_ref as D

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triplane_opt_ref as R  # noqa: E402

FAKE = 0x1000                                     # a non-null address nothing dereferences


def _net_t(sd):
    return {k: torch.as_tensor(v).double() for k, v in sd.items()}


def _nchw(planes):
    return torch.as_tensor(np.asarray(planes)).double().permute(0, 3, 1, 2).contiguous()


@pytest.fixture
def exact_two_pi(monkeypatch):
    """oracle/ref_cpu.py run in float64 multiplies by 2 * np.pi unrounded; the statement's constant is float32(2 pi), what an fp32
    run of the reference (and the kernels) multiply by.  For a comparison in float64 the statement takes the oracle's constant."""
    monkeypatch.setattr(D, "TWO_PI", 2 * np.pi)


# ------------------------------------------------------------------------------------------------ the statement
@pytest.mark.parametrize("S", [2, 8, 16])
def test_forward_statement_matches_the_cpu_oracle(S, exact_two_pi):
    sd, net = D.synthetic_net()
    planes = D.make_planes(S, 0.4, 5)
    coords = D.mixed_coords(40, S, 6)
    coords = coords[np.abs(coords).max(axis=1) < 1e5]                          # grid_sample's own index arithmetic stays in range
    want = O.decoder_forward(_net_t(sd), _nchw(planes), torch.as_tensor(coords).double()).numpy()
    got = D.forward(net, planes, coords).logit
    assert np.abs(got - want).max() < 1e-11
    beyond = D.coords_family("beyond", 16, S, np.random.RandomState(1))
    z0 = D.mlp(net, np.concatenate([np.zeros((1, 64)), np.ones((1, 64))], axis=1))[4][0]
    assert np.abs(D.forward(net, planes, beyond).logit - z0).max() < 1e-15          # zero features: one value


def test_grid_rule_and_volume_match_the_cpu_oracle(exact_two_pi):
    sd, net = D.synthetic_net()
    for res in (1, 5, 7):
        axis = torch.linspace(-1, 1, res).numpy()                               # res = 1: [-1]
        assert axis[0] == -1.0 and np.array_equal(D.grid_coords(axis), O.grid_coords(res).numpy())
    lat = torch.randn(1, 96, 8, 8, generator=torch.Generator().manual_seed(3)) * 0.3
    rng = torch.rand(96, generator=torch.Generator().manual_seed(4)).reshape(1, 96, 1, 1) + 0.5
    mid = torch.randn(96, generator=torch.Generator().manual_seed(5)).reshape(1, 96, 1, 1) * 0.1
    planes, prod = D.planes_prepare(lat[0].numpy(), rng.reshape(-1).numpy(), mid.reshape(-1).numpy())
    want = O.decode_volume({k: torch.as_tensor(v) for k, v in sd.items()}, lat, rng, mid, 5)      # the oracle's fp32 run
    got = D.forward(net, planes, D.grid_coords(torch.linspace(-1, 1, 5).numpy())).logit.reshape(5, 5, 5)
    assert np.abs(got - want.numpy()).max() < 1e-4
    assert np.array_equal(D.planes_prepare(lat[0].numpy(), None, None)[0].transpose(0, 3, 1, 2).reshape(96, 8, 8), lat[0].double().numpy())
    assert (prod >= 0).all() and np.abs(planes).max() <= prod.max() + np.abs(mid).max()


def test_golden_g6_within_the_forward_bound(gold):
    """The reference's own fp32 MultiTriplane (golden g6, planes 0.5 * randn, coordinates in [-1.2, 1.2] and eight hand-picked
    border points) against the float64 statement: an fp32 evaluation, so inside the bound the split kernel gets."""
    g = gold("g6_decoder")
    _, net = D.synthetic_net()
    planes = np.ascontiguousarray(g["planes"].transpose(0, 2, 3, 1))
    fw = D.forward(net, planes, g["coords"])
    ratio = np.abs(fw.logit - g["logits"]) / D.forward_bound(net, planes, fw).bound
    print(f"g6: max |fp32 reference - float64| {np.abs(fw.logit - g['logits']).max():.2e}, max error / bound {ratio.max():.3f}")
    assert ratio.max() < 1.0


def test_loss_statements_match_autograd_of_the_cpu_oracle(exact_two_pi):
    sd, net = D.synthetic_net()
    S = 8
    planes = D.make_planes(S, 0.3, 7)
    rs = np.random.RandomState(8)
    coords = rs.uniform(-1.05, 1.05, (300, 3)).astype(np.float32)
    gt = (rs.rand(300) < 0.5).astype(np.float32)
    nt = _net_t(sd)
    p = _nchw(planes).requires_grad_(True)
    z = O.decoder_forward(nt, p, torch.as_tensor(coords).double())
    loss = -F.binary_cross_entropy_with_logits(z, torch.as_tensor(gt).double())
    loss.backward()
    got = D.points_loss_grad(net, planes, coords, gt)
    assert abs(got.loss - float(loss)) < 1e-13 and np.abs(got.logits - z.detach().numpy()).max() < 1e-11
    assert np.abs(got.dplanes.transpose(0, 3, 1, 2) - p.grad.numpy()).max() < 1e-13
    assert (got.A >= np.abs(got.dplanes) - 1e-18).all() and (got.A1 >= 0).all() and (got.Aw >= 0).all()
    one = D.points_loss_grad(net, planes, coords[:1], gt[:1])                   # one point, nothing cancels: A is |gradient| itself
    assert np.abs(one.A - np.abs(one.dplanes)).max() <= 1e-15 * one.A.max() and one.A.max() > 0
    sig = 1.0 / (1.0 + np.exp(-one.logits[0]))
    assert np.abs(one.A - abs(sig - gt[0]) * one.A1).max() <= 1e-12 * one.A.max()        # A = |d bce / d z| A1 for one point
    assert np.array_equal(one.cnt > 0, one.A1 > 0) or (one.cnt >= (one.A1 > 0)).all()
    # the fit terms against tests/triplane_opt_ref.py (its partner is r + 1e-2 noise in float64: hand it the fp32 partner)
    idx = rs.randint(0, 300, 77)
    r = rs.uniform(-1, 1, (50, 3)).astype(np.float32)
    noise = rs.randn(50, 3).astype(np.float32)
    noise64 = (D.partner(r, noise).astype(np.float64) - r) * 100.0
    p = _nchw(planes).requires_grad_(True)
    bce, mse = R.data_pair_terms(nt, p, torch.as_tensor(coords).double(), torch.as_tensor(gt).double(), idx,
                                 torch.as_tensor(r).double(), torch.as_tensor(noise64))
    (bce + float(np.float32(R.PAIR_W)) * mse).backward()
    got = D.fit_loss_grad(net, planes, coords, gt, idx, r, noise, R.PAIR_W)
    assert np.abs(got.parts - [float(bce), float(mse)]).max() < 1e-13
    assert np.abs(got.dplanes.transpose(0, 3, 1, 2) - p.grad.numpy()).max() < 1e-12 * np.abs(p.grad.numpy()).max() + 1e-16
    only_pairs = D.fit_loss_grad(net, planes, coords, gt, [], r, noise, R.PAIR_W)
    only_data = D.fit_loss_grad(net, planes, coords, gt, idx, r[:0], noise[:0], R.PAIR_W)
    assert only_pairs.parts[0] == 0.0 and only_data.parts[1] == 0.0
    assert np.abs(only_pairs.dplanes + only_data.dplanes - got.dplanes).max() < 1e-15


@pytest.mark.parametrize("clip", [0, 1])
@pytest.mark.parametrize("with_range", [False, True])
def test_x0_grad_statement_matches_autograd_of_the_clamp_chain(clip, with_range):
    gen = torch.Generator().manual_seed(13)
    S, sr, srm1 = 8, 1.7716, 1.4624
    x = torch.randn(96, S, S, generator=gen).double()
    eps = torch.randn(192, S, S, generator=gen).double()
    x[0, 0, 0], eps[0, 0, 0] = 1.0 / float(np.float32(sr)), 0.0                 # lands on the clamp's edge up to rounding
    rng = (torch.rand(96, generator=gen) + 0.5).double() if with_range else None
    dpl = torch.randn(3, S, S, 32, generator=gen).double()
    xr, er = x.clone().requires_grad_(True), eps[:96].clone().requires_grad_(True)
    x0 = float(np.float32(sr)) * xr - float(np.float32(srm1)) * er
    if clip:
        x0 = x0.clamp(-1, 1)
    planes = x0 * (rng.reshape(96, 1, 1) if with_range else 1.0)
    gx, ge = torch.autograd.grad((planes.reshape(3, 32, S, S) * dpl.permute(0, 3, 1, 2)).sum(), (xr, er))
    g_direct, cot, _ = D.x0_grad(dpl.numpy(), None if rng is None else rng.numpy(), x.numpy(), eps.numpy(), sr, srm1, clip)
    assert np.abs(g_direct - gx.numpy()).max() < 1e-14 and np.abs(cot[:96] - ge.numpy()).max() < 1e-14
    assert np.array_equal(cot[96:], np.zeros((96, S, S)))
    if clip:
        assert int((g_direct == 0).sum()) > 100


# ------------------------------------------------------------------------------------------------ the forward bound
def _forward_case(S=16, n_each=300, amp=D.AMP_FWD):
    sd, net = D.synthetic_net()
    planes = D.make_planes(S, amp, 21)
    coords = np.concatenate([D.mixed_coords(n_each, S, 22), np.random.RandomState(23).uniform(-1.1, 1.1, (2053, 3)).astype(np.float32)])
    fw = D.forward(net, planes, coords)
    return sd, net, planes, coords, fw, D.forward_bound(net, planes, fw)


def test_forward_bound_passes_the_honest_result():
    """float64 with the kernel's rounding points applied (fp32 taps, features, phases; sin / cos off by SIN_ABS; the hi/lo split
    with fp16 subnormals kept) stays inside the bound, for the synthetic weights and for both layers rebalanced by 2^+-4."""
    sd, net, planes, coords, fw, fb = _forward_case()
    for k in (-4, -2, 0, 2, 4):
        net_k = D.net64(D.scaled_state_dict(sd, k))
        fw_k = D.forward(net_k, planes, coords)
        assert np.abs(fw_k.logit - fw.logit).max() < 1e-13                     # positively homogeneous: the same function
        b = D.forward_bound(net_k, planes, fw_k).bound
        e = np.abs(D.honest_forward(net_k, planes, coords) - fw_k.logit)
        print(f"s = 2^{k:+d}: honest max error {e.max():.2e}, bound median {np.median(b):.2e}, max error / bound {(e / b).max():.3f}")
        assert (e / b).max() < 1.0


def test_forward_bound_rejects_mutated_references():
    sd, net, planes, coords, fw, fb = _forward_case()
    n = len(coords)
    assert n % 32 not in (0, 1)
    tail = fw.logit.copy()
    tail[n - n % 32 + 1:] = fw.logit[n - n % 32:-1]
    mut = {
        "u and v swapped on plane xy": D.forward(net, planes, coords, plane_axes=((1, 0), (1, 2), (0, 2))).logit,
        "plane xz dropped": D.forward(net, planes, coords, planes_used=(0, 1)).logit,
        "align_corners=False": D.forward(net, planes, coords, align_corners=False).logit,
        "sin and cos blocks swapped": D.forward(net, planes, coords, swap_sincos=True).logit,
        "b1 missing": D.forward(net, planes, coords, no_b1=True).logit,
        "w_lo term dropped": D.honest_forward(net, planes, coords, drop_wlo=True),
        "x_lo term dropped": D.honest_forward(net, planes, coords, drop_xlo=True),
        "lo parts below 2^-14 flushed": D.honest_forward(net, planes, coords, scale_mode="flush"),
        "border tap reads the clamped texel": D.forward(net, planes, coords, clamp_border=True).logit,
        "tail tile: point i gets point i-1's result": tail,
    }
    bad = []
    for name, z in mut.items():
        e = np.abs(z - fw.logit)
        factor = (e / fb.bound).max()
        print(f"{name:45s} max error {e.max():.2e}  rejection factor {factor:10.2f}")
        if not factor > 1.0:
            bad.append(name)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the backward bound
def _rel_runs(fn, net, *args, **kw):
    return [fn(D.permuted_net(net, s), *args, dtype=torch.float32, **kw).dplanes for s in range(D.REL_RUNS)]


def test_permuted_net_is_the_same_function():
    _, net = D.synthetic_net()
    pool = D.survivor_pool(16)
    a = D.points_loss_grad(net, pool.planes, pool.coords[:50], np.ones(50))
    b = D.points_loss_grad(D.permuted_net(net, 3), pool.planes, pool.coords[:50], np.ones(50))
    assert np.abs(a.dplanes - b.dplanes).max() < 1e-15 and abs(a.loss - b.loss) < 1e-14


def test_backward_bound_rejects_mutated_references():
    _, net = D.synthetic_net()
    S = 16
    pool = D.survivor_pool(S)
    planes = pool.planes
    out = {}
    # a texel's gradient missing one of 512 shared contributions
    c = np.concatenate([np.repeat(pool.coords[:1], 512, 0), pool.coords[1:513]])
    gt = (np.arange(len(c)) % 2).astype(np.float32)
    ref = D.points_loss_grad(net, planes, c, gt)
    rel = D.measured_rel(_rel_runs(D.points_loss_grad, net, planes, c, gt), ref)
    bound = D.backward_bound(ref, rel)
    lost = D.points_loss_grad(net, planes, np.delete(c, 3, 0), np.delete(gt, 3), npts_div=len(c)).dplanes
    out["one of 512 shared contributions lost"] = (rel, np.abs(lost - ref.dplanes), bound, ref)
    # the border column's weights using wx0 for wx1
    cb = pool.coords[:400].copy()
    cb[:, 0] = np.random.RandomState(2).uniform(0.9, 1.0, 400).astype(np.float32)        # between the last two columns
    cb = D.filtered(net, planes, cb)
    gtb = (np.arange(len(cb)) % 2).astype(np.float32)
    refb = D.points_loss_grad(net, planes, cb, gtb)
    relb = D.measured_rel(_rel_runs(D.points_loss_grad, net, planes, cb, gtb), refb)
    bug = D.points_loss_grad(net, planes, cb, gtb, border_w_bug=True).dplanes
    out["border column weighted with wx0"] = (relb, np.abs(bug - refb.dplanes), D.backward_bound(refb, relb), refb)
    # 1 / npts replaced by 1 / (npts rounded up to 32)
    c33, gt33 = pool.coords[600:633], (np.arange(33) % 2).astype(np.float32)
    ref33 = D.points_loss_grad(net, planes, c33, gt33)
    rel33 = D.measured_rel(_rel_runs(D.points_loss_grad, net, planes, c33, gt33), ref33)
    out["1 / npts taken as 1 / 64 for 33 points"] = (rel33, np.abs(ref33.dplanes * (33 / 64) - ref33.dplanes),
                                                     D.backward_bound(ref33, rel33), ref33)
    # the pair term's sign flipped on the partner
    pp = D.pair_pool(S, on_faces=64)
    args = (planes, pool.coords[:40], gt[:40], np.arange(40), pp.r[:64], pp.noise[:64], 0.3)
    reff = D.fit_loss_grad(net, *args)
    relf = D.measured_rel(_rel_runs(D.fit_loss_grad, net, *args), reff)
    flip = D.fit_loss_grad(net, *args, flip_partner=True).dplanes
    out["pair cotangent with the wrong sign on the partner"] = (relf, np.abs(flip - reff.dplanes), D.backward_bound(reff, relf), reff)
    bad = []
    for name, (rel, err, bound, ref) in out.items():
        m = ref.A > 0
        factor = (err[m] / bound[m]).max()
        print(f"{name:52s} REL {rel:.2e}  rejection factor {factor:10.2f}")
        assert (err[~m] == 0).all() or name.startswith("border")
        if not factor > 1.0:
            bad.append(name)
    assert not bad, bad


def test_kink_filter_keeps_nine_candidates_in_ten():
    shares = {f"single S={S}": D.survivor_pool(S).rejected for S in (2, 8, 16)}
    shares.update({f"pairs S={S}": D.pair_pool(S, on_faces=64).rejected for S in (2, 16)})
    print(shares)
    assert all(0.0 < v <= 0.10 for v in shares.values()), shares
    _, net = D.synthetic_net()
    assert D.kink_margin(net, D.make_planes(16, D.AMP_BWD, 16), D.coords_family("beyond", 4, 16, np.random.RandomState(0))).min() > 10


# ------------------------------------------------------------------------------------------------ the split's range
SPLIT_TABLE = {0: (3.3e-7, 3.9e-4), 4: (4.4e-6, 1.3e-3), 8: (6.6e-5, 5.6e-2), 10: (2.5e-4, 0.39), 12: (1.1e-3, 1.3)}


def test_split_range_model():
    """The simulation behind the supported-scale statement in csrc/decode.hip and INTEGRATION.md: 4096 Fourier-feature vectors, the
    synthetic weights with W1, b1 -> s (W1, b1), W2 -> W2 / s, the hi/lo split in numpy's fp16 (subnormals kept, or lo parts below
    2^-14 flushed), float64 accumulation.  Each figure within a factor 3 of the recorded table; 2^16 overflows fp16."""
    sd, net = D.synthetic_net()
    ang = np.random.RandomState(31).uniform(-20, 20, (4096, 64))
    x1 = np.concatenate([np.sin(ang), np.cos(ang)], axis=1).astype(np.float32)
    want = D.mlp(net, x1.astype(np.float64))[4]
    for k, (kept, flushed) in SPLIT_TABLE.items():
        for sgn in ((1,) if k == 0 else (1, -1)):
            net_k = D.net64(D.scaled_state_dict(sd, sgn * k))
            ek = np.abs(D.split_model(net_k, x1) - want).max()
            ef = np.abs(D.split_model(net_k, x1, scale_mode="flush") - want).max()
            print(f"s = 2^{sgn * k:+d}: subnormals kept {ek:.2e}  fp16 subnormals flushed {ef:.2e}")
            assert kept / 3 < ek < kept * 3 and flushed / 3 < ef < flushed * 3, (k, sgn, ek, ef)
    assert not np.isfinite(D.split_model(D.net64(D.scaled_state_dict(sd, 16)), x1)).all()


# ------------------------------------------------------------------------------------------------ argument checks
def test_decoder_calls_refuse_bad_sizes_before_any_device_work():
    from ishapediting_amd import _lib
    L = _lib.lib()
    w = _lib.DecoderWeightsC(*([FAKE] * 7))
    err = lambda: L.ishap_last_error().decode()      # noqa: E731
    for S in (0, -3):
        assert L.ishap_triplane_decode_points(FAKE, S, C.byref(w), FAKE, 32, FAKE, None) == -2 and "plane size" in err()
        assert L.ishap_triplane_decode_grid(FAKE, S, C.byref(w), FAKE, 4, FAKE, None) == -2 and "plane size" in err()
        assert L.ishap_triplane_points_loss_grad(FAKE, S, C.byref(w), FAKE, FAKE, FAKE, FAKE, 32, FAKE, FAKE, FAKE, None) == -2
        assert "plane size" in err()
    for n in (0, -1):
        assert L.ishap_triplane_decode_points(FAKE, 16, C.byref(w), FAKE, n, FAKE, None) == -2 and "no points" in err()
        assert L.ishap_triplane_points_loss_grad(FAKE, 16, C.byref(w), FAKE, FAKE, FAKE, FAKE, n, FAKE, FAKE, FAKE, None) == -2
        assert "no points" in err()
    assert L.ishap_triplane_decode_grid(FAKE, 16, C.byref(w), FAKE, 0, FAKE, None) == -2
    for S in (0, 1):
        assert L.ishap_triplane_fit_loss_grad(FAKE, S, C.byref(w), FAKE, FAKE, FAKE, 32, FAKE, FAKE, 32, 0.3, FAKE, FAKE, None) == -2
        assert "plane size" in err()
    assert L.ishap_triplane_fit_loss_grad(FAKE, 16, C.byref(w), FAKE, FAKE, FAKE, 0, FAKE, FAKE, 0, 0.3, FAKE, FAKE, None) == -2
    for S in (10, 0, -8, 6):                         # S * S % 32 != 0 would leave pixels unwritten
        assert L.ishap_x0_grad_to_cotangent(FAKE, FAKE, FAKE, FAKE, 1.5, 0.5, 1, S, FAKE, FAKE, None) == -2, S
        assert "x0_grad_to_cotangent" in err() and "multiple of 32" in err()
        assert L.ishap_planes_prepare(FAKE, None, None, S, FAKE, None) == -2 and "planes_prepare" in err()
