"""tests/field_ref.py held to what the project already trusts, on the CPU: torch autograd of the decoder statement, a central
difference of decoder_ref's forward, and a list of mutations the gradient bound has to reject."""
import ctypes as C
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import decoder_ref as D
from tests import field_ref as F

H = 1e-6                      # central-difference step
CASES = ((2, 265), (8, 265), (128, 265))


@lru_cache(maxsize=None)
def case(S, n):
    _, net = D.synthetic_net()
    planes = D.make_planes(S, D.AMP_BWD, S)
    coords = D.coords_family("uniform", n, S, np.random.RandomState(5))
    keep = F.gradient_filter(net, planes, coords)
    ref = F.field_grad(net, planes, coords)
    return SimpleNamespace(net=net, planes=planes, coords=coords, keep=keep, ref=ref, S=S)


@pytest.mark.parametrize("S,n", CASES)
def test_field_grad_is_autograd_of_the_statement(S, n):
    """1e-12 relative to the largest component, on EVERY point (float64 against float64: no filter is needed); the torch twin
    that is differentiated gives decoder_ref._decode_t's logits."""
    c = case(S, n)
    z, g = F.autograd_grad(c.net, c.planes, c.coords)
    P = torch.as_tensor(c.planes.reshape(-1, 32).astype(np.float64))
    zt = D._decode_t(D._net_t(c.net, torch.float64), P, c.coords, S, torch.float64, []).numpy()
    assert np.abs(z - zt).max() <= 1e-12 * max(1.0, np.abs(zt).max())
    assert np.abs(z - c.ref.logit).max() <= 1e-12 * max(1.0, np.abs(zt).max())
    assert np.abs(g - c.ref.grad).max() <= 1e-12 * np.abs(g).max()
    assert np.abs(g).max() > 0


@pytest.mark.parametrize("S,n", CASES)
def test_field_grad_matches_a_central_difference(S, n):
    """cd = (z(x + h) - z(x - h)) / 2h at h = 1e-6 on the filtered points, per axis, against
        4 |z(x + h) - 2 z(x) + z(x - h)| / 2h  +  512 * 2^-53 * (sum |w3| |h2| + |b3|) / h.
    The first term is the float64 network's own second difference: where the field is smooth it is h |z''| / 2, far above the
    difference quotient's h^2 |z'''| / 6; where a ReLU kink or a cell boundary lies inside the stencil it is EXACTLY the
    quotient's error (a kink of slope jump J at distance a < h gives cd - z' = J (h - a) / 2h and a second difference of
    J (h - a)); 4 is the margin.  The second term is the evaluation noise of two float64 logits (the longest chain of sums
    behind a logit is 32 + 128 + 128 + 128 terms: under 512 roundings of a number no larger than sum |w3| |h2| + |b3|), divided
    by 2h, twice.  Measured here: largest |cd - grad| 4.6e-10 (S = 2), 6.8e-10 (S = 8), 3.6e-7 (S = 128); largest error / bound
    0.0024, 0.0010, 0.29; median bound 3.3e-7, 1.1e-5, 3.1e-3 at median |grad| 0.1, 0.75, 12."""
    c = case(S, n)
    x = c.coords[c.keep].astype(np.float64)
    ref = F.field_grad(c.net, c.planes, c.coords[c.keep])
    assert len(x) > 0.8 * n
    noise = 512 * 2.0 ** -53 * (np.abs(ref.fw.h2) @ np.abs(c.net.w3) + abs(c.net.b3)) / H
    for a in range(3):
        e = np.zeros(3)
        e[a] = H
        zp, zm = F.forward_at(c.net, c.planes, x + e).logit, F.forward_at(c.net, c.planes, x - e).logit
        cd = (zp - zm) / (2 * H)
        bound = 4 * np.abs(zp - 2 * ref.logit + zm) / (2 * H) + noise
        err = np.abs(cd - ref.grad[:, a])
        print(f"S {S} axis {a}: max |cd - grad| {err.max():.2e}, max err / bound {(err / bound).max():.3f}, median bound {np.median(bound):.2e}")
        assert (err <= bound).all()


@pytest.mark.parametrize("S,n", CASES)
def test_bound_passes_fp32_and_rejects_mutations(S, n):
    c = case(S, n)
    rel = F.measured_rel(c.net, c.planes, c.coords, c.ref, c.keep)
    bound = F.grad_bound(c.ref, rel)
    m = c.keep[:, None] & np.ones(3, bool)[None, :]
    # the honest fp32 result: autograd in float32 in an order REL was not measured on
    _, g32 = F.autograd_grad(D.permuted_net(c.net, D.REL_RUNS + 3), c.planes, c.coords, torch.float32)
    ratio = (np.abs(g32 - c.ref.grad)[m] / np.maximum(bound[m], 1e-300)) * (bound[m] > 0)
    assert (np.abs(g32 - c.ref.grad)[m] <= bound[m]).all(), ratio.max()
    print(f"S {S}: REL {rel:.2e}, honest fp32 worst error / bound {ratio.max():.3f}, kept {c.keep.mean():.3f}")
    for name in F.MUTATIONS:
        mu = F.field_grad(c.net, c.planes, c.coords, mutation=name)
        over = (np.abs(mu.grad - c.ref.grad)[m] / np.maximum(bound[m], 1e-300)).max()
        print(f"  {name}: rejected by a factor of {over:.0f}")
        assert over > 10, name


def test_filter_keeps_enough_of_the_uniform_cases():
    """the condition tests/test_gpu_field.py asserts, on the CPU: at most 15 % of the uniform points are left out"""
    for S, n in CASES:
        assert case(S, n).keep.mean() >= 0.85


def test_float64_projection_is_monotone_and_bounded():
    _, net = D.synthetic_net()
    planes = D.make_planes(8, D.AMP_FWD, 8)
    pts = F.sign_change_points(net, planes, 32, 400, 0)
    voxel = 2.0 / 31
    prev = None
    for it in (0, 1, 4):
        r = F.project(net, planes, pts, it, 0.5 * voxel, voxel, 1e-4, 1e-12)
        assert (np.abs(r.z) <= np.abs(r.z_start)).all()
        assert (np.sqrt(((r.x - pts) ** 2).sum(1)) <= voxel * (1 + 1e-12)).all()
        assert (r.accepted <= it).all() and (r.accepted >= 0).all()
        nn = np.sqrt((r.normal ** 2).sum(1))
        assert (np.abs(nn - 1) < 1e-12).all()
        if prev is not None:
            assert (np.abs(r.z) <= np.abs(prev) + 0).all()          # more iterations never end further from the level set
        prev = r.z
    assert np.array_equal(F.project(net, planes, pts, 0, 0.5 * voxel, voxel, 1e-4, 1e-12).x, pts.astype(np.float64))
    assert np.abs(prev).mean() < 0.1 * np.abs(r.z_start).mean()


def test_normal_bound_covers_a_perturbed_gradient():
    rs = np.random.RandomState(3)
    g = rs.randn(500, 3) * np.exp(rs.randn(500, 1))
    b = np.abs(g) * 10.0 ** rs.uniform(-6, -1.5, (500, 3))
    for _ in range(8):
        dg = b * rs.uniform(-1, 1, b.shape)
        assert (np.abs(F.normal_of(g + dg) - F.normal_of(g)) <= F.normal_bound(g, b)).all()


# ----------------------------------------------------------------------------------------------------------- ABI, no GPU needed
FAKE = C.c_void_p(0x1000)


def test_abi_exports_and_refusals():
    from ishapediting_amd import _lib
    L = _lib.lib()
    assert L.ishap_version() >= 18
    w = _lib.DecoderWeightsC(*([0x1000] * 7))
    bw = C.byref(w)
    assert L.ishap_triplane_field_grad(FAKE, 1, bw, FAKE, 32, FAKE, FAKE, None) == -2          # S < 2
    assert L.ishap_triplane_field_grad(FAKE, 8, bw, FAKE, 0, FAKE, FAKE, None) == -2           # no points
    for k in (0, 3, 5, 6):                                                                     # a null pointer
        a = [FAKE, 8, bw, FAKE, 32, FAKE, FAKE, None]
        a[k] = None
        assert L.ishap_triplane_field_grad(*a) == -2
    assert L.ishap_triplane_field_grad(FAKE, 8, C.byref(_lib.DecoderWeightsC(*([0x1000] * 6 + [None]))), FAKE, 32, FAKE, FAKE, None) == -2
    good = [FAKE, 8, bw, FAKE, 32, 4, 0.01, 0.02, 1e-4, 1e-12, FAKE, FAKE, FAKE, FAKE, None]
    for k, v in ((1, 1), (4, 0), (5, -1), (5, 65), (6, 0.0), (9, 0.0), (7, -1.0), (8, -1.0), (0, None), (3, None), (10, None), (11, None),
                 (12, None), (13, None)):
        a = list(good)
        a[k] = v
        assert L.ishap_triplane_project(*a) == -2, (k, v)
    assert b"requirement failed" in L.ishap_last_error()
