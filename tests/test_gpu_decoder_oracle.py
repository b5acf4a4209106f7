"""The triplane decoder kernels (csrc/decode.hip, decode_bwd.hip, decode_fit.hip) through their ABI calls, one launch per case,
against the float64 statement of tests/decoder_ref.py: tail lanes and the `pt = npts - 1` stand-in, the second pass of both
grid-stride loops, grids whose size is no multiple of 32, a non-uniform axis, texel centres, borders, corners, the fade band and
far-away points, shared-texel atomics, saturated logits of both signs, empty batch / pair halves, the relative scale of the two
hidden layers, and the un-normalise / x0 bridge kernels with null and non-null range / middle and clip 0 / 1.

Bounds (derived in tests/decoder_ref.py, none tuned to what the device gives; tests/test_decoder_ref_host.py shows that they pass
the honest result and reject every listed mutation):
  logits     |dev - ref64| <= forward_bound per point (first order through the float64 network, SIN_ABS = 3e-6).
  gradients  per texel and channel |dev - ref64| <= 4 REL A + Aw + cnt u A + u |ref| + 4 u A1, REL measured on the CPU at test time.
  loss       |dev - ref64| <= 2^-20 (1 + sum |bce_i| / n).
Every output starts as a NaN bit pattern (accumulated outputs: as zeros or the stated start values) with 256 canary elements
behind it; afterwards everything inside is finite and no canary changed.  Both forward kernels, planes_prepare and x0_grad give
the same bits on a second call.

Measured on an MI355X (all 69 cases pass):
  forward     worst error / bound over all point and grid cases 0.047 (mixed-S128; 0.034 at planes 0.4 * randn, 0.014 at 65575
              points, 0.009 at res 41); max |dev - ref64| 3.6e-6 at 65575 points, 1.8e-5 at planes 0.4 * randn.  SIN_ABS = 3e-6
              held: no case comes near a bound built on it (the sin / cos term is 6 % of the bound, the kernel uses 1 - 5 % of
              the whole).
  scale sweep s: max |dev - ref64| / worst error over bound            CPU model of the split alone (test_split_range_model)
              2^-4   3.9e-6 / 0.011                                    4.5e-6
              2^-2   2.7e-6 / 0.011
              2^0    2.8e-6 / 0.013                                    3.3e-7
              2^+2   2.8e-6 / 0.012
              2^+4   3.7e-6 / 0.012                                    3.6e-6
              2^+8   5.6e-5 / 0.037   2^-8   6.6e-5 / 0.025            6.4e-5 / 6.2e-5      (not asserted)
              2^+12  1.1e-3 / 0.056   2^-12  9.2e-4 / 0.025            1.0e-3 / 1.1e-3      (not asserted)
              Inside 2^+-4 the device's error is its sin / cos and fp32 roundings, not the split; from 2^+-8 on the split's
              subnormal lo parts dominate and the device follows the model.  fp16 subnormals survive conversion and MFMA.
  REL (CPU, per backward case) and the device's worst error / bound
              points_loss_grad  n1 2.2e-3 / 0.08   n33 1.6e-2 / 0.17   n1024 1.8e-5 / 0.27   n8229 1.2e-7 / 0.06
                                shared 2.3e-4 / 0.25   border 8.6e-5 / 0.34   sat50 gt0 1.4e-2 / 0.06, gt1 1.9e-2 / 0.18,
                                mixed 1.4e-2 / 0.06   sat100 gt0 9.0e-3 / 0.23, gt1 1.1e-2 / 0.13, mixed 9.0e-3 / 0.23
              fit_loss_grad     b0-r7 5.6e-4 / 0.89   b0-r64 8.4e-3 / 0.10   b5-r0 1.3e-4 / 0.17   b5-r7 5.6e-4 / 0.89
                                b5-r64 8.4e-3 / 0.10   b32-r0 1.5e-4 / 0.24   b32-r7 5.6e-4 / 0.90   b32-r64 8.4e-3 / 0.10
                                b877-r0 8.8e-4 / 0.19   b877-r7 7.5e-4 / 0.08   b877-r64 6.4e-4 / 0.07   S2-b32-r7 1.2e-7 / 0.09
                                S2-b877-r64 1.2e-7 / 0.005   pairw0 3.2e-4 / 0.12   start 8.4e-3 / 0.40
              (1.2e-7 = 2 u is REL's floor; the r7 cases' 0.89 sits on one element of the seven pairs whose z(r) - z(r + delta)
              nearly cancels.)  planes_prepare at most 0.5 of its bound.
  loss        points_loss_grad adds one float atomic per point: |dev - ref64| 7e-8 (n1), 5e-8 (n33), 3.5e-7 (n1024), 1.2e-6 (n8229)
              against 1.6e-6 -- a random walk of npts half-ulp roundings (predicted sigma 9e-7 at 8229 points, in an order that
              changes from run to run).  n8229 passes at 0.74 of the bound the issue sets; it is the one check here without
              a wide margin, and at the product's 40 000 points the same sum is good to about 3e-6.  fit_loss_grad (one atomic
              per wave) is within 9e-8 everywhere.
"""
import ctypes as C
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import decoder_ref as D

pytestmark = pytest.mark.gpu

NAN_BITS, CANARY_BITS, NCANARY = 0x7FC0BEEF, 0x5A5AA5A5, 256
U = D.U


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def guarded(n, start=None):
    """device float32 buffer of n elements (NaN bit pattern, or `start`) with NCANARY canary elements behind it"""
    host = torch.full((n + NCANARY,), NAN_BITS, dtype=torch.int32)
    if start is not None:
        host[:n] = torch.as_tensor(np.asarray(start, np.float32).reshape(-1)).view(torch.int32)
    host[n:] = CANARY_BITS
    return host.to(dev()).view(torch.float32)


def read(buf, n, tag):
    """the n elements inside, after checking that they are finite and that no canary changed"""
    host = buf.cpu()
    assert bool((host[n:].view(torch.int32) == CANARY_BITS).all()), f"{tag}: a canary changed"
    out = host[:n].numpy().copy()
    assert np.isfinite(out).all(), f"{tag}: {int((~np.isfinite(out)).sum())} element(s) not written or not finite"
    return out


def put(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).contiguous().to(dev())


class Weights:
    """the seven tensors on the device, the C struct, and the transposed copies points_loss_grad wants"""

    def __init__(self, sd):
        self.t = [put(np.asarray(sd[k], np.float32)) for k in D.NET_KEYS]
        self.c = L().DecoderWeightsC(*[t.data_ptr() for t in self.t])
        self.w1t, self.w2t = self.t[1].t().contiguous(), self.t[3].t().contiguous()


def L():
    from ishapediting_amd import _lib
    return _lib


def decode_points(w, planes_d, S, coords):
    """two calls of ishap_triplane_decode_points on fresh guarded buffers -> logits (asserted bitwise equal)"""
    n = len(coords)
    c_d = put(coords)
    outs = []
    for _ in range(2):
        out = guarded(n)
        L().check(L().lib().ishap_triplane_decode_points(planes_d.data_ptr(), S, C.byref(w.c), c_d.data_ptr(), n, out.data_ptr(),
                                                         L().stream_ptr(dev())))
        torch.cuda.synchronize()
        outs.append(read(out, n, "logits"))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "decode_points: a second call gave other bits"
    return outs[0]


def decode_grid(w, planes_d, S, axis):
    res = len(axis)
    a_d = put(axis)
    outs = []
    for _ in range(2):
        out = guarded(res ** 3)
        L().check(L().lib().ishap_triplane_decode_grid(planes_d.data_ptr(), S, C.byref(w.c), a_d.data_ptr(), res, out.data_ptr(),
                                                       L().stream_ptr(dev())))
        torch.cuda.synchronize()
        outs.append(read(out, res ** 3, "volume"))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "decode_grid: a second call gave other bits"
    return outs[0]


def check_forward(tag, got, net, planes, coords):
    fw = D.forward(net, planes, coords)
    fb = D.forward_bound(net, planes, fw)
    err = np.abs(got.astype(np.float64) - fw.logit)
    i = int(np.argmax(err / fb.bound))
    print(f"{tag}: n {len(coords)} max |dev - ref64| {err.max():.2e} bound median {np.median(fb.bound):.2e} "
          f"worst error / bound {err[i] / fb.bound[i]:.3f} at point {i} {coords[i]}")
    assert (err <= fb.bound).all(), (tag, i, err[i], fb.bound[i])
    return fw


# ------------------------------------------------------------------------------------------------ decode_points
def _uniform(n, seed):
    return np.random.RandomState(seed).uniform(-1.1, 1.1, (n, 3)).astype(np.float32)


POINT_CASES = [
    dict(name="n1", S=16, n=1, why="one point: 31 stand-in lanes read point npts - 1 = 0"),
    dict(name="n31", S=16, n=31, why="one tail lane"),
    dict(name="n32", S=16, n=32, why="exactly one tile"),
    dict(name="n33", S=16, n=33, why="a second tile with one valid lane, in a second wave"),
    dict(name="n2053", S=16, n=2048 + 5, why="many blocks and a 5-point tail"),
    dict(name="n65575", S=16, n=65536 + 32 + 7, why="second pass of the grid-stride loop (256 blocks x 8 waves x 32), with a tail"),
    dict(name="n2053-amp0.4", S=16, n=2048 + 5, amp=0.4, why="phases of tens of radians: the fract range reduction in turns"),
    dict(name="mixed-S2", S=2, mixed=41, why="one cell per plane; every family (tests/decoder_ref.coords_family)"),
    dict(name="mixed-S8", S=8, mixed=41, why="centres, faces, one ulp outside, fade band, beyond it, 1e6"),
    dict(name="mixed-S16", S=16, mixed=41, why="the same at the size the other cases use"),
    dict(name="mixed-S128", S=128, mixed=41, why="the product's plane size: texel coordinates up to 127"),
]


@lru_cache(maxsize=None)
def _point_case(name):
    c = next(c for c in POINT_CASES if c["name"] == name)
    S = c["S"]
    coords = D.mixed_coords(c["mixed"], S, 40 + S) if "mixed" in c else _uniform(c["n"], 50 + c["n"] % 97)
    return S, D.make_planes(S, c.get("amp", D.AMP_FWD), 30 + S), coords


@pytest.mark.parametrize("name", [c["name"] for c in POINT_CASES])
def test_decode_points_against_float64(name):
    sd, net = D.synthetic_net()
    S, planes, coords = _point_case(name)
    got = decode_points(Weights(sd), put(planes), S, coords)
    fw = check_forward(name, got, net, planes, coords)
    if "mixed" in name:
        n = len(coords) // len(D.FAMILIES)
        k = D.FAMILIES.index("beyond")
        assert np.ptp(fw.logit[k * n:(k + 1) * n]) < 1e-15            # beyond the fade band: the network's value at zero features
        assert len(np.unique(got[k * n:(k + 1) * n])) == 1


# ------------------------------------------------------------------------------------------------ decode_grid
GRID_CASES = [
    dict(name="res1", res=1, why="a single point, the axis given as [-1]"),
    dict(name="res5", res=5, why="125 points: 29 tail lanes, i/j/k of a small grid"),
    dict(name="res7", res=7, why="343 points: 23 tail lanes"),
    dict(name="res24", res=24, why="13824 = 432 tiles: no tail, many blocks"),
    dict(name="res41", res=41, why="68921 points: the second loop pass, a 25-point tail and the i/j/k decomposition in one case"),
    dict(name="res7-nonuniform", res=7, nonuniform=True, why="the kernel reads lin[]: it must not assume a linspace"),
]


@pytest.mark.parametrize("name", [c["name"] for c in GRID_CASES])
def test_decode_grid_against_float64_and_decode_points(name):
    c = next(c for c in GRID_CASES if c["name"] == name)
    sd, net = D.synthetic_net()
    S, res = 16, c["res"]
    planes = D.make_planes(S, D.AMP_FWD, 30 + S)
    if c.get("nonuniform"):
        axis = np.sort(np.random.RandomState(60).uniform(-1.1, 1.1, res)).astype(np.float32)
    else:
        axis = torch.linspace(-1, 1, res).numpy()                     # what decode_planes_grid hands the kernel; res = 1: [-1]
    assert axis[0] == -1.0 or c.get("nonuniform")
    w, planes_d = Weights(sd), put(planes)
    vol = decode_grid(w, planes_d, S, axis)
    coords = D.grid_coords(axis)
    check_forward(name, vol, net, planes, coords)
    pts = decode_points(w, planes_d, S, coords)
    assert np.array_equal(vol.view(np.uint32), pts.view(np.uint32)), "grid path and points path differ"


# ------------------------------------------------------------------------------------------------ scale of the two layers
@pytest.mark.parametrize("k", [-4, -2, 0, 2, 4])
def test_scale_invariance_inside_the_supported_range(k):
    """W1, b1 -> 2^k (W1, b1), W2 -> W2 / 2^k: the same function; the bound (whose subnormal term follows the weights) must hold."""
    sd, _ = D.synthetic_net()
    sd_k = D.scaled_state_dict(sd, k)
    S, planes, coords = _point_case("n2053")
    got = decode_points(Weights(sd_k), put(planes), S, coords)
    check_forward(f"s=2^{k:+d}", got, D.net64(sd_k), planes, coords)


def test_scale_sweep_beyond_the_supported_range_is_reported():
    """2^+-8 and 2^+-12: beyond what the kernel can claim (fp16 lo parts, then hi parts, sink into the subnormals; 2^16 overflows
    fp16 and is not run).  Printed, not asserted: the measured row goes next to the CPU model's in the module docstring."""
    sd, _ = D.synthetic_net()
    S, planes, coords = _point_case("n2053")
    planes_d = put(planes)
    for k in (8, -8, 12, -12):
        sd_k = D.scaled_state_dict(sd, k)
        got = decode_points(Weights(sd_k), planes_d, S, coords)
        net_k = D.net64(sd_k)
        fw = D.forward(net_k, planes, coords)
        fb = D.forward_bound(net_k, planes, fw)
        err = np.abs(got - fw.logit)
        print(f"s=2^{k:+d}: max |dev - ref64| {err.max():.2e} bound median {np.median(fb.bound):.2e} worst error / bound {(err / fb.bound).max():.3f}")


def test_zero_planes_and_zero_biases():
    """All-zero planes with b1 = b2 = 0.  With W1's cos block zeroed as well every pre-activation is exactly 0 (sin 0 = 0 exactly,
    cos 0 = 1 meets zero weights), every ReLU sits at 0 and the logit is b3 exactly; with the cos block in place the point is an
    ordinary one and the float64 bound applies."""
    sd, _ = D.synthetic_net()
    S, _, coords = _point_case("n33")
    planes = np.zeros((3, S, S, 32), np.float32)
    sd0 = {k: np.array(v, np.float32) for k, v in sd.items()}
    sd0["1.bias"][:] = 0
    sd0["3.bias"][:] = 0
    got = decode_points(Weights(sd0), put(planes), S, coords)
    check_forward("zero planes", got, D.net64(sd0), planes, coords)
    sd0["1.weight"][:, 64:] = 0
    got = decode_points(Weights(sd0), put(planes), S, coords)
    assert np.array_equal(got, np.full(len(coords), sd0["5.bias"].reshape(-1)[0], np.float32))


# ------------------------------------------------------------------------------------------------ points_loss_grad
def _w3_scaled(sd, net, planes, coords, target):
    """w3 scaled and b3 shifted so that the logits of these points span [-target, +target]: z' = f (z - (max z + min z) / 2).
    (Scaling alone reaches one sign: the synthetic logits of a case lie in about [-0.6, 0.1].)"""
    z = D.forward(net, planes, coords).logit
    f = 2.0 * target / (z.max() - z.min())
    out = dict(sd)
    out["5.weight"] = (sd["5.weight"] * np.float32(f)).astype(np.float32)
    out["5.bias"] = np.full_like(sd["5.bias"], f * (net.b3 - 0.5 * (z.max() + z.min())))
    return out


LOSS_CASES = [
    dict(name="n1", S=16, n=1, why="one block, one point"),
    dict(name="n33", S=8, n=33, why="33 blocks; 1 / npts with npts no multiple of the forward's tile"),
    dict(name="n1024", S=16, n=1024, why="the size the existing norm test uses, now per texel"),
    dict(name="n8229", S=8, n=8192 + 37, why="blocks capped at 8192: 37 blocks take a second point"),
    dict(name="shared", S=16, kind="shared", why="512 points at one interior coordinate + 512 spread out: atomics into 4 texels per plane"),
    dict(name="border", S=8, kind="border", why="coordinates exactly +-1 on one, two, three axes: border row / column / corner; the out-of-range taps get nothing"),
    dict(name="allout", S=16, kind="allout", why="every tap out of range: dplanes entirely zero, loss finite"),
] + [dict(name=f"sat{t}-gt{g}", S=8, n=33, sat=t, gt=g, why=f"logits spanning -{t} .. +{t}, gt {g}: expf(-z) overflowing to +inf for z < -88 and "
          "underflowing for z > 88, bce = z through fmaxf(z, 0), sigmoid - gt cancelling to 0 or saturating at +-1, "
          "log1pf(expf(-|z|)) underflowing") for t in (50, 100) for g in ("0", "1", "mixed")]


@lru_cache(maxsize=None)
def _loss_case(name):
    c = next(c for c in LOSS_CASES if c["name"] == name)
    sd, net = D.synthetic_net()
    S = c["S"]
    pool = D.survivor_pool(S)
    assert pool.rejected <= 0.10, pool.rejected                       # the filter cannot hollow a case out
    planes, kind = pool.planes, c.get("kind")
    if kind == "shared":
        coords = np.concatenate([np.repeat(pool.coords[:1], 512, 0), pool.coords[1:513]])
    elif kind == "border":
        coords = D.filtered(net, planes, D.coords_family("faces", 200, S, np.random.RandomState(70)))
        assert len(coords) > 150 and sum((np.abs(coords) == 1).sum(axis=1) == 3) > 5
    elif kind == "allout":
        coords = D.coords_family("beyond", 64, S, np.random.RandomState(71))
    else:
        coords = np.resize(pool.coords, (c["n"], 3))                    # n8229: every survivor up to eight times
    n = len(coords)
    gt = {"0": np.zeros(n), "1": np.ones(n)}.get(c.get("gt"), (np.random.RandomState(72).rand(n) < 0.5) * 1.0).astype(np.float32)
    if "sat" in c:
        sd = _w3_scaled(sd, net, planes, coords, c["sat"])
        net = D.net64(sd)
        z = D.forward(net, planes, coords).logit
        assert z.min() <= -0.9 * c["sat"] and z.max() >= 0.9 * c["sat"], (z.min(), z.max())      # both signs saturate
        if c["gt"] == "mixed":                                                                  # both targets at both ends
            gt[np.argsort(z)[[0, 1, -2, -1]]] = [0, 1, 0, 1]
    ref = D.points_loss_grad(net, planes, coords, gt)
    g32 = [D.points_loss_grad(D.permuted_net(net, s), planes, coords, gt, dtype=torch.float32).dplanes for s in range(D.REL_RUNS)]
    rel = D.measured_rel(g32, ref) if (ref.A > 0).any() else 0.0
    return SimpleNamespace(sd=sd, net=net, S=S, planes=planes, coords=coords, gt=gt, ref=ref, rel=rel)


def check_gradient(tag, got, ref, rel, extra=0.0):
    bound = D.backward_bound(ref, rel) + extra
    err = np.abs(got.astype(np.float64) - ref.dplanes)
    m = ref.A > 0
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    print(f"{tag}: REL {rel:.2e} touched elements {int(m.sum())} max |dev - ref64| {err.max():.2e} max |ref64| {np.abs(ref.dplanes).max():.2e} "
          f"worst error / bound {ratio[i]:.3f} at {i}")
    assert (err <= bound).all(), (tag, i, err[i], bound[i])


@pytest.mark.parametrize("name", [c["name"] for c in LOSS_CASES])
def test_points_loss_grad_against_float64(name):
    c = _loss_case(name)
    n, S = len(c.coords), c.S
    w = Weights(c.sd)
    planes_d, coords_d, gt_d = put(c.planes), put(c.coords), put(c.gt)
    dpl, loss, logits = guarded(c.planes.size), guarded(1), guarded(n)
    L().check(L().lib().ishap_triplane_points_loss_grad(planes_d.data_ptr(), S, C.byref(w.c), w.w1t.data_ptr(), w.w2t.data_ptr(),
                                                        coords_d.data_ptr(), gt_d.data_ptr(), n, dpl.data_ptr(), loss.data_ptr(),
                                                        logits.data_ptr(), L().stream_ptr(dev())))
    torch.cuda.synchronize()
    got = read(dpl, c.planes.size, "dplanes").reshape(c.planes.shape)
    got_loss, got_logits = float(read(loss, 1, "loss")[0]), read(logits, n, "logits")
    check_forward(name, got_logits, c.net, c.planes, c.coords)
    lb = 2.0 ** -20 * (1 + c.ref.bce_abs_mean)
    print(f"{name}: loss64 {c.ref.loss:.6e} |dev - 64| {abs(got_loss - c.ref.loss):.2e} bound {lb:.2e}; max |logit| {np.abs(c.ref.logits).max():.1f}")
    assert abs(got_loss - c.ref.loss) <= lb, (name, got_loss, c.ref.loss, lb)
    untouched = ~D.touched_texels(c.coords, S).reshape(3, S, S)
    assert (got[untouched] == 0.0).all(), f"{name}: {int((got[untouched] != 0).sum())} element(s) no tap reaches are not 0.0"
    if name == "allout":
        assert (got == 0.0).all() and untouched.all()
        return
    check_gradient(name, got, c.ref, c.rel)


# ------------------------------------------------------------------------------------------------ fit_loss_grad
FIT_CASES = [dict(name=f"b{b}-r{r}", S=16, nbatch=b, nrand=r, why="partial tiles of both kinds; an empty half launches no item of it")
             for b in (0, 5, 32, 1000 - 123) for r in (0, 7, 64) if b + r > 0] + [
    dict(name="S2-b32-r7", S=2, nbatch=32, nrand=7, why="the smallest plane the call accepts: every point in the one cell"),
    dict(name="S2-b877-r64", S=2, nbatch=877, nrand=64, why="4 texels per plane take every atomic"),
    dict(name="pairw0", S=16, nbatch=32, nrand=64, pair_w=0.0, why="pair_w = 0: the pairs give a mse and no gradient"),
    dict(name="start", S=16, nbatch=32, nrand=64, start=True, why="dplanes and loss_parts start non-zero: the call adds"),
]


@lru_cache(maxsize=None)
def _fit_case(name):
    c = next(c for c in FIT_CASES if c["name"] == name)
    sd, net = D.synthetic_net()
    S = c["S"]
    pool, pairs = D.survivor_pool(S), D.pair_pool(S, on_faces=64)
    assert pool.rejected <= 0.10 and pairs.rejected <= 0.10, (pool.rejected, pairs.rejected)
    rs = np.random.RandomState(80 + c["nbatch"] + c["nrand"])
    coords = pool.coords[:300]
    gt = (rs.rand(300) < 0.5).astype(np.float32)
    idx = rs.randint(0, 300, c["nbatch"]).astype(np.int32)              # out of order
    if len(idx) > 1:
        idx[-1] = idx[0]                                                # and with a repeat
    r, noise = pairs.r[:c["nrand"]], pairs.noise[:c["nrand"]]
    if c["nrand"] == 64:
        assert (np.abs(D.partner(r, noise)) > 1).any(axis=1).sum() >= 5  # partners leaving the cube
    pair_w = c.get("pair_w", 0.3)
    args = (pool.planes, coords, gt, idx, r, noise, pair_w)
    ref = D.fit_loss_grad(net, *args)
    r32 = [D.fit_loss_grad(D.permuted_net(net, s), *args, dtype=torch.float32) for s in range(D.REL_RUNS)]
    rel = D.measured_rel([x.dplanes for x in r32], ref) if (ref.A > 0).any() else 0.0
    mse_spread = max(abs(x.parts[1] - ref.parts[1]) for x in r32)
    return SimpleNamespace(sd=sd, net=net, S=S, planes=pool.planes, coords=coords, gt=gt, idx=idx, r=r, noise=noise, pair_w=pair_w,
                           ref=ref, rel=rel, mse_spread=mse_spread, start=c.get("start", False))


@pytest.mark.parametrize("name", [c["name"] for c in FIT_CASES])
def test_fit_loss_grad_against_float64(name):
    """loss_parts: bce within 2^-20 (1 + bce) (its terms are positive); mse within 4 x the spread of the fp32 autograd runs +
    2^-20 mse (z(r) - z(r + delta) cancels: the same argument as the gradient's REL)."""
    c = _fit_case(name)
    S, nb, nr = c.S, len(c.idx), len(c.r)
    w = Weights(c.sd)
    rs = np.random.RandomState(90)
    start_g = (rs.randn(*c.planes.shape) * 1e-3).astype(np.float32) if c.start else np.zeros_like(c.planes)
    start_l = np.array([1.5, -2.25], np.float32) if c.start else np.zeros(2, np.float32)
    planes_d, coords_d, gt_d, idx_d = put(c.planes), put(c.coords), put(c.gt), put(c.idx, torch.int32)
    r_d, noise_d = put(c.r.reshape(-1, 3)), put(c.noise.reshape(-1, 3))
    dpl, parts = guarded(c.planes.size, start_g), guarded(2, start_l)
    L().check(L().lib().ishap_triplane_fit_loss_grad(planes_d.data_ptr(), S, C.byref(w.c), coords_d.data_ptr(), gt_d.data_ptr(),
                                                     idx_d.data_ptr(), nb, r_d.data_ptr(), noise_d.data_ptr(), nr, c.pair_w,
                                                     dpl.data_ptr(), parts.data_ptr(), L().stream_ptr(dev())))
    torch.cuda.synchronize()
    got = read(dpl, c.planes.size, "dplanes").reshape(c.planes.shape).astype(np.float64) - start_g
    got_parts = read(parts, 2, "loss_parts").astype(np.float64) - start_l
    bce, mse = c.ref.parts
    b_bce = 2.0 ** -20 * (1 + bce) + 2 * U * abs(float(start_l[0]))
    b_mse = 4 * c.mse_spread + 2.0 ** -20 * mse + 2 * U * abs(float(start_l[1]))
    print(f"{name}: bce64 {bce:.6e} |dev - 64| {abs(got_parts[0] - bce):.2e} bound {b_bce:.2e}; mse64 {mse:.6e} |dev - 64| "
          f"{abs(got_parts[1] - mse):.2e} bound {b_mse:.2e}")
    assert abs(got_parts[0] - bce) <= b_bce and abs(got_parts[1] - mse) <= b_mse
    if nb == 0:
        assert got_parts[0] == 0.0
    if nr == 0:
        assert got_parts[1] == 0.0
    # a non-zero start: every atomic add then rounds a value no larger than |start| + A, and so does taking the start off again
    extra = (c.ref.cnt + 1) * U * np.abs(start_g) + U * c.ref.A if c.start else 0.0
    if not c.start:
        allc = np.concatenate([c.coords[c.idx], c.r.reshape(-1, 3), D.partner(c.r, c.noise).reshape(-1, 3)])
        untouched = ~D.touched_texels(allc, S).reshape(3, S, S)
        assert (got[untouched] == 0.0).all()
    check_gradient(name, got, c.ref, c.rel, extra)


# ------------------------------------------------------------------------------------------------ planes_prepare, x0_grad
PREPARE_CASES = [
    dict(name="S8-none", S=8, form="none", why="two 32-pixel tiles per plane; range and middle null: the r = 1, m = 0 branch (what "
         "MultiTriplane._planes passes), a pure transpose, bit for bit"),
    dict(name="S16-none", S=16, form="none", why="null range / middle at the size the other cases use"),
    dict(name="S128-none", S=128, form="none", why="null range / middle at the product's size: 512 tiles per plane"),
    dict(name="S8-range", S=8, form="range", why="range given, middle null"),
    dict(name="S16-middle", S=16, form="middle", why="range null, middle given"),
    dict(name="S8-both", S=8, form="both", why="both given at the smallest size"),
    dict(name="S16-both", S=16, form="both", why="both given"),
    dict(name="S128-both", S=128, form="both", why="both given at the product's size (prepare_planes with a checkpoint's statistics)"),
]


@pytest.mark.parametrize("name", [c["name"] for c in PREPARE_CASES])
def test_planes_prepare_against_float64(name):
    """latent * range + middle, one multiply-add per element: |dev - ref64| <= 2^-23 |result| + 2^-24 |latent range| (the result's
    rounding, and the product's when the multiply-add is not fused), which is inside rtol 1e-6 of the result wherever
    |latent range| <= 14 |result|; asserted as rtol 1e-6 on those elements as well.  No fp32 multiply-add can promise rtol 1e-6
    where the two terms cancel further than that."""
    c = next(c for c in PREPARE_CASES if c["name"] == name)
    S, form = c["S"], c["form"]
    rs = np.random.RandomState(100 + S)
    lat = rs.randn(96, S, S).astype(np.float32)
    rng = (rs.rand(96) + 0.5).astype(np.float32) if form in ("range", "both") else None
    mid = (rs.randn(96) * 0.3).astype(np.float32) if form in ("middle", "both") else None
    lat_d = put(lat)
    rng_d, mid_d = (None if v is None else put(v) for v in (rng, mid))
    outs = []
    for _ in range(2):
        out = guarded(lat.size)
        L().check(L().lib().ishap_planes_prepare(lat_d.data_ptr(), L().ptr(rng_d), L().ptr(mid_d), S, out.data_ptr(),
                                                 L().stream_ptr(dev())))
        torch.cuda.synchronize()
        outs.append(read(out, lat.size, "planes"))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    want, prod = D.planes_prepare(lat, rng, mid)
    err = np.abs(outs[0].reshape(3, S, S, 32) - want)
    bound = 2.0 ** -23 * np.abs(want) + 2.0 ** -24 * prod
    plain = prod <= 14 * np.abs(want)
    print(f"planes_prepare {name}: max error / bound {(err / (bound + 1e-300)).max():.3f}; max error / |result| where nothing "
          f"cancels {(err[plain] / np.abs(want[plain])).max():.2e} ({int((~plain).sum())} cancelling elements)")
    assert (err <= bound).all()
    assert plain.mean() > 0.9 and (err[plain] <= 1e-6 * np.abs(want[plain])).all()
    if form == "none":
        assert np.array_equal(outs[0].reshape(3, S, S, 32), want.astype(np.float32))


def _edge_inputs(S, rs):
    """x, eps [96 / 192, S, S] for sr = 2, srm1 = 0.5 (every product exact, so a fused and an unfused multiply-add agree):
    sr x - srm1 eps exactly -1, +1 and one ulp either side of each in the first eight pixels of every channel; elsewhere values
    with 12-bit mantissas, none within 2^-10 of the clamp's edges."""
    x = np.round(rs.randn(96, S, S) * 0.5 * 1024) / 1024
    eps = np.round(rs.randn(192, S, S) * 1024) / 1024
    x0u = 2 * x - 0.5 * eps[:96]
    x = np.where(np.abs(np.abs(x0u) - 1) < 2.0 ** -10, 0.0, x)
    eps[:96] = np.where(np.abs(np.abs(2 * x - 0.5 * eps[:96]) - 1) < 2.0 ** -10, 0.0, eps[:96])
    edge = np.array([0.5, -0.5, 0.5 + 2.0 ** -24, 0.5 - 2.0 ** -25, -0.5 - 2.0 ** -24, -0.5 + 2.0 ** -25, 1.0, -1.0])
    x[:, 0, :8] = edge
    eps[:96, 0, :8] = np.array([0, 0, 0, 0, 0, 0, 2.0, -2.0])
    x, eps = x.astype(np.float32), eps.astype(np.float32)
    assert np.array_equal(x[:, 0, :8].astype(np.float64), np.broadcast_to(edge, (96, 8)))
    return x, eps


X0_CASES = [dict(name=f"S{S}-clip{clip}-{'range' if wr else 'norange'}", S=S, clip=clip, with_range=wr, why=why)
            for S, clip, wr, why in [
    (8, 1, True, "the guided step's form (clip 1, range given) at two tiles per plane; the clamp's edges block one ulp outside only"),
    (8, 0, True, "clip = 0: nothing is blocked, also at and beyond the edges"),
    (8, 1, False, "range null: the factor 1 branch, with the clamp"),
    (8, 0, False, "range null and clip = 0: g_direct = sr dplanes, cot = -srm1 dplanes, transposed"),
    (16, 1, True, "the size the existing autograd test uses, now with the edge values"),
    (16, 0, False, "both branches off at S = 16"),
    (128, 1, True, "the product's size: 512 tiles per plane, the variance half 96 * 128 * 128 elements further on"),
    (128, 0, True, "clip = 0 at the product's size"),
    (128, 1, False, "range null at the product's size"),
]]


@pytest.mark.parametrize("name", [c["name"] for c in X0_CASES])
def test_x0_grad_against_float64(name):
    """The clamp's edges: torch's clamp passes the gradient at equality and the kernel's strict < / > must agree; one ulp outside is
    blocked, one ulp inside passes.  g_direct and the eps half of cot_out at rtol 1e-6 (one product each); the variance half is 0.0."""
    c = next(c for c in X0_CASES if c["name"] == name)
    S, clip, with_range = c["S"], c["clip"], c["with_range"]
    rs = np.random.RandomState(110 + S)
    x, eps = _edge_inputs(S, rs)
    sr, srm1 = 2.0, 0.5
    rng = (rs.rand(96) + 0.5).astype(np.float32) if with_range else None
    dpl = rs.randn(3, S, S, 32).astype(np.float32)
    g_want, cot_want, margin = D.x0_grad(dpl, rng, x, eps, sr, srm1, clip)
    assert (margin[:, 0, :8] == np.array([0, 0, 2.0 ** -23, -2.0 ** -24, 2.0 ** -23, -2.0 ** -24, 0, 0])).all()
    dpl_d, x_d, eps_d = put(dpl), put(x), put(eps)
    rng_d = None if rng is None else put(rng)
    outs = []
    for _ in range(2):
        g, cot = guarded(96 * S * S), guarded(192 * S * S)
        L().check(L().lib().ishap_x0_grad_to_cotangent(dpl_d.data_ptr(), L().ptr(rng_d), x_d.data_ptr(), eps_d.data_ptr(), sr, srm1,
                                                       clip, S, g.data_ptr(), cot.data_ptr(), L().stream_ptr(dev())))
        torch.cuda.synchronize()
        outs.append((read(g, 96 * S * S, "g_direct"), read(cot, 192 * S * S, "cot_out")))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(*outs))
    g_got, cot_got = outs[0][0].reshape(96, S, S), outs[0][1].reshape(192, S, S)
    assert (np.abs(g_got - g_want) <= 1e-6 * np.abs(g_want)).all()
    assert (np.abs(cot_got[:96] - cot_want[:96]) <= 1e-6 * np.abs(cot_want[:96])).all()
    assert (cot_got[96:] == 0.0).all()
    blocked = g_want[:, 0, :8] == 0
    assert np.array_equal(blocked.all(axis=0), np.array([0, 0, 1, 0, 1, 0, 0, 0], bool) & bool(clip))
    assert np.array_equal(g_got[:, 0, :8] == 0, blocked)
