"""The triplane decoder (csrc/decode.hip, decode_bwd.hip, decode_fit.hip on decode_mlp.h) restated in float64 on the kernels' fp32 inputs, with
the per-element error bounds the GPU oracle (tests/test_gpu_decoder_oracle.py) holds the kernels to.  Held to what the project
already trusts (oracle/ref_cpu.py, golden g6_decoder, tests/triplane_opt_ref.py) by tests/test_decoder_ref_host.py.

The statement (MultiTriplane.forward, axisnetworks.py:537-562)
  planes [3][S][S][32] channels-last (xy, yz, xz; the FIRST coordinate of a pair indexes W), bilinear, align_corners=True,
  zero padding:  ix = (u + 1) / 2 * (S - 1), taps (floor ix, floor ix + 1) x (floor iy, floor iy + 1), out-of-range taps give 0;
  f = sum of the three samples;  y = f @ B;  ang = float32(2 pi) * y;  x1 = [sin ang | cos ang];
  h1 = relu(W1 x1 + b1);  h2 = relu(W2 h1 + b2);  logit = w3 . h2 + b3.
  Dense grid: point index ((i * res) + j) * res + k -> (axis[i], axis[j], axis[k]), x slowest.
  points_loss_grad: loss = -mean BCEWithLogits(logit, gt), d loss / d planes.
  fit_loss_grad:    {mean BCEWithLogits on coords[idx], mean (z(r) - z(r + 0.01 noise))^2}, d (bce + pair_w mse) / d planes; the
                    partner coordinate is formed in fp32 (noise * 0.01f, then the add) as the reference does.

Forward bound (u = 2^-24, the fp32 unit roundoff).  First order: every local error is carried to the logit by the absolute value
of the float64 network's own derivative d logit / d (that quantity), so that signs cancel inside a matrix product exactly as
they do in the network, and the local errors are then summed in absolute value.  (An interval through sum |W| is about 2e-3
at the synthetic weights and would pass a kernel that drops the lo terms.)  The local errors:
  texel coordinate   ix = fl(fl(u + 1) / 2 * (S - 1)): two roundings of a number of size |ix| -> d_ix = 2 u |ix|; ix - floor ix and
                     (floor ix + 1) - ix are exact.  One rounded value per coordinate x, y, z (the two planes that sample a
                     coordinate compute the same ix), carried by d logit / d ix = the bilinear slopes of the float64 cell through
                     the network.  Within d_ix of a cell boundary (texel centres) the fp32 point may sit in the neighbouring
                     cell; there the slope is replaced by twice the largest |texel| of the 4 x 4 neighbourhood, per channel.
  features           product of the two axis weights, weight * texel, four adds per plane: 5 u sum_q |w_q| |texel_q|; the two
                     adds over the planes: 2 u sum_planes |f_plane|.
  phases             a 32-term fp32 fma chain plus the final value: (32 + 1) u sum |f| |B|.
  angle              2 pi * y, * (1 / 2 pi), and the rounded constant: 3 u |ang|.
  sin / cos          SIN_ABS = 3e-6 absolute, the figure csrc/decode.hip's comment claims for v_sin_f32 / v_cos_f32 (not measured
                     in isolation anywhere; a kernel that exceeds a bound built on it is a finding, not a reason to raise it).
  split layers       x = x_hi + x_lo + dx, |x_lo| <= 2^-11 |x|, |dx| <= 2^-11 |x_lo| <= 2^-22 |x| while x_lo is a NORMAL fp16; the same
                     for w; the dropped w_lo x_lo <= 2^-22 |w| |x|: 3 * 2^-22 relative to sum |W| |x|.  fp32 accumulation: K step s
                     (inputs 16 s .. 16 s + 15, the kernel's fragment order) is three v_mfma_f32_32x32x16_f16 (w_hi x_hi, w_lo x_hi,
                     w_hi x_lo), each adding 16 exact products (22 significant bits) to the accumulator; modelled as the fp32
                     matrix instruction is documented, an fma chain in some order of the 16: at most 16 roundings per
                     instruction, each of a partial sum no larger than |C_in(s)| + sum |products of the step|, C_in(s) the
                     float64 partial sum entering the step: 48 u sum_s (|C_in(s)| + (1 + 2^-10) sum_step |w| |x|).  (A flat
                     128 u sum |W| |x| is 1.7 x this at the synthetic weights and leaves the three lo-term mutations at a
                     rejection factor of 1.0 -- the partial sums of a layer are far below sum |W| |x| until its end.)
                     A lo part below 2^-14 is an fp16 SUBNORMAL (spacing 2^-24): its rounding error is 2^-25
                     absolute, not relative: 2^-25 (sum_{w_lo subnormal} |x| + sum_{x_lo subnormal} |w|).  Bias add: u |pre|.
  output             128 fmas, the lane exchange and b3: 130 u sum |w3| |h2|.
ReLU: a unit counts as active in the derivative whenever its float64 pre-activation is above MINUS its own error bound (an interval
bound, cheap and loose, so more units count), so that a unit at the kink cannot hide a path.

Backward bound.  For every texel and channel A = sum over points and taps |w_q| |d loss / d feature|, in float64: what the
gradient element would be if nothing cancelled.  A tap weight is ix - floor ix (or its complement) of a texel coordinate that
carries 2 u |ix| ABSOLUTE error, so a weight of 1e-3 is only good to 1e-3 relative, in any fp32 implementation; that part is
derived, not measured: Aw = sum |d w_q| |d loss / d feature| with |d w_q| = 2 u (|ix| |wy| + |iy| |wx|) + u |w_q|.
|kernel - ref| <= 4 REL A + D, D = Aw + cnt u A + u |ref| + 4 u A1 the derived terms (derived_terms below), with
REL = max (|g32 - g64| - D) / A of torch autograd on THIS statement in float32 and float64, measured where the test runs
(without the split REL is 1e-3 on 33 points, set by one small weight, and up to 1e3 at saturated logits, set by fp32
denormals; either would pass a texel that lost one of 512 contributions).  The 4 is the margin
tests/test_gpu_triplane_opt.py gives an fp32 computation in another summation order.  backward_bound adds the absolute
rounding of sigmoid(z) - gt, which no relative figure covers once the logit saturates.

Kinks.  ReLU' is discontinuous, so backward inputs keep away from it: a point is kept when all 256 float64 pre-activations are
further from 0 than 10 x the unit's forward error bound IN THE BACKWARD KERNELS (exact-fp32 products, software sin / cos):
the same local errors with SIN_SOFT = 2^-22 for sin / cos and, for the phases and the layers, the running error of an fp32 fma
chain sum_k half_ulp(partial sum_k) (<= u sum_k |partial sum_k|), the largest over the summation orders the two kernels use (decode_bwd.hip: bias first, k
ascending; decode_mlp.h: 32-blocks, within a block the pairs (8g + e, 8g + 4 + e) of one K = 2 matrix instruction, bias last),
each carried to the unit by the absolute value of the per-point derivative d pre / d (that quantity).
"""
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
SIN_ABS = 3e-6                                   # csrc/decode.hip: "Absolute error ~3e-6 in the features"
SIN_SOFT = 2.0 ** -22                            # sinf / cosf of ocml and decode.h's sincos_cw (~1e-7 absolute)
SPLIT_REL = 3 * 2.0 ** -22                      # hi/lo representation and the dropped lo x lo product
ACC_ROUNDINGS = 3 * 16                           # per K step: three matrix instructions of 16 products each
OUT_ULPS = 130
TWO_PI = float(np.float32(2 * np.pi))          # the reference multiplies an fp32 tensor by 2 * np.pi: the constant rounds to fp32
PLANE_AXES = ((0, 1), (1, 2), (0, 2))            # (u -> W, v -> H) of planes xy, yz, xz
NET_KEYS = ("0._B", "1.weight", "1.bias", "3.weight", "3.bias", "5.weight", "5.bias")


def net64(sd):
    """state dict (torch or numpy, fp32 values) -> float64 numpy arrays B [32,64], W1, b1, W2, b2, w3 [128], b3"""
    a = [np.asarray(sd[k].detach().cpu().numpy() if torch.is_tensor(sd[k]) else sd[k], np.float64) for k in NET_KEYS]
    return SimpleNamespace(B=a[0], W1=a[1], b1=a[2], W2=a[3], b2=a[4], w3=a[5].reshape(-1), b3=float(a[6].reshape(-1)[0]))


def scaled_state_dict(sd, k):
    """W1, b1 -> 2^k (W1, b1), W2 -> W2 / 2^k: the network is positively homogeneous, so the logit is unchanged; exact in fp32
    (asserted: no element leaves the normal range)."""
    out = {n: torch.as_tensor(np.asarray(v)).float().clone() for n, v in sd.items()}
    s = 2.0 ** k
    for n, f in (("1.weight", s), ("1.bias", s), ("3.weight", 1.0 / s)):
        t = out[n] * f
        assert bool(torch.equal(t / f, out[n])) and bool(torch.isfinite(t).all())
        out[n] = t
    return out


def grid_coords(axis):
    """the kernel's dense-grid rule: index (i res + j) res + k -> (axis[i], axis[j], axis[k])"""
    a = np.asarray(axis, np.float32)
    g = np.meshgrid(a, a, a, indexing="ij")
    return np.stack(g, axis=-1).reshape(-1, 3)


# ----------------------------------------------------------------------------------------------------------- taps
def taps(coords, S, dtype=np.float64, plane_axes=PLANE_AXES, align_corners=True, border_w_bug=False):
    """Bilinear taps of [N,3] coordinates, every operation in `dtype` in the kernels' order.  tex [N,3,4] flat texel index
    (p S + y) S + x or -1, w [N,3,4], order nw ne sw se; wx, wy [N,3,2]; ix, iy, x0, y0 [N,3]."""
    c = np.asarray(coords).astype(dtype)
    n = c.shape[0]
    one, two, sm1 = dtype(1), dtype(2), dtype(S - 1)
    tex = np.full((n, 3, 4), -1, np.int64)
    w = np.zeros((n, 3, 4), dtype)
    wx, wy = np.zeros((n, 3, 2), dtype), np.zeros((n, 3, 2), dtype)
    ixs, iys = np.zeros((n, 3), dtype), np.zeros((n, 3), dtype)
    x0s, y0s = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64)
    for p, (a, b) in enumerate(plane_axes):
        if align_corners:
            ix, iy = ((c[:, a] + one) / two) * sm1, ((c[:, b] + one) / two) * sm1
        else:
            ix, iy = ((c[:, a] + one) * dtype(S) - one) / two, ((c[:, b] + one) * dtype(S) - one) / two
        fx, fy = np.floor(ix), np.floor(iy)
        x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
        wx[:, p, 1], wx[:, p, 0] = ix - fx, (fx + one) - ix
        wy[:, p, 1], wy[:, p, 0] = iy - fy, (fy + one) - iy
        ixs[:, p], iys[:, p], x0s[:, p], y0s[:, p] = ix, iy, x0, y0
        for q in range(4):
            xx, yy = x0 + (q & 1), y0 + (q >> 1)
            wxq = wx[:, p, q & 1]
            if border_w_bug and (q & 1):             # mutation: the last column weighted with wx0
                wxq = np.where(xx == S - 1, wx[:, p, 0], wxq)
            w[:, p, q] = wxq * wy[:, p, q >> 1]
            ok = (xx >= 0) & (xx < S) & (yy >= 0) & (yy < S)
            tex[:, p, q] = np.where(ok, (p * S + yy) * S + xx, -1)
    return SimpleNamespace(tex=tex, w=w, wx=wx, wy=wy, ix=ixs, iy=iys, x0=x0s, y0=y0s, S=S)


def touched_texels(coords, S):
    """bool [3 S S]: texels some in-range tap of some point reaches, in float64 OR in the kernels' fp32 arithmetic (a point within
    an ulp of a cell boundary may sit on either side).  Everything outside is exactly 0.0 in a scattered gradient."""
    m = np.zeros(3 * S * S, bool)
    for dt in (np.float64, np.float32):
        t = taps(np.asarray(coords, np.float32), S, dt)
        m[t.tex[t.tex >= 0]] = True
    return m


def _gather(P, t, planes_used=(0, 1, 2), clamp_border=False):
    """features [N,32], sum |w| |texel| [N,32], per-plane features [N,3,32]"""
    n, S = t.tex.shape[0], t.S
    fp = np.zeros((n, 3, 32), P.dtype)
    fabs = np.zeros((n, 32), P.dtype)
    for p in planes_used:
        for q in range(4):
            tx = t.tex[:, p, q]
            ok = tx >= 0
            if clamp_border:                         # mutation: out-of-range taps read the clamped texel
                xx, yy = np.clip(t.x0[:, p] + (q & 1), 0, S - 1), np.clip(t.y0[:, p] + (q >> 1), 0, S - 1)
                tx, ok = (p * S + yy) * S + xx, np.ones(n, bool)
            v = P[np.where(ok, tx, 0)] * (t.w[:, p, q] * ok)[:, None]
            fp[:, p] += v
            fabs += np.abs(v)
    return (fp[:, 0] + fp[:, 1]) + fp[:, 2], fabs, fp


def mlp(net, x1, no_b1=False):
    pre1 = x1 @ net.W1.T + (0.0 if no_b1 else net.b1)
    h1 = np.maximum(pre1, 0.0)
    pre2 = h1 @ net.W2.T + net.b2
    h2 = np.maximum(pre2, 0.0)
    return pre1, h1, pre2, h2, h2 @ net.w3 + net.b3


def forward(net, planes, coords, *, plane_axes=PLANE_AXES, planes_used=(0, 1, 2), align_corners=True, swap_sincos=False,
            no_b1=False, clamp_border=False):
    """float64 forward of `planes` [3,S,S,32] (fp32 values) at `coords` [N,3] (fp32 values).  The keyword arguments are the
    mutations of tests/test_decoder_ref_host.py; the defaults are the statement."""
    planes = np.asarray(planes)
    S = planes.shape[1]
    P = planes.reshape(-1, 32).astype(np.float64)
    t = taps(np.asarray(coords, np.float32), S, np.float64, plane_axes, align_corners)
    f, fabs, fp = _gather(P, t, planes_used, clamp_border)
    y = f @ net.B
    ang = TWO_PI * y
    s, c = np.sin(ang), np.cos(ang)
    x1 = np.concatenate([c, s] if swap_sincos else [s, c], axis=1)
    pre1, h1, pre2, h2, z = mlp(net, x1, no_b1)
    return SimpleNamespace(logit=z, f=f, fabs=fabs, fp=fp, y=y, ang=ang, sin=s, cos=c, x1=x1, pre1=pre1, h1=h1, pre2=pre2, h2=h2,
                           taps=t, P=P, S=S)


# ----------------------------------------------------------------------------------------------------------- forward bound
def _window_max(planes):
    """G [3, S + 5, S + 5, 32]: entry (y0 + 3, x0 + 3) = max |texel| over rows y0-1..y0+2, columns x0-1..x0+2 (0 outside)"""
    a = torch.as_tensor(np.abs(np.asarray(planes, np.float64))).permute(0, 3, 1, 2)
    g = torch.nn.functional.max_pool2d(torch.nn.functional.pad(a, (4, 4, 4, 4)), 4, 1)
    return g.permute(0, 2, 3, 1).contiguous().numpy()


COORD_PLANES = (((0, 0), (2, 0)), ((0, 1), (1, 0)), ((1, 1), (2, 1)))   # x, y, z -> the (plane, axis) pairs that sample it


def feature_error(fw, planes):
    """Errors of the fp32 features against the float64 ones (module docstring: texel coordinate + features):
    local [N,32] the roundings (and, within d_ix of a cell boundary, the coordinate term through the neighbourhood maximum);
    d [N,3] the error of the texel coordinate of x, y, z (ONE rounded value each: both planes that sample a coordinate compute
    the same ix) and slope [N,3,32] = d features / d that texel coordinate, signed;  total [N,32] = local + sum d |slope|."""
    t, P, S = fw.taps, fw.P, fw.S
    n = t.tex.shape[0]
    G = _window_max(planes)
    local = 5 * U * fw.fabs + 2 * U * np.abs(fw.fp).sum(axis=1)
    d, slope = np.zeros((n, 3)), np.zeros((n, 3, 32))
    sl = {}
    for p in range(3):
        tq = [P[np.maximum(t.tex[:, p, q], 0)] * (t.tex[:, p, q] >= 0)[:, None] for q in range(4)]
        sl[p, 0] = (tq[1] - tq[0]) * t.wy[:, p, 0, None] + (tq[3] - tq[2]) * t.wy[:, p, 1, None]
        sl[p, 1] = (tq[2] - tq[0]) * t.wx[:, p, 0, None] + (tq[3] - tq[1]) * t.wx[:, p, 1, None]
    for a, pairs in enumerate(COORD_PLANES):
        for p, ax in pairs:
            ic, frac = (t.ix[:, p], t.wx[:, p, 1]) if ax == 0 else (t.iy[:, p], t.wy[:, p, 1])
            da = 2 * U * np.abs(ic)
            near = (frac <= da) | (frac >= 1.0 - da)
            g = 2.0 * G[p, np.clip(t.y0[:, p], -3, S + 1) + 3, np.clip(t.x0[:, p], -3, S + 1) + 3]
            d[:, a] = da
            slope[:, a] += np.where(near[:, None], 0.0, sl[p, ax])
            local += np.where(near[:, None], da[:, None] * g, 0.0)
    total = local + (d[:, :, None] * np.abs(slope)).sum(axis=1)
    return SimpleNamespace(local=local, d=d, slope=slope, total=total)


def _sub_mask(a):
    """True where the lo part of an fp32 value's hi/lo fp16 split is an fp16 subnormal (or zero)"""
    a32 = np.asarray(a, np.float32)
    lo = a32 - a32.astype(np.float16).astype(np.float32)
    return np.abs(lo) < 2.0 ** -14


def split_local_error(W, x, pre, chunk=4096):
    """local error of one hi/lo-split layer at each output [N,128] (module docstring: split layers)"""
    aw = np.abs(W)
    k = W.shape[1]
    ws = np.ascontiguousarray(W.reshape(W.shape[0], k // 16, 16).transpose(1, 2, 0))            # [step, 16, out]
    mw = _sub_mask(W).astype(np.float64).T
    out = np.empty_like(pre)
    for i in range(0, x.shape[0], chunk):
        xc = x[i:i + chunk]
        ax = np.abs(xc)
        sub = 2.0 ** -25 * (ax @ mw + (_sub_mask(xc) * 1.0) @ aw.T)
        xs = np.ascontiguousarray(xc.reshape(len(xc), k // 16, 16).transpose(1, 0, 2))            # [step, n, 16]
        part = xs @ ws                                                                          # each step's own sum
        c_in, run = np.zeros_like(part[0]), (1 + 2.0 ** -10) * (ax @ aw.T)
        for step in part:                                                                       # |partial sum entering each step|
            run += np.abs(c_in)
            c_in += step
        out[i:i + chunk] = SPLIT_REL * (ax @ aw.T) + ACC_ROUNDINGS * U * run + sub + U * np.abs(pre[i:i + chunk])
    return out


def forward_bound(net, planes, fw, sin_abs=SIN_ABS, local=split_local_error):
    """-> SimpleNamespace(bound [N], e1, e2 [N,128] interval bounds of the pre-activations, parts: the bound's terms)"""
    ferr = feature_error(fw, planes)
    aB = np.abs(net.B)
    yloc = (32 + 1) * U * (np.abs(fw.f) @ aB)
    angloc = 3 * U * np.abs(fw.ang)
    loc1 = local(net.W1, fw.x1, fw.pre1)
    loc2 = local(net.W2, fw.h1, fw.pre2)
    # interval bounds of the pre-activations: the masks, nothing else
    angerr = angloc + TWO_PI * (yloc + ferr.total @ aB)
    e1 = (np.concatenate([angerr, angerr], axis=1) + sin_abs) @ np.abs(net.W1).T + loc1
    m1 = fw.pre1 > -e1
    e2 = (e1 * m1) @ np.abs(net.W2).T + loc2
    m2 = fw.pre2 > -e2
    # d logit / d (each quantity), through the inclusive masks
    g2 = net.w3[None, :] * m2
    g1 = (g2 @ net.W2) * m1
    gx = g1 @ net.W1
    gang = gx[:, :64] * fw.cos - gx[:, 64:] * fw.sin
    gy = TWO_PI * gang
    gf = gy @ net.B.T
    parts = SimpleNamespace(
        feat=(np.abs(gf) * ferr.local).sum(1) + (ferr.d * np.abs(np.einsum("nc,nac->na", gf, ferr.slope))).sum(1), phase=(np.abs(gy) * yloc).sum(1), angle=(np.abs(gang) * angloc).sum(1),
        sincos=np.abs(gx).sum(1) * sin_abs, layer1=(np.abs(g1) * loc1).sum(1), layer2=(np.abs(g2) * loc2).sum(1),
        out=OUT_ULPS * U * (np.abs(fw.h2) @ np.abs(net.w3)) + U * np.abs(fw.logit))
    bound = sum(vars(parts).values())
    return SimpleNamespace(bound=bound, e1=e1, e2=e2, parts=parts)


# ----------------------------------------------------------------------------------------------------------- kink filter
def _fit_order(blocks):
    """decode_mlp.h's order (the fit and field kernels) inside a product of K = 32 * blocks: k = 32 q + 8 g + e and + 4 (the two K slots of one
    v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain), either first"""
    a, b = [], []
    for q in range(blocks):
        for g in range(4):
            for e in range(4):
                k = 32 * q + 8 * g + e
                a += [k, k + 4]
                b += [k + 4, k]
    return np.array(a), np.array(b)


def _half_ulp(s):
    """half an fp32 ulp of a partial sum: what one rounding to nearest can add (<= u |s|, 0.72 u |s| on average)"""
    _, e = np.frexp(s)
    return np.where(s == 0, 0.0, np.ldexp(U, e - 1))


def _chain_error(W, x, bias, chunk=128):
    """sum_k half_ulp(partial sum_k) of pre = W x + bias as an fp32 fma chain: the largest over decode_bwd.hip's order (bias
    first, k ascending) and decode_mlp.h's (its k order, bias last).  x [N,K], W [out,K] -> [N,out]"""
    oa, ob = _fit_order(W.shape[1] // 32)
    out = np.zeros((x.shape[0], W.shape[0]))
    for i in range(0, x.shape[0], chunk):
        terms = x[i:i + chunk, None, :] * W[None, :, :]                        # [n, out, k]
        e = _half_ulp(bias[None, :, None] + np.cumsum(terms, axis=2)).sum(axis=2)
        for o in (oa, ob):
            c = np.cumsum(terms[:, :, o], axis=2)
            e = np.maximum(e, _half_ulp(c).sum(axis=2) + _half_ulp(c[:, :, -1] + bias[None, :]))
        out[i:i + chunk] = e
    return out


def kink_margin(net, planes, coords, chunk=128):
    """For each point the smallest |pre-activation| / (unit's forward error bound in the backward kernels) over the 256 hidden
    units (module docstring: Kinks).  A point is usable when this is above 10."""
    fw = forward(net, planes, coords)
    ferr = feature_error(fw, planes)
    yloc = _chain_error(net.B.T, fw.f, np.zeros(64))
    angloc = 3 * U * np.abs(fw.ang)
    loc1 = _chain_error(net.W1, fw.x1, net.b1)
    loc2 = _chain_error(net.W2, fw.h1, net.b2)
    aW1, aW2 = np.abs(net.W1), np.abs(net.W2)
    out = np.zeros(len(fw.logit))
    for i in range(0, len(out), chunk):
        sl = slice(i, i + chunk)
        c, s = fw.cos[sl, None, :], fw.sin[sl, None, :]

        def carried(Jx):          # errors of features, phases, angles and sin / cos through d pre / d x1 = Jx [n,128,128]
            Dy = Jx[:, :, :64] * c - Jx[:, :, 64:] * s
            Jf = TWO_PI * Dy @ net.B.T
            e = np.einsum("nik,nk->ni", np.abs(Jf), ferr.local[sl])
            e += np.einsum("nia,na->ni", np.abs(np.einsum("nic,nac->nia", Jf, ferr.slope[sl])), ferr.d[sl])
            e += np.einsum("nik,nk->ni", np.abs(Dy), TWO_PI * yloc[sl] + angloc[sl])
            return e + SIN_SOFT * np.abs(Jx).sum(axis=2)
        e1 = carried(np.broadcast_to(net.W1, (c.shape[0], 128, 128))) + loc1[sl]
        m1 = fw.pre1[sl] > -e1
        e2 = carried((net.W2[None] * m1[:, None, :]) @ net.W1) + (loc1[sl] * m1) @ aW2.T + loc2[sl]
        out[sl] = np.minimum((np.abs(fw.pre1[sl]) / e1).min(axis=1), (np.abs(fw.pre2[sl]) / e2).min(axis=1))
    return out


def away_from_kinks(net, planes, coords, factor=10.0):
    return kink_margin(net, planes, coords) > factor


# ----------------------------------------------------------------------------------------------------------- the split model
def split_layer(W, x, scale_mode="keep", drop_wlo=False, drop_xlo=False):
    """W x as csrc/decode.hip forms it: w_hi x_hi + w_lo x_hi + w_hi x_lo with fp16 parts (numpy's conversion: round to nearest
    even, subnormals kept), accumulated in float64.  scale_mode 'flush': every fp16 subnormal (a part below 2^-14, hi or lo) becomes 0."""
    def parts(a):
        a32 = np.asarray(a, np.float32)
        with np.errstate(over="ignore"):
            hi = a32.astype(np.float16)
            lo = (a32 - hi.astype(np.float32)).astype(np.float16)
        hi, lo = hi.astype(np.float64), lo.astype(np.float64)
        if scale_mode == "flush":
            hi, lo = (np.where(np.abs(v) < 2.0 ** -14, 0.0, v) for v in (hi, lo))
        return hi, lo
    wh, wl = parts(W)
    xh, xl = parts(x)
    out = xh @ wh.T
    if not drop_wlo:
        out = out + xh @ wl.T
    if not drop_xlo:
        out = out + xl @ wh.T
    return out


def split_model(net, x1, **kw):
    """logits of Fourier features x1 [N,128] through the two split layers (fp32 activations between them) and the float64 output"""
    with np.errstate(invalid="ignore", over="ignore"):
        h1 = np.maximum(split_layer(net.W1, x1, **kw) + net.b1, 0.0).astype(np.float32)
        h2 = np.maximum(split_layer(net.W2, h1, **kw) + net.b2, 0.0)
        return h2 @ net.w3 + net.b3


def honest_forward(net, planes, coords, seed=0, **kw):
    """The float64 result with the kernel's rounding points applied: fp32 taps, features and phases, sin / cos off by SIN_ABS
    (random signs), the hi/lo split of split_model."""
    planes = np.asarray(planes, np.float32)
    t = taps(np.asarray(coords, np.float32), planes.shape[1], np.float32)
    f, _, _ = _gather(planes.reshape(-1, 32), t)
    y = (f.astype(np.float32) @ net.B.astype(np.float32)).astype(np.float32)
    ang = (np.float32(TWO_PI) * y).astype(np.float64)
    x1 = np.concatenate([np.sin(ang), np.cos(ang)], axis=1)
    sign = np.random.RandomState(seed).randint(0, 2, x1.shape) * 2 - 1
    return split_model(net, (x1 + SIN_ABS * sign).astype(np.float32), **kw)


# ----------------------------------------------------------------------------------------------------------- gradients
def _net_t(net, dtype):
    return SimpleNamespace(**{k: torch.as_tensor(np.asarray(v, np.float64)).to(dtype) for k, v in vars(net).items()})


def _decode_t(nt, P, coords, S, dtype, rec, border_w_bug=False):
    """logits of `coords` in torch (differentiable in the flat planes P [3 S S, 32]); the taps come from taps() in the same
    precision.  Appends (tex, |w|, features) to rec for the magnitude scatter."""
    npd = np.float32 if dtype == torch.float32 else np.float64
    t = taps(np.asarray(coords, np.float32), S, npd, border_w_bug=border_w_bug)
    tex = torch.as_tensor(t.tex)
    w = torch.as_tensor(t.w).to(dtype) * (tex >= 0)
    fp = [sum(P[tex[:, p, q].clamp(min=0)] * w[:, p, q, None] for q in range(4)) for p in range(3)]
    f = (fp[0] + fp[1]) + fp[2]
    ok = t.tex >= 0                 # |error of an fp32 tap weight|: the two texel coordinates (2 u |ix| each) and the product
    dw = [2 * U * (np.abs(t.ix)[:, :, None] * np.abs(t.wy[:, :, q >> 1, None]) + np.abs(t.iy)[:, :, None] * np.abs(t.wx[:, :, q & 1, None]))
          for q in range(4)]
    dw = (np.concatenate(dw, axis=2) + U * np.abs(t.w)) * ok
    rec.append((tex, w.abs(), f, torch.as_tensor(dw, dtype=torch.float64)))
    ang = TWO_PI * (f @ nt.B)
    x = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    h = torch.relu(x @ nt.W1.T + nt.b1)
    h = torch.relu(h @ nt.W2.T + nt.b2)
    return h @ nt.w3 + nt.b3


def _scatter_abs(rec, ntex, grads, weights_error=False, count=False):
    A = torch.zeros((ntex, 32), dtype=torch.float64)
    for i, (tex, aw, f, dw) in enumerate(rec):
        g = grads[i].double().abs()
        if weights_error:
            aw = dw
        if count:
            aw, g = (tex >= 0).double(), torch.ones_like(g)
        for p in range(3):
            for q in range(4):
                A.index_add_(0, tex[:, p, q].clamp(min=0), g * aw[:, p, q, None].double())
    return A.numpy()


def _bce(z, gt):
    return torch.clamp(z, min=0) - z * gt + torch.log1p(torch.exp(-z.abs()))


def points_loss_grad(net, planes, coords, gt, dtype=torch.float64, npts_div=None, border_w_bug=False):
    """-> loss = -mean BCE, dplanes [3,S,S,32], logits, A (magnitude scatter), bce_abs_mean = sum |bce_i| / n.
    npts_div / border_w_bug: mutations."""
    planes = np.asarray(planes)
    S = planes.shape[1]
    P = torch.as_tensor(planes.reshape(-1, 32).astype(np.float64)).to(dtype).requires_grad_(True)
    rec = []
    z = _decode_t(_net_t(net, dtype), P, coords, S, dtype, rec, border_w_bug)
    bce = _bce(z, torch.as_tensor(np.asarray(gt, np.float64)).to(dtype))
    loss = -bce.sum() / float(npts_div or len(z))
    f = rec[0][2]
    dzdf, = torch.autograd.grad(z.sum() / len(z), f, retain_graph=True)
    dldf, = torch.autograd.grad(loss, f, retain_graph=True)
    gP, = torch.autograd.grad(loss, P)
    sc = lambda g, **kw: _scatter_abs(rec, 3 * S * S, [g], **kw).reshape(planes.shape)      # noqa: E731
    return SimpleNamespace(loss=float(loss.detach()), dplanes=gP.double().numpy().reshape(planes.shape), logits=z.detach().double().numpy(),
                           bce_abs_mean=float(bce.abs().sum() / len(z)), A=sc(dldf), A1=sc(dzdf), Aw=sc(dldf, weights_error=True),
                           cnt=sc(dldf, count=True))


def partner(r, noise):
    """r + 0.01 noise as the reference and the kernel form it: fp32 multiply, fp32 add"""
    return np.asarray(r, np.float32) + np.asarray(noise, np.float32) * np.float32(0.01)


def fit_loss_grad(net, planes, coords, gt, idx, r, noise, pair_w, dtype=torch.float64, flip_partner=False):
    """-> parts [bce mean, mse], dplanes = d (bce + pair_w mse) / d planes, A.  idx may repeat; nbatch or nrand may be 0."""
    planes = np.asarray(planes)
    S = planes.shape[1]
    P = torch.as_tensor(planes.reshape(-1, 32).astype(np.float64)).to(dtype).requires_grad_(True)
    nt, rec = _net_t(net, dtype), []
    idx = np.asarray(idx, np.int64)
    bce = mse = torch.zeros((), dtype=dtype)
    A1 = np.zeros((3 * S * S, 32))
    if len(idx):
        z = _decode_t(nt, P, np.asarray(coords, np.float32)[idx], S, dtype, rec)
        bce = _bce(z, torch.as_tensor(np.asarray(gt, np.float64)[idx]).to(dtype)).mean()
        dzdf, = torch.autograd.grad(z.sum() / len(z), rec[0][2], retain_graph=True)
        A1 = _scatter_abs(rec[:1], 3 * S * S, [dzdf])
    if len(r):
        za = _decode_t(nt, P, r, S, dtype, rec)
        zb = _decode_t(nt, P, partner(r, noise), S, dtype, rec)
        if flip_partner:                              # mutation: the partner's cotangent with the wrong sign
            zb = 2 * zb.detach() - zb
        mse = ((za - zb) ** 2).mean()
    total = bce + float(np.float32(pair_w)) * mse
    fs = [x[2] for x in rec]
    dldf = [torch.zeros_like(f) if g is None else g for f, g in zip(fs, torch.autograd.grad(total, fs, retain_graph=True, allow_unused=True))]
    gP, = torch.autograd.grad(total, P, allow_unused=True)
    g = gP if gP is not None else torch.zeros_like(P)
    sc = lambda **kw: _scatter_abs(rec, 3 * S * S, dldf, **kw).reshape(planes.shape)      # noqa: E731
    return SimpleNamespace(parts=np.array([float(bce.detach()), float(mse.detach())]), dplanes=g.double().numpy().reshape(planes.shape),
                           A=sc(), A1=np.asarray(A1).reshape(planes.shape), Aw=sc(weights_error=True), cnt=sc(count=True))


def permuted_net(net, seed):
    """The same function with the phases and the hidden units of both layers renumbered: every matrix product of an fp32
    run then sums in another order.  seed 0: the net itself."""
    if seed == 0:
        return net
    rs = np.random.RandomState(seed)
    p0, p1, p2 = rs.permutation(64), rs.permutation(128), rs.permutation(128)
    px = np.concatenate([p0, 64 + p0])
    return SimpleNamespace(B=net.B[:, p0], W1=net.W1[p1][:, px], b1=net.b1[p1], W2=net.W2[p2][:, p1], b2=net.b2[p2],
                           w3=net.w3[p2], b3=net.b3)


DZ_ULPS = 4           # roundings behind sigmoid(z) - gt (derived_terms)
REL_RUNS = 4          # fp32 autograd runs (summation orders) REL is the largest over


def derived_terms(ref):
    """The parts of the backward bound that follow from the arithmetic alone:
    Aw         the fp32 tap weights (module docstring);
    cnt u A    cnt float atomics into one element, in any order: fewer than cnt roundings of partial sums no larger than A;
    u |ref|    the stored value;
    4 u A1     the kernels form d bce / d z = sigmoid(z) - gt from a rounded sigmoid, an ABSOLUTE error of a few u (expf: 2 u,
               the add, the division, each relative to a sigmoid <= 1) however small the difference is: at a saturated logit with
               a matching target the float64 difference is 1e-44 and the fp32 one is 0.  A1 is the magnitude scatter of
               d (mean z) / d features over the data points."""
    return ref.Aw + ref.cnt * U * ref.A + U * np.abs(ref.dplanes) + DZ_ULPS * U * ref.A1


def measured_rel(g32s, ref):
    """REL of the backward bound: the largest (|fp32 - fp64| - derived terms) / A of autograd on this statement, over the fp32
    runs g32s (the net and REL_RUNS - 1 renumberings of it: one run's largest ratio sits on a single element whose feature
    gradient nearly cancels, and a kernel in yet another order would exceed 4 x that one sample about one time in six);
    at least 2 u: the product w * d feature and the add round once each."""
    m = ref.A > 0
    d = derived_terms(ref)
    return max([2 * U] + [float((np.maximum(np.abs(g - ref.dplanes) - d, 0.0)[m] / ref.A[m]).max()) for g in g32s])


def backward_bound(ref, rel):
    return 4 * rel * ref.A + derived_terms(ref)


# ----------------------------------------------------------------------------------------------------------- un-normalise, x0 route
def planes_prepare(latent, rng, mid):
    """latent [96,S,S] * range + middle -> planes [3,S,S,32] in float64, and |latent range| (the product the add rounds with)"""
    lat = np.asarray(latent, np.float64)
    S = lat.shape[-1]
    r = np.ones(96) if rng is None else np.asarray(rng, np.float64)
    m = np.zeros(96) if mid is None else np.asarray(mid, np.float64)
    prod = lat * r[:, None, None]
    cl = lambda a: np.ascontiguousarray(a.reshape(3, 32, S, S).transpose(0, 2, 3, 1))      # noqa: E731
    return cl(prod + m[:, None, None]), cl(np.abs(prod))


def x0_grad(dplanes, rng, x, model_out, sr, srm1, clip):
    """The clamp chain of ishap_x0_grad_to_cotangent: gx0 = dplanes range 1[-1 <= sr x - srm1 eps <= 1] (equality passes, as
    torch's clamp does); g_direct = sr gx0 [96,S,S]; cot_out [192,S,S] = (-srm1 gx0, 0).  Also |sr x - srm1 eps| - 1 in float64."""
    d = np.asarray(dplanes, np.float64)                                                       # [3,S,S,32]
    S = d.shape[1]
    g = d.transpose(0, 3, 1, 2).reshape(96, S, S)
    if rng is not None:
        g = g * np.asarray(rng, np.float64)[:, None, None]
    x0u = float(np.float32(sr)) * np.asarray(x, np.float64) - float(np.float32(srm1)) * np.asarray(model_out, np.float64)[:96]
    if clip:
        g = np.where((x0u < -1.0) | (x0u > 1.0), 0.0, g)
    cot = np.concatenate([-float(np.float32(srm1)) * g, np.zeros_like(g)], axis=0)
    return float(np.float32(sr)) * g, cot, np.abs(x0u) - 1.0


# ----------------------------------------------------------------------------------------------------------- inputs
AMP_FWD = 0.05        # planes of the forward cases: phases of a few radians, feature roundings well under the layers' terms
AMP_BWD = 0.02        # planes of the backward cases: the kink filter keeps > 90 % (the unit bounds grow with the features)


def synthetic_net():
    """(fp32 numpy state dict, float64 net) of synthetic.decoder_state_dict()"""
    from ishapediting_amd import synthetic
    sd = {k: v.numpy() for k, v in synthetic.decoder_state_dict().items()}
    return sd, net64(sd)


def make_planes(S, amp, seed):
    return (np.random.RandomState(seed).randn(3, S, S, 32) * amp).astype(np.float32)


def coords_family(name, n, S, rs):
    """[n,3] fp32 coordinates of one family of the forward table (tests/test_gpu_decoder_oracle.py)"""
    band = 2.0 / max(S - 1, 1)
    u = rs.uniform(-1.0, 1.0, (n, 3))
    pick = rs.randint(1, 8, n)[:, None] >> np.arange(3)[None, :] & 1 > 0          # a non-empty subset of the axes per point
    sign = rs.randint(0, 2, (n, 3)) * 2.0 - 1.0
    if name == "uniform":
        c = rs.uniform(-1.1, 1.1, (n, 3))
    elif name == "centres":                       # weights exactly 0 / 1
        c = 2.0 * rs.randint(0, S, (n, 3)) / max(S - 1, 1) - 1.0
    elif name == "faces":                         # exactly +-1 on one, two or three axes
        c = np.where(pick, sign, u)
    elif name == "eps_out":                       # one ulp outside
        c = np.where(pick, sign * (1.0 + 2.0 ** -23), u)
    elif name == "fade":                          # 1 < |c| < 1 + 2 / (S - 1): one column of taps still in range
        c = np.where(pick, sign * (1.0 + band * rs.uniform(0.02, 0.98, (n, 3))), u)
    elif name == "beyond":                        # no tap of any plane in range
        c = sign * (1.0 + band * rs.uniform(1.05, 3.0, (n, 3)))
    elif name == "far":                           # (u + 1) / 2 (S - 1) <= 6.4e7 for S = 128: far below 2^31
        c = np.where(pick, sign * 1e6, u)
    else:
        raise KeyError(name)
    return c.astype(np.float32)


FAMILIES = ("uniform", "centres", "faces", "eps_out", "fade", "beyond", "far")


def mixed_coords(n_each, S, seed):
    rs = np.random.RandomState(seed)
    return np.concatenate([coords_family(f, n_each, S, rs) for f in FAMILIES], axis=0)


_POOLS = {}


def survivor_pool(S, n=1100, seed=11):
    """Uniform candidates in the cube that pass the kink filter on make_planes(S, AMP_BWD, S) with the synthetic weights.
    -> SimpleNamespace(planes, coords, rejected = share of the candidates the filter dropped)"""
    key = ("single", S, n, seed)
    if key not in _POOLS:
        _, net = synthetic_net()
        planes = make_planes(S, AMP_BWD, S)
        c = np.random.RandomState(seed).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
        keep = away_from_kinks(net, planes, c)
        _POOLS[key] = SimpleNamespace(planes=planes, coords=c[keep], rejected=1.0 - float(keep.mean()))
    return _POOLS[key]


def pair_pool(S, n=256, seed=12, on_faces=0):
    """Pairs (r, noise) whose two points r and r + 0.01 noise both pass the filter; the first `on_faces` candidates have one
    coordinate exactly +-1 (their partners leave the cube about half the time)."""
    key = ("pair", S, n, seed, on_faces)
    if key not in _POOLS:
        _, net = synthetic_net()
        planes = make_planes(S, AMP_BWD, S)
        rs = np.random.RandomState(seed)
        r = rs.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
        noise = rs.randn(n, 3).astype(np.float32)
        r[np.arange(on_faces), rs.randint(0, 3, on_faces)] = (rs.randint(0, 2, on_faces) * 2 - 1).astype(np.float32)
        keep = away_from_kinks(net, planes, r) & away_from_kinks(net, planes, partner(r, noise))
        _POOLS[key] = SimpleNamespace(planes=planes, r=r[keep], noise=noise[keep], rejected=1.0 - float(keep.mean()))
    return _POOLS[key]


def filtered(net, planes, coords):
    """the points of `coords` (built from survivors: on borders, corners ...) that are themselves away from every kink"""
    c = np.asarray(coords, np.float32)
    return c[away_from_kinks(net, planes, c)]
