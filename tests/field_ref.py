"""The decoder's field in space (csrc/decode_field.hip on decode_mlp.h) restated in float64 on top of tests/decoder_ref.py: the analytic
d logit / d coordinate, the level-set projection, and the bounds tests/test_gpu_field.py holds the kernels to.  Held to torch
autograd, to a central difference and to a list of mutations by tests/test_field_ref_host.py.

The statement (notation of decoder_ref's docstring).  Forward: decoder_ref.forward.  Backward from d logit = 1:
  g2 = w3 [pre2 > 0];  g1 = (W2^T g2) [pre1 > 0];  gx = W1^T g1;  d ang = gx_sin cos(ang) - gx_cos sin(ang);
  d y = float32(2 pi) d ang;  df = B d y  (32 channels).
For plane p with axes (a, b) and the cell (texels t_nw t_ne t_sw t_se, out-of-range texels 0; weights wx0 wx1 wy0 wy1)
  sx = (t_ne - t_nw) wy0 + (t_se - t_sw) wy1,   sy = (t_sw - t_nw) wx0 + (t_se - t_ne) wx1          per channel,
  grad[a] += (S - 1) / 2 sum_c df[c] sx[c],      grad[b] += (S - 1) / 2 sum_c df[c] sy[c];
every coordinate is sampled by two planes (decoder_ref.COORD_PLANES).  On a cell boundary floor() picks the cell: the
right-sided derivative.

Gradient bound, per point and axis:  |kernel - ref| <= 4 REL A + D.
  A    what the component would be if nothing cancelled anywhere: absolute values through every layer and the slope,
         Adf = |B| (2 pi) (|cos| Agx_sin + |sin| Agx_cos),  Agx = |W1|^T ((|W2|^T (|w3| [pre2 > 0])) [pre1 > 0]),
         A[a] = (S - 1) / 2 sum over the two planes of a, sum_c Adf[c] ((|t_ne| + |t_nw|) w_0 + (|t_se| + |t_sw|) w_1).
  REL  measured where the test runs: the largest (|g32 - g64| - D) / A of torch autograd of THIS statement with respect to the
       coordinates in float32 against float64, over REL_RUNS renumberings of the network (decoder_ref.permuted_net), on the
       filtered points; at least 2 u.  The fp32 run forms the texel coordinate exactly as the kernel does (the same three
       operations), so what a rounded coordinate does to the features behind it is part of what REL measures.  The 4 is the
       project's margin for an fp32 computation in another summation order.
  D    the parts that follow from the arithmetic alone:
         the slope's weights: wy1 = iy - floor iy carries the texel coordinate's 2 u |iy| (two roundings of a number of size
           |iy|; the subtraction is exact), wy0 moves the other way, so d sx = 2 u |iy| |(t_se - t_sw) - (t_ne - t_nw)| and
           likewise d sy = 2 u |ix| |the same cross difference|, carried by (S - 1) / 2 |df|;
         the scale: (S - 1) * 0.5f is exact, the product with it rounds once: u |ref|;
         the stored value: u |ref|.
Filter.  A gradient is compared where decoder_ref.away_from_kinks holds (ReLU' jumps) and where every texel coordinate is
further than d_ix = 2 u |ix| from a cell boundary (the slopes jump).  Everywhere else the logit is still compared and the
gradient must be finite.

Logits.  decoder_ref.forward_bound with SIN_SOFT (decode.h's sincos_cw; decode_mlp.h's mlp_forward, which the fit shares).  Its layer term is written for
decode.hip's split products; it covers this kernel's exact-fp32 products too: a K = 2 matrix instruction is a k-ordered
fma pair, so a layer is a 128-step fma chain whose error is at most u sum_k |partial sum_k|, and inside K step s of 16 every
partial sum is at most |C_in(s)| + sum_step |w| |x|: at most 16 u sum_s (|C_in(s)| + sum_step |w| |x|), a third of the
48 u sum_s (...) the bound holds.  The output layer here is 64 fmas per lane half, the exchange and b3: 66 roundings of
OUT_ULPS = 130.

Normal.  n = -g / |g|.  With |dg_j| <= b_j (the gradient bound) first order gives dn = -(dg - n (n . dg)) / |g|, so
  |dn_i| <= (b_i + |n_i| sum_j |n_j| b_j) / |g|  +  2 (|b| / |g|)^2  +  u |n_i|;
the second term bounds the remainder of the expansion (|n' - n| <= 2 |dg| / |g| for any two vectors, squared once more for the
part first order leaves out), the last is the stored value: the kernel normalises in double and rounds once per component.

Projection (csrc/decode_field.hip, ishap_triplane_project): x = x0, (z, g) = field(x), scale = 1; `iterations` times: a point
with |z| <= tol or |g|^2 < gmin stops; else d = -scale z g / max(|g|^2, gmin), |d| clipped to step_max, x + d clipped into the
ball of radius max_move around x0; the trial is taken, and scale reset to 1, when |z_trial| < |z|, else scale halves.
"""
from types import SimpleNamespace

import numpy as np
import torch

from tests import decoder_ref as D

U = D.U
MUTATIONS = ("no_scale", "drop_plane", "wrong_wy", "swap_yz", "wrong_sign", "swap_dsincos", "no_mask1")


def _cell(fw):
    """texels of every point's cell, [3][4] arrays [N,32] (nw ne sw se; 0 out of range)"""
    t, P = fw.taps, fw.P
    return [[P[np.maximum(t.tex[:, p, q], 0)] * (t.tex[:, p, q] >= 0)[:, None] for q in range(4)] for p in range(3)]


def feature_cotangent(net, fw, mutation=None):
    """df [N,32] = d logit / d features, and Adf: the same with absolute values through every layer"""
    m1, m2 = fw.pre1 > 0, fw.pre2 > 0
    if mutation == "no_mask1":
        m1 = np.ones_like(m1)
    g1 = ((net.w3[None, :] * m2) @ net.W2) * m1
    gx = g1 @ net.W1
    s, c = (fw.cos, fw.sin) if mutation == "swap_dsincos" else (fw.sin, fw.cos)
    df = (D.TWO_PI * (gx[:, :64] * c - gx[:, 64:] * s)) @ net.B.T
    a1 = ((np.abs(net.w3)[None, :] * m2) @ np.abs(net.W2)) * m1
    ax = a1 @ np.abs(net.W1)
    adf = (D.TWO_PI * (ax[:, :64] * np.abs(c) + ax[:, 64:] * np.abs(s))) @ np.abs(net.B).T
    return df, adf


def field_grad(net, planes, coords, mutation=None, fw=None):
    """-> SimpleNamespace(logit [N], grad [N,3], A [N,3], D [N,3], fw).  `mutation`: one of MUTATIONS (host tests) or None.
    fw: a forward already made (forward_at, for float64 coordinates); by default decoder_ref.forward of the fp32 coordinates."""
    assert mutation is None or mutation in MUTATIONS
    fw = D.forward(net, planes, coords) if fw is None else fw
    t, S = fw.taps, fw.S
    df, adf = feature_cotangent(net, fw, mutation)
    cell = _cell(fw)
    scale = 1.0 if mutation == "no_scale" else (S - 1) / 2.0
    n = len(fw.logit)
    grad, A, Dt = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    for p, axes in enumerate(D.PLANE_AXES):
        if mutation == "drop_plane" and p == 2:
            continue
        if mutation == "swap_yz" and p == 1:
            axes = axes[::-1]
        nw, ne, sw, se = cell[p]
        wx, wy = t.wx[:, p], t.wy[:, p]
        wy_s = wx if mutation == "wrong_wy" else wy
        sx = (ne - nw) * wy_s[:, 0, None] + (se - sw) * wy_s[:, 1, None]
        sy = (sw - nw) * wx[:, 0, None] + (se - ne) * wx[:, 1, None]
        asx = (np.abs(ne) + np.abs(nw)) * wy[:, 0, None] + (np.abs(se) + np.abs(sw)) * wy[:, 1, None]
        asy = (np.abs(sw) + np.abs(nw)) * wx[:, 0, None] + (np.abs(se) + np.abs(ne)) * wx[:, 1, None]
        cross = np.abs((se - sw) - (ne - nw))
        grad[:, axes[0]] += scale * (df * sx).sum(1)
        grad[:, axes[1]] += scale * (df * sy).sum(1)
        A[:, axes[0]] += scale * (adf * asx).sum(1)
        A[:, axes[1]] += scale * (adf * asy).sum(1)
        Dt[:, axes[0]] += scale * 2 * U * np.abs(t.iy[:, p]) * (np.abs(df) * cross).sum(1)
        Dt[:, axes[1]] += scale * 2 * U * np.abs(t.ix[:, p]) * (np.abs(df) * cross).sum(1)
    if mutation == "wrong_sign":
        grad = -grad
    return SimpleNamespace(logit=fw.logit, grad=grad, A=A, D=Dt + 2 * U * np.abs(grad), fw=fw)


def away_from_boundaries(coords, S):
    """bool [N]: every texel coordinate further than d_ix = 2 u |ix| from a cell boundary"""
    t = D.taps(np.asarray(coords, np.float32), S)
    ok = np.ones(len(t.ix), bool)
    for ic, frac in ((t.ix, t.wx[:, :, 1]), (t.iy, t.wy[:, :, 1])):
        d = 2 * U * np.abs(ic)
        ok &= ((frac > d) & (frac < 1.0 - d)).all(axis=1)
    return ok


def gradient_filter(net, planes, coords):
    """the points whose gradient is compared (module docstring: Filter)"""
    return D.away_from_kinks(net, planes, coords) & away_from_boundaries(coords, np.asarray(planes).shape[1])


# ----------------------------------------------------------------------------------------------------------- autograd
def decode_coords_t(nt, P, c, S):
    """logits of coordinates c [N,3] in torch, differentiable in c: decoder_ref._decode_t takes its tap weights from numpy, so
    this twin forms them in torch, in the kernels' order and in c's precision (floor is piecewise constant: its derivative is 0)"""
    dtype = c.dtype
    fp = []
    for p, (a, b) in enumerate(D.PLANE_AXES):
        ix, iy = ((c[:, a] + 1) / 2) * (S - 1), ((c[:, b] + 1) / 2) * (S - 1)
        fx, fy = torch.floor(ix).detach(), torch.floor(iy).detach()
        wx, wy = (((fx + 1) - ix), ix - fx), (((fy + 1) - iy), iy - fy)
        x0, y0 = fx.clamp(-2, 2 ** 30).long(), fy.clamp(-2, 2 ** 30).long()
        acc = 0
        for q in range(4):
            xx, yy = x0 + (q & 1), y0 + (q >> 1)
            ok = (xx >= 0) & (xx < S) & (yy >= 0) & (yy < S)
            tex = torch.where(ok, (p * S + yy) * S + xx, torch.zeros_like(xx))
            acc = acc + P[tex] * ((wx[q & 1] * wy[q >> 1]) * ok.to(dtype))[:, None]
        fp.append(acc)
    f = (fp[0] + fp[1]) + fp[2]
    ang = D.TWO_PI * (f @ nt.B)
    x = torch.cat([torch.sin(ang), torch.cos(ang)], dim=1)
    h = torch.relu(x @ nt.W1.T + nt.b1)
    h = torch.relu(h @ nt.W2.T + nt.b2)
    return h @ nt.w3 + nt.b3


def autograd_grad(net, planes, coords, dtype=torch.float64):
    """(logits [N], d logit / d coordinate [N,3]) by torch autograd in `dtype`, as float64 numpy"""
    planes = np.asarray(planes)
    S = planes.shape[1]
    P = torch.as_tensor(planes.reshape(-1, 32).astype(np.float64)).to(dtype)
    c = torch.as_tensor(np.asarray(coords, np.float32).astype(np.float64)).to(dtype).requires_grad_(True)
    z = decode_coords_t(D._net_t(net, dtype), P, c, S)
    g, = torch.autograd.grad(z.sum(), c)
    return z.detach().double().numpy(), g.double().numpy()


def measured_rel(net, planes, coords, ref, keep):
    """REL of the gradient bound (module docstring) on the points `keep`"""
    rel = 2 * U
    m = keep[:, None] & (ref.A > 0)
    if not m.any():
        return rel
    for s in range(D.REL_RUNS):
        _, g32 = autograd_grad(D.permuted_net(net, s), planes, coords, torch.float32)
        rel = max(rel, float((np.maximum(np.abs(g32 - ref.grad) - ref.D, 0.0)[m] / ref.A[m]).max()))
    return rel


def grad_bound(ref, rel):
    """[N,3]: 4 REL A + D"""
    return 4 * rel * ref.A + ref.D


def normal_of(grad, gmin=0.0):
    """-g / |g| [N,3]; 0 where |g|^2 < gmin or g = 0"""
    g = np.asarray(grad, np.float64)
    n2 = (g * g).sum(1)
    ok = (n2 >= gmin) & (n2 > 0)
    return np.where(ok[:, None], -g / np.sqrt(np.where(ok, n2, 1.0))[:, None], 0.0)


def normal_bound(grad, bound):
    """[N,3]: the gradient bound carried through the normalisation (module docstring: Normal)"""
    g = np.asarray(grad, np.float64)
    norm = np.sqrt((g * g).sum(1))
    safe = np.where(norm > 0, norm, 1.0)
    n = np.abs(g) / safe[:, None]
    first = (bound + n * (n * bound).sum(1, keepdims=True)) / safe[:, None]
    second = 2 * ((bound * bound).sum(1) / safe ** 2)[:, None]
    return np.where(norm[:, None] > 0, first + second + U * n, np.inf)


# ----------------------------------------------------------------------------------------------------------- projection
def project(net, planes, coords, iterations, step_max, max_move, tol, gmin):
    """the projection in float64 -> SimpleNamespace(x [N,3], z [N], normal [N,3], accepted [N], z_start [N])"""
    x0 = np.asarray(coords, np.float32).astype(np.float64)

    def field(x):
        r = field_grad(net, planes, x, fw=forward_at(net, planes, x))
        return r.logit, r.grad
    x = x0.copy()
    z, g = field(x)
    z_start = z.copy()
    scale = np.ones(len(x))
    accepted = np.zeros(len(x), np.int64)
    for _ in range(iterations):
        g2 = (g * g).sum(1)
        active = ~(np.abs(z) <= tol) & ~(g2 < gmin)
        d = (-scale * z / np.maximum(g2, gmin))[:, None] * g
        dn = np.sqrt((d * d).sum(1))
        d = d * np.where(dn > step_max, step_max / np.where(dn > 0, dn, 1.0), 1.0)[:, None]
        e = (x + d) - x0
        en = np.sqrt((e * e).sum(1))
        e = e * np.where(en > max_move, max_move / np.where(en > 0, en, 1.0), 1.0)[:, None]
        xt = np.where(active[:, None], x0 + e, x)
        zt, gt = field(xt)
        take = active & (np.abs(zt) < np.abs(z))
        x, z, g = np.where(take[:, None], xt, x), np.where(take, zt, z), np.where(take[:, None], gt, g)
        scale = np.where(take, 1.0, np.where(active, scale * 0.5, scale))
        accepted += take
    return SimpleNamespace(x=x, z=z, normal=normal_of(g, gmin), accepted=accepted, z_start=z_start)


def forward_at(net, planes, x64):
    """decoder_ref.forward from its own pieces at FLOAT64 coordinates (forward itself rounds its coordinates to fp32, which is
    right for a kernel's inputs and wrong for the float64 trajectory of the projection)"""
    planes = np.asarray(planes)
    S = planes.shape[1]
    P = planes.reshape(-1, 32).astype(np.float64)
    t = D.taps(np.asarray(x64, np.float64), S, np.float64)
    f, fabs, fp = D._gather(P, t)
    y = f @ net.B
    ang = D.TWO_PI * y
    s, c = np.sin(ang), np.cos(ang)
    x1 = np.concatenate([s, c], axis=1)
    pre1, h1, pre2, h2, z = D.mlp(net, x1)
    return SimpleNamespace(logit=z, f=f, fabs=fabs, fp=fp, y=y, ang=ang, sin=s, cos=c, x1=x1, pre1=pre1, h1=h1, pre2=pre2, h2=h2,
                           taps=t, P=P, S=S)


def sign_change_points(net, planes, res, count, seed):
    """`count` cell centres of a res^3 grid over [-1, 1]^3 whose cell's eight corner logits (float64) change sign"""
    axis = np.linspace(-1.0, 1.0, res).astype(np.float32)
    z = D.forward(net, planes, D.grid_coords(axis)).logit.reshape(res, res, res) > 0
    corners = [z[i:res - 1 + i, j:res - 1 + j, k:res - 1 + k] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    anyp, allp = np.logical_or.reduce(corners), np.logical_and.reduce(corners)
    cells = np.argwhere(anyp & ~allp)
    assert len(cells) >= count, f"only {len(cells)} sign-changing cells"
    pick = cells[np.random.RandomState(seed).permutation(len(cells))[:count]]
    a64 = axis.astype(np.float64)
    return ((a64[pick] + a64[pick + 1]) / 2).astype(np.float32)
