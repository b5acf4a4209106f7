"""GroupNorm32 (+ FiLM, SiLU, 2x2 mean pool) and its input gradient in float64, for tests/test_gpu_groupnorm_oracle.py.

Statement: y = act(film(GN(x))) as guided_diffusion defines it -- GroupNorm32 (32 groups, eps 1e-5, biased variance),
`h * (1 + scale) + shift`, SiLU, AvgPool2d(2) -- on the float64 values of the fp16 inputs, nothing rounded; the input gradient is
float64 autograd of that statement, composed with the pool / nearest upsample that GB_UNPOOL / GB_SUM4 stand for and with the
addends `add` (through the same resampling) and `add2` (at the map's own resolution).

Restatement: the same computation with the kernels' rounding points (csrc/gn_act.h, csrc/gn_bwd_terms.h): statistics cast to
fp32, fp16 after the affine, fp16(1 + fp16(scale)), fp16 product and fp16 sum in FiLM, fp16 output, fp16 pooled output; backward:
the recomputed fp16 pre-activation, the fp16 rounding in front of add2 and the fp16 result.

Bounds: one function per compared quantity, each a count of rounding points (derived in the docstring of
tests/test_gpu_groupnorm_oracle.py).  Tensors are NHWC, [N][H][W][C] float64, parameters [C], FiLM rows [N][C]."""
import torch

EPS = 1e-5
U = 2.0 ** -11            # fp16 rounding, relative
A = 2.0 ** -20            # fp32 arithmetic of a few operations, __expf, v_rcp_f32
SUB = 2.0 ** -25          # fp16 rounding, absolute (half a subnormal quantum)
SILU_D1 = 1.0998          # max |SiLU'|
SILU_D2 = 0.5             # max |SiLU''|


def f16r(t):
    return t.to(torch.float16).double()


def f32r(t):
    return t.to(torch.float32).double()


def silu(v):
    return v * torch.sigmoid(v)


def silu_grad(v):
    sg = torch.sigmoid(v)
    return sg * (1.0 + v * (1.0 - sg))


def pool2(t):
    n, h, w, c = t.shape
    return t.reshape(n, h // 2, 2, w // 2, 2, c).mean((2, 4))


def up2(t):
    return t.repeat_interleave(2, 1).repeat_interleave(2, 2)


def sum4(t):
    """[N][2H][2W][C] -> [N][H][W][C]: the four copies of a nearest upsample added"""
    n, h, w, c = t.shape
    return t.reshape(n, h // 2, 2, w // 2, 2, c).sum((2, 4))


def per_channel(v, C):
    """[N][32] group values -> [N][1][1][C]"""
    return v.repeat_interleave(C // 32, 1)[:, None, None, :]


def group_mean(t):
    """mean over a group's pixels and channels: [N][H][W][C] -> [N][32]"""
    n, h, w, c = t.shape
    return t.reshape(n, h * w, 32, c // 32).mean((1, 3))


def group_stats(x):
    """(mean, var, rstd) [N][32] in float64"""
    mean = group_mean(x)
    var = group_mean((x - per_channel(mean, x.shape[3])) ** 2)
    return mean, var, 1.0 / torch.sqrt(var + EPS)


def stats32(x):
    """the (mean, rstd) a kernel stores: float64 statistics cast to fp32 (as float64 tensors)"""
    mean, _, rstd = group_stats(x)
    return f32r(mean), f32r(rstd)


def _film_rows(emb, C):
    return emb[:, None, None, :C], emb[:, None, None, C:2 * C]


# ------------------------------------------------------------------------------------------------------------ forward
def forward_statement(x, gamma, beta, emb=None, film=False, act=True, pool=False, stats=None):
    """float64, nothing rounded; stats: (mean, rstd) [N][32] to use instead of x's own (constants)"""
    C = x.shape[3]
    if stats is None:
        mean, _, rstd = group_stats(x)
    else:
        mean, rstd = stats
    y = (x - per_channel(mean, C)) * per_channel(rstd, C) * gamma + beta
    if film:
        scale, shift = _film_rows(emb, C)
        y = y * (1.0 + scale) + shift
    if act:
        y = silu(y)
    return pool2(y) if pool else y


def forward_restatement(x, gamma, beta, emb=None, film=False, act=True, pool=False, stats=None, split=False):
    """with the kernels' rounding points; stats default to the fp32 casts of x's float64 statistics.  split: the head's form has no
    fp16 rounding point before the hi / lo split, and returns hi + lo"""
    C = x.shape[3]
    mean, rstd = stats32(x) if stats is None else stats
    pre = (x - per_channel(mean, C)) * per_channel(rstd, C) * gamma + beta
    if split:
        y = silu(pre) if act else pre
        hi = f16r(y)
        return hi + f16r(y - hi)
    pre = f16r(pre)
    if film:
        scale, shift = _film_rows(emb, C)
        sc = f16r(1.0 + f16r(scale))
        pre = f16r(f16r(pre * sc) + f16r(shift))
    y = f16r(silu(pre)) if act else pre
    return f16r(pool2(y)) if pool else y


def stats_error(mean, var, quantum=None):
    """(E_mean [N][32], E_rstd relative [N][32]): what a kernel's (mean, rstd) may differ from the float64 values by; quantum:
    (q_sum, q_sq) = the rounding of one group's sum / sum of squares over the element count, for fixed-point sums"""
    e_mean = 2.0 ** -23 * mean.abs() + 2.0 ** -24 * torch.sqrt(var)
    e_rstd = torch.full_like(mean, 2.0 ** -22)
    if quantum is not None:
        q_sum, q_sq = quantum
        e_mean = e_mean + q_sum
        e_rstd = e_rstd + 0.5 * (q_sq + 2.0 * mean.abs() * q_sum + q_sum * q_sum) / (var + EPS)
    return e_mean, e_rstd


def _xhat_error(x, mean, rstd, e_mean, e_rstd):
    C = x.shape[3]
    xhat = (x - per_channel(mean, C)) * per_channel(rstd, C)
    return xhat, per_channel(rstd * e_mean, C) + xhat.abs() * per_channel(e_rstd, C)


def pre_error(x, gamma, beta, emb, film, e_stats):
    """(pre, bound on the error of the kernel's fp16 pre-activation against the float64 one, xhat, dxhat)"""
    C = x.shape[3]
    mean, var, rstd = group_stats(x)
    xhat, dxhat = _xhat_error(x, mean, rstd, *e_stats)
    p = xhat * gamma + beta
    aff = A * (xhat.abs() * gamma.abs() + beta.abs()) + gamma.abs() * dxhat       # fp32 arithmetic and the statistics' own error
    if not film:
        return p, U * p.abs() + SUB + aff, xhat, dxhat
    scale, shift = _film_rows(emb, C)
    sc, sh = 1.0 + scale, shift
    pre = p * sc + sh
    # the affine's fp16 rounding and the rounding of sc = fp16(1 + fp16(scale)), each through the product; the fp16 product; the
    # fp16 sum; fp16(scale) and fp16(shift) themselves (zero for fp16 rows)
    err = (U * (2.0 * p.abs() * sc.abs() + (p * sc).abs() + pre.abs()) + 3.0 * SUB + aff * sc.abs() +
           p.abs() * (f16r(scale) - scale).abs() + (f16r(shift) - shift).abs())
    return pre, err, xhat, dxhat


def forward_bound(x, gamma, beta, emb=None, film=False, act=True, pool=False, e_stats=None, split=False):
    """element bound on |kernel - forward_statement|"""
    if e_stats is None:
        mean, var, _ = group_stats(x)
        e_stats = stats_error(mean, var)
    pre, err, _, _ = pre_error(x, gamma, beta, emb, film, e_stats)
    y = silu(pre) if act else pre
    sp = SILU_D1 if act else 1.0
    if split:           # no fp16 rounding point: the fp32 arithmetic, the statistics, and lo's own rounding (2^-22 relative)
        p_abs = (err - U * pre.abs() - SUB)
        return sp * p_abs + (2.0 * A + 2.0 ** -21) * y.abs() + SUB
    b = sp * err + (2.0 * A * y.abs() if act else 0.0)
    if not pool:
        return b + (U * y.abs() + SUB if act else 0.0)         # without SiLU the pre-activation IS the output: rounded once
    b = b + (U * y.abs() + SUB if act else 0.0)
    yp = pool2(y)
    return pool2(b) + U * yp.abs() + SUB + A * pool2(y.abs())


def pooled_input_bound(x):
    return U * pool2(x).abs() + 2.0 ** -22 * 4.0 * pool2(x.abs()) + SUB


def slab_sum(slices, bias=None, bias2=None, res=None):
    """(sum, sum of magnitudes) of pending slices [nslab][N][H][W][C] + bias + bias2 + res (res already at the map's resolution)"""
    s, a = slices.sum(0), slices.abs().sum(0)
    for t in (bias, bias2, res):
        if t is not None:
            s, a = s + t, a + t.abs()
    return s, a


def materialised_bound(s, a):
    return U * s.abs() + 2.0 ** -22 * a + SUB


def may_flip(s, a):
    """True where fp16(fp32 sum in slice order) may differ from fp16(s): s within 2^-22 a of a rounding boundary"""
    r = f16r(s)
    e = torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -14)))
    half_ulp = 2.0 ** (e - 11)
    return (half_ulp - (s - r).abs()) <= 2.0 ** -22 * a


# ------------------------------------------------------------------------------------------------------------ backward
GB_SAME, GB_UNPOOL, GB_SUM4 = 0, 1, 2


def resample(y, gmode):
    return y if gmode == GB_SAME else (pool2(y) if gmode == GB_UNPOOL else up2(y))


def upstream(g, gmode):
    """the gradient arriving at the map's own resolution"""
    return g if gmode == GB_SAME else (up2(g) * 0.25 if gmode == GB_UNPOOL else sum4(g))


def backward_statement(g, x, gamma, beta, emb=None, film=False, act=True, gmode=GB_SAME, add=None, add2=None):
    """float64 autograd: d/dx [ sum(g * R(y(x))) + sum(add * R(x)) + sum(add2 * x) ], R the pool / upsample gmode stands for"""
    xv = x.clone().requires_grad_(True)
    loss = (g * resample(forward_statement(xv, gamma, beta, emb, film, act), gmode)).sum()
    if add is not None:
        loss = loss + (add * resample(xv, gmode)).sum()
    if add2 is not None:
        loss = loss + (add2 * xv).sum()
    return torch.autograd.grad(loss, xv)[0]


def gn_bwd_ref(up, x, mu, rs, gam, bet, esc, esh, film, act):
    """gn_bwd_term (csrc/gn_bwd_terms.h) in float64 with its fp16 rounding points: gn_affine rounds the pre-activation, FiLM's
    scale is fp16(1 + fp16(scale)), its product and sum each round to fp16 (gn_film).  Returns dyh, xhat."""
    xhat = (x - mu) * rs
    u, mult = up, gam
    if film or act:
        pre = f16r(xhat * gam + bet)
        if film:
            sc = f16r(1.0 + f16r(esc))
            pre = f16r(f16r(pre * sc) + f16r(esh))
            mult = mult * sc
        if act:
            sg = torch.sigmoid(pre)
            u = u * (sg * (1.0 + pre * (1.0 - sg)))
    return u * mult, xhat


def backward_restatement(g, x, stats, gamma, beta, emb=None, film=False, act=True, gmode=GB_SAME, add=None, add2=None):
    """the kernels' computation on the given (mean, rstd) [N][32]: gn_bwd_term, the two group means, gn_bwd_dx, + add in fp32,
    fp16 in front of add2, fp16 result"""
    C = x.shape[3]
    mu, rs = per_channel(stats[0], C), per_channel(stats[1], C)
    esc, esh = _film_rows(emb, C) if film else (0.0, 0.0)
    dyh, xhat = gn_bwd_ref(upstream(g, gmode), x, mu, rs, gamma, beta, esc, esh, film, act)
    m1, m2 = per_channel(group_mean(dyh), C), per_channel(group_mean(dyh * xhat), C)
    v = rs * ((dyh - m1) - xhat * m2)
    if add is not None:
        v = v + upstream(add, gmode)
    if add2 is not None:
        v = f16r(v) + add2
    return f16r(v)


def backward_bound(g, x, gamma, beta, emb=None, film=False, act=True, gmode=GB_SAME, add=None, add2=None, quantum=0.0, dup=None,
                   e_stats=None):
    """element bound on |kernel - backward_statement| for a kernel that runs on the fp32 casts of the float64 statistics (e_stats:
    another bound on the statistics' error, for a pass chained on a forward kernel's own stats_out).
    quantum: rounding of one group mean formed from fixed-point channel sums; dup: bound on the error of the upstream value itself
    (a pending gradient whose fp32 slice sum may round to the neighbouring fp16 value)"""
    C = x.shape[3]
    M = lambda t: per_channel(group_mean(t), C)
    mean, var, rstd = group_stats(x)
    if e_stats is None:
        e_stats = (2.0 ** -24 * mean.abs(), torch.full_like(mean, 2.0 ** -24))     # the cast to fp32
    pre, err, xhat, dxhat = pre_error(x, gamma, beta, emb, film, e_stats)
    up = upstream(g, gmode)
    sc = (1.0 + _film_rows(emb, C)[0]) if film else 1.0
    mult = gamma * sc
    act_d = silu_grad(pre) if act else 1.0
    dyh = up * act_d * mult
    rs = per_channel(rstd, C)
    ax = xhat.abs()
    # eps_d: a one-ulp flip of the recomputed fp16 pre-activation (the FiLM roundings and the statistics' cast with it) through SiLU''
    eps_d = (up * mult).abs() * SILU_D2 * torch.maximum(2.0 * U * pre.abs(), err) if act else torch.zeros_like(x)
    if dup is not None:
        eps_d = eps_d + dup * (act_d * mult).abs()
    rel = A + (U if film else 0.0)                        # fp32 arithmetic; with FiLM mult carries sc = fp16(1 + fp16(scale))
    d = dyh.abs()
    b = rs * (eps_d + M(eps_d) + ax * M(eps_d * ax)) + rel * rs * (d + M(d) + ax * M(d * ax))
    b = b + rs * (dxhat * M(dyh * xhat).abs() + ax * M(d * dxhat))              # xhat's own error in the second group mean
    b = b + rs * (1.0 + ax) * quantum
    core = rs * ((dyh - M(dyh)) - xhat * M(dyh * xhat))
    if add is not None:
        core = core + upstream(add, gmode)
    if add2 is not None:
        b = b + U * core.abs() + SUB                      # the fp16 rounding in front of add2 (as a separate fp16 add of two maps)
        core = core + add2
    return b + U * core.abs() + SUB
