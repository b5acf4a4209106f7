"""The UNet (gd/unet.py:427-671, oracle/ref_cpu.UNetOracle) in float64, block by block, for tests/test_unet_ref_host.py,
tests/test_gpu_backward_blocks.py and tests/test_gpu_forward_blocks.py.  Tensors are NCHW float64; `emb` is the time embedding [N][4 * model_channels].

Statement: `UNetRef.block` / `.head` are the blocks as guided_diffusion defines them on float64 values, nothing rounded
(ref_cpu's `_gn` forces fp32; here GroupNorm is float64 too).  `block_vjp` / `head_vjp` are float64 autograd of ONE block at a
GIVEN input and a GIVEN incoming gradient, so an error found with them belongs to exactly that block.

Restatement: `block_vjp_manual(..., rnd=True)` is the same vector-Jacobian product written out by hand the way csrc/backward.hip
composes it, with `.half().double()` wherever the device keeps fp16:
  forward values the backward re-reads -- GroupNorm statistics cast to fp32; the fp16 pre-activation, FiLM with
    sc = fp16(1 + fp16(scale)) and an fp16 product and sum (groupnorm_ref.forward_restatement); the pooled activation; h1; each
    layer's output inside a block; the attention's normalised input, qkv and a, with exp(s - max) in fp16 under the P V product;
  gradient maps between launches -- dact (conv2's and qkv's input gradients), dh1, the conv1 input gradient, dxs (the 1x1 skip's),
    dA, dqkv (with dS and P in fp16 under dS k, dS^T q and P^T dA), and each layer's result, with the separate fp16 rounding in front of add2 (groupnorm_ref.backward_restatement);
  the head: the cotangent in fp16 and the head convolution's fp32 weight rounded to fp16 in the input-gradient operand (ConvW::wT
    is packed in fp16 for every convolution; only the forward operand of the head is hi/lo split).
With rnd=False the same code is the unrounded product (equal to autograd to 1e-12, asserted in the host test).
e_r(block) = |rounded - unrounded| / |unrounded| (relative L2) is the yardstick of the GPU test's bound; it is computed from
this file alone.

Mutations (`MUTATIONS`): switches of the hand-written product, each a mistake the composition in csrc/backward.hip could make.

The forward, block by block (tests/test_gpu_forward_blocks.py): `forward_positions` gives every block the pass's OWN output of the
block before it as input, `forward_position_errors` the statement (`block`, `head`), the restatement (`block(rnd=True)`: fp16
after every launch that stores fp16; `head_restatement`: fp32 statistics, no fp16 point, the hi/lo-split product) and e_r, for the
whole batch and per image.  `FORWARD_MUTATIONS` are switches (`mut=`, off by default) through emb, film_rows, resblock, attention,
block, head and forward_positions; `FORWARD_CONFIGS` adds forward-only configurations to CONFIGS' three; `forward_sites` lists
every GroupNorm forward and every convolution launch of a pass with the options csrc/unet.hip gives it."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from ishapediting_amd.unet_spec import build_spec

EPS = 1e-5
GB_SAME, GB_UNPOOL, GB_SUM4 = 0, 1, 2

MUTATIONS = (
    "skip_dropped",             # a ResBlock's skip-branch gradient (dy itself, or the 1x1 skip's dxs) never added
    "add2_dropped",             # the skip-connection gradient S owed to an input block never added
    "attn_residual_dropped",    # AttentionBlock: x + proj(a) differentiated without the x
    "unpool_one",               # GB_UNPOOL with factor 1 instead of 1/4
    "sum4_one_tap",             # GB_SUM4 reading one of the four taps
    "halves_swapped",           # d/d[h | skip]: the skip channels handed on as h and the reverse
    "split_shifted",            # d/d[h | skip] split 8 channels away from the seam
    "film_dropped",             # GroupNorm backward under FiLM without (1 + scale) in the upstream multiplier
    "skips_swapped",            # skip gradients popped in forward order: two input blocks of one shape get each other's
    "timestep_row",             # image 1 differentiated with the FiLM row of image 0
)

# Mistakes the FORWARD's composition (csrc/unet.hip) could make; switches `mut=` of emb / film_rows / resblock / attention / block /
# head and of forward_positions.  "The other image" of image n is n ^ 1 (other_image).
FORWARD_MUTATIONS = (
    "film_row",                 # a ResBlock reads the FiLM row of the other image
    "film_dropped",             # out_layers without h * (1 + scale) + shift
    "film_halves_swapped",      # (shift | scale) read where (scale | shift) is stored
    "emb_silu_dropped",         # emb_layers without its SiLU
    "temb_sincos_swapped",      # the timestep embedding as sin | cos instead of cos | sin
    "stats_other_image",        # every GroupNorm of the block normalises with the other image's (mean, rstd)
    "skip_identity_dropped",    # a ResBlock's xs (identity, pooled / upsampled x, or the 1x1 skip convolution) never added
    "pool_one_tap",             # a down ResBlock takes one pixel of four, on h and on xs
    "up_shifted",               # an up ResBlock's nearest upsampling shifted by one pixel, on h and on xs
    "attn_residual_dropped",    # AttentionBlock: proj(a) without the x
    "attn_heads_new_order",     # q | k | v taken as three contiguous thirds (QKVAttention) instead of per head (legacy)
    "attn_scale",               # scores times 1 / d instead of 1 / sqrt(d)
    "halves_swapped",           # an output block reads [skip | h]
    "seam_shifted",             # the skip half read 8 channels off
    "skips_swapped",            # hs popped out of order: the skip of another input block of the same shape
    "head_silu_dropped",        # the head's GroupNorm without its SiLU
    "head_lo_dropped",          # the head's convolution without the lo partial products: a plain fp16 head
)

ACC_REL = 2.0 ** -16            # tests/test_gpu_igemm_oracle.ACC_REL: fp32 accumulation, relative to the sum of magnitudes


def f16r(t):
    return t.to(torch.float16).double()


def _id(t):
    return t


def silu_grad(v):
    sg = torch.sigmoid(v)
    return sg * (1.0 + v * (1.0 - sg))


def _pc(v, C):
    """[N][32] group values -> [N][C][1][1]"""
    return v.repeat_interleave(C // 32, 1)[:, :, None, None]


def _gmean(t):
    """mean over a group's pixels and channels: [N][C][H][W] -> [N][32]"""
    n, c = t.shape[:2]
    return t.reshape(n, 32, -1).mean(2)


def group_stats(x, rnd):
    """(mean, rstd) [N][32]; rnd: cast to fp32 as the kernels store them"""
    mean = _gmean(x)
    var = _gmean((x - _pc(mean, x.shape[1])) ** 2)
    rstd = 1.0 / torch.sqrt(var + EPS)
    if rnd:
        mean, rstd = mean.float().double(), rstd.float().double()
    return mean, rstd


def pool2(t):
    return F.avg_pool2d(t, 2, 2)


def up2(t):
    return t.repeat_interleave(2, 2).repeat_interleave(2, 3)


def _upstream(g, gmode, mut):
    """the gradient arriving at the GroupNorm's own resolution"""
    if gmode == GB_SAME:
        return g
    if gmode == GB_UNPOOL:
        return up2(g) * (1.0 if mut == "unpool_one" else 0.25)
    if mut == "sum4_one_tap":
        return g[:, :, ::2, ::2]
    return pool2(g) * 4.0


def _film(emb_rows, C, rnd):
    """(sc, shift) [N][C][1][1]: sc = 1 + scale, on the device fp16(1 + fp16(scale))"""
    scale, shift = emb_rows[:, :C, None, None], emb_rows[:, C:2 * C, None, None]
    if rnd:
        return f16r(1.0 + f16r(scale)), f16r(shift)
    return 1.0 + scale, shift


def _gn_pre(x, stats, gamma, beta, emb_rows, film, rnd):
    """(xhat, the pre-activation the SiLU reads, sc)"""
    R = f16r if rnd else _id
    C = x.shape[1]
    xhat = (x - _pc(stats[0], C)) * _pc(stats[1], C)
    pre = R(xhat * gamma[None, :, None, None] + beta[None, :, None, None])
    sc = None
    if film:
        sc, sh = _film(emb_rows, C, rnd)
        pre = R(R(pre * sc) + sh)
    return xhat, pre, sc


def other_image(N):
    """index of the image a mutation confuses image n with: n ^ 1 (the last image of an odd batch: itself)"""
    idx = torch.arange(N) ^ 1
    return torch.where(idx < N, idx, torch.arange(N))


def gn_forward(x, gamma, beta, emb_rows=None, film=False, act=True, pool=False, rnd=False, mut=None):
    """act(film(GN(x))) (+ 2x2 mean pool); rnd: groupnorm_ref.forward_restatement's rounding points"""
    R = f16r if rnd else _id
    stats = group_stats(x, rnd)
    if mut == "stats_other_image":
        stats = tuple(s[other_image(x.shape[0])] for s in stats)
    _, pre, _ = _gn_pre(x, stats, gamma, beta, emb_rows, film, rnd)
    y = R(F.silu(pre)) if act else pre
    return R(pool2(y)) if pool else y


def gn_backward(g, x, gamma, beta, emb_rows=None, film=False, act=True, gmode=GB_SAME, add=None, add2=None, rnd=False, mut=None):
    """input gradient of act(film(GN(x))) composed with the resampling gmode stands for, + add through the same resampling, + add2 at
    x's resolution; rnd: groupnorm_ref.backward_restatement's rounding points (recomputed fp16 pre-activation, fp16 in front of
    add2, fp16 result)"""
    R = f16r if rnd else _id
    C = x.shape[1]
    stats = group_stats(x, rnd)
    xhat, pre, sc = _gn_pre(x, stats, gamma, beta, emb_rows, film, rnd)
    u = _upstream(g, gmode, mut)
    mult = gamma[None, :, None, None]
    if film and mut != "film_dropped":
        mult = mult * sc
    if act:
        u = u * silu_grad(pre)
    dyh = u * mult
    m1, m2 = _pc(_gmean(dyh), C), _pc(_gmean(dyh * xhat), C)
    v = _pc(stats[1], C) * ((dyh - m1) - xhat * m2)
    if add is not None:
        v = v + _upstream(add, gmode, mut)
    if add2 is not None:
        v = R(v) + add2
    return R(v)


def _conv(x, w, b, pad):
    return F.conv2d(x, w, b, padding=pad)


def _convT(g, w, pad):
    """input gradient of conv2d(., w, padding=pad)"""
    return F.conv_transpose2d(g, w, padding=pad)


Position = namedtuple("Position", "name kind blk x_in g_out add2 got")


def block_kind(blk):
    """a name for what the block is made of, e.g. 'res+skip1x1', 'res|attn|res:up', 'conv'"""
    parts = []
    for l in blk.layers:
        if l.kind == "res":
            parts.append("res" + (":up" if l.up else ":down" if l.down else "") + ("+skip1x1" if l.cin != l.cout else ""))
        else:
            parts.append(l.kind)
    return ("cat " if blk.skip_ch else "") + "|".join(parts)


class UNetRef:
    def __init__(self, cfg, sd):
        self.cfg = cfg
        self.spec = build_spec(cfg)
        self.w = {k: v.detach().double() for k, v in sd.items()}

    def p(self, name):
        return self.w[name]

    # ---------------------------------------------------------------------------------------------------- embeddings
    def emb(self, ts, mut=None):
        """gd/nn.py:102-120 (the sinusoid in fp32, as the reference and the device form it) and time_embed (gd/unet.py:651)"""
        dim = self.cfg.model_channels
        half = dim // 2
        freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
        args = torch.as_tensor(ts, dtype=torch.float32)[:, None] * freqs[None]
        parts = [torch.sin(args), torch.cos(args)] if mut == "temb_sincos_swapped" else [torch.cos(args), torch.sin(args)]
        e = torch.cat(parts, dim=-1).double()
        e = F.linear(e, self.p("time_embed.0.weight"), self.p("time_embed.0.bias"))
        return F.linear(F.silu(e), self.p("time_embed.2.weight"), self.p("time_embed.2.bias"))

    def film_rows(self, r, emb, mut=None):
        e = emb if mut == "emb_silu_dropped" else F.silu(emb)
        return F.linear(e, self.p(f"{r.path}.emb_layers.1.weight"), self.p(f"{r.path}.emb_layers.1.bias"))

    # ---------------------------------------------------------------------------------------------------- statement
    def resblock(self, r, x, emb, rnd=False, mut=None):
        R = f16r if rnd else _id
        P = r.path
        one_tap = r.down and mut == "pool_one_tap"
        h = gn_forward(x, self.p(f"{P}.in_layers.0.weight"), self.p(f"{P}.in_layers.0.bias"), pool=r.down and not one_tap, rnd=rnd,
                       mut=mut)
        xs = x
        if r.up:
            h, xs = up2(h), up2(x)
            if mut == "up_shifted":
                h, xs = torch.roll(h, 1, 3), torch.roll(xs, 1, 3)
        elif one_tap:
            h, xs = h[:, :, ::2, ::2], x[:, :, ::2, ::2]
        elif r.down:
            xs = R(pool2(x))
        h1 = R(_conv(h, self.p(f"{P}.in_layers.2.weight"), self.p(f"{P}.in_layers.2.bias"), 1))
        rows = self.film_rows(r, emb, mut)
        if mut == "film_row":
            rows = rows[other_image(rows.shape[0])]
        elif mut == "film_halves_swapped":
            rows = torch.cat([rows[:, r.cout:], rows[:, :r.cout]], dim=1)
        h = gn_forward(h1, self.p(f"{P}.out_layers.0.weight"), self.p(f"{P}.out_layers.0.bias"), rows, film=mut != "film_dropped",
                       rnd=rnd, mut=mut)
        h = _conv(h, self.p(f"{P}.out_layers.3.weight"), self.p(f"{P}.out_layers.3.bias"), 1)
        if r.cin != r.cout:
            xs = _conv(xs, self.p(f"{P}.skip_connection.weight"), self.p(f"{P}.skip_connection.bias"), 0)
        return R(h if mut == "skip_identity_dropped" else xs + h), h1

    def _attn_parts(self, a, x, rnd, mut=None):
        """(qkv [N][3C][T], q, k, v [N*heads][d][T], P [N*heads][T][T], a [N][C][T]); gd/unet.py:337-354, legacy head order"""
        R = f16r if rnd else _id
        P = a.path
        n, c, hh, ww = x.shape
        xn = gn_forward(x, self.p(f"{P}.norm.weight"), self.p(f"{P}.norm.bias"), act=False, rnd=rnd, mut=mut).reshape(n, c, -1)
        qkv = R(F.conv1d(xn, self.p(f"{P}.qkv.weight"), self.p(f"{P}.qkv.bias")))
        d = c // a.heads
        if mut == "attn_heads_new_order":       # QKVAttention (gd/unet.py:361-383): q | k | v as three contiguous thirds
            q, k, v = (t.reshape(n * a.heads, d, -1) for t in qkv.chunk(3, dim=1))
        else:
            q, k, v = qkv.reshape(n * a.heads, 3 * d, -1).split(d, dim=1)
        sc = torch.einsum("bct,bcs->bts", q, k) / (d if mut == "attn_scale" else math.sqrt(d))
        w = torch.softmax(sc, dim=-1)
        if rnd:         # the kernel's P V product takes exp(s - max) in fp16; the denominator sums the unrounded values
            pu = torch.exp(sc - sc.max(-1, keepdim=True).values)
            o = torch.einsum("bts,bcs->bct", f16r(pu), v) / pu.sum(-1)[:, None, :]
        else:
            o = torch.einsum("bts,bcs->bct", w, v)
        return qkv, q, k, v, w, R(o.reshape(n, c, -1))

    def attention(self, a, x, rnd=False, mut=None):
        R = f16r if rnd else _id
        n, c, hh, ww = x.shape
        o = self._attn_parts(a, x, rnd, mut)[5]
        o = F.conv1d(o, self.p(f"{a.path}.proj_out.weight"), self.p(f"{a.path}.proj_out.bias"))
        return R(o if mut == "attn_residual_dropped" else x.reshape(n, c, -1) + o).reshape(n, c, hh, ww)

    def layer(self, l, x, emb, rnd=False, mut=None):
        if l.kind == "conv":
            R = f16r if rnd else _id
            return R(_conv(x, self.p(f"{l.path}.weight"), self.p(f"{l.path}.bias"), 1))
        if l.kind == "res":
            return self.resblock(l, x, emb, rnd, mut)[0]
        return self.attention(l, x, rnd, mut)

    def block(self, blk, x, emb, rnd=False, mut=None):
        for l in blk.layers:
            x = self.layer(l, x, emb, rnd, mut)
        return x

    def head(self, h, mut=None):
        h = gn_forward(h, self.p("out.0.weight"), self.p("out.0.bias"), act=mut != "head_silu_dropped")
        return _conv(h, self.p("out.2.weight"), self.p("out.2.bias"), 1)

    def head_restatement(self, h, lo=True):
        """the head as the device forms it (csrc/unet.hip forward_head): GroupNorm + SiLU on fp32 statistics with no fp16 rounding
        point, the activation split into a_hi = fp16(a), a_lo = fp16(a - a_hi) (groupnorm_ref.forward_restatement(split=True)
        returns their sum), the fp32 weight into w_hi, w_lo alike (pack_conv_split_kernel), and three of the four partial products
        on the fp16 MFMA with fp32 accumulation: a_hi w_hi + a_lo w_hi + a_hi w_lo, + the fp32 bias.  lo=False drops the two `lo`
        products: a plain fp16 head."""
        from tests import groupnorm_ref as G
        a = G.forward_restatement(h.permute(0, 2, 3, 1), self.p("out.0.weight"), self.p("out.0.bias"), split=True).permute(0, 3, 1, 2)
        a_hi = f16r(a)
        a_lo = a - a_hi
        w = self.p("out.2.weight")
        w_hi = f16r(w)
        w_lo = f16r(w - w_hi)
        out = _conv(a_hi, w_hi, self.p("out.2.bias"), 1)
        if lo:
            out = out + _conv(a_lo, w_hi, None, 1) + _conv(a_hi, w_lo, None, 1)
        return out

    def head_bound(self, h, e_stats=None):
        """element bound on |device head - head(h)|: the GroupNorm oracle's bound of the split form, b_a, through the convolution's
        |w|, + the implicit-GEMM oracle's fp32 accumulation term ACC_REL * (conv(|a|, |w|) + |bias|)"""
        from tests import groupnorm_ref as G
        gam, bet = self.p("out.0.weight"), self.p("out.0.bias")
        b_a = G.forward_bound(h.permute(0, 2, 3, 1), gam, bet, split=True, e_stats=e_stats).permute(0, 3, 1, 2)
        a = gn_forward(h, gam, bet)
        w, b = self.p("out.2.weight").abs(), self.p("out.2.bias").abs()
        return _conv(b_a, w, None, 1) + ACC_REL * _conv(a.abs(), w, b, 1)

    def forward(self, x, ts, rnd=False):
        """(out, {(group, index): block output}); rnd: every block output (and x itself) as the device's fp16 torso holds it"""
        emb = self.emb(ts)
        acts = {}
        h = f16r(x) if rnd else x
        hs = []
        for i, blk in enumerate(self.spec.input_blocks):
            h = self.block(blk, h, emb, rnd)
            acts[(0, i)] = h
            hs.append(h)
        h = self.block(self.spec.middle_block, h, emb, rnd)
        acts[(1, 0)] = h
        for i, blk in enumerate(self.spec.output_blocks):
            h = self.block(blk, torch.cat([h, hs.pop()], dim=1), emb, rnd)
            acts[(2, i)] = h
        return self.head(h), acts

    # ---------------------------------------------------------------------------------------------------- autograd VJPs
    def block_vjp(self, blk, x_in, emb, g_out):
        """float64 autograd of one block at a given input and incoming gradient; an output block's result comes as its two halves"""
        xv = x_in.detach().clone().requires_grad_(True)
        (gx,) = torch.autograd.grad((self.block(blk, xv, emb.detach()) * g_out).sum(), xv)
        if blk.skip_ch:
            return gx[:, :blk.cin - blk.skip_ch], gx[:, blk.cin - blk.skip_ch:]
        return gx

    def head_vjp(self, h, cot):
        hv = h.detach().clone().requires_grad_(True)
        return torch.autograd.grad((self.head(hv) * cot).sum(), hv)[0]

    # ---------------------------------------------------------------------------------------------------- hand-written VJPs
    def _res_vjp(self, r, x, emb, dy, add2, rnd, mut):
        R = f16r if rnd else _id
        P = r.path
        n1w, n1b = self.p(f"{P}.in_layers.0.weight"), self.p(f"{P}.in_layers.0.bias")
        n2w, n2b = self.p(f"{P}.out_layers.0.weight"), self.p(f"{P}.out_layers.0.bias")
        rows = self.film_rows(r, emb)
        if mut == "timestep_row" and rows.shape[0] > 1:
            rows = torch.cat([rows[:1], rows[:1], rows[2:]])
        h1 = self.resblock(r, x, emb, rnd)[1]                       # what the forward saved (its own FiLM rows, never mutated)
        dact = R(_convT(dy, self.p(f"{P}.out_layers.3.weight"), 1))
        dh1 = gn_backward(dact, h1, n2w, n2b, rows, film=True, rnd=rnd, mut=mut)
        da = R(_convT(dh1, self.p(f"{P}.in_layers.2.weight"), 1))
        add = dy
        if r.cin != r.cout:
            add = R(_convT(dy, self.p(f"{P}.skip_connection.weight"), 0))
        if mut == "skip_dropped":
            add = None
        gmode = GB_UNPOOL if r.down else (GB_SUM4 if r.up else GB_SAME)
        return gn_backward(da, x, n1w, n1b, gmode=gmode, add=add, add2=add2, rnd=rnd, mut=mut)

    def _attn_vjp(self, a, x, dy, rnd, mut):
        R = f16r if rnd else _id
        P = a.path
        n, c, hh, ww = x.shape
        d = c // a.heads
        qkv, q, k, v, w, o = self._attn_parts(a, x, rnd)
        dA = R(torch.einsum("oc,not->nct", self.p(f"{P}.proj_out.weight")[:, :, 0], dy.reshape(n, c, -1)))
        dAh, oh = dA.reshape(n * a.heads, d, -1), o.reshape(n * a.heads, d, -1)
        D = (dAh * oh).sum(1)                                          # [B][T], from the stored (fp16) a as the kernel forms it
        dP = torch.einsum("bct,bcs->bts", dAh, v)
        dS = R(w * (dP - D[:, :, None]) / math.sqrt(d))                # dS and P are fp16 operands of the second products
        dq = torch.einsum("bts,bcs->bct", dS, k)
        dk = torch.einsum("bts,bct->bcs", dS, q)
        dv = torch.einsum("bts,bct->bcs", R(w), dAh)
        dqkv = R(torch.cat([dq, dk, dv], dim=1).reshape(n, 3 * c, -1))
        dact = R(torch.einsum("oc,not->nct", self.p(f"{P}.qkv.weight")[:, :, 0], dqkv)).reshape(n, c, hh, ww)
        return gn_backward(dact, x, self.p(f"{P}.norm.weight"), self.p(f"{P}.norm.bias"), act=False,
                           add=None if mut == "attn_residual_dropped" else dy, rnd=rnd)

    def block_vjp_manual(self, blk, x_in, emb, g_out, add2=None, rnd=True, mut=None):
        """the block's VJP as csrc/backward.hip composes it (+ add2, the skip gradient owed to the block's input); rnd: with the
        device's fp16 rounding points; mut: one of MUTATIONS.  An output block's result comes as its two halves."""
        R = f16r if rnd else _id
        xs = [x_in]
        for l in blk.layers[:-1]:
            xs.append(self.layer(l, xs[-1], emb, rnd))
        g = g_out
        for i in range(len(blk.layers) - 1, -1, -1):
            l = blk.layers[i]
            if l.kind == "conv":
                g = R(_convT(g, self.p(f"{l.path}.weight"), 1))
            elif l.kind == "res":
                g = self._res_vjp(l, xs[i], emb, g, add2 if (i == 0 and mut != "add2_dropped") else None, rnd, mut)
            else:
                g = self._attn_vjp(l, xs[i], g, rnd, mut)
        assert blk.layers[0].kind == "res" or add2 is None, "only a ResBlock takes the owed skip gradient"
        if not blk.skip_ch:
            return g
        ch = blk.cin - blk.skip_ch
        if mut == "halves_swapped":
            g = torch.roll(g, -ch, 1)
        elif mut == "split_shifted":
            g = torch.roll(g, -8, 1)
        return g[:, :ch], g[:, ch:]

    def head_vjp_manual(self, h, cot, rnd=True):
        R = f16r if rnd else _id
        dact = R(_convT(R(cot), R(self.p("out.2.weight")), 1))
        return gn_backward(dact, h, self.p("out.0.weight"), self.p("out.0.bias"), rnd=rnd)

    # ---------------------------------------------------------------------------------------------------- the composition
    def skip_source(self, j, F_):
        """the output block whose part 2 is S(j), the skip gradient of input block j, or None when the backward started below it"""
        i = len(self.spec.input_blocks) - 1 - j
        return i if i <= F_ else None

    def swap_partner(self, j, F_):
        """for 'skips_swapped': a neighbouring input block whose output has the shape of block j's and whose S exists too"""
        ib = self.spec.input_blocks
        for k in (j ^ 1, j + 1, j - 1):
            if 0 <= k < len(ib) and k != j and (ib[k].cout, ib[k].res_out) == (ib[j].cout, ib[j].res_out) and \
                    self.skip_source(k, F_) is not None and self.skip_source(j, F_) is not None:
                return k
        return None

    def positions(self, x, acts, grads, F_, full, cot=None, dx=None):
        """Every identity of the backward's composition as a Position (name, kind, block, input, incoming gradient, owed addend,
        what the pass produced).  acts: {(group, index): block output}; grads: {(group, index, part): gradient map}; x: the fp16
        values of the network input; F_: the output block the pass started from; full: it started from the model output (cot)."""
        sp = self.spec
        n_in = len(sp.input_blocks)
        S = lambda j: None if self.skip_source(j, F_) is None else grads[(2, self.skip_source(j, F_), 2)]
        pos = []
        if full:
            pos.append(Position("head", "head", None, acts[(2, F_)], cot, None, grads[(2, F_, 0)]))
        for i in range(F_, -1, -1):
            blk = sp.output_blocks[i]
            h = acts[(2, i - 1)] if i else acts[(1, 0)]
            pos.append(Position(blk.name, block_kind(blk), blk, torch.cat([h, acts[(0, n_in - 1 - i)]], dim=1), grads[(2, i, 0)], None,
                                (grads[(2, i, 1)], grads[(2, i, 2)])))
        pos.append(Position(sp.middle_block.name, block_kind(sp.middle_block), sp.middle_block, acts[(0, n_in - 1)], grads[(1, 0, 0)],
                            S(n_in - 1), grads[(0, n_in - 1, 0)]))
        for i in range(n_in - 1, 0, -1):
            blk = sp.input_blocks[i]
            pos.append(Position(blk.name, block_kind(blk), blk, acts[(0, i - 1)], grads[(0, i, 0)], S(i - 1), grads[(0, i - 1, 0)]))
        pos.append(Position(sp.input_blocks[0].name, "conv", sp.input_blocks[0], x, grads[(0, 0, 0)], None, dx))
        return pos

    def position_vjp(self, pos, emb, rnd, mut=None):
        """the right-hand side of a position's identity: statement (rnd False) or restatement, as a tuple of tensors"""
        if pos.blk is None:
            return (self.head_vjp_manual(pos.x_in, pos.g_out, rnd),)
        r = self.block_vjp_manual(pos.blk, pos.x_in, emb, pos.g_out, pos.add2, rnd, mut)
        return r if isinstance(r, tuple) else (r,)

    def position_autograd(self, pos, emb):
        """the same right-hand side by autograd of the statement (+ the owed addend)"""
        if pos.blk is None:
            return (self.head_vjp(pos.x_in, pos.g_out),)
        r = self.block_vjp(pos.blk, pos.x_in, emb, pos.g_out)
        if isinstance(r, tuple):
            return r
        return (r if pos.add2 is None else r + pos.add2,)

    def applies(self, mut, pos, N, F_):
        """does the mutation change anything at this position"""
        if pos.blk is None or pos.kind == "conv":
            return False
        res = [l for l in pos.blk.layers if l.kind == "res"]
        if mut in ("skip_dropped", "film_dropped"):
            return bool(res)
        if mut == "timestep_row":
            return bool(res) and N > 1
        if mut == "add2_dropped":
            return pos.add2 is not None
        if mut == "attn_residual_dropped":
            return any(l.kind == "attn" for l in pos.blk.layers)
        if mut == "unpool_one":
            return any(l.down for l in res)
        if mut == "sum4_one_tap":
            return any(l.up for l in res)
        if mut in ("halves_swapped", "split_shifted"):
            return bool(pos.blk.skip_ch)
        return False            # skips_swapped is a mutation of the addend, not of the block (see simulate / the host test)

    def simulate(self, x, ts, F_, full, cot):
        """the device's pass on the CPU: the rounded forward, then the rounded hand-written backward chained through the whole
        network from output block F_ (or from the head with the output cotangent).  Returns (acts, grads, dx, x16): inputs at
        which the host tests evaluate statement, restatement and mutations, of the magnitudes the device sees."""
        sp = self.spec
        emb = self.emb(ts)
        x16 = f16r(x)
        _, acts = self.forward(x, ts, rnd=True)
        n_in = len(sp.input_blocks)
        grads = {}
        g = f16r(cot)
        if full:
            g = self.head_vjp_manual(acts[(2, F_)], g)
        skip = {}
        for i in range(F_, -1, -1):
            blk = sp.output_blocks[i]
            h = acts[(2, i - 1)] if i else acts[(1, 0)]
            grads[(2, i, 0)] = g
            gh, gs = self.block_vjp_manual(blk, torch.cat([h, acts[(0, n_in - 1 - i)]], dim=1), emb, g)
            grads[(2, i, 1)], grads[(2, i, 2)] = gh, gs
            skip[n_in - 1 - i] = gs
            g = gh
        grads[(1, 0, 0)] = g
        g = self.block_vjp_manual(sp.middle_block, acts[(0, n_in - 1)], emb, g, skip.get(n_in - 1))
        for i in range(n_in - 1, 0, -1):
            grads[(0, i, 0)] = g
            g = self.block_vjp_manual(sp.input_blocks[i], acts[(0, i - 1)], emb, g, skip.get(i - 1))
        grads[(0, 0, 0)] = g
        dx = self.block_vjp_manual(sp.input_blocks[0], x16, emb, g)
        return acts, grads, dx, x16

    # ---------------------------------------------------------------------------------------------------- the forward's composition
    def forward_swap_partner(self, j):
        """for 'skips_swapped': another input block whose output has the shape of block j's"""
        ib = self.spec.input_blocks
        for k in (j ^ 1, j + 1, j - 1):
            if 0 <= k < len(ib) and k != j and (ib[k].cout, ib[k].res_out) == (ib[j].cout, ib[j].res_out):
                return k
        return None

    def forward_positions(self, x16, acts, out, mut=None):
        """One FPosition (name, kind, block, input, what the pass produced) per block of the forward, the input taken from the
        pass's OWN block outputs so that nothing is chained.  x16: the fp16 values of the network input; acts: {(group, index):
        block output}; out: the model output.  mut: the mistakes of the concatenation ('halves_swapped', 'seam_shifted',
        'skips_swapped') change the input an output block is given; every other value leaves the positions as they are."""
        sp = self.spec
        ib = sp.input_blocks
        n_in = len(ib)
        pos = [FPosition(ib[0].name, "conv", ib[0], x16, acts[(0, 0)])]
        for i in range(1, n_in):
            pos.append(FPosition(ib[i].name, block_kind(ib[i]), ib[i], acts[(0, i - 1)], acts[(0, i)]))
        pos.append(FPosition(sp.middle_block.name, block_kind(sp.middle_block), sp.middle_block, acts[(0, n_in - 1)], acts[(1, 0)]))
        for i, blk in enumerate(sp.output_blocks):
            h = acts[(2, i - 1)] if i else acts[(1, 0)]
            j = n_in - 1 - i
            skip = acts[(0, j)]
            if mut == "skips_swapped" and self.forward_swap_partner(j) is not None:
                skip = acts[(0, self.forward_swap_partner(j))]
            elif mut == "seam_shifted":
                skip = torch.roll(skip, -8, 1)
            x = torch.cat([skip, h] if mut == "halves_swapped" else [h, skip], dim=1)
            pos.append(FPosition(blk.name, block_kind(blk), blk, x, acts[(2, i)]))
        pos.append(FPosition("head", "head", None, acts[(2, len(sp.output_blocks) - 1)], out))
        return pos

    def position_forward(self, pos, emb, rnd, mut=None):
        """the block of a position at its input: statement (rnd False) or restatement; mut: one of FORWARD_MUTATIONS (the
        concatenation's are in the position's input already, 'temb_sincos_swapped' in emb = self.emb(ts, mut))"""
        if pos.blk is None:
            if mut == "head_lo_dropped":
                return self.head_restatement(pos.x_in, lo=False)
            return self.head_restatement(pos.x_in) if rnd else self.head(pos.x_in, mut)
        return self.block(pos.blk, pos.x_in, emb, rnd, mut)

    def forward_applies(self, mut, pos, N):
        """does the forward mutation change anything at this position"""
        if pos.blk is None:
            return mut in ("head_silu_dropped", "head_lo_dropped")
        if pos.kind == "conv":
            return False
        res = [l for l in pos.blk.layers if l.kind == "res"]
        if mut in ("film_dropped", "film_halves_swapped", "emb_silu_dropped", "temb_sincos_swapped", "skip_identity_dropped"):
            return bool(res)
        if mut == "film_row":
            return bool(res) and N > 1
        if mut == "stats_other_image":
            return N > 1
        if mut == "pool_one_tap":
            return any(l.down for l in res)
        if mut == "up_shifted":
            return any(l.up for l in res)
        if mut == "attn_heads_new_order":               # with one head the two orders are the same
            return any(l.kind == "attn" and l.heads > 1 for l in pos.blk.layers)
        if mut in ("attn_residual_dropped", "attn_scale"):
            return any(l.kind == "attn" for l in pos.blk.layers)
        if mut in ("halves_swapped", "seam_shifted"):
            return bool(pos.blk.skip_ch)
        if mut == "skips_swapped":
            ob = self.spec.output_blocks
            return bool(pos.blk.skip_ch) and self.forward_swap_partner(len(self.spec.input_blocks) - 1 - ob.index(pos.blk)) is not None
        return False


def rel_l2(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


def gn_backward_sites(spec):
    """[(HW of the GroupNorm's input, C, gmode, film, act, what)] of every GroupNorm backward of a full-depth pass, in the order
    csrc/backward.hip meets them"""
    sites = []
    S = spec.cfg.image_size
    sites.append((S * S, spec.final_ch, GB_SAME, 0, 1, "head"))

    def walk(blk):
        res = blk.res_out
        for l in reversed(blk.layers):
            if l.kind == "res":
                res_x = res // 2 if l.up else (res * 2 if l.down else res)
                sites.append((res * res, l.cout, GB_SAME, 1, 1, f"{l.path} out_layers"))
                sites.append((res_x * res_x, l.cin, GB_UNPOOL if l.down else (GB_SUM4 if l.up else GB_SAME), 0, 1, f"{l.path} in_layers"))
                res = res_x
            elif l.kind == "attn":
                sites.append((res * res, l.channels, GB_SAME, 0, 0, f"{l.path} norm"))
        assert res == blk.res_in, blk.name

    for blk in reversed(spec.output_blocks):
        walk(blk)
    walk(spec.middle_block)
    for blk in reversed(spec.input_blocks):
        walk(blk)
    return sites


# ------------------------------------------------------------------------------------------------------------ configurations
def cfg_top():
    """A, "top": 128^2 and 64^2 maps, 64 channels, no attention level reached (the middle block's own attention runs on the 64^2
    map): every GroupNorm backward takes a full-map route"""
    from ishapediting_amd.unet_spec import UNetConfig
    return UNetConfig(image_size=128, in_channels=6, model_channels=64, out_channels=12, num_res_blocks=1,
                      attention_resolutions="8", channel_mult=(1, 1), num_head_channels=64)


def cfg_deep():
    """B, "deep": tests/test_gpu_chains._cfg_mid -- 32^2 / 16^2 / 8^2 maps, 64 / 128 / 256 channels, attention at 16 and 8: every
    GroupNorm backward is group-local, the 256-channel layers leave pending split-K gradients"""
    from ishapediting_amd.unet_spec import UNetConfig
    return UNetConfig(image_size=32, in_channels=6, model_channels=64, out_channels=12, num_res_blocks=1,
                      attention_resolutions="16,8", channel_mult=(1, 2, 4), num_head_channels=64)


def cfg_tiny2():
    """C: tiny_config(2) -- 32 channels (one per group), the 96-channel concatenation, two ResBlocks per level"""
    from ishapediting_amd.unet_spec import tiny_config
    return tiny_config(2)


# name -> (config, weight seed, N, timesteps, [pass: an output block to start from, or "out" for the full depth])
CONFIGS = {
    "top": (cfg_top, 311, 1, [617.0], ["last", "out"]),
    "deep": (cfg_deep, 91, 2, [617.0, 23.0], [2, "out"]),
    "tiny2": (cfg_tiny2, 102, 2, [617.0, 23.0], [1]),
}


def make_inputs(name, start):
    """(cfg, state_dict, x, ts, F, full, cot) of one pass: x = randn, cot = 0.1 randn in the shape of the tapped block's output
    (or of the model output), from a generator seeded by the configuration"""
    from ishapediting_amd import synthetic
    fn, seed, N, ts, _ = CONFIGS[name]
    cfg = fn()
    spec = build_spec(cfg)
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(cfg, seed))
    g = torch.Generator().manual_seed(seed + 1000)
    x = torch.randn(N, cfg.in_channels, cfg.image_size, cfg.image_size, generator=g).double()       # fp32 values: what a device gets
    n_out = len(spec.output_blocks)
    full = start == "out"
    F_ = n_out - 1 if start in ("out", "last") else int(start)
    if full:
        shape = (N, cfg.out_channels, cfg.image_size, cfg.image_size)
    else:
        shape = (N, spec.output_blocks[F_].cout, spec.output_blocks[F_].res_out, spec.output_blocks[F_].res_out)
    cot = (0.1 * torch.randn(shape, generator=g)).double()
    return cfg, sd, x, ts, F_, full, cot


def position_errors(ref, pos, emb):
    """(statement, e_r per part, error of pos.got per part, distance of pos.got from the ROUNDED product per part): relative L2, all
    in units of the unrounded product's norm"""
    st = ref.position_vjp(pos, emb, rnd=False)
    rs = ref.position_vjp(pos, emb, rnd=True)
    got = pos.got if isinstance(pos.got, tuple) else (pos.got,)
    return (st, [rel_l2(r, s) for r, s in zip(rs, st)], [rel_l2(g, s) for g, s in zip(got, st)],
            [float((g - r).norm() / s.norm()) for g, r, s in zip(got, rs, st)])


# ------------------------------------------------------------------------------------------------------------ the forward, block by block
FPosition = namedtuple("FPosition", "name kind blk x_in got")

# Forward-only configurations: name -> (config, weight seed, N, timesteps).  CONFIGS' three (at their own N and timesteps), and
#   top2   cfg_top, N = 2 at timesteps 617 and 23: the full-map routes with two images -- a statistic from a convolution's epilogue
#          or a FiLM row filed under the wrong image has nowhere to show in `top` (N = 1);
#   deep8  cfg_deep, N = 8 at eight distinct timesteps: the batched tile forms (M = 8 H W) and, with 8 * 4 heads * 12 parts above
#          the 256 compute units attn8_applicable allows, the UNFUSED attention on the 8x8 map (qkv GEMM, attention kernel at T = 64,
#          proj_out left pending), which no batch below 6 reaches with these channels.
#   wide   16^2 / 8^2 maps, 96 / 288 channels (no multiple of 64), heads of 32 channels, N = 2: the one forward form the others (and
#          full_config) never launch -- a convolution whose K split is reduced IN PLACE (conv2 of a 96 -> 288 ResBlock behind a
#          separately launched 1x1 skip, K = 2592; the head at K = 3 * 288 * 9), three and nine channels per GroupNorm group.
def cfg_wide():
    from ishapediting_amd.unet_spec import UNetConfig
    return UNetConfig(image_size=16, in_channels=6, model_channels=96, out_channels=12, num_res_blocks=1,
                      attention_resolutions="2", channel_mult=(1, 3), num_head_channels=32)


FORWARD_CONFIGS = {name: (fn, seed, N, ts) for name, (fn, seed, N, ts, _) in CONFIGS.items()}
FORWARD_CONFIGS["top2"] = (cfg_top, 311, 2, [617.0, 23.0])
FORWARD_CONFIGS["deep8"] = (cfg_deep, 91, 8, [617.0, 23.0, 981.0, 2.0, 333.0, 150.0, 760.0, 499.0])
FORWARD_CONFIGS["wide"] = (cfg_wide, 77, 2, [617.0, 23.0])


def make_forward_inputs(name):
    """(cfg, state_dict, x, ts) of one forward: x = randn from a generator seeded by the configuration (for CONFIGS' three, the x
    of make_inputs).  In the forward-only configurations image n is scaled by IMAGE_SCALES[n]: randn images of one size have nearly
    the same GroupNorm statistics (at 128^2 the other image's statistics moved the first ResBlock by 4 bounds only), and a statistic
    filed under the wrong image should be as visible as a wrong FiLM row."""
    from ishapediting_amd import synthetic
    fn, seed, N, ts = FORWARD_CONFIGS[name]
    cfg = fn()
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(cfg, seed))
    g = torch.Generator().manual_seed(seed + 1000)
    x = torch.randn(N, cfg.in_channels, cfg.image_size, cfg.image_size, generator=g)
    if name not in CONFIGS:
        x = x * torch.tensor(IMAGE_SCALES[:N])[:, None, None, None]
    return cfg, sd, x.double(), ts


IMAGE_SCALES = [1.0, 0.6, 1.4, 0.8, 1.2, 0.5, 0.9, 1.3]


def rel_l2_images(a, b, scale=None):
    """|a - b| / |scale| per image (scale: b)"""
    scale = b if scale is None else scale
    n = a.shape[0]
    return ((a - b).reshape(n, -1).norm(dim=1) / (scale.reshape(n, -1).norm(dim=1) + 1e-300)).tolist()


def forward_position_errors(ref, pos, emb, cache=None):
    """(statement, e_r, error of pos.got, distance of pos.got from the ROUNDED restatement): relative L2 in units of the statement's
    norm; each of the last three as (whole batch, [per image]) -- per image in units of that image's own statement, so that an error
    confined to one image of N is not diluted by the others.  cache: a dict that keeps (input, statement, restatement) per position
    name; a later pass whose input at that position has the same bits (another mode of the same forward) reuses them."""
    hit = cache.get(pos.name) if cache is not None else None
    if hit is not None and torch.equal(hit[0], pos.x_in):
        st, rs = hit[1], hit[2]
    else:
        st = ref.position_forward(pos, emb, rnd=False)
        rs = ref.position_forward(pos, emb, rnd=True)
        if cache is not None:
            cache[pos.name] = (pos.x_in, st, rs)
    both = lambda a, b: (float((a - b).norm() / st.norm()), rel_l2_images(a, b, st))
    return st, both(rs, st), both(pos.got, st), both(pos.got, rs)


GnSite = namedtuple("GnSite", "HW C film act pool split pending what")
ConvSite = namedtuple("ConvSite", "M cin cout taps K2 ups H W pending sums what")


def forward_sites(spec, N):
    """([GnSite], [ConvSite]): every GroupNorm forward and every convolution launch of a forward pass, in the order csrc/unet.hip
    meets them, with the options the executor gives each (res_forward, attn_forward, forward_head).  A map of at most 1024 pixels
    is a 'small map': its convolutions gather no statistics (sums 0) and a block's last convolution, conv1 in front of a
    group-local GroupNorm and proj_out ASK to leave their split-K slices pending (pending 1; whether there is a split is the
    planner's answer).  GnSite.pending: the producer was asked so.  cin is the padded K per tap (round_up(cin, 32); the stem's
    in_pad; the head's 3 * C of the hi | lo | hi split); K2 the columns of a 1x1 skip folded into conv2's launch.  The fused 8x8
    attention (one launch for qkv, attention and proj_out) is listed as no convolution; it applies while N * heads * 12 <= 256."""
    cfg = spec.cfg
    ru = lambda a, b: (a + b - 1) // b * b
    small = lambda hw: hw <= 1024
    gns, convs = [], []
    S = cfg.image_size
    in_pad = ru(cfg.in_channels, 64) if cfg.in_channels >= 64 else ru(cfg.in_channels, 32)

    def walk(blk, pend):
        res = blk.res_in
        for l in blk.layers:
            if l.kind == "conv":
                convs.append(ConvSite(N * res * res, in_pad, l.cout, 9, 0, 0, res, res, 0, int(not small(res * res)), l.path))
                pend = 0
            elif l.kind == "res":
                ro = res // 2 if l.down else (res * 2 if l.up else res)
                sm = small(ro * ro)
                gns.append(GnSite(res * res, l.cin, 0, 1, int(l.down), 0, pend, f"{l.path} in_layers"))
                convs.append(ConvSite(N * ro * ro, ru(l.cin, 32), l.cout, 9, 0, int(l.up), ro, ro, int(sm), int(not sm), f"{l.path} conv1"))
                gns.append(GnSite(ro * ro, l.cout, 1, 1, 0, 0, int(sm), f"{l.path} out_layers"))
                skip, k2 = l.cin != l.cout, 0
                folded = skip and not l.down and not l.up and ru(l.cout, 32) % 64 == 0 and ru(l.cin, 32) % 64 == 0
                if folded:
                    k2 = ru(l.cin, 32)
                elif skip:
                    convs.append(ConvSite(N * ro * ro, ru(l.cin, 32), l.cout, 1, 0, 0, ro, ro, 0, 0, f"{l.path} skip"))
                pend = int(sm and (folded or not skip))
                convs.append(ConvSite(N * ro * ro, ru(l.cout, 32), l.cout, 9, k2, 0, ro, ro, pend, int(not sm), f"{l.path} conv2"))
                res = ro
            else:
                T, C = res * res, l.channels
                gns.append(GnSite(T, C, 0, 0, 0, 0, pend, f"{l.path} norm"))
                fused = T == 64 and C // l.heads == 64 and C % 64 == 0 and C // 16 <= 72 and N * l.heads * 12 <= 256
                if not fused:
                    convs.append(ConvSite(N * T, C, 3 * C, 1, 0, 0, res, res, 0, 0, f"{l.path} qkv"))
                    convs.append(ConvSite(N * T, C, C, 1, 0, 0, res, res, int(small(T)), int(not small(T)), f"{l.path} proj_out"))
                pend = int(small(T))
        assert res == blk.res_out, blk.name
        return pend

    pend = 0
    for blk in spec.input_blocks:
        pend = walk(blk, pend)
    pend = walk(spec.middle_block, pend)
    for blk in spec.output_blocks:
        pend = walk(blk, pend)
    gns.append(GnSite(S * S, spec.final_ch, 0, 1, 0, 1, 0, "head"))
    convs.append(ConvSite(N * S * S, 3 * spec.final_ch, cfg.out_channels, 9, 0, 0, S, S, 0, 0, "head"))
    return gns, convs
