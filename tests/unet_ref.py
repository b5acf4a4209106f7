"""The UNet (gd/unet.py:427-671, oracle/ref_cpu.UNetOracle) in float64, block by block, for tests/test_unet_ref_host.py and
tests/test_gpu_backward_blocks.py.  Tensors are NCHW float64; `emb` is the time embedding [N][4 * model_channels].

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

Mutations (`MUTATIONS`): switches of the hand-written product, each a mistake the composition in csrc/backward.hip could make."""
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


def gn_forward(x, gamma, beta, emb_rows=None, film=False, act=True, pool=False, rnd=False):
    """act(film(GN(x))) (+ 2x2 mean pool); rnd: groupnorm_ref.forward_restatement's rounding points"""
    R = f16r if rnd else _id
    _, pre, _ = _gn_pre(x, group_stats(x, rnd), gamma, beta, emb_rows, film, rnd)
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
    def emb(self, ts):
        """gd/nn.py:102-120 (the sinusoid in fp32, as the reference and the device form it) and time_embed (gd/unet.py:651)"""
        dim = self.cfg.model_channels
        half = dim // 2
        freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
        args = torch.as_tensor(ts, dtype=torch.float32)[:, None] * freqs[None]
        e = torch.cat([torch.cos(args), torch.sin(args)], dim=-1).double()
        e = F.linear(e, self.p("time_embed.0.weight"), self.p("time_embed.0.bias"))
        return F.linear(F.silu(e), self.p("time_embed.2.weight"), self.p("time_embed.2.bias"))

    def film_rows(self, r, emb):
        return F.linear(F.silu(emb), self.p(f"{r.path}.emb_layers.1.weight"), self.p(f"{r.path}.emb_layers.1.bias"))

    # ---------------------------------------------------------------------------------------------------- statement
    def resblock(self, r, x, emb, rnd=False):
        R = f16r if rnd else _id
        P = r.path
        h = gn_forward(x, self.p(f"{P}.in_layers.0.weight"), self.p(f"{P}.in_layers.0.bias"), pool=r.down, rnd=rnd)
        xs = x
        if r.up:
            h, xs = up2(h), up2(x)
        elif r.down:
            xs = R(pool2(x))
        h1 = R(_conv(h, self.p(f"{P}.in_layers.2.weight"), self.p(f"{P}.in_layers.2.bias"), 1))
        h = gn_forward(h1, self.p(f"{P}.out_layers.0.weight"), self.p(f"{P}.out_layers.0.bias"), self.film_rows(r, emb), film=True,
                       rnd=rnd)
        h = _conv(h, self.p(f"{P}.out_layers.3.weight"), self.p(f"{P}.out_layers.3.bias"), 1)
        if r.cin != r.cout:
            xs = _conv(xs, self.p(f"{P}.skip_connection.weight"), self.p(f"{P}.skip_connection.bias"), 0)
        return R(xs + h), h1

    def _attn_parts(self, a, x, rnd):
        """(qkv [N][3C][T], q, k, v [N*heads][d][T], P [N*heads][T][T], a [N][C][T]); gd/unet.py:337-354, legacy head order"""
        R = f16r if rnd else _id
        P = a.path
        n, c, hh, ww = x.shape
        xn = gn_forward(x, self.p(f"{P}.norm.weight"), self.p(f"{P}.norm.bias"), act=False, rnd=rnd).reshape(n, c, -1)
        qkv = R(F.conv1d(xn, self.p(f"{P}.qkv.weight"), self.p(f"{P}.qkv.bias")))
        d = c // a.heads
        q, k, v = qkv.reshape(n * a.heads, 3 * d, -1).split(d, dim=1)
        sc = torch.einsum("bct,bcs->bts", q, k) / math.sqrt(d)
        w = torch.softmax(sc, dim=-1)
        if rnd:         # the kernel's P V product takes exp(s - max) in fp16; the denominator sums the unrounded values
            pu = torch.exp(sc - sc.max(-1, keepdim=True).values)
            o = torch.einsum("bts,bcs->bct", f16r(pu), v) / pu.sum(-1)[:, None, :]
        else:
            o = torch.einsum("bts,bcs->bct", w, v)
        return qkv, q, k, v, w, R(o.reshape(n, c, -1))

    def attention(self, a, x, rnd=False):
        R = f16r if rnd else _id
        n, c, hh, ww = x.shape
        o = self._attn_parts(a, x, rnd)[5]
        o = F.conv1d(o, self.p(f"{a.path}.proj_out.weight"), self.p(f"{a.path}.proj_out.bias"))
        return R(x.reshape(n, c, -1) + o).reshape(n, c, hh, ww)

    def layer(self, l, x, emb, rnd=False):
        if l.kind == "conv":
            R = f16r if rnd else _id
            return R(_conv(x, self.p(f"{l.path}.weight"), self.p(f"{l.path}.bias"), 1))
        if l.kind == "res":
            return self.resblock(l, x, emb, rnd)[0]
        return self.attention(l, x, rnd)

    def block(self, blk, x, emb, rnd=False):
        for l in blk.layers:
            x = self.layer(l, x, emb, rnd)
        return x

    def head(self, h):
        h = gn_forward(h, self.p("out.0.weight"), self.p("out.0.bias"))
        return _conv(h, self.p("out.2.weight"), self.p("out.2.bias"), 1)

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
