"""Every GroupNorm kernel form, one launch at a time, against float64 (tests/groupnorm_ref.py).

Each case in CASES is one launch through ishap_group_norm32_run (include/ishap.h): the call turns the descriptor into the
GnApplyArgs / GnBwdArgs (+ SlabSrc) the executor builds and goes through the executor's launchers (csrc/norm_api.hip).  Every
case asserts (1) kernel name, route and parts; (2) the element bounds below; (3) canaries: outputs start as NaN bit patterns with
256 canary elements behind them, written elements end finite, canaries keep their bits; (4) a second call gives the same bits,
and so does ISHAP_GN_PARTS=1 for the cases whose plan has several parts (one child process for all of them).

Inputs.  Every case's x holds all families at once: a constant group (image 0, group 0: var = 0, rstd = 1 / sqrt(eps)), offset
groups (1..4: |mean| = 100, spread 0.1), normal groups; with SiLU some channels carry beta = +-20 (saturated); with FiLM some
channels carry scale = -1 exactly (sc = 0); backward: g = 0 on groups 5, 6 of image 0, where dx must equal add + add2 bit for bit.
The worst ratio of error to bound is printed per family.

Bounds (u = 2^-11, a = 2^-20: fp32 arithmetic, __expf, v_rcp_f32; s' = max |SiLU'| = 1.0998 with act, else 1; 2^-25 is added
for every fp16 rounding: half a subnormal quantum, the format's absolute floor).
Statistics: mean within E_m = 2^-23 |mean| + 2^-24 sqrt(var); rstd within E_r = 2^-22 relative.  Route 4 reads 64-bit fixed-point
channel sums: each is rounded by half a unit, so a group's sum / count moves by q1 = 0.5 / (STAT_SCALE_SUM * HW), its sum of
squares / count by q2 = 0.5 / (STAT_SCALE_SQ * HW): E_m += q1, E_r += 0.5 (q2 + 2 |mean| q1) / (var + eps).
Forward, against the statement: the kernel's xhat differs from the float64 one by dxh = rstd E_m + |xhat| E_r (a point the first
count missed: at |mean| = 100, spread 0.1 the cast of the mean to fp32 alone moves xhat by 6e-5).  The pre-activation's error is
    e = u (2 |p| |sc| + |p sc| + |p sc + sh|) + (a (|xhat gamma| + |beta|) + |gamma| dxh) |sc|
(p the affine output, sc = 1 + scale, sh the shift; without FiLM: e = u |p| + the second bracket).  The factor 2 on the first term
is a second point the first count missed: sc = fp16(1 + fp16(scale)) is rounded itself, which moves the product by u |p| |sc|.
    |y - y*| <= (u + 2a) |y*| + s' e          (without SiLU the rounded pre-activation IS the output: |y - y*| <= e)
A pooled pixel: a quarter of the sum of the four bounds + u |y*| + a mean|y_i|.  The head's split form (hi + lo) has no fp16
rounding point: s' (second bracket) + (2a + 2^-21) |y*|.  xcopy: bit for bit.  xpool: u |ref| + 2^-22 sum |x|.  A materialised ya:
u |ref| + 2^-22 A, A the sum of magnitudes of slices, biases and residual; everything downstream of ya is judged on the kernel's own ya.
Backward, against float64 autograd of the statement, the kernel running on the fp32 casts of the float64 statistics (E_m =
2^-24 |mean|, E_r = 2^-24), with M the group mean of magnitudes, m2 = mean_g(dyh xhat):
    eps_d = |up mult| 0.5 max(2u |pre|, e)     (a flip of the recomputed fp16 pre-activation through SiLU'' <= 0.5; 0 without act)
    |dx - dx*| <= u |dx*| + rstd [eps_d + M(eps_d) + |xhat| M(eps_d |xhat|)] + (a + u_film) rstd (|dyh| + M|dyh| + |xhat| M|dyh xhat|)
                  + rstd (dxh |m2| + |xhat| M(|dyh| dxh)) + rstd (1 + |xhat|) q
u_film = u with FiLM (mult carries the rounded sc), q the fixed-point quantum of the full-map route's csums (2^-25 over the rows
of one block, or over HW for caller-given sums).  add enters the fp32 sum; add2 does NOT share that rounding: the kernels round
to fp16 in front of add2 ("as a separate fp16 add of the two maps", norm_bwd.hip), so with add2 one more u |dx* + add| is counted
-- a third point the first count missed.  A pending gradient is fp16(fp32 sum of the slices): where the float64 sum lies within
2^-22 A of a rounding boundary the kernel may hold the neighbouring fp16 value, and eps_d grows by 2u |g| there (only there).

The CPU tests at the end check the table against the planner, that it covers every instance the launchers list, that out-of-
contract descriptors are refused before any HIP call, the restatement against the statement, and that the bounds reject mutated
references.

Worst error / bound over all cases on an MI355X: out 0.996 (normal 0.996, offset 0.912, constant 0.718, saturated 0.568,
sc = 0 0.300), dx 0.999 (normal 0.997, constant 0.994, offset 0.990, saturated 0.996, sc = 0 0.908), xpool 0.998, ya 0.148,
mean 0.433, rstd 0.247.  The mean of the constant group is 0: 3.0 is its own fp32 value.  59 GPU tests in 6.3 s."""
import ctypes as C
import dataclasses
import hashlib
import json
import os
import re
import subprocess
import sys
import time
import zlib

import pytest
import torch

from tests import groupnorm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ishapediting_amd", "csrc")
CANARY16, CANARY32 = 0x7E5A, 0x7FC0BEEF
TAIL = 256
GB_SAME, GB_UNPOOL, GB_SUM4 = R.GB_SAME, R.GB_UNPOOL, R.GB_SUM4


def _stat_scales():
    src = open(os.path.join(CSRC, "common.h")).read()
    get = lambda k: float(re.search(rf"#define {k} ([0-9.]+)f", src).group(1))
    return get("STAT_SCALE_SUM"), get("STAT_SCALE_SQ")


STAT_SCALE_SUM, STAT_SCALE_SQ = _stat_scales()


@dataclasses.dataclass(frozen=True)
class Case:
    shape: tuple                # (N, H, W, C)
    route: int                  # 1 / 4 full map, 2 / 3 group-local
    kernel: str                 # expected kernel name
    parts: int                  # expected workgroups per (image, group); 0 on the full map
    bwd: bool = False
    film: bool = False
    act: bool = True
    pool: bool = False
    split: bool = False
    gmode: int = GB_SAME
    csplit: int = 0             # forward: lazy concatenation x | x2; backward: split output dx | dx2
    sums: bool = False          # forward route 4: always the caller's sums; backward route 1: sums_ready
    nslab: int = 0              # pending source
    pend: str = ""              # forward pending: "bias,bias2,res" / "res_ups"
    add: bool = False
    add2: bool = False
    quiet: bool = False         # optional outputs (stats_out, xpool) not requested
    chain: bool = False         # backward on the forward kernel's own stats_out

    @property
    def N(self): return self.shape[0]
    @property
    def H(self): return self.shape[1]
    @property
    def W(self): return self.shape[2]
    @property
    def C(self): return self.shape[3]
    @property
    def local(self): return self.route in (2, 3)


def _l(v, f, a, p): return f"gn_local_kernel<{v}, {str(f).lower()}, {str(a).lower()}, {str(p).lower()}>"
def _b(v, f, a, s): return f"gn_bwd_local_kernel<{v}, {str(f).lower()}, {str(a).lower()}, {str(s).lower()}>"
def _a(f, a, p, s): return f"gn_apply_kernel<{str(f).lower()}, {str(a).lower()}, {str(p).lower()}, {str(s).lower()}>"
def _ba(f, a): return f"gn_bwd_apply_kernel<{str(f).lower()}, {str(a).lower()}>"


T, F = True, False
CASES = {
    # ---- forward, group-local: VEC 8 / 4 / 2 / 1 x (SiLU + pool, FiLM + SiLU, SiLU, plain)
    "fwd local v8 SiLU, 32^2 x 256": Case((1, 32, 32, 256), 2, _l(8, F, T, F), 1),
    "fwd local v8 FiLM, two images": Case((2, 32, 32, 256), 2, _l(8, T, T, F), 1, film=T),
    "fwd local v8 pool + xpool": Case((1, 32, 32, 256), 2, _l(8, F, T, T), 1, pool=T),
    "fwd local v8 plain, concatenation 96 + 160": Case((1, 32, 32, 256), 2, _l(8, F, F, F), 1, act=F, csplit=96),
    "fwd local v4 SiLU, pending 5 slices + bias, bias2, res": Case((1, 32, 32, 256), 2, _l(4, F, T, F), 1, nslab=5,
                                                                  pend="bias,bias2,res"),
    "fwd local v4 FiLM, 32^2 x 128": Case((1, 32, 32, 128), 2, _l(4, T, T, F), 1, film=T),
    "fwd local v4 pool, 16x8 x 1024": Case((1, 16, 8, 1024), 2, _l(4, F, T, T), 1, pool=T),
    "fwd local v4 plain, the widest C at 8^2": Case((1, 8, 8, 40832), 2, _l(4, F, F, F), 1, act=F, quiet=T),
    "fwd local v2 SiLU, 8x16, 8 parts": Case((1, 8, 16, 256), 3, _l(2, F, T, F), 8),
    "fwd local v2 FiLM, two images, 4 parts": Case((2, 16, 16, 128), 3, _l(2, T, T, F), 4, film=T),
    "fwd local v2 pool, 16x8, 2 parts": Case((1, 16, 8, 64), 3, _l(2, F, T, T), 2, pool=T, quiet=T),
    "fwd local v2 plain, 10x10": Case((1, 10, 10, 64), 3, _l(2, F, F, F), 1, act=F),
    "fwd local v2 SiLU, 6x6": Case((1, 6, 6, 64), 2, _l(2, F, T, F), 1),
    "fwd local v2 SiLU, pending 1 slice + res_ups, concatenation": Case((1, 16, 16, 256), 3, _l(2, F, T, F), 8, nslab=1,
                                                                       pend="res_ups", csplit=96),
    "fwd local v1 SiLU, C = 32": Case((1, 8, 8, 32), 3, _l(1, F, T, F), 1),
    "fwd local v1 FiLM, C = 96": Case((1, 8, 8, 96), 3, _l(1, T, T, F), 1, film=T),
    "fwd local v1 pool, C = 32, 16x8": Case((1, 16, 8, 32), 3, _l(1, F, T, T), 1, pool=T),
    "fwd local v1 plain, C = 32, 6x6": Case((1, 6, 6, 32), 2, _l(1, F, F, F), 1, act=F),
    # ---- forward, full map: the five apply instances on two-pass statistics (route 1) and on the caller's sums (route 4)
    "fwd full split, two-pass": Case((1, 16, 16, 64), 1, _a(F, T, F, T), 0, split=T),
    "fwd full split, sums": Case((1, 8, 16, 64), 4, _a(F, T, F, T), 0, split=T, sums=T),
    "fwd full pool, two-pass, 16x8": Case((1, 16, 8, 64), 1, _a(F, T, T, F), 0, pool=T),
    "fwd full pool, sums, 64^2 x 128": Case((1, 64, 64, 128), 4, _a(F, T, T, F), 0, pool=T, sums=T),
    "fwd full FiLM, two-pass, two images, 10x10": Case((2, 10, 10, 64), 1, _a(T, T, F, F), 0, film=T),
    "fwd full FiLM, sums": Case((2, 16, 16, 64), 4, _a(T, T, F, F), 0, film=T, sums=T),
    "fwd full SiLU, two-pass, 6x6": Case((1, 6, 6, 64), 1, _a(F, T, F, F), 0),
    "fwd full SiLU, sums, concatenation 96 + 160": Case((1, 8, 16, 256), 4, _a(F, T, F, F), 0, sums=T, csplit=96),
    "fwd full plain, two-pass, 8x16": Case((1, 8, 16, 96), 1, _a(F, F, F, F), 0, act=F),
    "fwd full plain, sums, 6x6": Case((1, 6, 6, 64), 4, _a(F, F, F, F), 0, act=F, sums=T, quiet=T),
    # ---- backward, group-local: VEC x (FiLM, SiLU, plain) x (fp32 staging: GB_UNPOOL / GB_SUM4, fp16 staging: GB_SAME)
    "bwd local v8 FiLM, UNPOOL": Case((1, 32, 32, 256), 2, _b(8, T, T, T), 1, bwd=T, film=T, gmode=GB_UNPOOL),
    "bwd local v8 SiLU, SUM4 + add": Case((1, 32, 32, 256), 2, _b(8, F, T, T), 1, bwd=T, gmode=GB_SUM4, add=T),
    "bwd local v8 plain, UNPOOL + add + add2": Case((1, 32, 32, 256), 2, _b(8, F, F, T), 1, bwd=T, act=F, gmode=GB_UNPOOL, add=T,
                                                   add2=T),
    "bwd local v8 FiLM, two images": Case((2, 32, 32, 256), 2, _b(8, T, T, F), 1, bwd=T, film=T),
    "bwd local v8 SiLU, split output 96 | 160": Case((1, 32, 32, 256), 2, _b(8, F, T, F), 1, bwd=T, csplit=96, add=T, add2=T),
    "bwd local v8 plain": Case((1, 32, 32, 256), 2, _b(8, F, F, F), 1, bwd=T, act=F),
    "bwd local v4 FiLM, SUM4": Case((1, 32, 32, 128), 2, _b(4, T, T, T), 1, bwd=T, film=T, gmode=GB_SUM4),
    "bwd local v4 SiLU, UNPOOL, pending 5 slices": Case((1, 32, 32, 256), 2, _b(4, F, T, T), 1, bwd=T, gmode=GB_UNPOOL, nslab=5),
    "bwd local v4 plain, SUM4": Case((1, 32, 32, 128), 2, _b(4, F, F, T), 1, bwd=T, act=F, gmode=GB_SUM4),
    "bwd local v4 FiLM": Case((1, 32, 32, 128), 2, _b(4, T, T, F), 1, bwd=T, film=T, add2=T),
    "bwd local v4 SiLU, pending 1 slice": Case((1, 32, 32, 256), 2, _b(4, F, T, F), 1, bwd=T, nslab=1),
    "bwd local v4 plain, the widest C at 8^2": Case((1, 8, 8, 40832), 2, _b(4, F, F, F), 1, bwd=T, act=F),
    "bwd local v2 FiLM, UNPOOL, two images, 4 parts": Case((2, 16, 16, 128), 3, _b(2, T, T, T), 4, bwd=T, film=T, gmode=GB_UNPOOL,
                                                          add=T),
    "bwd local v2 SiLU, SUM4, 8x16, 8 parts": Case((1, 8, 16, 256), 3, _b(2, F, T, T), 8, bwd=T, gmode=GB_SUM4),
    "bwd local v2 plain, UNPOOL, 6x6": Case((1, 6, 6, 64), 2, _b(2, F, F, T), 1, bwd=T, act=F, gmode=GB_UNPOOL),
    "bwd local v2 FiLM, 10x10": Case((1, 10, 10, 64), 3, _b(2, T, T, F), 1, bwd=T, film=T),
    "bwd local v2 SiLU, 2 parts, on the forward's own stats": Case((1, 16, 8, 64), 3, _b(2, F, T, F), 2, bwd=T, chain=T, add=T,
                                                                  add2=T),
    "bwd local v2 plain, split output, 8 parts": Case((1, 16, 16, 256), 3, _b(2, F, F, F), 8, bwd=T, act=F, csplit=96),
    "bwd local v1 FiLM, SUM4, C = 96": Case((1, 8, 8, 96), 3, _b(1, T, T, T), 1, bwd=T, film=T, gmode=GB_SUM4),
    "bwd local v1 SiLU, UNPOOL, C = 32": Case((1, 8, 8, 32), 3, _b(1, F, T, T), 1, bwd=T, gmode=GB_UNPOOL),
    "bwd local v1 plain, SUM4, C = 32": Case((1, 6, 6, 32), 2, _b(1, F, F, T), 1, bwd=T, act=F, gmode=GB_SUM4),
    "bwd local v1 FiLM, C = 32": Case((1, 8, 8, 32), 3, _b(1, T, T, F), 1, bwd=T, film=T),
    "bwd local v1 SiLU, C = 32, 16x8": Case((1, 16, 8, 32), 3, _b(1, F, T, F), 1, bwd=T, add=T),
    "bwd local v1 plain, C = 96": Case((1, 8, 8, 96), 2, _b(1, F, F, F), 1, bwd=T, act=F),
    # ---- backward, full map: the apply instances with the sums gathered here and given by the caller, all three gmodes
    "bwd full FiLM, sums gathered, 64^2 x 128": Case((1, 64, 64, 128), 1, _ba(T, T), 0, bwd=T, film=T, add=T, add2=T),
    "bwd full FiLM, sums ready, UNPOOL, two images": Case((2, 16, 16, 64), 1, _ba(T, T), 0, bwd=T, film=T, sums=T,
                                                         gmode=GB_UNPOOL),
    "bwd full SiLU, sums gathered, SUM4, 6x6": Case((1, 6, 6, 64), 1, _ba(F, T), 0, bwd=T, gmode=GB_SUM4, add=T),
    "bwd full SiLU, sums ready, split output 96 | 160, 8x16": Case((1, 8, 16, 256), 1, _ba(F, T), 0, bwd=T, sums=T, csplit=96,
                                                                  add2=T),
    "bwd full plain, sums gathered, 10x10, UNPOOL": Case((2, 10, 10, 64), 1, _ba(F, F), 0, bwd=T, act=F, gmode=GB_UNPOOL),
    "bwd full plain, sums ready": Case((1, 8, 16, 96), 1, _ba(F, F), 0, bwd=T, act=F, sums=T),
}


# ---------------------------------------------------------------------------------------------------------------- operands
def _gen(c: Case, salt=""):
    return torch.Generator().manual_seed(zlib.crc32(repr((c.shape, c.bwd, c.film, c.act, c.gmode, c.csplit, c.nslab, salt)).encode()))


def _f16(t):
    return t.to(torch.float16)


def families(c: Case):
    """boolean masks [N][1][1][C] / [C] of the input families"""
    N, C_ = c.N, c.C
    grp = torch.arange(C_) // (C_ // 32)
    img0 = torch.zeros(N, 1, 1, 1, dtype=torch.bool)
    img0[0] = True
    const = img0 & (grp == 0)
    offset = ((grp >= 1) & (grp <= 4)).expand(N, 1, 1, C_)
    zero_g = img0 & ((grp == 5) | (grp == 6))
    ch = torch.arange(C_)
    sat = ((ch % 16 == 5) | (ch % 16 == 11)) if c.act else torch.zeros(C_, dtype=torch.bool)
    sc0 = (ch % 8 == 3) if c.film else torch.zeros(C_, dtype=torch.bool)
    return dict(const=const, offset=offset, zero_g=zero_g, sat=sat, sc0=sc0)


def make_x(c: Case):
    N, H, W, C_ = c.shape
    g = _gen(c, "x")
    fam = families(c)
    x = 0.5 * torch.randn(N, H, W, C_, generator=g) + R.per_channel(torch.randn(N, 32, generator=g), C_)
    sign = torch.where(torch.arange(C_) // (C_ // 32) % 2 == 0, 100.0, -100.0)
    x = torch.where(fam["offset"], sign + 0.1 * torch.randn(N, H, W, C_, generator=g), x)
    x = torch.where(fam["const"], torch.tensor(3.0), x)
    return _f16(x)


def make_params(c: Case):
    g = _gen(c, "p")
    fam = families(c)
    gamma = 1.0 + 0.3 * torch.randn(c.C, generator=g)
    beta = 0.2 * torch.randn(c.C, generator=g)
    ch = torch.arange(c.C)
    beta = torch.where(fam["sat"], torch.where(ch % 16 == 5, 20.0, -20.0), beta)
    emb_ld = 2 * c.C + 8
    emb = _f16(0.4 * torch.randn(c.N, emb_ld, generator=g)).float()        # the model's FiLM rows are fp16 values
    emb[:, :c.C] = torch.where(fam["sc0"], torch.tensor(-1.0), emb[:, :c.C])
    return gamma.float(), beta.float(), emb, emb_ld


def g_shape(c: Case):
    N, H, W, C_ = c.shape
    return {GB_SAME: (N, H, W, C_), GB_UNPOOL: (N, H // 2, W // 2, C_), GB_SUM4: (N, 2 * H, 2 * W, C_)}[c.gmode]


def split_slices(target, nslab, g, extra=()):
    """fp32 slices [nslab][...] whose sum (+ extra) is close to target"""
    sl = [0.3 * torch.randn(target.shape, generator=g) for _ in range(nslab - 1)]
    rest = target.float()
    for t in sl + list(extra):
        rest = rest - t
    return torch.stack(sl + [rest]).float()


def channel_sums(x):
    """[N][C][2] int64 fixed point (sum, sum of squares) of x [N][H][W][C] float64"""
    s = torch.round(x.sum((1, 2)) * STAT_SCALE_SUM)
    q = torch.round((x * x).sum((1, 2)) * STAT_SCALE_SQ)
    return torch.stack([s, q], -1).to(torch.int64)


# ---------------------------------------------------------------------------------------------------------------- the call
def _canary(shape, dtype):
    it, v = {torch.float16: (torch.int16, CANARY16 - (1 << 16) if CANARY16 >= 1 << 15 else CANARY16),
             torch.float32: (torch.int32, CANARY32)}[dtype]
    n = 1
    for s in shape:
        n *= s
    return torch.full((n + TAIL,), v, dtype=it).view(dtype)


def _bits(t):
    return t.view({torch.float16: torch.int16, torch.float32: torch.int32}[t.dtype])


def _check_written(name, flat, n):
    """the first n elements finite, the tail still canaries"""
    assert torch.equal(_bits(flat[n:]), _bits(_canary((0,), flat.dtype))), f"{name}: the canaries behind the buffer changed"
    bad = (~torch.isfinite(flat[:n].float())).sum().item()
    assert bad == 0, f"{name}: {bad} written elements are not finite"


def _untouched(name, flat):
    assert torch.equal(_bits(flat), _bits(_canary((flat.numel() - TAIL,), flat.dtype))), f"{name}: written though not requested"


def fill_desc(c: Case, p):
    """GroupNormDescC of a case; p: name -> address (int) of each buffer the case passes"""
    from ishapediting_amd._lib import GroupNormDescC
    d = GroupNormDescC()
    d.backward, d.N, d.H, d.W, d.C, d.route = int(c.bwd), c.N, c.H, c.W, c.C, c.route
    d.film, d.act, d.pool, d.split, d.gmode = int(c.film), int(c.act), int(c.pool), int(c.split), c.gmode
    d.sums_ready = int(c.bwd and c.sums)
    d.csplit, d.emb_ld = c.csplit, (2 * c.C + 8 if c.film else 0)
    d.nslab = c.nslab
    for k, v in p.items():
        setattr(d, k, v)
    return d


def buffer_names(c: Case):
    """the pointer fields a case passes (beside zstride / ldr / res_ups)"""
    n = ["gamma", "beta", "scratch"] + (["emb"] if c.film else [])
    if c.bwd:
        n += ["x", "stats", "dx"] + (["ws"] if c.nslab else ["g"]) + (["add"] if c.add else []) + (["add2"] if c.add2 else [])
        n += (["dx2"] if c.csplit else []) + (["csums"] if c.sums else [])
    else:
        n += ["out"] + (["ws", "ya"] if c.nslab else ["x"]) + (["x2", "xcopy"] if c.csplit else [])
        n += (["sums"] if c.sums else []) + (["sums2"] if c.sums and c.csplit else [])
        n += ["bias", "bias2", "res"] if "bias" in c.pend else (["res"] if c.pend == "res_ups" else [])
        if not c.quiet or c.route == 1:
            n += ["stats_out"]
        if c.pool and not c.quiet:
            n += ["xpool"]
    return n


def _run(L, d, dev):
    from ishapediting_amd import _lib
    route, parts, kern = C.c_int(), C.c_int(), C.create_string_buffer(96)
    _lib.check(L.ishap_group_norm32_run(C.byref(d), 1, _lib.stream_ptr(dev), C.byref(route), C.byref(parts), kern, len(kern)))
    torch.cuda.synchronize()
    return kern.value.decode(), route.value, parts.value


def _ratio(got, ref, bound, masks):
    """worst |got - ref| / bound overall and per family"""
    r = (got - ref).abs() / bound
    out = {"all": r.max().item()}
    for k, m in masks.items():
        m = m.expand_as(r) if m.dim() == r.dim() else m.expand(r.shape)
        if m.any():
            out[k] = r[m].max().item()
    return r, out


def _assert_ratio(what, r, worst):
    if worst["all"] > 1.0:
        idx = [int(v) for v in torch.unravel_index(r.argmax(), r.shape)]
        raise AssertionError(f"{what}: {(r > 1).sum().item()} elements over the bound, worst {worst['all']:.3g} x at {idx}")


def run_case(c: Case, check=True):
    """-> (kernel, route, parts, {quantity: {family: worst ratio}}, sha256 of the outputs' bytes, seconds)"""
    from ishapediting_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    t0 = time.time()
    N, H, W, C_ = c.shape
    HW = H * W
    fam = families(c)
    x16 = make_x(c)
    gamma, beta, emb, emb_ld = make_params(c)
    g = _gen(c, "g")
    keep = []                                   # device tensors alive until the launch has run
    p = {}

    def dev_in(name, t):
        t = t.contiguous().to(dev)
        keep.append(t)
        p[name] = t.data_ptr()
        return t

    outs = {}

    def dev_out(name, shape, dtype=torch.float16, passed=True):
        t = _canary(shape, dtype).to(dev)
        outs[name] = (t, passed)
        if passed:
            p[name] = t.data_ptr()
        return t

    dev_in("gamma", gamma), dev_in("beta", beta)
    if c.film:
        dev_in("emb", emb)
    scratch = torch.empty(int(L.ishap_group_norm32_scratch_bytes(N, HW, C_)), dtype=torch.uint8, device=dev)
    p["scratch"] = scratch.data_ptr()
    Ca = c.csplit or C_
    xd = x16.double()
    want = buffer_names(c)
    slab_ref = None
    if not c.bwd:
        if c.nslab:
            tgt = x16[..., :Ca]
            bias = 0.3 * torch.randn(Ca, generator=g) if "bias" in c.pend else None
            bias2 = 0.3 * torch.randn(Ca, generator=g) if "bias2" in c.pend else None
            res = res_full = None
            ldr = Ca + 8
            if c.pend:
                rs = (N, H // 2, W // 2, Ca) if c.pend == "res_ups" else (N, H, W, Ca)
                res = _f16(0.5 * torch.randn(rs, generator=g))
                res_full = R.up2(res.double()) if c.pend == "res_ups" else res.double()
            extra = [t.float() for t in (bias, bias2) if t is not None] + ([res_full.float()] if res is not None else [])
            slices = split_slices(tgt, c.nslab, g, extra)
            zstride = N * HW * Ca + 64
            ws = torch.zeros(c.nslab, zstride)
            ws[:, :N * HW * Ca] = slices.reshape(c.nslab, -1)
            dev_in("ws", ws)
            p["zstride"] = zstride
            if bias is not None:
                dev_in("bias", bias)
            if bias2 is not None:
                dev_in("bias2", bias2)
            if res is not None:
                rp = torch.full(res.shape[:3] + (ldr,), float("nan"), dtype=torch.float16)
                rp[..., :Ca] = res
                dev_in("res", rp)
                p["ldr"], p["res_ups"] = ldr, int(c.pend == "res_ups")
            slab_ref = R.slab_sum(slices.double(), *(t.double() if t is not None else None for t in (bias, bias2)), res_full)
            dev_out("ya", (N, HW, Ca))
        else:
            dev_in("x", x16[..., :Ca])
        if c.csplit:
            dev_in("x2", x16[..., Ca:])
            dev_out("xcopy", (N, HW, C_))
        if c.sums:
            dev_in("sums", channel_sums(xd[..., :Ca]))
            if c.csplit:
                dev_in("sums2", channel_sums(xd[..., Ca:]))
        Ho, Wo = (H // 2, W // 2) if c.pool else (H, W)
        dev_out("out", (N, Ho * Wo, 3 * C_ if c.split else C_))
        dev_out("stats_out", (N, 32, 2), torch.float32, "stats_out" in want)
        if c.pool:
            dev_out("xpool", (N, Ho * Wo, C_), passed="xpool" in want)
    else:
        dev_in("x", x16)
        gs = g_shape(c)
        g16 = _f16(torch.randn(gs, generator=g))
        g16 = torch.where(fam["zero_g"], torch.tensor(0.0, dtype=torch.float16), g16)
        dup = None
        if c.nslab:
            slices = split_slices(g16, c.nslab, g)
            slices = torch.where(fam["zero_g"], torch.tensor(0.0), slices)
            rows = gs[0] * gs[1] * gs[2]
            zstride = rows * C_ + 64
            ws = torch.zeros(c.nslab, zstride)
            ws[:, :rows * C_] = slices.reshape(c.nslab, -1)
            dev_in("ws", ws)
            p["zstride"] = zstride
            s64, a64 = R.slab_sum(slices.double())
            g16 = _f16(s64)
            dup = R.upstream(torch.where(R.may_flip(s64, a64), 2.0 * R.U * s64.abs() + 2.0 ** -24, torch.tensor(0.0, dtype=torch.float64)),
                             c.gmode)
        else:
            dev_in("g", g16)
        add = _f16(torch.randn(gs, generator=g)) if c.add else None
        add2 = _f16(torch.randn(N, H, W, C_, generator=g)) if c.add2 else None
        if add is not None:
            dev_in("add", add)
        if add2 is not None:
            dev_in("add2", add2)
        mean64, var64, rstd64 = R.group_stats(xd)
        e_stats = None
        if c.chain:                             # the forward kernel's own statistics, checked against their bound first
            fc = dataclasses.replace(c, bwd=False, add=False, add2=False, chain=False, kernel="", parts=0)
            so = _canary((N, 32, 2), torch.float32).to(dev)
            fo = _canary((N, HW, C_), torch.float16).to(dev)
            fd = fill_desc(fc, dict(gamma=p["gamma"], beta=p["beta"], scratch=p["scratch"], x=p["x"], out=fo.data_ptr(),
                                    stats_out=so.data_ptr()))
            _run(L, fd, dev)
            st = so[:N * 64].view(N, 32, 2).clone()
            e_stats = R.stats_error(mean64, var64)
            sc_ = st.cpu().double()
            assert ((sc_[..., 0] - mean64).abs() <= e_stats[0]).all() and ((sc_[..., 1] / rstd64 - 1).abs() <= e_stats[1]).all()
        else:
            st = torch.stack([mean64, rstd64], -1).float().to(dev)
        keep.append(st)
        p["stats"] = st.data_ptr()
        if c.sums:                              # the caller's csums: float64 sums of the restated terms, in fixed point
            s32 = st.cpu().double()
            esc, esh = (emb.double()[:, None, None, :C_], emb.double()[:, None, None, C_:2 * C_]) if c.film else (0.0, 0.0)
            dyh, xh = R.gn_bwd_ref(R.upstream(g16.double(), c.gmode), xd, R.per_channel(s32[..., 0], C_), R.per_channel(s32[..., 1], C_),
                                   gamma.double(), beta.double(), esc, esh, c.film, c.act)
            cs = torch.stack([dyh.sum((1, 2)), (dyh * xh).sum((1, 2))], -1)
            dev_in("csums", torch.round(cs * STAT_SCALE_SUM).to(torch.int64))
        dev_out("dx", (N, HW, c.csplit or C_))
        if c.csplit:
            dev_out("dx2", (N, HW, C_ - c.csplit))
    assert sorted(k for k in p if k not in ("zstride", "ldr", "res_ups")) == sorted(want), (sorted(p), sorted(want))
    d = fill_desc(c, p)

    def snapshot():
        return {k: t.cpu() for k, (t, _) in outs.items()}

    def reset():
        for k, (t, _) in outs.items():
            t.copy_(_canary((t.numel() - TAIL,), t.dtype))

    name, route, parts = _run(L, d, dev)
    first = snapshot()
    digest = hashlib.sha256(b"".join(first[k].numpy().tobytes() for k in sorted(first))).hexdigest()
    if not check:
        return name, route, parts, {}, digest, time.time() - t0
    assert (name, route, parts) == (c.kernel, c.route, c.parts), f"ran {name} on route {route} with {parts} parts"
    reset()
    _run(L, d, dev)
    second = snapshot()
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(second[k])), f"{k}: a second identical call gave other bits"

    worst = {}
    gm, bt, em = gamma.double(), beta.double(), emb.double()
    if not c.bwd:
        x_used = xd
        if c.nslab:
            ya = first["ya"]
            _check_written("ya", ya, N * HW * Ca)
            ya = ya[:N * HW * Ca].view(N, H, W, Ca).double()
            r, worst["ya"] = _ratio(ya, slab_ref[0], R.materialised_bound(*slab_ref), {})
            _assert_ratio("ya", r, worst["ya"])
            x_used = torch.cat([ya, xd[..., Ca:]], -1)
        if c.csplit:
            xc = first["xcopy"]
            _check_written("xcopy", xc, N * HW * C_)
            assert torch.equal(_bits(xc[:N * HW * C_].view(N, H, W, C_)), _bits(_f16(x_used))), "xcopy is not the concatenation"
        mean, var, rstd = R.group_stats(x_used)
        quantum = (0.5 / (STAT_SCALE_SUM * HW), 0.5 / (STAT_SCALE_SQ * HW)) if c.route == 4 else None
        e_stats = R.stats_error(mean, var, quantum)
        so, passed = outs["stats_out"]
        if passed:
            sv = first["stats_out"]
            _check_written("stats_out", sv, N * 64)
            sv = sv[:N * 64].view(N, 32, 2).double()
            gmask = {"const": fam["const"].reshape(N, -1)[:, ::C_ // 32], "offset": fam["offset"].reshape(N, -1)[:, ::C_ // 32]}
            r, worst["mean"] = _ratio(sv[..., 0], mean, e_stats[0] + 1e-300, gmask)
            _assert_ratio("mean", r, worst["mean"])
            r, worst["rstd"] = _ratio(sv[..., 1] / rstd, torch.ones_like(rstd), e_stats[1], gmask)
            _assert_ratio("rstd", r, worst["rstd"])
        else:
            _untouched("stats_out", first["stats_out"])
        Ho, Wo = (H // 2, W // 2) if c.pool else (H, W)
        ov = first["out"]
        wid = 3 * C_ if c.split else C_
        _check_written("out", ov, N * Ho * Wo * wid)
        ov = ov[:N * Ho * Wo * wid].view(N, Ho, Wo, wid)
        if c.split:
            assert torch.equal(_bits(ov[..., :C_]), _bits(ov[..., 2 * C_:])), "split: the two hi blocks differ"
            y = ov[..., :C_].double() + ov[..., C_:2 * C_].double()
        else:
            y = ov.double()
        ref = R.forward_statement(x_used, gm, bt, em, c.film, c.act, c.pool)
        bound = R.forward_bound(x_used, gm, bt, em, c.film, c.act, c.pool, e_stats, c.split)
        masks = {"normal": ~(fam["const"] | fam["offset"] | fam["sat"] | fam["sc0"]), "const": fam["const"], "offset": fam["offset"],
                 "saturated": fam["sat"], "sc = 0": fam["sc0"]}
        r, worst["out"] = _ratio(y, ref, bound, masks)
        _assert_ratio("out", r, worst["out"])
        if c.pool:
            xp, passed = outs["xpool"]
            if passed:
                xv = first["xpool"]
                _check_written("xpool", xv, N * Ho * Wo * C_)
                r, worst["xpool"] = _ratio(xv[:N * Ho * Wo * C_].view(N, Ho, Wo, C_).double(), R.pool2(x_used),
                                           R.pooled_input_bound(x_used), {})
                _assert_ratio("xpool", r, worst["xpool"])
            else:
                _untouched("xpool", first["xpool"])
    else:
        gd = g16.double()
        ad = add.double() if add is not None else None
        a2 = add2.double() if add2 is not None else None
        rpb = max(8, HW // 256)
        quantum = 0.0 if c.local else 2.0 ** -25 / (HW if c.sums else rpb) + (2.0 ** -25 / HW if c.sums else 0.0)
        ref = R.backward_statement(gd, xd, gm, bt, em, c.film, c.act, c.gmode, ad, a2)
        bound = R.backward_bound(gd, xd, gm, bt, em, c.film, c.act, c.gmode, ad, a2, quantum, dup, e_stats)
        n1 = N * HW * (c.csplit or C_)
        _check_written("dx", first["dx"], n1)
        dx = first["dx"][:n1].view(N, H, W, -1)
        if c.csplit:
            n2 = N * HW * (C_ - c.csplit)
            _check_written("dx2", first["dx2"], n2)
            dx = torch.cat([dx, first["dx2"][:n2].view(N, H, W, -1)], -1)
        masks = {"normal": ~(fam["const"] | fam["offset"] | fam["sat"] | fam["sc0"] | fam["zero_g"]), "const": fam["const"],
                 "offset": fam["offset"], "saturated": fam["sat"], "sc = 0": fam["sc0"]}
        r, worst["dx"] = _ratio(dx.double(), ref, bound, masks)
        _assert_ratio("dx", r, worst["dx"])
        # g = 0 on whole groups: dx is add + add2 there, bit for bit
        exact = torch.zeros(N, H, W, C_, dtype=torch.float64)
        if ad is not None:
            exact = R.f16r(exact + R.upstream(ad, c.gmode))
        if a2 is not None:
            exact = exact + a2
        z = fam["zero_g"].expand(N, H, W, C_)
        assert torch.equal(dx[z].double(), R.f16r(exact)[z]), "g = 0: dx is not add + add2"
    return name, route, parts, worst, digest, time.time() - t0


_DIGESTS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_launch_matches_float64(case):
    name, route, parts, worst, digest, dt = run_case(CASES[case])
    _DIGESTS[case] = digest
    print(f"\n  {name} route {route} parts {parts}: worst / bound " +
          "; ".join(f"{q} " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()) for q, w in worst.items()) + f" ({dt:.2f} s)")


_CHILD = f"""
import json, sys
sys.path.insert(0, {ROOT!r})
from tests import test_gpu_groupnorm_oracle as T
print(json.dumps({{n: T.run_case(T.CASES[n], check=False)[4] for n in json.loads(sys.argv[1])}}))
"""


@pytest.mark.gpu
def test_one_part_gives_the_same_bits():
    """norm_local.hip: the result does not depend on how many workgroups share a group.  Every case whose plan has several parts,
    run again in ONE child process with ISHAP_GN_PARTS=1 (the switch is read once per process)"""
    names = [n for n, c in CASES.items() if c.parts > 1]
    assert len(names) >= 4
    env = {k: v for k, v in os.environ.items() if not k.startswith("ISHAP_")}
    env["ISHAP_GN_PARTS"] = "1"
    r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(names)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    one = json.loads(r.stdout.strip().splitlines()[-1])
    for n in names:
        if n not in _DIGESTS:
            _DIGESTS[n] = run_case(CASES[n], check=False)[4]
        assert one[n] == _DIGESTS[n], f"{n}: one part per group gives other bits"


# ---------------------------------------------------------------------------------------------------------------- CPU checks
def _fake_ptrs(c: Case):
    p = {k: (1 << 40) + (i << 24) for i, k in enumerate(buffer_names(c))}
    if c.nslab:
        gs = g_shape(c) if c.bwd else (c.N, c.H, c.W, c.csplit or c.C)
        p["zstride"] = gs[0] * gs[1] * gs[2] * gs[3] + 64
        if c.pend:
            p["ldr"], p["res_ups"] = (c.csplit or c.C) + 8, int(c.pend == "res_ups")
    return p


def _dry(d):
    from ishapediting_amd import _lib
    L = _lib.lib()
    route, parts, kern = C.c_int(), C.c_int(), C.create_string_buffer(96)
    rc = L.ishap_group_norm32_run(C.byref(d), 0, None, C.byref(route), C.byref(parts), kern, len(kern))
    msg = L.ishap_last_error()
    return rc, kern.value.decode(), route.value, parts.value, (msg.decode() if msg else "")


@pytest.mark.parametrize("case", list(CASES))
def test_table_matches_the_planner(case):
    """the expected kernel, route and parts are what ishap_group_norm32_plan gives the shape and what launch = 0 gives the
    case's own descriptor"""
    from ishapediting_amd import _lib
    c = CASES[case]
    o = [C.c_int() for _ in range(8)]
    kern = C.create_string_buffer(96)
    _lib.check(_lib.lib().ishap_group_norm32_plan(c.N, c.H, c.W, c.C, int(c.bwd), int(c.nslab > 0), int(c.film), int(c.act), int(c.pool),
                                                  c.gmode, c.route, *[C.byref(v) for v in o], kern, len(kern)))
    if not c.split:         # the planner has no split argument: the head's form is the apply kernel's own choice
        assert (kern.value.decode(), o[0].value, o[1].value) == (c.kernel, c.route, c.parts)
    rc, name, route, parts, msg = _dry(fill_desc(c, _fake_ptrs(c)))
    assert rc == 0, msg
    assert (name, route, parts) == (c.kernel, c.route, c.parts)


def test_table_covers_every_instance():
    """every instance the launchers' tables name (norm.hip, norm_bwd.hip, norm_local.hip) has a case; the full-map instances on
    both of their statistics sources"""
    tf = ("false", "true")
    inst = set()
    src = open(os.path.join(CSRC, "norm.hip")).read() + open(os.path.join(CSRC, "norm_bwd.hip")).read()
    inst |= set(re.findall(r'"(gn_(?:bwd_)?apply_kernel<[^"]+>)"', src))
    loc = open(os.path.join(CSRC, "norm_local.hip")).read()
    vecs = sorted({int(v) for v in re.findall(r"p\.vec == (\d)", loc)} | {1})
    for table, kern in (("kFwd", "gn_local_kernel"), ("kBwd", "gn_bwd_local_kernel")):
        body = re.search(rf"{table}\[\d\] = \{{(.*?)\}};", loc, re.S).group(1)
        rows = re.findall(rf"{kern}<V, (\w+), (\w+), (\w+)>", body)
        assert len(rows) == (4 if table == "kFwd" else 6)
        inst |= {f"{kern}<{v}, {a}, {b}, {c_}>" for v in vecs for a, b, c_ in rows}
    assert len(inst) == 5 + 3 + 4 * 4 + 4 * 6, sorted(inst)
    have = {c.kernel for c in CASES.values()}
    assert have == inst, (sorted(inst - have), sorted(have - inst))
    for k in inst:
        if "apply" in k:
            srcs = {(c.sums, c.route) for c in CASES.values() if c.kernel == k}
            assert len({s for s, _ in srcs}) == 2, k
    assert {c.parts for c in CASES.values()} >= {0, 1, 2, 4, 8}
    for bwd in (False, True):
        for local in (False, True):
            assert {c.gmode for c in CASES.values() if c.bwd and c.local == local} == {0, 1, 2}


def _refusals():
    base = CASES["fwd local v8 SiLU, 32^2 x 256"]
    full = CASES["fwd full SiLU, two-pass, 6x6"]
    film = CASES["fwd local v4 FiLM, 32^2 x 128"]
    cat = CASES["fwd local v8 plain, concatenation 96 + 160"]
    pend = CASES["fwd local v4 SiLU, pending 5 slices + bias, bias2, res"]
    bw = CASES["bwd local v8 plain"]
    bsp = CASES["bwd local v8 SiLU, split output 96 | 160"]
    S = lambda **kw: (lambda d: [setattr(d, k, v) for k, v in kw.items()])
    return [
        ("null x", base, S(x=None), "input"),
        ("null out", base, S(out=None), "out"),
        ("null gamma", base, S(gamma=None), "null argument"),
        ("null scratch", base, S(scratch=None), "null argument"),
        ("null stats on route 1", full, S(stats_out=None), "stats_out"),
        ("backward: null stats", bw, S(stats=None), "x, stats, dx"),
        ("backward: null g", bw, S(g=None), "upstream gradient"),
        ("C % 32", base, S(C=200), "GroupNorm32 dims"),
        ("N > 16", base, S(N=17), "GroupNorm32 dims"),
        ("csplit % 8", cat, S(csplit=100), "csplit"),
        ("csplit % 32 on a local route", cat, S(csplit=104), "multiple of 32"),
        ("backward csplit % 8", bsp, S(csplit=100), "csplit"),
        ("csplit without dx2", bsp, S(dx2=None), "dx2 and csplit"),
        ("concatenation without xcopy", cat, S(xcopy=None), "go together"),
        ("concatenation on the full map without sums", cat, S(route=1), "sums and sums2"),
        ("pool with odd H", base, S(pool=1, H=31), "even H and W"),
        ("pool with FiLM", film, S(pool=1), "no FiLM"),
        ("FiLM without SiLU", film, S(act=0), "FiLM is followed by SiLU"),
        ("FiLM with emb_ld < 2C", film, S(emb_ld=128), "emb_ld"),
        ("split on a group-local route", base, S(split=1), "no group-local kernel"),
        ("split without SiLU", full, S(split=1, act=0), "split variant"),
        ("pending on a full-map route", pend, S(route=1), "pending source"),
        ("pending with x", pend, S(x=1 << 41), "input"),
        ("pending with a short zstride", pend, S(zstride=1024), "zstride"),
        ("residual with ldr below the channels", pend, S(ldr=128), "ldr"),
        ("backward pending with a bias", CASES["bwd local v4 SiLU, pending 1 slice"], S(bias=1 << 41), "neither bias nor residual"),
        ("a group that does not fit in LDS", base, S(H=64, W=64, C=2048), "does not fit in LDS"),
        ("backward fp32 staging that does not fit", CASES["bwd local v8 SiLU, SUM4 + add"], S(H=64, W=64, C=1024), "does not fit in LDS"),
        ("route 4 stand-in: H*W % 64", CASES["fwd full SiLU, two-pass, 6x6"], S(route=4), "route 4"),
        ("sums on route 1", CASES["fwd full plain, sums, 6x6"], S(route=1, stats_out=1 << 41), "route 4 only"),
        ("sums_ready on a local route", CASES["bwd full plain, sums ready"], S(route=2), "sums_ready"),
        ("UNPOOL with odd W", CASES["bwd local v2 plain, UNPOOL, 6x6"], S(W=5), "even H and W"),
        ("backward route 4", bw, S(route=4), "backward route"),
        ("gmode 3", bw, S(gmode=3), "gmode"),
        ("xpool without pool", base, S(xpool=1 << 41), "xpool"),
    ]


@pytest.mark.parametrize("i", range(len(_refusals())))
def test_run_rejects_out_of_contract_input(i):
    """refused with a message before any HIP call (launch = 0 throughout: nothing here can reach a kernel)"""
    what, c, mutate, words = _refusals()[i]
    d = fill_desc(c, _fake_ptrs(c))
    rc, _, _, _, msg = _dry(d)
    assert rc == 0, msg                  # the unchanged descriptor passes: the refusal below is the mutation's
    mutate(d)
    rc, _, _, _, msg = _dry(d)
    assert rc != 0, what
    assert "requirement failed" in msg and words in msg, (what, msg)


def test_run_reports_a_short_name_buffer_and_a_null_descriptor():
    from ishapediting_amd import _lib
    L = _lib.lib()
    c = CASES["fwd local v8 SiLU, 32^2 x 256"]
    kern = C.create_string_buffer(8)
    assert L.ishap_group_norm32_run(C.byref(fill_desc(c, _fake_ptrs(c))), 0, None, None, None, kern, len(kern)) == -2
    assert L.ishap_group_norm32_run(None, 0, None, None, None, None, 0) == -2


def _small(c: Case, shape):
    return dataclasses.replace(c, shape=shape)


_CPU_FORMS = [dict(film=F, act=T, pool=F), dict(film=T, act=T, pool=F), dict(film=F, act=T, pool=T), dict(film=F, act=F, pool=F)]


def _cpu_operands(form, gmode=GB_SAME, shape=(2, 8, 8, 64)):
    c = Case(shape, 2, "", 1, film=form["film"], act=form["act"], pool=form["pool"], gmode=gmode)
    x = make_x(c).double()
    gamma, beta, emb, _ = make_params(c)
    return c, x, gamma.double(), beta.double(), emb.double()


@pytest.mark.parametrize("form", range(4))
def test_restatement_meets_the_statement(form):
    """forward and backward restatements (the kernels' rounding points) lie within the bounds of the statement, on every family"""
    f = _CPU_FORMS[form]
    c, x, gm, bt, em = _cpu_operands(f)
    ref = R.forward_statement(x, gm, bt, em, **f)
    got = R.forward_restatement(x, gm, bt, em, **f)
    assert ((got - ref).abs() <= R.forward_bound(x, gm, bt, em, **f)).all()
    sp = R.forward_restatement(x, gm, bt, None, False, True, False, split=True)
    st = R.forward_statement(x, gm, bt, None, False, True, False)
    assert ((sp - st).abs() <= R.forward_bound(x, gm, bt, None, False, True, False, split=True)).all()
    if f["pool"]:
        return
    g = torch.Generator().manual_seed(5)
    for gmode in (GB_SAME, GB_UNPOOL, GB_SUM4):
        c = dataclasses.replace(c, gmode=gmode)
        gr = _f16(torch.randn(g_shape(c), generator=g)).double()
        ad = _f16(torch.randn(g_shape(c), generator=g)).double()
        a2 = _f16(torch.randn(c.shape, generator=g)).double()
        ref = R.backward_statement(gr, x, gm, bt, em, f["film"], f["act"], gmode, ad, a2)
        got = R.backward_restatement(gr, x, R.stats32(x), gm, bt, em, f["film"], f["act"], gmode, ad, a2)
        assert ((got - ref).abs() <= R.backward_bound(gr, x, gm, bt, em, f["film"], f["act"], gmode, ad, a2)).all(), gmode


def test_bounds_reject_mutated_references():
    """every bound passes the restatement and rejects each listed kernel bug by at least 10 x"""
    film = dict(film=T, act=T, pool=F)
    c, x, gm, bt, em = _cpu_operands(film)
    N, H, W, C_ = c.shape
    mean, var, rstd = R.group_stats(x)
    m32, r32 = R.stats32(x)
    ref = R.forward_statement(x, gm, bt, em, **film)
    bound = R.forward_bound(x, gm, bt, em, **film)
    worst = lambda y, ref=ref, bound=bound: ((y - ref).abs() / bound).max().item()
    assert worst(R.forward_restatement(x, gm, bt, em, **film)) <= 1.0
    fwd = lambda stats=None, x_=x, e=em: R.forward_restatement(x_, gm, bt, e, **film, stats=stats)
    assert worst(fwd((m32.roll(1, 1), r32.roll(1, 1)))) > 10, "stats of the neighbouring group"
    cnt = H * W * C_ // 32
    assert worst(fwd((m32, 1.0 / torch.sqrt(var * cnt / (cnt - 1) + R.EPS)))) > 10, "unbiased variance"
    e_m, e_r = R.stats_error(mean, var)
    live = var > 0                                       # eps shows in rstd, which has its own bound (the constant group: 1 / 0)
    assert (((1.0 / torch.sqrt(var[live])) / rstd[live] - 1).abs() / e_r[live]).min() > 10, "variance without eps"
    assert (((1.0 / torch.sqrt(var * cnt / (cnt - 1) + R.EPS))[live] / rstd[live] - 1).abs() / e_r[live]).min() > 10, "unbiased variance"
    # statistics bounds: a dropped last row / last 8-channel vector of the group (wide groups: C = 512)
    cw, xw, _, _, _ = _cpu_operands(dict(film=F, act=T, pool=F), shape=(1, 6, 6, 512))
    mw, vw, rw = R.group_stats(xw)
    em_, er_ = R.stats_error(mw, vw)
    stats_ok = lambda m, r: bool(((m - mw).abs() <= em_).all() and ((r / rw - 1).abs() <= er_).all())
    assert stats_ok(*R.stats32(xw))
    short = xw.clone()
    short[:, -1] = 0                                     # the last row never summed, the divisor unchanged
    ms = R.group_mean(short)
    vs = R.group_mean(short * short) - ms * ms
    assert (((ms - mw).abs() / em_).max() > 10) and not stats_ok(ms, 1 / torch.sqrt(vs.clamp_min(0) + R.EPS)), "a dropped last row"
    short = xw.clone()
    short[..., torch.arange(512) % 16 >= 8] = 0
    ms = R.group_mean(short)
    assert ((ms - mw).abs() / em_).max() > 10, "a dropped last 8-channel vector"
    # FiLM
    sc_as_scale = em.clone()
    sc_as_scale[:, :C_] -= 1.0
    assert worst(fwd(e=sc_as_scale)) > 10, "sc = scale instead of 1 + scale"
    swapped = torch.cat([em[:, C_:2 * C_], em[:, :C_], em[:, 2 * C_:]], 1)
    assert worst(fwd(e=swapped)) > 10, "shift and scale swapped"
    # pool
    pl = dict(film=F, act=T, pool=T)
    refp, bp = R.forward_statement(x, gm, bt, None, **pl), R.forward_bound(x, gm, bt, None, **pl)
    full = R.forward_restatement(x, gm, bt, None, False, True, False)
    assert worst(R.f16r(R.pool2(full)), refp, bp) <= 1.0
    two = R.f16r(full.reshape(N, H // 2, 2, W // 2, 2, C_)[:, :, :, :, 0].mean(2))
    assert worst(two, refp, bp) > 10, "a pooled pixel from a 2x1 window"
    # backward
    g = torch.Generator().manual_seed(9)
    plain = dict(film=F, act=T)
    for gmode in (GB_SAME, GB_UNPOOL, GB_SUM4):
        cg = dataclasses.replace(c, gmode=gmode)
        gr = _f16(torch.randn(g_shape(cg), generator=g)).double()
        a2 = _f16(torch.randn(c.shape, generator=g)).double()
        refb = R.backward_statement(gr, x, gm, bt, None, **plain, gmode=gmode, add2=a2)
        bb = R.backward_bound(gr, x, gm, bt, None, **plain, gmode=gmode, add2=a2)
        ok = R.backward_restatement(gr, x, (m32, r32), gm, bt, None, **plain, gmode=gmode, add2=a2)
        assert worst(ok, refb, bb) <= 1.0
        no_a2 = R.backward_restatement(gr, x, (m32, r32), gm, bt, None, **plain, gmode=gmode)
        assert worst(no_a2, refb, bb) > 10, "a missing add2"
        shifted = torch.cat([ok[..., :32], ok[..., 32:].roll(8, 3)], -1)
        assert worst(shifted, refb, bb) > 10, "dx2 off by 8 channels"
        if gmode == GB_UNPOOL:
            assert worst(R.backward_restatement(4.0 * gr, x, (m32, r32), gm, bt, None, **plain, gmode=gmode, add2=a2), refb, bb) > 10, \
                "UNPOOL without the / 4"
        if gmode == GB_SUM4:
            three = gr.clone()
            three[:, 1::2, 1::2] = 0
            assert worst(R.backward_restatement(three, x, (m32, r32), gm, bt, None, **plain, gmode=gmode, add2=a2), refb, bb) > 10, \
                "SUM4 with three addends"
    # m2 without xhat: the second group mean formed from dyh alone
    gr = _f16(torch.randn(c.shape, generator=g)).double()
    refb = R.backward_statement(gr, x, gm, bt, None, **plain)
    bb = R.backward_bound(gr, x, gm, bt, None, **plain)
    mu, rs = R.per_channel(m32, C_), R.per_channel(r32, C_)
    dyh, xh = R.gn_bwd_ref(gr, x, mu, rs, gm, bt, 0.0, 0.0, False, True)
    m1 = R.per_channel(R.group_mean(dyh), C_)
    assert worst(R.f16r(rs * ((dyh - m1) - xh * R.per_channel(R.group_mean(dyh * xh), C_))), refb, bb) <= 1.0
    assert worst(R.f16r(rs * ((dyh - m1) - xh * m1)), refb, bb) > 10, "m2 without xhat"
    # slab sums
    sl = torch.randn(5, 1, 4, 4, 32, generator=g).double()
    bias = torch.randn(32, generator=g).double()
    s, a = R.slab_sum(sl, bias)
    ok = lambda v: ((v - s).abs() / R.materialised_bound(s, a)).max().item()
    assert ok(R.f16r(s)) <= 1.0
    assert ok(R.f16r(s - sl[-1])) > 10, "a slab sum missing its last slice"
    assert ok(R.f16r(s - bias)) > 10, "a slab sum missing its bias"
