"""Every implicit-GEMM kernel form, one launch at a time, against a float64 convolution on the CPU.

Each case in CASES is one launch through ishap_igemm_run (include/ishap.h). That call describes the launch with the
ConvLaunch record the executor's conv_op (csrc/unet.hip) uses and fills IgemmArgs with the same function (igemm_fill,
csrc/igemm.hip: fields, K split, deferred reduce), so the oracle launch and the layer launch go through one fill; then it launches. The result is compared with torch conv2d /
matmul in float64 of the same fp16 values, zero-padded per image. A case asserts four things:
  1. form: the kernel name the call reports is the case's expected name;
  2. values: |gpu - ref| <= 2^-11 |ref| + 2^-16 A for every element, where A = sum |x w| (+ |bias| + |bias2| + |res|) is the same
     reference on magnitudes. This covers one fp16 rounding plus fp32 accumulation. A dropped 64-wide K step, a wrong tap or
     a leaked border row is orders of magnitude over it (test_bounds_reject_mutated_references). NCHW fp32 output has no fp16 term;
  3. canaries: out, res and ws start as a NaN bit pattern. Whatever lies outside [M][N] at stride ldo (padding channels, the
     words in front of an offset pointer, the tail) keeps it bit for bit, and every written element is finite;
  4. sums: the GroupNorm statistics (stat_out) are checked against float64 sums of the kernel's own stored fp16 outputs, per
     (image, channel). The GroupNorm-backward sums (gb_csums) are checked against a float64 restatement of gn_bwd_term
     (csrc/gn_bwd_terms.h) with its fp16 rounding points (csrc/gn_act.h).
The CPU tests at the end check the table against the planner and against the IgemmForm enum. They check that out-of-contract
descriptors are refused before any HIP call, and that the bounds reject mutated references."""
import ctypes as C
import dataclasses
import os
import re
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.groupnorm_ref import gn_bwd_ref      # gn_bwd_term (csrc/gn_bwd_terms.h) in float64 with its fp16 rounding points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON_H = os.path.join(ROOT, "ishapediting_amd", "csrc", "common.h")

F16_REL = 2.0 ** -11          # one fp16 rounding of the result
ACC_REL = 2.0 ** -16          # fp32 accumulation, relative to the sum of magnitudes
SUM_REL, SUM_ABS = 1e-5, 1e-6
OUT_F16, OUT_NCHW_F32 = 0, 2
CANARY16 = 0x7E5A             # fp16 NaN
CANARY32 = 0x7FC0BEEF         # fp32 NaN
CANARY64 = 0x7FF8DEAD0BADF00D
TAIL = 256                    # canary elements behind every written buffer


def _stat_scales():
    src = open(COMMON_H).read()
    get = lambda k: float(re.search(rf"#define {k} ([0-9.]+)f", src).group(1))
    return get("STAT_SCALE_SUM"), get("STAT_SCALE_SQ")


STAT_SCALE_SUM, STAT_SCALE_SQ = _stat_scales()


@dataclasses.dataclass(frozen=True)
class Case:
    form: str                   # the IgemmForm (common.h) this case proves
    shape: tuple                # (M, Cin, N, taps, K2, H, W, pending, epilogue sums): ishap_igemm_plan's arguments
    kernel: str                 # expected kernel name
    ksplit: int                 # expected K split
    ldx: int = 0                # 0: Cin; more: a channel slice of a wider activation (the lazy skip concatenation)
    ldo: int = 0                # 0: N; more: canary channels between output rows
    out_ofs: int = 0            # halfs in front of the output pointer (4 = 8 bytes: the fragment-layout epilogue)
    res: str = ""               # "", "sep" (own buffer), "alias" (res = out, in place), "ups" (half-resolution residual)
    bias: bool = True
    ups: bool = False           # half-size source, upsampled on the fly
    nchw: bool = False          # fp32 NCHW output (the head)
    gb: str = ""                # GroupNorm-backward sums instead of statistics: "plain", "film", "act", "film+act"
    chunk: int = 0              # chunk_tiles
    reduce_res: str = ""        # pending launches: the residual of the ishap_igemm_reduce run ("", "sep", "ups")

    @property
    def M(self): return self.shape[0]
    @property
    def Cin(self): return self.shape[1]
    @property
    def N(self): return self.shape[2]
    @property
    def taps(self): return self.shape[3]
    @property
    def K2(self): return self.shape[4]
    @property
    def H(self): return self.shape[5]
    @property
    def W(self): return self.shape[6]
    @property
    def pending(self): return self.shape[7]
    @property
    def stats(self): return self.shape[8] and not self.gb
    @property
    def imgs(self): return self.M // (self.H * self.W)
    @property
    def K(self): return self.taps * self.Cin + self.K2
    @property
    def lx(self): return self.ldx or self.Cin
    @property
    def lo(self): return self.ldo or self.N
    @property
    def xrows(self): return self.M // 4 if self.ups else self.M
    @property
    def npad(self): return (self.N + 127) // 128 * 128


_H64, _H32 = "igemm4_halo_kernel<64, 6>", "igemm4_halo_kernel<32, 6>"
_BIG128, _BIG64 = "igemm4_kernel<128, 128, 128, 5, 3, 1>", "igemm4_kernel<128, 128, 64, 5, 3, 1>"
CASES = {
    "halo 64^2, stats, chunks of 128": Case("ig4_halo", (4096, 256, 256, 9, 0, 64, 64, 0, 1), _H64, 1, res="sep", chunk=128),
    "halo 64^2, GN-backward sums, FiLM + SiLU": Case("ig4_halo", (4096, 256, 256, 9, 0, 64, 64, 0, 1), _H64, 1, gb="film+act"),
    "halo 32^2, two images, stats, ldx > Cin, ldo > N": Case("ig4_halo", (2048, 128, 512, 9, 0, 32, 32, 0, 1), _H32, 1, ldx=192,
                                                             ldo=520),
    "halo 32^2 split: stats in the reduce, in place": Case("ig4_halo", (1024, 512, 256, 9, 0, 32, 32, 0, 1), _H32, 4, res="alias"),
    "halo 32^2 split: GN-backward sums in the reduce, SiLU": Case("ig4_halo", (1024, 512, 256, 9, 0, 32, 32, 0, 1), _H32, 4,
                                                                  gb="act"),
    "128-tile head: N = 192, NCHW fp32": Case("ig4_128", (16384, 768, 192, 9, 0, 128, 128, 0, 0), _BIG128, 1, nchw=True),
    "128-tile, folded source + bias2, chunks of 64": Case("ig4_128", (16384, 256, 256, 9, 512, 128, 128, 0, 0), _BIG128, 1,
                                                          chunk=64),
    "128-tile, upsampled source, ldx > Cin": Case("ig4_128", (16384, 256, 256, 9, 0, 128, 128, 0, 0), _BIG128, 1, ups=True,
                                                  ldx=320, res="sep"),
    "128-tile, 8 images, 2 rows per tile, stats": Case("ig4_128", (32768, 128, 192, 9, 0, 64, 64, 0, 1), _BIG64, 1, res="sep"),
    "128-tile, 8 images, GN-backward sums, fragment epilogue": Case("ig4_128", (32768, 128, 192, 9, 0, 64, 64, 0, 1), _BIG64, 1,
                                                                    gb="plain", out_ofs=4),
    "128x64 tiles, stats, in place": Case("ig4_tall", (4096, 512, 512, 9, 0, 64, 64, 0, 1), "igemm4_kernel<128, 64, 64, 6, 3, 1>", 1,
                                          res="alias"),
    "two-team, uneven chunks, stats": Case("ig4_teams", (1024, 1344, 512, 9, 0, 32, 32, 0, 1), "igemm4_kernel<64, 64, 32, 6, 3, 2>",
                                           2),
    "6-slot ring, 8 slices, stats in the reduce": Case("ig4_64", (256, 1536, 768, 9, 0, 16, 16, 0, 1),
                                                       "igemm4_kernel<64, 64, 16, 6, 3, 1>", 8, res="sep"),
    "4-slot ring, pending slices, reduce with res_ups": Case("ig4_64_ring4", (256, 512, 512, 9, 0, 16, 16, 1, 0),
                                                             "igemm4_kernel<64, 64, 16, 4, 3, 1>", 8, reduce_res="ups"),
    "8x8 maps, folded source, pending slices": Case("ig4_w8", (64, 1024, 1024, 9, 2048, 8, 8, 1, 0),
                                                    "igemm4_kernel<64, 64, 8, 4, 3, 1>", 16, reduce_res="sep"),
    "64-tile, N = 12, split": Case("ig4_64", (4096, 384, 12, 9, 0, 64, 64, 0, 0), "igemm4_kernel<64, 64, 64, 6, 3, 1>", 4, ldo=16),
    "igemm2 128-tile 1x1, fragment epilogue, ldx > Cin": Case("ig2_128", (32768, 128, 128, 1, 0, 64, 64, 0, 0),
                                                              "igemm2_kernel<128, 128, 4, false, 1>", 1, ldx=192, out_ofs=4,
                                                              res="sep"),
    "igemm2 128-tile 3x3 on 512 8x8 images": Case("ig2_128", (32768, 128, 128, 9, 0, 8, 8, 0, 0),
                                                  "igemm2_kernel<128, 128, 4, true, 1>", 1),
    "igemm2 64-tile, folded source + bias2": Case("ig2_64", (4096, 256, 512, 9, 512, 64, 64, 0, 0),
                                                  "igemm2_kernel<64, 64, 4, true, 1>", 1, res="sep"),
    "igemm2 64-tile 1x1, N = 36, ldx > Cin, ldo > N": Case("ig2_64", (4096, 256, 36, 1, 0, 64, 64, 0, 0),
                                                           "igemm2_kernel<64, 64, 4, false, 1>", 1, ldx=384, ldo=40),
    "igemm2 sliced 1x1, pending": Case("ig2_64", (64, 3072, 1024, 1, 0, 8, 8, 1, 0), "igemm2_kernel<64, 64, 4, false, 1>", 16,
                                       reduce_res="sep"),
    "igemm2 two-team, folded source": Case("ig2_teams", (1024, 512, 512, 9, 1280, 32, 32, 0, 0),
                                           "igemm2_kernel<64, 64, 4, true, 2>", 2),
    "igemm2 two-team, 24x24 map, stats": Case("ig2_teams", (576, 128, 128, 9, 0, 24, 24, 0, 1),
                                              "igemm2_kernel<64, 64, 4, true, 2>", 1, res="sep"),
    "skinny 1x1": Case("skinny", (64, 1024, 1024, 1, 0, 8, 8, 0, 0), "igemm_skinny_kernel<2, false>", 1, res="sep"),
    "skinny 1x1, N = 12": Case("skinny", (64, 1024, 12, 1, 0, 8, 8, 0, 0), "igemm_skinny_kernel<2, false>", 1, ldo=16),
    "BK = 32, 3x3, N = 12": Case("reg32", (4096, 96, 12, 9, 0, 64, 64, 0, 0), "igemm_kernel<64, 64, 32, 2, 2, true>", 1, ldo=16),
    "BK = 32, 1x1, res_ups": Case("reg32", (4096, 96, 256, 1, 0, 64, 64, 0, 0), "igemm_kernel<64, 64, 32, 2, 2, false>", 1,
                                  res="ups"),
    "BK = 32, 3x3, N = 4, Cin = 32": Case("reg32", (1024, 32, 4, 9, 0, 32, 32, 0, 0), "igemm_kernel<64, 64, 32, 2, 2, true>", 1,
                                          ldx=40, ldo=8, res="sep"),
}


# ---------------------------------------------------------------------------------------------------------------- operands
def _f16(t):
    return t.to(torch.float16)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def make_inputs(c: Case):
    """fp16 operands of a case (CPU), seeded by the shape: cases of one shape share operands and reference"""
    g = _gen(hash(("x",) + c.shape[:7] + (c.lx, c.ups)) & 0x7FFFFFFF)
    X = torch.full((c.xrows, c.lx), float("nan"), dtype=torch.float16)     # columns >= Cin are never read
    X[:, :c.Cin] = _f16(0.5 + 0.5 * torch.randn(c.xrows, c.Cin, generator=g))
    s = 1.0 / np.sqrt(c.K)
    w = _f16((torch.randn(c.N, c.Cin, 3, 3, generator=g) + 0.2) * s) if c.taps == 9 else _f16((torch.randn(c.N, c.Cin, generator=g)
                                                                                                + 0.2) * s)
    X2 = W2 = None
    if c.K2:
        X2 = _f16(0.3 + 0.5 * torch.randn(c.M, c.K2, generator=g))
        W2 = _f16((torch.randn(c.N, c.K2, generator=g) + 0.2) * s)
    return X, w, X2, W2


def pack_weights(w, W2, npad):
    """[round_up(N, 128)][ldw] fp16, column tap * Cin + c (tap = 3 ky + kx), the folded source's K2 columns after, rows >= N
    zero (pack_conv_weight, csrc/misc.hip)"""
    N = w.shape[0]
    cols = w.permute(0, 2, 3, 1).reshape(N, -1) if w.dim() == 4 else w
    if W2 is not None:
        cols = torch.cat([cols, W2], 1)
    out = torch.zeros(npad, cols.shape[1], dtype=torch.float16)
    out[:N] = cols
    return out


def conv_ref(c: Case, X, w, X2, W2, magnitude=False):
    """float64 [M][N]: the 3x3 (zero padding per image) or 1x1 convolution of the fp16 operands (+ the folded source);
    magnitude: the same on |x|, |w|"""
    f = (lambda t: t.double().abs()) if magnitude else (lambda t: t.double())
    x = f(X[:, :c.Cin])
    if c.taps == 1:
        y = x @ f(w).t()
    else:
        hs, wsrc = (c.H // 2, c.W // 2) if c.ups else (c.H, c.W)
        x = x.reshape(c.imgs, hs, wsrc, c.Cin).permute(0, 3, 1, 2)
        if c.ups:
            x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
        y = F.conv2d(x, f(w), padding=1).permute(0, 2, 3, 1).reshape(c.M, c.N)
    if X2 is not None:
        y = y + f(X2) @ f(W2).t()
    return y


_REF_CACHE = {}


def reference(c: Case, ops):
    key = c.shape[:7] + (c.lx, c.ups)
    if key not in _REF_CACHE:
        _REF_CACHE.clear()
        _REF_CACHE[key] = (conv_ref(c, *ops), conv_ref(c, *ops, magnitude=True))
    return _REF_CACHE[key]


def upsample_rows(t, imgs, H, W):
    """rows of a (H/2, W/2) map -> rows of the (H, W) map (nearest neighbour)"""
    C_ = t.shape[1]
    t = t.reshape(imgs, H // 2, W // 2, C_).repeat_interleave(2, 1).repeat_interleave(2, 2)
    return t.reshape(imgs * H * W, C_)


def value_ratio(gpu, ref, mag, f16=True):
    """|gpu - ref| / (2^-11 |ref| + 2^-16 A) per element (<= 1 passes); gpu, ref, mag float64 tensors"""
    bound = ACC_REL * mag + (F16_REL * ref.abs() if f16 else 0.0)
    return (gpu - ref).abs() / bound


def sums_ratio(got, want, scale_terms):
    """|got - want| / (1e-5 sum |term| + 1e-6) per entry"""
    return (got - want).abs() / (SUM_REL * scale_terms + SUM_ABS)


def stat_ref(y, imgs):
    """(sum, sum of squares, sum |y|) per (image, channel) of stored outputs y [M][N] (float64)"""
    y = y.reshape(imgs, -1, y.shape[1])
    return y.sum(1), (y * y).sum(1), y.abs().sum(1)


def f16r(t):
    return t.to(torch.float16).double()


def gb_operands(c: Case):
    g = _gen(7 + c.M + c.N)
    N, imgs = c.N, c.imgs
    gx = _f16(0.3 + torch.randn(c.M, N, generator=g))
    stats = torch.empty(imgs, 32, 2)
    stats[..., 0] = 0.3 + 0.1 * torch.randn(imgs, 32, generator=g)
    stats[..., 1] = 1.0 / (0.8 + 0.4 * torch.rand(imgs, 32, generator=g))
    gamma = 1.0 + 0.3 * torch.randn(N, generator=g)
    beta = 0.2 * torch.randn(N, generator=g)
    emb_ld = 2 * N + 8
    emb = 0.4 * torch.randn(imgs, emb_ld, generator=g)
    return gx, stats, gamma, beta, emb, emb_ld


def gb_sums_ref(c: Case, y, gx, stats, gamma, beta, emb):
    """per (image, channel): sum dyh, sum dyh * xhat and their magnitude sums, from the stored gradient y [M][N]"""
    film, act = "film" in c.gb, "act" in c.gb
    imgs, HW, N = c.imgs, c.H * c.W, c.N
    grp = torch.arange(N) // (N // 32)
    st = stats.double()
    mu = st[:, grp, 0][:, None, :]                   # [imgs][1][N]
    rs = st[:, grp, 1][:, None, :]
    esc = emb.double()[:, None, :N]
    esh = emb.double()[:, None, N:2 * N]
    dyh, xhat = gn_bwd_ref(y.reshape(imgs, HW, N), gx.double().reshape(imgs, HW, N), mu, rs, gamma.double(), beta.double(), esc,
                           esh, film, act)
    t1, t2 = dyh, dyh * xhat
    return t1.sum(1), t2.sum(1), t1.abs().sum(1), t2.abs().sum(1)


# ---------------------------------------------------------------------------------------------------------------- the call
def _buf(t, ofs_elems=0):
    from ishapediting_amd._lib import IgemmBufC
    if t is None:
        return IgemmBufC(None, 0)
    es = t.element_size()
    return IgemmBufC(t.data_ptr() + ofs_elems * es, (t.numel() - ofs_elems) * es)


def make_desc(c: Case, bufs, ldr=0):
    """ishap_igemm_desc of a case; bufs: name -> (tensor, element offset) or tensor"""
    from ishapediting_amd._lib import IgemmDescC
    d = IgemmDescC()
    d.M, d.N, d.Cin, d.taps, d.K2, d.H, d.W = c.M, c.N, c.Cin, c.taps, c.K2, c.H, c.W
    d.ldx, d.ldx2, d.ldw, d.ldo, d.ldr = c.lx, c.K2, c.K, c.lo, ldr
    d.ups, d.res_ups = int(c.ups), int(c.res == "ups")
    d.out_mode = OUT_NCHW_F32 if c.nchw else OUT_F16
    d.pending, d.chunk_tiles = c.pending, c.chunk
    for name, v in bufs.items():
        if name in ("gb_emb_ld", "gb_film", "gb_act"):
            setattr(d, name, v)
        else:
            setattr(d, name, _buf(*v) if isinstance(v, tuple) else _buf(v))
    return d


def _canary(n, dtype):
    bits = {torch.float16: (torch.int16, CANARY16), torch.float32: (torch.int32, CANARY32), torch.int64: (torch.int64, CANARY64)}
    it, v = bits[dtype]
    if it == torch.int16:
        v = v - (1 << 16) if v >= 1 << 15 else v
    return torch.full((n,), v, dtype=it).view(dtype)


def _bits(t):
    return t.view({torch.float16: torch.int16, torch.float32: torch.int32, torch.int64: torch.int64}[t.dtype])


def _out_mask(c: Case, n_total):
    """True at the elements a launch writes: out[m][n] at out_ofs + m * ldo + n, n < N (fp16 rows) / all M*N (NCHW)"""
    mask = torch.zeros(n_total, dtype=torch.bool)
    if c.nchw:
        mask[:c.M * c.N] = True
    else:
        mask[c.out_ofs:c.out_ofs + c.M * c.lo].view(c.M, c.lo)[:, :c.N] = True
    return mask


def _check_canaries(name, flat_cpu, mask):
    b = _bits(flat_cpu)
    keep = _canary(1, flat_cpu.dtype)
    bad = (b[~mask] != _bits(keep)[0]).sum().item()
    assert bad == 0, f"{name}: {bad} elements outside the written region lost their canary"
    nonfin = (~torch.isfinite(flat_cpu[mask].float())).sum().item()
    assert nonfin == 0, f"{name}: {nonfin} written elements are not finite"


def run_case(c: Case):
    from ishapediting_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    t0 = time.time()
    X, w, X2, W2 = make_inputs(c)
    Wt = pack_weights(w, W2, c.npad)
    g = _gen(11 + c.M + 3 * c.N + c.K)
    bias = (0.5 * torch.randn(c.N, generator=g)) if c.bias else None
    bias2 = (0.5 * torch.randn(c.N, generator=g)) if c.K2 else None
    res_rows = c.M // 4 if c.res == "ups" else c.M
    res_vals = _f16(torch.randn(res_rows, c.N, generator=g)) if c.res else None

    # device buffers; every written one starts as canaries
    dX, dWt = X.to(dev), Wt.to(dev)
    dX2 = X2.to(dev) if X2 is not None else None
    if c.nchw:
        out = _canary(c.M * c.N + TAIL, torch.float32)
    else:
        out = _canary(c.out_ofs + c.M * c.lo + TAIL, torch.float16)
        if c.res == "alias":        # in place: the residual is the output buffer's current contents
            out[c.out_ofs:c.out_ofs + c.M * c.lo].view(c.M, c.lo)[:, :c.N] = res_vals
    out = out.to(dev)
    bufs = {"X": dX, "Wt": dWt, "out": (out, c.out_ofs)}
    ldr = 0
    res_dev = None
    if c.K2:
        bufs["X2"] = dX2
    if bias is not None:
        bufs["bias"] = bias.to(dev)
    if bias2 is not None:
        bufs["bias2"] = bias2.to(dev)
    if c.res == "alias":
        bufs["res"], ldr = (out, c.out_ofs), c.lo
    elif c.res:
        ldr = c.N + 8                                        # padding channels between residual rows: canaries, never read
        res_dev = _canary(res_rows * ldr + TAIL, torch.float16)
        res_dev[:res_rows * ldr].view(res_rows, ldr)[:, :c.N] = res_vals
        res_dev = res_dev.to(dev)
        res_before = res_dev.cpu().clone()
        bufs["res"] = res_dev
    ws = None
    if c.ksplit > 1:
        ws = _canary(c.ksplit * c.M * c.N + TAIL, torch.float32).to(dev)
        bufs["ws"] = ws
    stat = gbc = None
    if c.stats:
        stat = torch.zeros(c.imgs * c.N * 2 + TAIL, dtype=torch.int64)
        stat[c.imgs * c.N * 2:] = _canary(TAIL, torch.int64)
        stat = stat.to(dev)
        bufs["stat_out"] = stat
    if c.gb:
        gx, gst, gam, bet, emb, emb_ld = gb_operands(c)
        gbc = torch.zeros(c.imgs * c.N * 2 + TAIL, dtype=torch.int64)
        gbc[c.imgs * c.N * 2:] = _canary(TAIL, torch.int64)
        gbc = gbc.to(dev)
        bufs.update(gb_x=gx.to(dev), gb_stats=gst.to(dev), gb_gamma=gam.float().to(dev), gb_beta=bet.float().to(dev),
                    gb_emb=emb.float().to(dev), gb_csums=gbc, gb_emb_ld=emb_ld, gb_film=int("film" in c.gb),
                    gb_act=int("act" in c.gb))
    d = make_desc(c, bufs, ldr)
    ks, kern = C.c_int(), C.create_string_buffer(96)
    stream = _lib.stream_ptr(dev)
    _lib.check(L.ishap_igemm_run(C.byref(d), 1, stream, C.byref(ks), kern, len(kern)))
    torch.cuda.synchronize()
    name = kern.value.decode()
    assert (name, ks.value) == (c.kernel, c.ksplit), f"ran {name} with {ks.value} slices"

    conv, mag = reference(c, (X, w, X2, W2))
    worst = {}
    if c.pending and c.ksplit > 1:
        # the slices themselves: finite, the tail untouched, their sum the plain product
        wsc = ws.cpu()
        _check_canaries("ws", wsc, torch.arange(wsc.numel()) < c.ksplit * c.M * c.N)
        slices = wsc[:c.ksplit * c.M * c.N].view(c.ksplit, c.M, c.N).double().sum(0)
        r = value_ratio(slices, conv, mag, f16=False)
        worst["slices"] = r.max().item()
        assert worst["slices"] <= 1.0, f"slice sum off by {worst['slices']:.3g} x the bound"
        assert _bits(out.cpu()).eq(_bits(_canary(1, out.dtype))[0]).all(), "a pending launch wrote its output"
        # then the stand-alone reduce (slab_materialize) with bias, bias2 and its own residual
        rr = c.reduce_res
        res_rows = c.M // 4 if rr == "ups" else c.M
        res_vals = _f16(torch.randn(res_rows, c.N, generator=g)) if rr else None
        rd = {"out": (out, c.out_ofs), "ws": ws}
        if bias is not None:
            rd["bias"] = bufs["bias"]
        if bias2 is not None:
            rd["bias2"] = bufs["bias2"]
        if rr:
            rd["res"] = res_vals.to(dev)
        d = make_desc(dataclasses.replace(c, res="ups" if rr == "ups" else ""), rd, c.N if rr else 0)
        _lib.check(L.ishap_igemm_reduce(C.byref(d), c.ksplit, 1, stream))
        torch.cuda.synchronize()
        c = dataclasses.replace(c, res=rr)

    # the epilogue in float64: + bias + bias2 + residual
    ref, A = conv.clone(), mag.clone()
    for b in (bias, bias2):
        if b is not None:
            ref += b.double()
            A += b.double().abs()
    if c.res:
        rv = res_vals.double()
        if c.res == "ups":
            rv = upsample_rows(rv, c.imgs, c.H, c.W)
        ref += rv
        A += rv.abs()
    oc = out.cpu()
    _check_canaries("out", oc, _out_mask(c, oc.numel()))
    if c.nchw:
        y = oc[:c.M * c.N].view(c.imgs, c.N, c.H * c.W).permute(0, 2, 1).reshape(c.M, c.N).double()
    else:
        y = oc[c.out_ofs:c.out_ofs + c.M * c.lo].view(c.M, c.lo)[:, :c.N].double()
    r = value_ratio(y, ref, A, f16=not c.nchw)
    worst["out"] = r.max().item()
    if worst["out"] > 1.0:
        m, n = divmod(int(r.argmax()), c.N)
        bad = (r > 1).nonzero()
        raise AssertionError(f"{(r > 1).sum().item()} elements over the bound (worst {worst['out']:.3g} x at m={m}, n={n}: "
                             f"gpu {y[m, n].item():.6g}, ref {ref[m, n].item():.6g}; rows {bad[:, 0].min().item()}.."
                             f"{bad[:, 0].max().item()}, channels {bad[:, 1].min().item()}..{bad[:, 1].max().item()})")
    if res_dev is not None:
        assert torch.equal(_bits(res_dev.cpu()), _bits(res_before)), "the residual buffer changed"
    if ws is not None and not c.pending:
        wsc = ws.cpu()
        _check_canaries("ws tail", wsc[c.ksplit * c.M * c.N:], torch.zeros(TAIL, dtype=torch.bool))
    if c.stats:
        sc = stat.cpu()
        assert torch.equal(sc[c.imgs * c.N * 2:], _canary(TAIL, torch.int64)), "stat_out tail overwritten"
        st = sc[:c.imgs * c.N * 2].view(c.imgs, c.N, 2).double()
        s, q, sa = stat_ref(y, c.imgs)
        worst["sum"] = sums_ratio(st[..., 0] / STAT_SCALE_SUM, s, sa).max().item()
        worst["sumsq"] = sums_ratio(st[..., 1] / STAT_SCALE_SQ, q, q).max().item()
        assert worst["sum"] <= 1 and worst["sumsq"] <= 1, f"statistics off: {worst}"
    if c.gb:
        gc = gbc.cpu()
        assert torch.equal(gc[c.imgs * c.N * 2:], _canary(TAIL, torch.int64)), "gb_csums tail overwritten"
        got = gc[:c.imgs * c.N * 2].view(c.imgs, c.N, 2).double() / STAT_SCALE_SUM
        s1, s2, a1, a2 = gb_sums_ref(c, y, gx, gst, gam, bet, emb)
        worst["gb1"] = sums_ratio(got[..., 0], s1, a1).max().item()
        worst["gb2"] = sums_ratio(got[..., 1], s2, a2).max().item()
        assert worst["gb1"] <= 1 and worst["gb2"] <= 1, f"GroupNorm-backward sums off: {worst}"
    return name, ks.value, worst, time.time() - t0


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_kernel_form_matches_fp64_convolution(case):
    name, ks, worst, dt = run_case(CASES[case])
    print(f"\n  {name} ksplit {ks}: worst / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" ({dt:.1f} s)")


# ---------------------------------------------------------------------------------------------------------------- CPU checks
def _forms_in_common_h():
    src = open(COMMON_H).read()
    body = re.search(r"enum class IgemmForm \{(.*?)\};", src, re.S).group(1)
    return {m for m in re.findall(r"^\s*(\w+),", body, re.M)}


def form_of_kernel(name):
    """the IgemmForm a kernel instance belongs to (igemm_launch_main's naming)"""
    if name.startswith("igemm_skinny_kernel<"):
        return "skinny"
    if name.startswith("igemm_kernel<"):
        return "reg32"
    if name.startswith("igemm4_halo_kernel<"):
        return "ig4_halo"
    p = [int(v) if v.strip().lstrip("-").isdigit() else v.strip() for v in name[name.index("<") + 1:-1].split(",")]
    if name.startswith("igemm2_kernel<"):
        return "ig2_128" if p[0] == 128 else ("ig2_teams" if p[4] == 2 else "ig2_64")
    bm, bn, wd, nstw, _, halves = p
    if bm == 128:
        return "ig4_128" if bn == 128 else "ig4_tall"
    if wd == 8:
        return "ig4_w8"
    if halves == 2:
        return "ig4_teams"
    return "ig4_64_ring4" if nstw == 4 else "ig4_64"


def test_table_covers_every_form():
    forms = _forms_in_common_h()
    assert len(forms) == 12, forms
    assert {c.form for c in CASES.values()} == forms, "a kernel form without a per-launch oracle case (or a stale one)"
    for n, c in CASES.items():
        assert form_of_kernel(c.kernel) == c.form, n


def _plan(shape):
    from ishapediting_amd import _lib
    L = _lib.lib()
    ks, slot, kern = C.c_int(), C.c_int(), C.create_string_buffer(96)
    M, cin, cout, taps, k2, h, w, pending, sums = shape
    _lib.check(L.ishap_igemm_plan(M, cin, cout, taps, k2, h, w, 1, pending, sums, C.byref(ks), C.byref(slot), kern, len(kern)))
    return kern.value.decode(), ks.value


class _Fake:
    """a stand-in device buffer for descriptor checks without a GPU: an address and a size, nothing behind it"""
    _next = 1 << 40

    def __init__(self, numel, dtype):
        self.numel_, self.es = numel, torch.empty(0, dtype=dtype).element_size()
        self.addr = _Fake._next
        _Fake._next += (numel * self.es + (1 << 20)) // (1 << 20) * (1 << 20) + (1 << 20)

    def data_ptr(self): return self.addr
    def element_size(self): return self.es
    def numel(self): return self.numel_


def fake_bufs(c: Case):
    """buffers of exactly the sizes run_case allocates, as _Fake stand-ins, and the residual stride"""
    h, f, i64 = torch.float16, torch.float32, torch.int64
    b = {"X": _Fake(c.xrows * c.lx, h), "Wt": _Fake(c.npad * c.K, h),
         "out": (_Fake(c.M * c.N + TAIL, f), 0) if c.nchw else (_Fake(c.out_ofs + c.M * c.lo + TAIL, h), c.out_ofs)}
    if c.K2:
        b["X2"] = _Fake(c.M * c.K2, h)
    if c.bias:
        b["bias"] = _Fake(c.N, f)
    if c.K2:
        b["bias2"] = _Fake(c.N, f)
    ldr = 0
    if c.res == "alias":
        b["res"], ldr = b["out"], c.lo
    elif c.res:
        ldr = c.N + 8
        b["res"] = _Fake((c.M // 4 if c.res == "ups" else c.M) * ldr + TAIL, h)
    if c.ksplit > 1:
        b["ws"] = _Fake(c.ksplit * c.M * c.N + TAIL, f)
    if c.stats:
        b["stat_out"] = _Fake(c.imgs * c.N * 2 + TAIL, i64)
    if c.gb:
        b.update(gb_x=_Fake(c.M * c.N, h), gb_stats=_Fake(c.imgs * 64, f), gb_gamma=_Fake(c.N, f), gb_beta=_Fake(c.N, f),
                 gb_emb=_Fake(c.imgs * (2 * c.N + 8), f), gb_csums=_Fake(c.imgs * c.N * 2 + TAIL, i64), gb_emb_ld=2 * c.N + 8,
                 gb_film=int("film" in c.gb), gb_act=int("act" in c.gb))
    return b, ldr


def _dry(d):
    from ishapediting_amd import _lib
    L = _lib.lib()
    ks, kern = C.c_int(), C.create_string_buffer(96)
    rc = L.ishap_igemm_run(C.byref(d), 0, None, C.byref(ks), kern, len(kern))
    msg = L.ishap_last_error()
    return rc, kern.value.decode(), ks.value, (msg.decode() if msg else "")


@pytest.mark.parametrize("case", list(CASES))
def test_table_matches_the_planner(case):
    """each expected name is what the planner picks for the shape, and what ishap_igemm_run plans for the case's own descriptor"""
    c = CASES[case]
    assert _plan(c.shape) == (c.kernel, c.ksplit)
    bufs, ldr = fake_bufs(c)
    rc, name, ks, msg = _dry(make_desc(c, bufs, ldr))
    assert rc == 0, msg
    assert (name, ks) == (c.kernel, c.ksplit)


def need_bytes(c: Case, name, ldr=0):
    """the bytes of buffer `name` a launch of case c touches (the contract ishap_igemm_run checks)"""
    rrows = c.M // 4 if c.res == "ups" else c.M
    return {"X": ((c.xrows - 1) * c.lx + c.Cin) * 2, "X2": c.M * c.K2 * 2, "Wt": c.npad * c.K * 2,
            "out": c.M * c.N * 4 if c.nchw else ((c.M - 1) * c.lo + c.N) * 2, "res": ((rrows - 1) * ldr + c.N) * 2,
            "ws": c.ksplit * c.M * c.N * 4, "stat_out": c.imgs * c.N * 16, "gb_csums": c.imgs * c.N * 16,
            "gb_emb": ((c.imgs - 1) * (2 * c.N + 8) + 2 * c.N) * 4}[name]


def _mutants():
    """(what, case, change to the descriptor, words of the expected message); `short` mutants run twice: at exactly the bytes
    the launch touches (accepted) and one byte less (refused)"""
    halo = CASES["halo 32^2 split: stats in the reduce, in place"]
    n12 = CASES["64-tile, N = 12, split"]
    gb = CASES["halo 64^2, GN-backward sums, FiLM + SiLU"]
    short = lambda name: ("short", name)
    return [
        ("X", halo, short("X"), "X: needs"),
        ("upsampled source, ldx > Cin", CASES["128-tile, upsampled source, ldx > Cin"], short("X"), "X: needs"),
        ("X2", CASES["igemm2 64-tile, folded source + bias2"], short("X2"), "X2: needs"),
        ("weights: round_up(N, 128) rows", n12, short("Wt"), "Wt ("),
        ("output, ldo > N", n12, short("out"), "out: needs"),
        ("output at an offset, ldo > N", CASES["igemm2 128-tile 1x1, fragment epilogue, ldx > Cin"], short("out"), "out: needs"),
        ("NCHW output", CASES["128-tile head: N = 192, NCHW fp32"], short("out"), "out: needs"),
        ("half-resolution residual", CASES["BK = 32, 1x1, res_ups"], short("res"), "res: needs"),
        ("workspace", halo, short("ws"), "ws ("),
        ("stat_out", CASES["halo 32^2, two images, stats, ldx > Cin, ldo > N"], short("stat_out"), "stat_out ("),
        ("gb_csums", gb, short("gb_csums"), "gb_csums ("),
        ("gb_emb", gb, short("gb_emb"), "gb_emb: needs"),
        ("ldo not a multiple of 4", n12, lambda d: setattr(d, "ldo", 14), "ldo"),
        ("output pointer 2 bytes off", n12, lambda d: setattr(d.out, "ptr", d.out.ptr + 2), "out: needs"),
        ("residual pointer 2 bytes off", CASES["skinny 1x1"], lambda d: setattr(d.res, "ptr", d.res.ptr + 2), "res: needs"),
        ("ldx not a multiple of 8", CASES["BK = 32, 3x3, N = 4, Cin = 32"], lambda d: setattr(d, "ldx", 36), "ldx"),
        ("ldx below Cin", halo, lambda d: setattr(d, "ldx", 256), "ldx"),
        ("chunk_tiles = 12", CASES["halo 64^2, stats, chunks of 128"], lambda d: setattr(d, "chunk_tiles", 12), "chunk_tiles"),
        ("gb_* together with stat_out", gb, lambda d: setattr(d, "stat_out", d.gb_csums), "exclusive"),
        ("M not whole images", n12, lambda d: setattr(d, "M", 4032), "images"),
        ("taps = 4", n12, lambda d: setattr(d, "taps", 4), "taps"),
    ]


@pytest.mark.parametrize("i", range(len(_mutants())))
def test_run_rejects_out_of_contract_input(i):
    """refused before any HIP call (launch = 0 throughout: nothing here can reach a kernel)"""
    what, c, mutate, words = _mutants()[i]
    bufs, ldr = fake_bufs(c)
    d = make_desc(c, bufs, ldr)
    rc, _, _, msg = _dry(d)
    assert rc == 0, msg                  # the unchanged descriptor passes: the refusal below is the mutation's
    if isinstance(mutate, tuple):
        buf = getattr(d, mutate[1])
        buf.bytes = need_bytes(c, mutate[1], ldr)
        rc, _, _, msg = _dry(d)
        assert rc == 0, (what, "exactly the bytes touched", msg)
        buf.bytes -= 1
    else:
        mutate(d)
    rc, _, _, msg = _dry(d)
    assert rc != 0, what
    assert "requirement failed" in msg and words in msg, (what, msg)


def test_reduce_rejects_out_of_contract_input():
    from ishapediting_amd import _lib
    L = _lib.lib()
    c = CASES["4-slot ring, pending slices, reduce with res_ups"]
    bufs, _ = fake_bufs(c)
    bufs["res"] = _Fake(c.M // 4 * c.N + TAIL, torch.float16)
    assert L.ishap_igemm_reduce(C.byref(make_desc(dataclasses.replace(c, res="ups"), bufs, c.N)), 8, 0, None) == 0
    for what, nslab, mutate, words in [
        ("one slice", 1, None, "nslab"),
        ("workspace one float short", 8, lambda d: setattr(d.ws, "bytes", d.ws.bytes - 4 * (TAIL + 1)), "ws"),
        ("output one element short", 8, lambda d: setattr(d.out, "bytes", d.out.bytes - 2 * (TAIL + 1)), "out"),
        ("half-resolution residual one element short", 8, lambda d: setattr(d.res, "bytes", d.res.bytes - 2 * (TAIL + 1)), "res"),
        ("statistics", 8, lambda d: setattr(d, "stat_out", d.ws), "epilogue sums"),
    ]:
        bufs, _ = fake_bufs(c)
        bufs["res"] = _Fake(c.M // 4 * c.N + TAIL, torch.float16)
        d = make_desc(dataclasses.replace(c, res="ups"), bufs, c.N)
        if mutate:
            mutate(d)
        rc = L.ishap_igemm_reduce(C.byref(d), nslab, 0, None)
        msg = L.ishap_last_error().decode()
        assert rc != 0 and "requirement failed" in msg and words in msg, (what, rc, msg)


def _small_case(**kw):
    return Case("ig4_64", kw.pop("shape", (512, 128, 64, 9, 0, 16, 16, 0, 1)), "", 1, **kw)


def test_pack_and_reference_follow_the_kernels_k_order():
    """the packed weights with k = tap * Cin + c against a direct sum over the 3x3 window: the same convention the kernels use"""
    c = _small_case(shape=(128, 32, 8, 9, 64, 8, 8, 0, 0))
    X, w, X2, W2 = make_inputs(c)
    Wt = pack_weights(w, W2, c.npad).double()
    x = X[:, :c.Cin].double().reshape(c.imgs, c.H, c.W, c.Cin)
    cols = torch.zeros(c.imgs, c.H, c.W, 9 * c.Cin, dtype=torch.float64)
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        for yy in range(c.H):
            for xx in range(c.W):
                if 0 <= yy + dy < c.H and 0 <= xx + dx < c.W:
                    cols[:, yy, xx, tap * c.Cin:(tap + 1) * c.Cin] = x[:, yy + dy, xx + dx]
    direct = torch.cat([cols.reshape(c.M, -1), X2.double()], 1) @ Wt[:c.N].t()
    assert (Wt[c.N:] == 0).all()
    assert torch.allclose(direct, conv_ref(c, X, w, X2, W2), rtol=1e-12, atol=1e-12)


def test_bounds_reject_mutated_references():
    """the element bound passes the exact result rounded to fp16 and rejects each kernel bug it is meant to catch; the sums
    bound passes exact sums and rejects one tile's statistics filed under the next image"""
    c = _small_case()
    X, w, X2, W2 = make_inputs(c)
    ref, A = conv_ref(c, X, w, X2, W2), conv_ref(c, X, w, X2, W2, magnitude=True)
    ok = f16r(ref)
    assert value_ratio(ok, ref, A).max() <= 1.0

    def fails(y, what):
        assert value_ratio(f16r(y), ref, A).max() > 100.0, what

    w_drop = w.clone()
    w_drop[:, 64:128, 1, 1] = 0                          # one 64-wide K step of the centre tap
    fails(conv_ref(c, X, w_drop, X2, W2), "a dropped K step")
    fails(conv_ref(c, X, w.transpose(2, 3).contiguous(), X2, W2), "taps transposed")
    stacked = dataclasses.replace(c, shape=(c.M, c.Cin, c.N, 9, 0, c.H * c.imgs, c.W, 0, 1))     # one tall image: padding leaks
    fails(conv_ref(stacked, X, w, X2, W2), "images stacked")
    unwritten = ref.clone()
    unwritten[64:128] = 0
    fails(unwritten, "a 64-row block unwritten")

    y = f16r(ref)
    s, q, sa = stat_ref(y, c.imgs)
    assert sums_ratio(s, s, sa).max() <= 1.0
    moved_s, moved_q = s.clone(), q.clone()
    tile_s, tile_q = y[:64].sum(0), (y[:64] ** 2).sum(0)     # the first 64-row tile of image 0 ...
    moved_s[0] -= tile_s
    moved_q[0] -= tile_q
    moved_s[1] += tile_s                                     # ... filed under image 1
    moved_q[1] += tile_q
    assert sums_ratio(moved_s, s, sa).max() > 100.0
    assert sums_ratio(moved_q, q, q).max() > 100.0

    # the GroupNorm-backward restatement: with neither FiLM nor SiLU the terms are the upstream value times gamma
    gc = dataclasses.replace(c, gb="plain", shape=(512, 128, 64, 9, 0, 16, 16, 0, 1))
    gx, gst, gam, bet, emb, _ = gb_operands(gc)
    s1, s2, a1, a2 = gb_sums_ref(gc, y, gx, gst, gam, bet, emb)
    assert torch.allclose(s1, (y.reshape(2, -1, 64) * gam.double()).sum(1), rtol=1e-12)
    for film_act in ("film", "act", "film+act"):
        t1, _, _, _ = gb_sums_ref(dataclasses.replace(gc, gb=film_act), y, gx, gst, gam, bet, emb)
        assert sums_ratio(t1, s1, a1).max() > 100.0, film_act      # the options change the terms, far beyond the bound
