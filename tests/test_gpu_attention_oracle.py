"""Every attention kernel form, one launch at a time, against float64 attention on the CPU.

Each case in CASES is a shape (T tokens, head width d, heads, N images) run through ishap_attention_run (include/ishap.h), which
builds the AttnArgs the product builds and launches attn_fwd_kernel or attn_bwd_kernel (csrc/attention.hip).  ATTN8_CASES run
attn8_fused_kernel through ishap_attention8_run, as one launch (the rendezvous tenancy granted) and as two.  The reference is
tests/attention_ref.py: QKVAttentionLegacy in float64 on the same fp16 values, with float64 autograd for the gradients.

Bounds.  s_k = alpha sum_d q_d k_d with alpha = 1/sqrt(d), w = softmax(s), S_abs,k = alpha sum_d |q_d k_d|, and
E = d 2^-24 max_k S_abs,k + 2^-20: the error of one fp32-accumulated score (d products, each exact in fp32, plus the scale)
with __expf / __logf's own error folded into 2^-20.
  * forward, V1 = sum_k w_k |v_k|:  |a - a*| <= 2^-11 |a*| + (2^-10 + 2E) V1 + 2^-24.  2^-11 |a*| is the rounding of a to fp16;
    each P is rounded to fp16 before P V (2^-11 of every term) while the denominator sums the unrounded P, and the fp32 sum
    over T keys and 2E from the shift by the running maximum take the rest of the 2^-10 and 2E V1.
    |lse - lse*| <= 2E + 2^-20 (1 + |lse*|): the score error, log's error and the fp32 rounding of the result.
  * backward, D_abs = sum_d |dA| |a| and dP_abs,k = sum_d |dA| |v_k|:  G = sum_k alpha P_k (dP_abs,k + D_abs) |k_k| for dq,
    the same over queries with |q_q| for dk, G = sum_q P_qk |dA_q| for dv, and |dX - dX*| <= 2^-11 |dX*| + 3 2^-11 G + 2^-24.
    The three units of 2^-11 G: dS (or P for dv) rounded to fp16 before the second product, D_q computed from the fp16 a that
    the kernel reads, and the fp32 sums plus P recomputed from the fp32 lse.  The chained case (the backward on the kernel's own
    forward a and lse, the product's path) adds one unit for those inputs' own error: 4 2^-11 G.
  * attn8: qkv = xn Wqkv^T + b against 2^-11 |ref| + 2^-16 A (A = the same product on magnitudes, as in the igemm oracle);
    a and lse against the forward bound on the kernel's own qkv; each fp32 proj_out slice against 2^-16 A + 2^-40 on the
    kernel's own fp16 a (64 products accumulated in fp32: 64 2^-24 = 2^-18 A, with room).
These are the constants the derivation gives; nothing has been loosened.  test_bounds_reject_mutated_references shows that
each bound passes the exact result rounded as the kernel rounds it and rejects a list of plausible kernel bugs by 100x or more.

Every launch also checks:
  * canaries: outputs start as NaN bit patterns, with 256 elements behind and (where the alignment allows) 8 bytes in front;
    afterwards every element inside the output is finite and every canary is unchanged bit for bit;
  * bits: the XCD-aware and the plain grid (xcd_map 1 / 0) only move work between workgroups, and a second identical call
    repeats the first: all give the same bits.
Input families: normal (q, k, v, dA ~ N(0, 1)); uniform (q = 0: every P is 1, lse = log T); peaked (logits of +-40: the even
queries' winner in tile 0, the odd queries' in the last tile of the last team, so both the in-team rescale and the team merge
scale by e^-36 or less); cold (the keys of team 0's tiles score 100 below the rest: team 0's state merges with c0 ~ e^-100).
The backward also runs dA = 0 (dqkv exactly zero) and dA = a.
The CPU tests at the end check the table against the plan-only call, the refusal of out-of-contract descriptors, the
restatement against the statement, and the bounds against mutated references."""
import ctypes as C
import dataclasses
import math
import time
import zlib

import pytest
import torch

from tests import attention_ref as R

F16_REL = 2.0 ** -11
ACC_REL = 2.0 ** -16
CANARY16 = 0x7E5A             # fp16 NaN
CANARY32 = 0x7FC0BEEF         # fp32 NaN
TAIL = 256                    # canary elements behind every written buffer
FRONT = 8                     # canary bytes in front of the outputs that allow an 8-byte offset


@dataclasses.dataclass(frozen=True)
class Case:
    T: int
    d: int
    heads: int
    N: int
    fwd: str                    # expected forward kernel form
    bwd: str                    # expected backward kernel form
    chained: bool = False       # a full-size shape: also the backward on the kernel's own forward outputs
    why: str = ""

    @property
    def C(self): return self.heads * self.d


CASES = {
    "T64 d32 h1 N1": Case(64, 32, 1, 1, "attn_fwd_kernel<32,2>", "attn_bwd_kernel<32,2>/256",
                          why="tiny config; forward team 1 never live; backward with 256 threads"),
    "T64 d64 h16 N2": Case(64, 64, 16, 2, "attn_fwd_kernel<64,2>", "attn_bwd_kernel<64,2>/256", True,
                           why="8x8 level with ISHAP_ATTN8=0; item count % 8 == 0"),
    "T128 d32 h3 N1": Case(128, 32, 3, 1, "attn_fwd_kernel<32,2>", "attn_bwd_kernel<32,2>/512",
                           why="2 teams with one tile each; item count not % 8"),
    "T192 d64 h2 N3": Case(192, 64, 2, 3, "attn_fwd_kernel<64,2>", "attn_bwd_kernel<64,2>/512",
                           why="odd tile count; team 1 has one tile fewer"),
    "T256 d64 h12 N2": Case(256, 64, 12, 2, "attn_fwd_kernel<64,2>", "attn_bwd_kernel<64,2>/512", True,
                            why="full-size 16x16 level (768 channels)"),
    "T448 d64 h1 N1": Case(448, 64, 1, 1, "attn_fwd_kernel<64,2>", "attn_bwd_kernel<64,2>/512", why="largest 2-team forward"),
    "T512 d32 h2 N1": Case(512, 32, 2, 1, "attn_fwd_kernel<32,4>", "attn_bwd_kernel<32,2>/512", why="first 4-team forward, d = 32"),
    "T576 d64 h1 N2": Case(576, 64, 1, 2, "attn_fwd_kernel<64,4>", "attn_bwd_kernel<64,2>/512", why="9 tiles over 4 teams"),
    "T1024 d64 h8 N2": Case(1024, 64, 8, 2, "attn_fwd_kernel<64,4>", "attn_bwd_kernel<64,2>/512", True,
                            why="full-size 32x32 level"),
    "T1024 d64 h8 N8": Case(1024, 64, 8, 8, "attn_fwd_kernel<64,4>", "attn_bwd_kernel<64,2>/512", True,
                            why="the product's max batch"),
    "T2048 d64 h1 N1": Case(2048, 64, 1, 1, "attn_fwd_kernel<64,4>", "attn_bwd_kernel<64,2>/512", why="beyond product shapes"),
}
FAMILIES = ("normal", "uniform", "peaked", "cold")
FWD_FORMS = {f"attn_fwd_kernel<{d},{t}>" for d in (32, 64) for t in (2, 4)}
BWD_FORMS = {f"attn_bwd_kernel<{d},2>/{n}" for d in (32, 64) for n in (256, 512)}

# (C, N): why
ATTN8_CASES = {
    (64, 1): "trem = 4: parts 4-11 write no proj tile",
    (128, 8): "192 workgroups across images",
    (320, 1): "tper = 1, trem = 8",
    (768, 1): "12 heads, trem = 0",
    (1024, 1): "the product shape, up to TMAX = 6 tiles a part",
    (1152, 1): "the largest C the launcher accepts, tper = 6",
}


# ---------------------------------------------------------------------------------------------------------------- operands
def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))     # not hash(): str hashes change per process


def last_team_tile(T, teams):
    """the last tile of the last team that has one (the tile a peaked query's winner sits in)"""
    ntile = T // R.TILE
    owned = [t for t in range(ntile) if t % teams == teams - 1]
    return owned[-1] if owned else ntile - 1


def make_qkv(c: Case, family):
    """fp16 [N][T][3C] of an input family (CPU)"""
    g = _gen("qkv", c.T, c.d, c.heads, c.N, family)
    x = torch.randn(c.N, c.T, c.heads, 3, c.d, generator=g)
    alpha = 1.0 / math.sqrt(c.d)
    if family == "uniform":
        x[:, :, :, 0] = 0
    elif family == "peaked":
        x[:, :, :, :2] *= 0.25                                   # q and k small; the winners come from dims 0 and 1
        w0 = 5
        w1 = last_team_tile(c.T, R.fwd_teams(c.T)) * R.TILE + 37
        kk = 40.0 / (alpha * 16.0)
        x[:, :, :, 1, :2] = 0.25 * torch.randn(c.N, c.T, c.heads, 2, generator=g)
        x[:, w0, :, 1, 0] = kk
        x[:, w1, :, 1, 1] = kk
        x[:, 0::2, :, 0, 0], x[:, 0::2, :, 0, 1] = 16.0, -16.0   # even queries: +40 at w0, -40 at w1
        x[:, 1::2, :, 0, 0], x[:, 1::2, :, 0, 1] = -16.0, 16.0   # odd queries: the other way round
    elif family == "cold":
        teams = R.fwd_teams(c.T)
        cold = torch.zeros(c.T, dtype=torch.bool)
        if c.T == R.TILE:
            cold[32:] = True
        else:
            for t in range(0, c.T // R.TILE, teams):
                cold[t * R.TILE:(t + 1) * R.TILE] = True
        x[:, :, :, 0, 2] = 16.0
        x[:, :, :, 1, 2] = 0.0
        x[:, cold, :, 1, 2] = -100.0 / (alpha * 16.0)
    return x.reshape(c.N, c.T, 3 * c.C).half()


def make_dA(c: Case, family):
    return torch.randn(c.N, c.T, c.C, generator=_gen("dA", c.T, c.d, c.heads, c.N, family)).half()


# ---------------------------------------------------------------------------------------------------------------- bounds
def per_channel(t, c: Case):
    """[N*heads][T] -> [N][T][C] (each head's value over its d channels)"""
    return t.reshape(c.N, c.heads, c.T).permute(0, 2, 1).repeat_interleave(c.d, -1)


def fwd_ratios(c: Case, a, lse, a_ref, lse_ref, E, V1):
    """max |err| / bound of a and of lse"""
    Ec = per_channel(E, c)
    ba = F16_REL * a_ref.abs() + (2.0 ** -10 + 2 * Ec) * V1 + 2.0 ** -24
    bl = 2 * E + 2.0 ** -20 * (1 + lse_ref.abs())
    return ((a.double() - a_ref).abs() / ba).max().item(), ((lse.double() - lse_ref).abs() / bl).max().item()


def bwd_ratio(g, g_ref, G, units=3):
    return ((g.double() - g_ref).abs() / (F16_REL * g_ref.abs() + units * F16_REL * G + 2.0 ** -24)).max().item()


# ---------------------------------------------------------------------------------------------------------------- the calls
def _buf(t, ofs_bytes=0):
    from ishapediting_amd._lib import IgemmBufC
    if t is None:
        return IgemmBufC(None, 0)
    return IgemmBufC(t.data_ptr() + ofs_bytes, t.numel() * t.element_size() - ofs_bytes)


def attn_desc(c: Case, pas, xcd=-1, **bufs):
    from ishapediting_amd._lib import AttnDescC
    d = AttnDescC()
    d.pass_, d.N, d.T, d.C, d.heads, d.d, d.xcd_map = pas, c.N, c.T, c.C, c.heads, c.d, xcd
    for name, v in bufs.items():
        setattr(d, name, _buf(*v) if isinstance(v, tuple) else _buf(v))
    return d


def _canary(n, dtype):
    if dtype == torch.float16:
        return torch.full((n,), CANARY16, dtype=torch.int16).view(torch.float16)
    return torch.full((n,), CANARY32, dtype=torch.int32).view(torch.float32)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


class Out:
    """a device output of n elements behind `front` canary bytes, with TAIL canary elements after it"""

    def __init__(self, n, dtype, front, dev):
        self.n, self.f = n, front // torch.empty(0, dtype=dtype).element_size()
        self.t = _canary(self.f + n + TAIL, dtype).to(dev)

    def arg(self):
        return (self.t, self.f * self.t.element_size())

    def value(self, name):
        """the written elements (CPU); asserts the canaries and finiteness"""
        h = self.t.cpu()
        keep = _bits(_canary(1, h.dtype))[0]
        b = _bits(h)
        bad = (b[:self.f] != keep).sum().item() + (b[self.f + self.n:] != keep).sum().item()
        assert bad == 0, f"{name}: {bad} canary elements overwritten"
        v = h[self.f:self.f + self.n]
        nonfin = (~torch.isfinite(v.float())).sum().item()
        assert nonfin == 0, f"{name}: {nonfin} elements not finite (unwritten or overflowed)"
        return v


def run_fwd(c: Case, dqkv_in, xcd=-1):
    """one forward launch; returns (form, a [N][T][C] fp16 CPU, lse [N*heads][T] fp32 CPU)"""
    from ishapediting_amd import _lib
    L = _lib.lib()
    dev = dqkv_in.device
    out = Out(c.N * c.T * c.C, torch.float16, FRONT, dev)
    lse = Out(c.N * c.heads * c.T, torch.float32, FRONT, dev)
    d = attn_desc(c, 0, xcd, qkv=dqkv_in, out=out.arg(), lse=lse.arg())
    kern = C.create_string_buffer(64)
    _lib.check(L.ishap_attention_run(C.byref(d), 1, _lib.stream_ptr(dev), kern, len(kern)))
    torch.cuda.synchronize()
    return kern.value.decode(), out.value("a").view(c.N, c.T, c.C), lse.value("lse").view(c.N * c.heads, c.T)


def run_bwd(c: Case, dqkv_in, a, lse, dA, xcd=-1):
    """one backward launch on device inputs; returns (form, dqkv [N][T][3C] fp16 CPU)"""
    from ishapediting_amd import _lib
    L = _lib.lib()
    dev = dqkv_in.device
    dq = Out(c.N * c.T * 3 * c.C, torch.float16, FRONT, dev)
    d = attn_desc(c, 1, xcd, qkv=dqkv_in, out=a, lse=lse, dout=dA, dqkv=dq.arg())
    kern = C.create_string_buffer(64)
    _lib.check(L.ishap_attention_run(C.byref(d), 1, _lib.stream_ptr(dev), kern, len(kern)))
    torch.cuda.synchronize()
    return kern.value.decode(), dq.value("dqkv").view(c.N, c.T, 3 * c.C)


def same_bits(x, y):
    return torch.equal(_bits(x.contiguous()), _bits(y.contiguous()))


def check_case(c: Case):
    dev = torch.device("cuda", 0)
    worst = {}
    for fam in FAMILIES:
        qkv = make_qkv(c, fam)
        dA = make_dA(c, fam)
        a_ref, lse_ref, g_ref = R.statement(qkv, c.heads, c.d, dA)
        E, V1, G = R.magnitudes(qkv, c.heads, c.d, dA, a_ref)
        dqkv_in = qkv.to(dev)
        # forward: the product's xcd setting, then both grids explicitly, then a repeat
        form, a, lse = run_fwd(c, dqkv_in)
        assert form == c.fwd, f"forward ran {form}"
        for xcd in (0, 1, 1):
            _, a2, lse2 = run_fwd(c, dqkv_in, xcd)
            assert same_bits(a, a2) and same_bits(lse, lse2), f"{fam}: forward bits differ with xcd_map = {xcd}"
        ra, rl = fwd_ratios(c, a, lse, a_ref, lse_ref, E, V1)
        worst[f"{fam} a"], worst[f"{fam} lse"] = ra, rl
        assert ra <= 1.0 and rl <= 1.0, f"{fam}: forward over the bound: a {ra:.3g}, lse {rl:.3g}"
        # backward, isolated from the forward: the test's own fp16(a*) and fp32(lse*)
        a_in, lse_in, dA_in = a_ref.half().to(dev), lse_ref.float().to(dev), dA.to(dev)
        form, g = run_bwd(c, dqkv_in, a_in, lse_in, dA_in)
        assert form == c.bwd, f"backward ran {form}"
        for xcd in (0, 1, 1):
            _, g2 = run_bwd(c, dqkv_in, a_in, lse_in, dA_in, xcd)
            assert same_bits(g, g2), f"{fam}: backward bits differ with xcd_map = {xcd}"
        worst[f"{fam} dqkv"] = r = bwd_ratio(g, g_ref, G)
        assert r <= 1.0, f"{fam}: backward over the bound by {r:.3g}"
        if fam == "normal":
            # dA = 0: exactly zero; dA = a
            _, g0 = run_bwd(c, dqkv_in, a_in, lse_in, torch.zeros_like(dA_in))
            assert (g0 == 0).all(), "dA = 0 gave a non-zero gradient"
            dAa = a_ref.half()
            _, _, ga_ref = R.statement(qkv, c.heads, c.d, dAa)
            _, _, Ga = R.magnitudes(qkv, c.heads, c.d, dAa, a_ref)
            _, ga = run_bwd(c, dqkv_in, a_in, lse_in, dAa.to(dev))
            worst["dA=a dqkv"] = r = bwd_ratio(ga, ga_ref, Ga)
            assert r <= 1.0, f"dA = a: backward over the bound by {r:.3g}"
            if c.chained:
                # the product's path: the backward on the kernel's own forward outputs
                _, gc = run_bwd(c, dqkv_in, a.to(dev), lse.to(dev), dA_in)
                worst["chained dqkv"] = r = bwd_ratio(gc, g_ref, G, units=4)
                assert r <= 1.0, f"chained backward over the bound by {r:.3g}"
        del a_ref, g_ref, G, V1
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_attention_matches_fp64(case):
    c = CASES[case]
    t0 = time.time()
    worst = check_case(c)
    print(f"\n  {c.fwd} + {c.bwd} ({case}): worst / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) +
          f" ({time.time() - t0:.1f} s)")


# ---------------------------------------------------------------------------------------------------------------- attn8
def attn8_desc(N, Cc, heads=None, **bufs):
    from ishapediting_amd._lib import Attn8DescC
    d = Attn8DescC()
    d.N, d.C, d.heads = N, Cc, Cc // 64 if heads is None else heads
    for name, v in bufs.items():
        setattr(d, name, _buf(*v) if isinstance(v, tuple) else _buf(v))
    return d


def attn8_operands(Cc, N):
    g = _gen("attn8", Cc, N)
    xn = torch.randn(N, 64, Cc, generator=g).half()
    wqkv = (torch.randn(3 * Cc, Cc, generator=g) / math.sqrt(Cc)).half()
    bqkv = 0.5 * torch.randn(3 * Cc, generator=g)
    wproj = (torch.randn(Cc, Cc, generator=g) / math.sqrt(Cc)).half()
    return xn, wqkv, bqkv, wproj


def run_attn8(Cc, N, ops, one_launch):
    from ishapediting_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda", 0)
    heads = Cc // 64
    xn, wqkv, bqkv, wproj = (t.to(dev) for t in ops)
    outs = {"qkv": Out(N * 64 * 3 * Cc, torch.float16, FRONT, dev), "aout": Out(N * 64 * Cc, torch.float16, FRONT, dev),
            "lse": Out(N * heads * 64, torch.float32, FRONT, dev),
            "slices": Out(heads * N * 64 * Cc, torch.float32, 0, dev)}     # f32x4 stores: 16-byte aligned
    flags = torch.full((N * heads * 16,), 7, dtype=torch.int32, device=dev)  # the call zeroes them
    d = attn8_desc(N, Cc, xn=xn, wqkv=wqkv, bqkv=bqkv, wproj=wproj, flags=flags, **{k: o.arg() for k, o in outs.items()})
    granted = C.c_int(-1)
    _lib.check(L.ishap_attention8_run(C.byref(d), int(one_launch), 1, _lib.stream_ptr(dev), C.byref(granted)))
    torch.cuda.synchronize()
    if one_launch:
        assert granted.value == 1, "the rendezvous tenancy was not granted: the one-launch form did not run"
    else:
        assert granted.value == 0
    v = {k: o.value(k) for k, o in outs.items()}
    return (v["qkv"].view(N, 64, 3 * Cc), v["aout"].view(N, 64, Cc), v["lse"].view(N * heads, 64),
            v["slices"].view(heads, N * 64, Cc))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(ATTN8_CASES), ids=[f"C{c}-N{n}" for c, n in ATTN8_CASES])
def test_attention8_matches_fp64_stage_by_stage(shape):
    Cc, N = shape
    heads = Cc // 64
    t0 = time.time()
    ops = attn8_operands(Cc, N)
    xn, wqkv, bqkv, wproj = ops
    one = run_attn8(Cc, N, ops, True)
    two = run_attn8(Cc, N, ops, False)
    for name, x, y in zip(("qkv", "a", "lse", "slices"), one, two):
        assert same_bits(x, y), f"{name}: one launch and two launches differ"
    qkv, a, lse, slices = one
    worst = {}
    # stage 1: qkv = xn Wqkv^T + b
    x = xn.double().reshape(N * 64, Cc)
    ref = x @ wqkv.double().t() + bqkv.double()
    A = x.abs() @ wqkv.double().abs().t() + bqkv.double().abs()
    worst["qkv"] = ((qkv.reshape(N * 64, 3 * Cc).double() - ref).abs() / (F16_REL * ref.abs() + ACC_REL * A)).max().item()
    assert worst["qkv"] <= 1.0, f"qkv over the bound by {worst['qkv']:.3g}"
    # stage 2: the attention of the kernel's own qkv
    c = Case(64, 64, heads, N, "", "")
    a_ref, lse_ref = R.statement(qkv, heads, 64)
    E, V1 = R.magnitudes(qkv, heads, 64)
    worst["a"], worst["lse"] = fwd_ratios(c, a, lse, a_ref, lse_ref, E, V1)
    assert worst["a"] <= 1.0 and worst["lse"] <= 1.0, f"attention over the bound: {worst}"
    # ... what attn_fwd_kernel<64,2> computes from the same qkv: the same arithmetic up to a's final rounding.  attn8's
    # fp16(o * (1/sum)) compiles to one fused multiply-and-convert (v_fma_mixlo_f16, a single rounding), attn_fwd_kernel's to an
    # fp32 product and a conversion (two roundings), so a rare element differs by one fp16 ulp; lse is bitwise the same
    form, a2, lse2 = run_fwd(c, qkv.to(torch.device("cuda", 0)), 1)
    assert form == "attn_fwd_kernel<64,2>"
    assert same_bits(lse, lse2), "attn8's lse differs from attn_fwd_kernel<64,2> on the same qkv"
    ulps = (_bits(a).int() - _bits(a2).int()).abs()
    worst["a vs attn_fwd (ulp)"] = ulps.max().item()
    assert ulps.max() <= 1 and (ulps > 0).float().mean() <= 1e-3, \
        f"attn8's a differs from attn_fwd_kernel<64,2> on the same qkv: {(ulps > 0).sum().item()} elements, up to {ulps.max()} ulp"
    # stage 3: slice h = a_h Wproj[:, h*64 : (h+1)*64]^T on the kernel's own fp16 a
    ad = a.double().reshape(N * 64, Cc)
    wd = wproj.double()
    r = 0.0
    for h in range(heads):
        ah, wh = ad[:, h * 64:(h + 1) * 64], wd[:, h * 64:(h + 1) * 64]
        ref = ah @ wh.t()
        A = ah.abs() @ wh.abs().t()
        r = max(r, ((slices[h].double() - ref).abs() / (ACC_REL * A + 2.0 ** -40)).max().item())
    worst["slices"] = r
    assert r <= 1.0, f"proj_out slices over the bound by {r:.3g}"
    print(f"\n  attn8_fused_kernel C {Cc} N {N}, one launch and two: worst / bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + f" ({time.time() - t0:.1f} s)")


# ---------------------------------------------------------------------------------------------------------------- CPU checks
class _Fake:
    """a stand-in device buffer for descriptor checks without a GPU: an address and a size, nothing behind it"""
    _next = 1 << 40

    def __init__(self, nbytes):
        self.nbytes, self.addr = nbytes, _Fake._next
        _Fake._next += (nbytes + (1 << 20)) // (1 << 20) * (1 << 20) + (1 << 20)

    def data_ptr(self): return self.addr
    def element_size(self): return 1
    def numel(self): return self.nbytes


def need_bytes(c: Case):
    rows = c.N * c.T
    return {"qkv": rows * 3 * c.C * 2, "out": rows * c.C * 2, "lse": c.N * c.heads * c.T * 4, "dout": rows * c.C * 2,
            "dqkv": rows * 3 * c.C * 2}


def fake_desc(c: Case, pas):
    n = need_bytes(c)
    names = ("qkv", "out", "lse") if pas == 0 else ("qkv", "out", "lse", "dout", "dqkv")
    return attn_desc(c, pas, -1, **{k: _Fake(n[k]) for k in names})


def _dry(d):
    from ishapediting_amd import _lib
    L = _lib.lib()
    kern = C.create_string_buffer(64)
    rc = L.ishap_attention_run(C.byref(d), 0, None, kern, len(kern))
    msg = L.ishap_last_error()
    return rc, kern.value.decode(), (msg.decode() if msg else "")


def test_table_covers_every_form():
    assert {c.fwd for c in CASES.values()} == FWD_FORMS
    assert {c.bwd for c in CASES.values()} == BWD_FORMS
    assert any(c.T > 1024 for c in CASES.values()) and len({(c, n) for c, n in ATTN8_CASES}) == 6


@pytest.mark.parametrize("case", list(CASES))
def test_table_matches_the_plan(case):
    """each expected form is what the plan-only call reports for the case's descriptor (launch = 0: no HIP call)"""
    c = CASES[case]
    for pas, want in ((0, c.fwd), (1, c.bwd)):
        rc, name, msg = _dry(fake_desc(c, pas))
        assert rc == 0, msg
        assert name == want


def _mutants():
    """(what, pass, case, change to the descriptor, words of the expected message); ("short", buf) mutants run twice: at
    exactly the bytes the launch touches (accepted) and one element less (refused)"""
    c = CASES["T192 d64 h2 N3"]
    setf = lambda k, v: (lambda d: setattr(d, k, v))
    return [
        ("T % 64 != 0", 0, c, setf("T", 200), "tokens"),
        ("T = 0", 1, c, setf("T", 0), "tokens"),
        ("N = 0", 0, c, setf("N", 0), "images"),
        ("d = 48", 0, c, lambda d: (setattr(d, "d", 48), setattr(d, "C", 96)), "head width"),
        ("C != heads * d", 1, c, setf("C", 192), "channels"),
        ("xcd_map = 2", 0, c, setf("xcd_map", 2), "xcd_map"),
        ("pass = 2", 0, c, setf("pass_", 2), "pass"),
        ("forward qkv", 0, c, ("short", "qkv", 2), "buffer qkv:"),
        ("forward out", 0, c, ("short", "out", 2), "buffer out:"),
        ("forward lse", 0, c, ("short", "lse", 4), "buffer lse:"),
        ("backward qkv", 1, c, ("short", "qkv", 2), "buffer qkv:"),
        ("backward out", 1, c, ("short", "out", 2), "buffer out:"),
        ("backward lse", 1, c, ("short", "lse", 4), "buffer lse:"),
        ("backward dout", 1, c, ("short", "dout", 2), "buffer dout:"),
        ("backward dqkv", 1, c, ("short", "dqkv", 2), "buffer dqkv:"),
        ("null dout", 1, c, lambda d: setattr(d.dout, "ptr", None), "buffer dout:"),
        ("null qkv", 0, c, lambda d: setattr(d.qkv, "ptr", None), "buffer qkv:"),
        ("qkv 8 bytes off", 0, c, lambda d: setattr(d.qkv, "ptr", d.qkv.ptr + 8), "buffer qkv:"),
        ("backward out 8 bytes off", 1, c, lambda d: setattr(d.out, "ptr", d.out.ptr + 8), "buffer out:"),
    ]


@pytest.mark.parametrize("i", range(len(_mutants())), ids=[m[0] for m in _mutants()])
def test_run_rejects_out_of_contract_input(i):
    what, pas, c, mutate, words = _mutants()[i]
    d = fake_desc(c, pas)
    rc, _, msg = _dry(d)
    assert rc == 0, msg                  # the unchanged descriptor passes: the refusal below is the mutation's
    if isinstance(mutate, tuple):
        _, name, es = mutate
        buf = getattr(d, name)
        assert buf.bytes == need_bytes(c)[name]
        buf.bytes -= es
    else:
        mutate(d)
    rc, _, msg = _dry(d)
    assert rc != 0, what
    assert "requirement failed" in msg and words in msg, (what, msg)


def fake_attn8(Cc, N, heads=None):
    h = Cc // 64 if heads is None else heads
    rows = N * 64
    n = {"xn": rows * Cc * 2, "wqkv": 3 * Cc * Cc * 2, "bqkv": 3 * Cc * 4, "wproj": Cc * Cc * 2, "qkv": rows * 3 * Cc * 2,
         "aout": rows * Cc * 2, "lse": N * h * 64 * 4, "slices": h * rows * Cc * 4, "flags": N * h * 16 * 4}
    return attn8_desc(N, Cc, heads, **{k: _Fake(v) for k, v in n.items()}), n


def _dry8(d):
    from ishapediting_amd import _lib
    L = _lib.lib()
    granted = C.c_int(-1)
    rc = L.ishap_attention8_run(C.byref(d), 1, 0, None, C.byref(granted))
    msg = L.ishap_last_error()
    return rc, (msg.decode() if msg else ""), granted.value


def test_attention8_rejects_out_of_contract_input():
    """launch = 0: the checks only (ishap_cu_count falls back to 256 without a device; the co-residency case is above that)"""
    for Cc, N in ATTN8_CASES:
        rc, msg, granted = _dry8(fake_attn8(Cc, N)[0])
        assert rc == 0 and granted == 0, msg
    for what, d, words in [("d = 32 (C = 64, 2 heads)", fake_attn8(64, 1, heads=2)[0], "head width 64"),
                           ("C = 1216", fake_attn8(1216, 1)[0], "1152"),
                           ("N * heads * 12 = 384", fake_attn8(1024, 2)[0], "co-resident"),
                           ("N = 0", fake_attn8(64, 0)[0], "images")]:
        rc, msg, _ = _dry8(d)
        assert rc != 0 and "requirement failed" in msg and words in msg, (what, msg)
    for name in ("xn", "wqkv", "bqkv", "wproj", "qkv", "aout", "lse", "slices", "flags"):
        d, n = fake_attn8(320, 1)
        buf = getattr(d, name)
        assert buf.bytes == n[name]
        buf.bytes -= 2 if name in ("xn", "wqkv", "wproj", "qkv", "aout") else 4
        rc, msg, _ = _dry8(d)
        assert rc != 0 and f"buffer {name}:" in msg, (name, msg)
        d, _ = fake_attn8(320, 1)
        getattr(d, name).ptr = None
        rc, msg, _ = _dry8(d)
        assert rc != 0 and f"buffer {name}:" in msg, (name, "null", msg)


def test_peaked_and_cold_inputs_do_what_they_say():
    """the families' logits: peaked winners at +-40 in the tiles named, cold keys 100 below, uniform P = 1"""
    for c in (CASES["T576 d64 h1 N2"], CASES["T128 d32 h3 N1"]):
        q, k, _ = R.split_heads(make_qkv(c, "peaked"), c.heads, c.d)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(c.d)
        w1 = last_team_tile(c.T, R.fwd_teams(c.T)) * R.TILE + 37
        assert (s[..., 0::2, :].argmax(-1) == 5).all() and (s[..., 1::2, :].argmax(-1) == w1).all()
        assert s.max() > 38 and s.min() < -38
        top2 = s.topk(2, -1).values
        assert (top2[..., 0] - top2[..., 1] > 30).all()
        q, k, _ = R.split_heads(make_qkv(c, "cold"), c.heads, c.d)
        s = (q @ k.transpose(-1, -2)) / math.sqrt(c.d)
        cold = s[..., 0:R.TILE].mean(-1) - s[..., R.TILE:2 * R.TILE].mean(-1)
        assert (cold < -90).all() and (cold > -110).all()
    c = CASES["T192 d64 h2 N3"]
    _, lse = R.statement(make_qkv(c, "uniform"), c.heads, c.d)
    assert torch.allclose(lse, torch.full_like(lse, math.log(c.T)), rtol=0, atol=1e-12)


@pytest.mark.parametrize("shape", [(576, 32, 2, 2), (192, 64, 1, 3), (64, 64, 2, 1)])
def test_restatement_equals_the_statement(shape):
    """the tile-and-team walk of the kernels is the same function as the statement (forward and backward)"""
    T, d, heads, N = shape
    c = Case(T, d, heads, N, "", "")
    for fam in ("normal", "peaked"):
        qkv, dA = make_qkv(c, fam), make_dA(c, fam)
        a, lse, g = R.statement(qkv, heads, d, dA)
        a2, lse2 = R.restatement(qkv, heads, d)
        assert (a2 - a).abs().max() <= 1e-12 and (lse2 - lse).abs().max() <= 1e-12
        g2 = R.restatement(qkv, heads, d, dA, lse_in=lse, a_in=a)
        assert (g2 - g).abs().max() <= 1e-12


def test_bounds_reject_mutated_references():
    """each bound passes the exact result rounded as the kernel rounds it (a, dqkv to fp16, lse to fp32) and rejects each
    mutation of the restatement by at least 100x"""
    margins = {}

    def fwd_case(T, d, heads, N, fam):
        c = Case(T, d, heads, N, "", "")
        qkv = make_qkv(c, fam)
        a, lse = R.statement(qkv, heads, d)
        E, V1 = R.magnitudes(qkv, heads, d)
        ra, rl = fwd_ratios(c, a.half(), lse.float(), a, lse, E, V1)
        assert ra <= 1.0 and rl <= 1.0, (T, fam, ra, rl)
        return c, qkv, a, lse, E, V1

    def fwd_rejects(what, case, **mut):
        c, qkv, a, lse, E, V1 = case
        a2, lse2 = R.restatement(qkv, c.heads, c.d, **mut)
        margins[what] = max(fwd_ratios(c, a2.half(), lse2.float(), a, lse, E, V1))

    big = fwd_case(1024, 64, 1, 1, "normal")
    peaked = fwd_case(576, 64, 1, 1, "peaked")
    small = fwd_case(192, 64, 2, 2, "normal")
    fwd_rejects("one 64-key tile dropped (T = 1024)", big, drop_tile=9)
    fwd_rejects("merge without the c1 rescale (peaked)", peaked, no_c1=True)
    fwd_rejects("no corr rescale within a team (peaked)", peaked, no_corr=True)
    fwd_rejects("alpha = 1/d", small, alpha=1.0 / 64)
    fwd_rejects("q and k of a head swapped", small, layout="kqv")
    fwd_rejects("images offset by one head", small, image_offset=3 * 64)

    c = Case(192, 64, 2, 2, "", "")
    x = make_qkv(c, "normal").float().reshape(c.N, c.T, c.heads, 3, c.d)
    for offset, muts in [(False, [("P from the neighbouring query's lse", dict(lse_shift=1)), ("dK and dV swapped",
                                                                                                dict(swap_dkdv=True)),
                                  ("backward team 1's sum dropped", dict(drop_team1=True))]),
                         # -D_q is what removes a common offset of v from dS: with zero-mean v and dA it is a small
                         # share of the gradient (a margin of ~27), with v and dA of positive mean the whole of it
                         (True, [("dS without -D_q (v and dA of positive mean)", dict(no_D=True))])]:
        xo = x.clone()
        if offset:
            xo[..., 2, :] += 3.0
        qkv = xo.reshape(c.N, c.T, 3 * c.C).half()
        dA = (make_dA(c, "normal").float() + (1.0 if offset else 0.0)).half()
        a, lse, g = R.statement(qkv, c.heads, c.d, dA)
        _, _, G = R.magnitudes(qkv, c.heads, c.d, dA, a)
        assert bwd_ratio(g.half(), g, G) <= 1.0
        for what, mut in muts:
            g2 = R.restatement(qkv, c.heads, c.d, dA, lse_in=lse, a_in=a, **mut)
            margins[what] = bwd_ratio(g2.half(), g, G)
    print("\n  mutation margins (worst / bound): " + ", ".join(f"{k} {v:.0f}" for k, v in margins.items()))
    for what, m in margins.items():
        assert m > 100.0, (what, m)
