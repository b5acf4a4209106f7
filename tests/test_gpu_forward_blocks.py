"""Every block's output of the UNet forward pass (csrc/unet.hip) against a float64 forward of that block alone.

The kernels the forward launches each have a launch-by-launch float64 oracle; this module checks what csrc/unet.hip does BETWEEN
launches: which FiLM row a ResBlock reads for which image, whether the per-image GroupNorm sums of a convolution's epilogue (or of
the lazy concatenation) land on the right image, in what order `hs` is popped and where the seam of the concatenation lies, the
pooling / upsampling folded into neighbouring launches, the pending split-K slices the next GroupNorm adds up, the statistics
arena zeroed by the layout conversion, the prepared timestep rows and the deferred forward tail.  After one kept forward every
block's output (`block_output`) and the model output are read back, and each block is compared with `unet_ref.UNetRef.block`
evaluated at the DEVICE's own block input (fp16 -> float64; unet_ref.forward_positions).  Nothing is chained, so an error belongs
to exactly one block, and by the printed kind to one layer type.

Bound, per block, for the whole batch AND for every image on its own: relative L2 <= 4 * e_r, where e_r is the distance of
unet_ref's ROUNDED restatement of the block (fp16 wherever the device keeps fp16) from the unrounded one, computed from the
reference alone.  The factor is the backward test's and covers the same leftovers: fp32 accumulation order, __expf / v_rcp_f32,
fixed-point statistics, neighbouring-fp16 flips of an activation recomputed inside a multi-layer block.
tests/test_unet_ref_host.py shows that e_r is fp16 rounding at every block (2.1e-4 .. 6.1e-4) and that every mistake of the
composition it models moves a block by more than 10 (measured: 21 .. 2071) times this bound.

The head is fp32-grade and has two conditions of its own, both against the float64 head at the device's own last block output:
  1. every element within conv(b_a, |w|) + ACC_REL (conv(|a|, |w|) + |bias|): the GroupNorm oracle's bound of the split form
     (groupnorm_ref.forward_bound(split=True), with the fixed-point quantum of the epilogue sums where the map is full-size)
     through the convolution, + the implicit-GEMM oracle's accumulation term;
  2. relative L2 (whole batch and per image) below one tenth of the error of the reference's own head with the lo products dropped
     (3.0e-4 .. 3.2e-4): fp32-grade, not fp16-grade, by an order of magnitude.

Configurations (unet_ref.FORWARD_CONFIGS; the host test lists the launch forms they reach): top (128^2 / 64^2, N = 1), deep
(32^2 .. 8^2, N = 2, fused 8x8 attention), tiny2 (one channel per group, 96-channel concatenation), top2 (top at N = 2: full-map
routes with two images), deep8 (deep at N = 8, eight timesteps: batched tile forms, the unfused attention on the 8x8 map), wide
(96 / 288 channels: split-K reduced in place, the separately launched 1x1 skip, heads of 32 channels).  Modes: the plain sequence
(all six), and on deep and top the DEFERRED tail -- `overlap_tail=True` at a middle output block, `run_tail()` on the side stream
with its own scratch, non-tenant launch forms and chunked convolutions.  That the tail really was deferred is observed on the
output buffer: filled with NaN after the forward has completed, it is finite only because the head ran after `run_tail()`.  The
context under test is the only one at work and holds the device's tenancy while it plans the tail (the library defers only then;
`ishap_rendezvous_would_grant` is asserted beforehand); the replay itself runs without the tenancy.  When another context holds
it the library degrades this mode to the plain sequence, and the test would fail on the NaNs rather than pass unseen.

MEASURED (MI355X, all ten cases; the module takes 7.3 s, top2's float64 reference 2.5 s of it, top's 1.2 s).  Worst error / e_r per
block kind over the six configurations and both modes (whole batch or one image, whichever is larger), and in brackets the worst
distance of the device from the ROUNDED restatement in units of e_r:
    conv (stem)                   1.00 (0.05)        res                           1.00 (0.38)
    res:down                      1.01 (0.29)        res|attn                      1.00 (0.42)
    res+skip1x1                   1.07 (0.68)        res+skip1x1|attn              1.07 (0.85)
    res|attn|res (middle block)   1.01 (0.78)        cat res+skip1x1               1.18 (1.08)
    cat res+skip1x1|attn          1.01 (0.63)        cat res+skip1x1|res:up        1.08 (0.98)
    cat res+skip1x1|attn|res:up   1.07 (1.08)
    head: relative L2 3.8e-7 .. 6.0e-7 (the split restatement's own 3.3e-7 .. 5.5e-7; the bound 3.0e-5 .. 3.2e-5), worst element
    0.0133 of its bound (condition 1 has a margin of 75, condition 2 of 50)
The error is the fp16 rounding itself: no block comes near the factor 4, in either mode the head is fp32-grade, the deferred tail
and every bit equality hold, and the comparison found NO defect in the forward's composition.  Every ratio above 1.02 (1.06 ..
1.18) belongs to tiny2 and wide, at exactly the ResBlocks whose 1x1 skip is launched on its own (channel counts that are no
multiple of 64 cannot fold it into conv2's launch): that launch stores its result in fp16 before conv2 adds it as the residual, a
rounding the restatement does not have -- with it, e_r of tiny2's output_blocks.3 is 3.79e-4 on the CPU against the device's
3.82e-4.  It is left out because the restatement is the backward test's too.  The brackets read as in the backward test: a block
of one layer is explained by the restatement to 0.05 - 0.4 e_r, a block of two or three layers is as far from it as from the
unrounded block, because the activation between its layers is recomputed and a few per cent of its elements flip to the
neighbouring fp16 value."""
import os
import re
import time

import pytest
import torch

from tests import groupnorm_ref as G
from tests import unet_ref as U

pytestmark = pytest.mark.gpu
FACTOR = 4.0
T0 = time.time()


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _stat_scales():
    """the fixed-point scales of the epilogue's channel sums (csrc/common.h), as tests/test_gpu_groupnorm_oracle.py reads them"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ishapediting_amd", "csrc", "common.h")).read()
    get = lambda k: float(re.search(rf"#define {k} ([0-9.]+)f", src).group(1))
    return get("STAT_SCALE_SUM"), get("STAT_SCALE_SQ")


_MODELS, _CACHE = {}, {}


def _model(name):
    """one context, one reference and one cache of float64 block results per configuration, shared by its tests"""
    from ishapediting_amd.unet import UNetModel
    if name not in _MODELS:
        cfg, sd, x, ts = U.make_forward_inputs(name)
        m = UNetModel(cfg, dev(), max_batch=x.shape[0])
        m.load_state_dict(sd)
        ref = U.UNetRef(cfg, sd)
        _MODELS[name] = (m, ref, sd, x, ts, ref.emb(ts))
        _CACHE[name] = {}
    return _MODELS[name]


def _blocks(m, spec):
    """{(group, index): block output} of the last kept forward, fp16 on the device (joins a pending tail by itself)"""
    acts = {(0, i): m.block_output(0, i) for i in range(len(spec.input_blocks))}
    acts[(1, 0)] = m.block_output(1)
    acts.update({(2, i): m.block_output(2, i) for i in range(len(spec.output_blocks))})
    return acts


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


WORST, NEAR = {}, {}


def _check_positions(name, mode, ref, emb, x, acts, out):
    """every position of one pass under the module's bounds; prints error / e_r and the distance from the rounded restatement"""
    f64 = lambda t: t.double().cpu()
    acts = {k: f64(v) for k, v in acts.items()}
    out = f64(out)
    bad = []
    for pos in ref.forward_positions(U.f16r(x), acts, out):
        st, e_r, err, near = U.forward_position_errors(ref, pos, emb, _CACHE[name])
        if pos.blk is None:
            bad += _check_head(name, mode, ref, pos, st, e_r, err)
            continue
        rows = [("batch", err[0], e_r[0], near[0])] + [(f"image {n}", e, r, d) for n, (e, r, d) in enumerate(zip(err[1], e_r[1], near[1]))]
        worst = max(rows, key=lambda r: r[1] / r[2])
        print(f"{name}-{mode} {pos.name:18s} {pos.kind:30s} error {err[0]:.3e}  e_r {e_r[0]:.3e}  error / e_r {err[0] / e_r[0]:.2f}  "
              f"worst {worst[0]}: {worst[1] / worst[2]:.2f}  (from the rounded restatement: {max(r[3] / r[2] for r in rows):.2f} e_r)")
        WORST[pos.kind] = max(WORST.get(pos.kind, 0.0), worst[1] / worst[2])
        NEAR[pos.kind] = max(NEAR.get(pos.kind, 0.0), max(r[3] / r[2] for r in rows))
        for what, e, r, _ in rows:
            if not e <= FACTOR * r:
                bad.append((pos.name, pos.kind, what, e, r, e / r))
    print(f"{name}-{mode}: worst error / e_r per block kind so far (and worst distance from the rounded restatement): " +
          ", ".join(f"{k}: {v:.2f} ({NEAR[k]:.2f})" for k, v in sorted(WORST.items())))
    return bad


HEAD = {}


def _check_head(name, mode, ref, pos, st, e_r, err):
    S = ref.cfg.image_size
    h = pos.x_in
    e_stats = None
    if S * S > 1024:            # full-size map: the statistics come from the fixed-point channel sums of the last convolution's epilogue
        sc_sum, sc_sq = _stat_scales()
        mean, var, _ = G.group_stats(h.permute(0, 2, 3, 1))
        e_stats = G.stats_error(mean, var, (0.5 / (sc_sum * S * S), 0.5 / (sc_sq * S * S)))
    bound = ref.head_bound(h, e_stats)
    lo = ref.head_restatement(h, lo=False)
    l2_bound = 0.1 * U.rel_l2(lo, st)
    l2_img = [0.1 * v for v in U.rel_l2_images(lo, st)]
    elem = float(((pos.got - st).abs() / bound).max())
    print(f"{name}-{mode} head: relative L2 {err[0]:.3e} (per image at most {max(err[1]):.3e}); bound {l2_bound:.3e} = a tenth of the "
          f"lo-dropped head's {10 * l2_bound:.3e}; the split restatement's own {e_r[0]:.3e}; worst element {elem:.4f} of its bound")
    HEAD["l2"] = max(HEAD.get("l2", 0.0), err[0], *err[1])
    HEAD["elem"] = max(HEAD.get("elem", 0.0), elem)
    print(f"head so far: worst relative L2 {HEAD['l2']:.3e}, worst element {HEAD['elem']:.4f} of its bound")
    bad = []
    if not elem <= 1.0:
        bad.append(("head", "elementwise", elem))
    if not err[0] <= l2_bound:
        bad.append(("head", "relative L2", err[0], l2_bound))
    bad += [("head", f"relative L2 of image {n}", e, b) for n, (e, b) in enumerate(zip(err[1], l2_img)) if not e <= b]
    return bad


@pytest.mark.parametrize("name", list(U.FORWARD_CONFIGS))
def test_every_block_output_vs_float64_block(name):
    t0 = time.time()
    m, ref, sd, x, ts, emb = _model(name)
    out = m(x.float().to(dev()), ts, feat_layer=-1, keep_for_backward=True)
    acts = _blocks(m, ref.spec)
    torch.cuda.synchronize()
    bad = _check_positions(name, "plain", ref, emb, x, acts, out)
    print(f"{name}-plain: {time.time() - t0:.1f} s ({time.time() - T0:.1f} s since the module was imported)")
    assert not bad, bad


@pytest.mark.parametrize("name", ["deep", "top"])
def test_every_block_output_with_the_deferred_tail(name):
    """`overlap_tail=True` at a middle output block: the blocks after the tap and the head are planned by the forward and launched
    by `run_tail()` on the context's side stream; every block (those after the tap too) and the output under the plain pass's
    bounds, and bitwise the plain pass's.  On deep also a tail that only the NEXT forward's join enqueues: its output buffer must
    come out as the plain pass's, bit for bit, although that forward records a tail of its own at other timesteps."""
    from ishapediting_amd import _lib
    t0 = time.time()
    m, ref, sd, x, ts, emb = _model(name)
    xd = x.float().to(dev())
    k = len(ref.spec.output_blocks) // 2 - 1
    out0 = m(xd, ts, feat_layer=-1, keep_for_backward=True)
    acts0 = _blocks(m, ref.spec)
    torch.cuda.synchronize()
    assert _lib.lib().ishap_rendezvous_would_grant(m._h, _lib.stream_ptr(dev())) == 1, "the device's tenancy is held by someone else"
    out, tap = m(xd, ts, feat_layer=k, keep_for_backward=True, overlap_tail=True)
    torch.cuda.synchronize()
    out.fill_(float("nan"))             # the forward has completed: had it run the head, nothing would write `out` again
    torch.cuda.synchronize()
    m.run_tail()
    m.join_tail()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()), "the tail was not deferred: the model output was not written after run_tail()"
    acts = _blocks(m, ref.spec)
    torch.cuda.synchronize()
    assert torch.equal(tap, acts[(2, k)])
    bad = _check_positions(name, "tail", ref, emb, x, acts, out)
    print(f"{name}-tail: {time.time() - t0:.1f} s ({time.time() - T0:.1f} s since the module was imported)")
    assert not bad, bad
    assert torch.equal(out, out0) and _same(acts, acts0)
    # a second overlapped forward, its tail left to the read-out to enqueue (block_output joins by itself)
    out2, _ = m(xd, ts, feat_layer=k, keep_for_backward=True, overlap_tail=True)
    acts2 = _blocks(m, ref.spec)
    m.join_tail()
    torch.cuda.synchronize()
    assert torch.equal(out2, out0) and _same(acts2, acts0)
    if name != "deep":
        return
    # a tail nobody enqueued, with another forward started on the context: that forward's own join enqueues the first call's tail
    # before anything of the second is recorded -- a stale or early-cleared record of the tail's launches would show in `out3`
    out3, _ = m(xd, ts, feat_layer=k, keep_for_backward=True, overlap_tail=True)
    torch.cuda.synchronize()
    out3.fill_(float("nan"))            # as above: only a tail enqueued from here on can make it finite again
    out4, _ = m(xd, [t + 100.0 for t in ts], feat_layer=k, keep_for_backward=True, overlap_tail=True)
    m.join_tail()
    torch.cuda.synchronize()
    assert torch.equal(out3, out0), "the first call's output, its tail enqueued by the next forward's join"
    assert bool(torch.isfinite(out4).all()) and not torch.equal(out4, out0), "the second call ran at its own timesteps"


@pytest.mark.parametrize("name", ["deep", "tiny2"])
def test_forward_bit_equalities(name):
    """What must not change a bit of the model output or of any block: running the forward again (the statistics arena is zeroed
    again by the layout conversion's extra blocks: a short zeroing shows here), a backward in between, keep_for_backward=False
    (no launch decision reads the flag), prepared timestep rows (include/ishap.h promises bit identity) and dropping them again,
    and a context created for a larger batch than it serves."""
    from ishapediting_amd.unet import UNetModel
    m, ref, sd, x, ts, emb = _model(name)
    spec, cfg = ref.spec, ref.cfg
    xd = x.float().to(dev())
    N = xd.shape[0]
    out0 = m(xd, ts, feat_layer=-1, keep_for_backward=True)
    acts0 = _blocks(m, spec)
    out1 = m(xd, ts, feat_layer=-1, keep_for_backward=True)
    acts1 = _blocks(m, spec)
    torch.cuda.synchronize()
    assert torch.equal(out0, out1) and _same(acts0, acts1), "a second identical forward"
    cot = (0.1 * torch.randn(out0.shape, generator=torch.Generator().manual_seed(5))).to(dev())
    m.backward_from_output(cot)
    out2 = m(xd, ts, feat_layer=-1, keep_for_backward=True)
    acts2 = _blocks(m, spec)
    torch.cuda.synchronize()
    assert torch.equal(out0, out2) and _same(acts0, acts2), "the same forward after a backward"
    # keep_for_backward=False: the output and the tap of the kept run
    k = len(spec.output_blocks) // 2 - 1
    out_k, tap_k = m(xd, ts, feat_layer=k, keep_for_backward=True)
    out_n, tap_n = m(xd, ts, feat_layer=k, keep_for_backward=False)
    out_f = m(xd, ts, feat_layer=-1, keep_for_backward=False)
    torch.cuda.synchronize()
    assert torch.equal(out_k, out0) and torch.equal(tap_k, acts0[(2, k)])
    assert torch.equal(out_n, out0) and torch.equal(tap_n, tap_k) and torch.equal(out_f, out0), "keep_for_backward=False"
    # prepared rows: all images at one prepared timestep (the only case the library serves from the prepared rows)
    t1 = [ts[-1]] * N
    out_u = m(xd, t1, feat_layer=-1, keep_for_backward=True)
    acts_u = _blocks(m, spec)
    torch.cuda.synchronize()
    assert not torch.equal(out_u, out0) or len(set(ts)) == 1      # the timestep matters
    try:
        m.prepare_timesteps([3.0, ts[-1], 411.0])
        out_p = m(xd, t1, feat_layer=-1, keep_for_backward=True)
        acts_p = _blocks(m, spec)
        out_mixed = m(xd, ts, feat_layer=-1, keep_for_backward=True)          # differing timesteps: computed in the forward as ever
        torch.cuda.synchronize()
        assert torch.equal(out_p, out_u) and _same(acts_p, acts_u), "prepared timestep rows"
        assert torch.equal(out_mixed, out0)
    finally:
        m.prepare_timesteps([])
    out_d = m(xd, t1, feat_layer=-1, keep_for_backward=True)
    acts_d = _blocks(m, spec)
    torch.cuda.synchronize()
    assert torch.equal(out_d, out_u) and _same(acts_d, acts_u), "after the prepared rows were dropped"
    # a context for a larger batch
    big = UNetModel(cfg, dev(), max_batch=N + 2)
    big.load_state_dict(sd)
    out_b = big(xd, ts, feat_layer=-1, keep_for_backward=True)
    acts_b = _blocks(big, spec)
    torch.cuda.synchronize()
    assert torch.equal(out_b, out0) and _same(acts_b, acts0), "max_batch larger than the batch served"
    del big
