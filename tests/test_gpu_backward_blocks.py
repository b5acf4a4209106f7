"""Every block's input gradient of the UNet backward pass (csrc/backward.hip) against a float64 VJP of that block alone.

The kernels the pass launches each have a launch-by-launch float64 oracle; this module checks their COMPOSITION: which gradient
is added to which, which map is split, which route a GroupNorm takes, in what order the skip gradients are popped.  After one kept
forward and one backward, every block's output (`block_output`) and every block's gradient maps (`block_grad`) are read back, and
each block's outgoing gradient is compared with `unet_ref.UNetRef`'s VJP evaluated at the DEVICE's own block input and the
DEVICE's own incoming gradient (fp16 -> float64).  Nothing is chained, so an error belongs to exactly one block:

    output block i       (part 1, part 2) == VJP_i(part 0)                      each half asserted on its own
    output block i, h    part 1 of block i is bit-equal to part 0 of block i - 1 (the middle block for i = 0)
    last input block     G(in last) == VJP_mid(G(mid)) + S(last)
    input block i - 1    G(in i-1)  == VJP_in_i(G(in i)) + S(i-1)               S(j): part 2 of the output block that read hs[j]
    stem                 dx == VJP_stem(G(in 0)) * scale2[1]
    head (full depth)    G(out last) == VJP_head(fp16(cot))

Bound, per block (and per half of an output block): relative L2 <= 4 * e_r, where e_r is the distance of unet_ref's ROUNDED
restatement of the same VJP (fp16 wherever the device keeps fp16; listed in tests/unet_ref.py) from the unrounded one, computed
from the reference alone.  The factor 4 covers what the restatement leaves out: fp32 accumulation order, __expf / v_rcp_f32, the
fixed-point GroupNorm-backward sums, and the occasional neighbouring-fp16 flip of a recomputed value -- each below one fp16 unit
in the GroupNorm and implicit-GEMM oracles.  tests/test_unet_ref_host.py shows that every mistake of the composition it models
moves a block's result by more than 40 times this bound.  No block, element or case is left out.

Configurations (tests/unet_ref.CONFIGS; the host test asserts that together they reach every GroupNorm-backward route):
  top    128^2 / 64^2 maps, 64 channels, N = 1, from the last tap and from the output: the full-map routes -- sums from the dgrad
         epilogue (GB_SAME), two-pass GB_UNPOOL (the down ResBlock reads 128^2) and GB_SUM4 (the up ResBlock reads 64^2), the
         128 -> 64 convolutions with the 1x1 skip; the middle block's attention runs on the 64^2 map (4096 tokens);
  deep   test_gpu_chains._cfg_mid, N = 2 at timesteps 617 and 23, from tap 2 and from the output: the group-local routes,
         pending split-K gradients, attention backward;
  tiny2  tiny_config(2), N = 2, from tap 1: one channel per group, the 96-channel concatenation, two ResBlocks per level; once
         more with scale2 = (2^20, 2^-20) and the cotangent * 1e-6 * 2^20 in fp16, under the same bound.
x = randn, cotangent = 0.1 randn.  No gradient map of these passes sinks into fp16 subnormals (e_r stays between 2e-4 and 7e-4 at
every block), so `top` and `deep` run unscaled.

MEASURED (MI355X, all six passes; the module takes 7.4 s, the 128^2 float64 reference 1.3 - 1.6 s of it per pass).  Worst
error / e_r per block kind, and in brackets the worst distance of the device from the ROUNDED restatement in units of e_r:
    conv (stem)                   1.00 (0.06)        head                          1.00 (0.04)
    res                           1.00 (0.20)        res:down                      1.00 (0.34)
    cat res+skip1x1               1.00 (0.20)        cat res+skip1x1|res:up        1.00 (0.71)
    res|attn                      1.01 (0.61)        res+skip1x1|attn              1.02 (1.03)
    cat res+skip1x1|attn          1.01 (0.94)        cat res+skip1x1|attn|res:up   1.01 (0.90)
    res|attn|res (middle block)   1.01 (0.92)
The error is the fp16 rounding itself (ratio 1): no block kind comes near the factor 4, and the comparison found no bug in the
composition.  It did prompt two additions to the restatement, both already stated by the attention oracle: exp(s - max) goes
into the P V product in fp16, and dS and P go into the backward's second products in fp16.  What the brackets say: a block of ONE
layer is explained by the restatement to 0.03 - 0.34 e_r.  A block of two or three layers is as far from it as from the
unrounded product, because the activation between its layers cannot be read back and is recomputed: of a one-layer block's
OUTPUT, 1 - 5 % of the elements differ from the restatement's by one fp16 unit (fp32 accumulation order), the next layer's dense
products spread those flips over every element, and after a second or third layer 12 - 50 % differ -- measured on the forward of
these configurations.  That is the 'neighbouring-fp16 flip' term of the factor, not a missing rounding point."""
import time

import pytest
import torch

from ishapediting_amd import synthetic
from ishapediting_amd.unet_spec import build_spec, tiny_config
from tests import unet_ref as U

pytestmark = pytest.mark.gpu
FACTOR = 4.0


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _to_tap(ct):
    """[N][C][S][S] -> the tap's layout [N][S*S][C] fp16"""
    return ct.permute(0, 2, 3, 1).reshape(ct.shape[0], -1, ct.shape[1]).contiguous().half()


_MODELS = {}


def _model(name):
    """one context per configuration, shared by its passes"""
    from ishapediting_amd.unet import UNetModel
    if name not in _MODELS:
        cfg, sd, *_ = U.make_inputs(name, "out")
        N = U.CONFIGS[name][2]
        m = UNetModel(cfg, dev(), max_batch=N)
        m.load_state_dict(sd)
        _MODELS[name] = (m, U.UNetRef(cfg, sd))
    return _MODELS[name]


def _read_grads(m, spec, F_):
    f64 = lambda t: t.double().cpu()
    grads = {}
    for i in range(len(spec.input_blocks)):
        grads[(0, i, 0)] = f64(m.block_grad(0, i))
    grads[(1, 0, 0)] = f64(m.block_grad(1))
    for i in range(F_ + 1):
        for part in (0, 1, 2):
            grads[(2, i, part)] = f64(m.block_grad(2, i, part))
    return grads


def _backward(m, full, cot, scaled):
    """the pass; returns dx with the loss scale put back (exact: a power of two), so that it belongs to the stored gradient maps"""
    if scaled:
        assert not full
        scale2 = torch.tensor([2.0 ** 20, 2.0 ** -20], device=dev())
        return m.backward_input(_to_tap(cot * 1e-6 * 2.0 ** 20).to(dev()), scale2).double().cpu() * 2.0 ** 20
    if full:
        return m.backward_from_output(cot.float().to(dev())).double().cpu()
    return m.backward_input(_to_tap(cot).to(dev())).double().cpu()


CASES = [(name, start, False) for name, (_, _, _, _, starts) in U.CONFIGS.items() for start in starts] + [("tiny2", 1, True)]
WORST, NEAR = {}, {}


@pytest.mark.parametrize("name,start,scaled", CASES, ids=[f"{n}-{s}{'-scaled' if sc else ''}" for n, s, sc in CASES])
def test_every_block_input_gradient_vs_float64_vjp(name, start, scaled):
    t0 = time.time()
    m, ref = _model(name)
    cfg, sd, x, ts, F_, full, cot = U.make_inputs(name, start)
    spec = ref.spec
    f64 = lambda t: t.double().cpu()
    m(x.float().to(dev()), ts, feat_layer=-1 if full else F_, keep_for_backward=True, want_inter_feat=False)
    dx = _backward(m, full, cot, scaled)
    grads = _read_grads(m, spec, F_)
    acts = {(0, i): f64(m.block_output(0, i)) for i in range(len(spec.input_blocks))}
    acts[(1, 0)] = f64(m.block_output(1))
    acts.update({(2, i): f64(m.block_output(2, i)) for i in range(F_ + 1)})
    # a second backward on the same forward (the statistics scratch is zeroed again): the same bits in every map
    dx2 = _backward(m, full, cot, scaled)
    again = _read_grads(m, spec, F_)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx2)
    for k in grads:
        assert torch.equal(grads[k], again[k]), k
    # the h half of output block i is what the block below it receives
    for i in range(F_ + 1):
        below = grads[(2, i - 1, 0)] if i else grads[(1, 0, 0)]
        assert torch.equal(grads[(2, i, 1)], below), i
    if not full and not scaled:
        assert torch.equal(grads[(2, F_, 0)], U.f16r(cot))        # the pass started from the caller's cotangent
    emb = ref.emb(ts)
    bad = []
    for pos in ref.positions(U.f16r(x), acts, grads, F_, full, cot=U.f16r(cot), dx=dx):
        _, e_r, err, to_rounded = U.position_errors(ref, pos, emb)
        for part, (e, r, d) in enumerate(zip(err, e_r, to_rounded)):
            ratio = e / r
            print(f"{name}-{start}{'-scaled' if scaled else ''} {pos.name:18s} {pos.kind:30s} part {part}: error {e:.3e}  e_r {r:.3e}  "
                  f"error / e_r {ratio:.2f}  (from the rounded restatement: {d / r:.2f} e_r)")
            WORST[pos.kind] = max(WORST.get(pos.kind, 0.0), ratio)
            NEAR[pos.kind] = max(NEAR.get(pos.kind, 0.0), d / r)
            if not e <= FACTOR * r:
                bad.append((pos.name, pos.kind, part, e, r, ratio))
    print(f"{name}-{start}: {time.time() - t0:.1f} s; worst error / e_r per block kind so far (and worst distance from the rounded "
          "restatement): " + ", ".join(f"{k}: {v:.2f} ({NEAR[k]:.2f})" for k, v in sorted(WORST.items())))
    assert not bad, bad


def test_block_grad_refuses_what_it_cannot_serve():
    from ishapediting_amd.unet import UNetModel
    cfg = tiny_config(1)
    spec = build_spec(cfg)
    n_out = len(spec.output_blocks)
    m = UNetModel(cfg, dev())
    m.load_state_dict(synthetic.round_torso_to_fp16(synthetic.unet_state_dict(cfg, 101)))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(1, 6, 16, 16, generator=g).to(dev())
    k = 1
    ch, sz = m.tap_shape(k)
    cot = (0.1 * torch.randn(1, sz * sz, ch, generator=g)).half().to(dev())
    with pytest.raises(RuntimeError, match="only after a backward"):
        m.block_grad(1)                                         # a fresh context (the shape query alone would pass)
    m(x, [37.0], feat_layer=k, keep_for_backward=True, want_inter_feat=False)
    with pytest.raises(RuntimeError, match="only after a backward"):
        m.block_grad(1)                                         # a forward, no backward yet
    dx = m.backward_input(cot)
    ws = m.workspace_bytes()
    first = m.block_grad(0, 1).clone()
    assert m.block_grad(2, k).shape == (1, ch, sz, sz) and m.block_grad(2, 0, 2).shape[1] == spec.output_blocks[0].skip_ch
    assert m.block_grad(2, 0, 1).shape[1] == spec.output_blocks[0].cin - spec.output_blocks[0].skip_ch
    assert m.workspace_bytes() == ws                            # reading allocates nothing in the context
    assert torch.equal(m.backward_input(cot), dx) and torch.equal(m.block_grad(0, 1), first)
    for i in range(k + 1, n_out):
        with pytest.raises(RuntimeError, match="started below"):
            m.block_grad(2, i)                                  # above the tap the backward started from
    for group in (0, 1):
        for part in (1, 2):
            with pytest.raises(RuntimeError, match="output blocks only"):
                m.block_grad(group, 0, part)
    with pytest.raises(RuntimeError):
        m.block_grad(2, 0, 3)
    with pytest.raises(RuntimeError):
        m.block_grad(0, len(spec.input_blocks))
    m(x, [37.0], feat_layer=k, keep_for_backward=True, want_inter_feat=False)
    with pytest.raises(RuntimeError, match="stale"):
        m.block_grad(1)                                         # the forward reused the arena
    # a snapshot of a forward that only planned its tail holds the network up to the tap
    m(x, [37.0], feat_layer=k, keep_for_backward=True, want_inter_feat=False, overlap_tail=True)
    m.backward_input(cot)
    m.run_tail()
    m.join_tail()
    assert m.snapshot_save()
    assert torch.equal(m.block_grad(0, 1), first)               # neither the tail nor the save touches the gradient maps
    assert m.snapshot_restore()
    with pytest.raises(RuntimeError, match="stale"):
        m.block_grad(1)                                         # the maps belong to a pass before the restore
    assert torch.equal(m.backward_input(cot), dx) and torch.equal(m.block_grad(0, 1), first)
    with pytest.raises(RuntimeError):
        m.block_grad(2, k + 1)
    # a full-depth pass serves every output block
    m(x, [37.0], feat_layer=-1, keep_for_backward=True)
    m.backward_from_output(torch.randn(1, cfg.out_channels, 16, 16, generator=g).to(dev()))
    assert m.block_grad(2, n_out - 1).shape == (1, spec.final_ch, 16, 16)
    torch.cuda.synchronize()
