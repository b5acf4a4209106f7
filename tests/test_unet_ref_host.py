"""tests/unet_ref.py on the CPU: the float64 restatement of the UNet agrees with the project's statement of it
(oracle/ref_cpu.UNetOracle), its hand-written per-block VJP equals autograd, every mutation of that VJP is far outside the bound
tests/test_gpu_backward_blocks.py asserts, the three configurations of that test reach every GroupNorm-backward route, and no
block can leave a skip gradient owed (csrc/backward.hip's former `pending` fall-back)."""
import ctypes as C

import pytest
import torch

from ishapediting_amd import synthetic
from ishapediting_amd.unet_spec import build_spec, full_config, tiny_config
from tests import groupnorm_ref as G
from tests import unet_ref as U

T = torch.from_numpy
FACTOR = 4.0            # the GPU test's bound: relative L2 <= FACTOR * e_r(block)


@pytest.mark.parametrize("nrb", [1, 2])
def test_restatement_agrees_with_the_statement(gold, nrb):
    """UNetRef (float64) against UNetOracle(fp16=False) (fp32) on the golden inputs of tiny_config(nrb): model output and the
    input gradient of sum(out * ct).  Measured relative L2: output 1.0e-6 / 9.6e-7, input gradient 1.6e-6 / 1.6e-6 (nrb 1 / 2)
    -- the fp32 arithmetic of the statement.  Asserted at ten times that (below the 1e-4 the comparison may never exceed)."""
    from oracle import ref_cpu as O
    g = gold("g4_tiny_unet")
    cfg = tiny_config(nrb)
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(cfg, 100 + nrb))
    x, ts, ct = T(g[f"nrb{nrb}_x"]), T(g[f"nrb{nrb}_ts"]), T(g[f"nrb{nrb}_out_ct"])
    xo = x.clone().requires_grad_(True)
    out_o = O.UNetOracle(build_spec(cfg), sd, fp16=False).forward(xo, ts)
    (gx_o,) = torch.autograd.grad((out_o * ct).sum(), xo)
    xr = x.double().requires_grad_(True)
    out_r, _ = U.UNetRef(cfg, sd).forward(xr, ts.tolist())
    (gx_r,) = torch.autograd.grad((out_r * ct.double()).sum(), xr)
    e_out, e_gx = U.rel_l2(out_o.detach().double(), out_r.detach()), U.rel_l2(gx_o.double(), gx_r)
    print(f"nrb={nrb}: output {e_out:.2e}, input gradient {e_gx:.2e}")
    assert e_out < 1e-5 and e_gx < 1.6e-5


@pytest.mark.parametrize("gmode", [U.GB_SAME, U.GB_UNPOOL, U.GB_SUM4])
@pytest.mark.parametrize("film,act", [(True, True), (False, True), (False, False)])
def test_groupnorm_pieces_are_the_groupnorm_oracles(gmode, film, act):
    """unet_ref's NCHW GroupNorm forward / backward restatements are tests/groupnorm_ref.py's (NHWC), rounding point by rounding
    point: same values on fp16 inputs, with add and add2"""
    gen = torch.Generator().manual_seed(5 + gmode)
    N, C, H = 2, 64, 8
    Hg = H // 2 if gmode == U.GB_UNPOOL else (2 * H if gmode == U.GB_SUM4 else H)
    h = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64).half().double()
    x, g, add, add2 = h(N, C, H, H), h(N, C, Hg, Hg), h(N, C, Hg, Hg), h(N, C, H, H)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=gen, dtype=torch.float64), 0.1 * torch.randn(C, generator=gen, dtype=torch.float64)
    emb = 0.3 * torch.randn(N, 2 * C, generator=gen, dtype=torch.float64)
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    got = U.gn_backward(g, x, gamma, beta, emb, film, act, gmode, add, add2, rnd=True)
    want = G.backward_restatement(nhwc(g), nhwc(x), G.stats32(nhwc(x)), gamma, beta, emb, film, act, gmode, nhwc(add), nhwc(add2))
    assert torch.equal(nhwc(got), want)
    got = U.gn_forward(x, gamma, beta, emb, film, act, pool=gmode == U.GB_UNPOOL, rnd=True)
    want = G.forward_restatement(nhwc(x), gamma, beta, emb, film, act, pool=gmode == U.GB_UNPOOL)
    assert torch.equal(nhwc(got), want)
    stm = U.gn_backward(g, x, gamma, beta, emb, film, act, gmode, add, add2)
    want = G.backward_statement(nhwc(g), nhwc(x), gamma, beta, emb, film, act, gmode, nhwc(add), nhwc(add2))
    assert U.rel_l2(nhwc(stm), want) < 1e-12


@pytest.fixture(scope="module")
def passes():
    """per configuration, its deepest pass simulated on the CPU once: (ref, emb, N, F, positions, per-position (statement, e_r))"""
    out = {}
    for name, (_, _, N, ts, starts) in U.CONFIGS.items():
        start = starts[-1]
        cfg, sd, x, ts, F_, full, cot = U.make_inputs(name, start)
        ref = U.UNetRef(cfg, sd)
        emb = ref.emb(ts)
        acts, grads, dx, x16 = ref.simulate(x, ts, F_, full, cot)
        pos = ref.positions(x16, acts, grads, F_, full, cot=U.f16r(cot), dx=dx)
        out[name] = (ref, emb, N, F_, pos, [U.position_errors(ref, p, emb)[:2] for p in pos], grads)
    return out


@pytest.mark.parametrize("name", list(U.CONFIGS))
def test_hand_written_vjp_is_autograd(passes, name):
    """rnd=False: the product csrc/backward.hip's composition is restated from equals float64 autograd of the block (1e-12), at
    every position; the yardstick e_r is a few fp16 roundings (2e-4 for the stem's single one, up to 7e-4 for three layers)"""
    ref, emb, N, F_, pos, base, _ = passes[name]
    for p, (st, e_r) in zip(pos, base):
        for a, s in zip(ref.position_autograd(p, emb), st):
            assert U.rel_l2(a, s) < 1e-12, p.name
        assert all(1e-4 < e < 1e-3 for e in e_r), (p.name, e_r)       # no gradient map has sunk into fp16 subnormals


@pytest.mark.parametrize("name", list(U.CONFIGS))
def test_every_mutation_is_far_outside_the_bound(passes, name):
    """Each mistake the composition could make moves the affected block's result (for an output block: at least one of the two
    halves it is asserted on) by more than ten times the GPU test's bound for that block, FACTOR * e_r."""
    ref, emb, N, F_, pos, base, grads = passes[name]
    seen = set()
    for p, (st, e_r) in zip(pos, base):
        for mut in U.MUTATIONS:
            if mut == "skips_swapped":
                continue
            if not ref.applies(mut, p, N, F_):
                continue
            mv = ref.position_vjp(p, emb, rnd=False, mut=mut)
            ratio = max(U.rel_l2(m, s) / (FACTOR * e) for m, s, e in zip(mv, st, e_r))
            print(f"{name} {p.name:18s} {mut:22s} moves the result by {ratio:9.1f} x bound")
            assert ratio > 10.0, (p.name, mut, ratio)
            seen.add(mut)
    # the addend handed to the wrong input block of the same shape
    n_in = len(ref.spec.input_blocks)
    for j in range(n_in):
        k = ref.swap_partner(j, F_)
        if k is None:
            continue
        p, (st, e_r) = next((p, b) for p, b in zip(pos, base) if p.add2 is grads[(2, ref.skip_source(j, F_), 2)])
        ratio = U.rel_l2(st[0] - p.add2 + grads[(2, ref.skip_source(k, F_), 2)], st[0]) / (FACTOR * e_r[0])
        print(f"{name} {p.name:18s} skips_swapped ({j} <-> {k}) moves the result by {ratio:9.1f} x bound")
        assert ratio > 10.0, (p.name, j, k, ratio)
        seen.add("skips_swapped")
    # what this pass has no place for: one image, or no upsampling ResBlock below the block the pass starts from (tiny2, tap 1)
    layers = [l for p in pos if p.blk is not None for l in p.blk.layers]
    want = set(U.MUTATIONS)
    if N == 1:
        want.discard("timestep_row")
    if not any(l.kind == "res" and l.up for l in layers):
        want.discard("sum4_one_tap")
    assert seen == want, want ^ seen
    assert name != "deep" or seen == set(U.MUTATIONS)          # the deep configuration has a place for every one of them


def test_configurations_reach_every_groupnorm_backward_route():
    """(HW, C, gmode, FiLM, SiLU) of every GroupNorm backward of the three configurations, and the route the planner gives it:
    together they cover group-local and full-map passes for the gradient at the same, half and twice the resolution, with FiLM,
    without SiLU (attention), and the head."""
    from ishapediting_amd import _lib
    L = _lib.lib()
    seen = set()
    for name, (fn, _, N, _, _) in U.CONFIGS.items():
        for hw, c, gmode, film, act, what in U.gn_backward_sites(build_spec(fn())):
            side = int(round(hw ** 0.5))
            route = C.c_int()
            assert L.ishap_group_norm32_plan(N, side, side, c, 1, 0, film, act, 0, gmode, 0, C.byref(route), *[None] * 7, None, 0) == 0
            local = route.value in (2, 3)
            assert local == (hw <= 1024), (name, what, hw, route.value)
            seen.add(("local" if local else "full", gmode))
            seen.add(("local" if local else "full", "film" if film else ("plain" if not act else "silu")))
            if what == "head":
                seen.add(("local" if local else "full", "head"))
    for where in ("local", "full"):
        for kind in (U.GB_SAME, U.GB_UNPOOL, U.GB_SUM4, "film", "plain", "silu", "head"):
            assert (where, kind) in seen, (where, kind)


def test_no_block_can_leave_a_skip_gradient_owed():
    """csrc/backward.hip hands the skip gradient owed to an input block's output to the first layer of the block after it, which
    must be a ResBlock (it adds it as add2).  build_spec only builds the resblock_updown variant: the middle block and every
    input block but the stem begin with a ResBlock, in every configuration the tests and the product use -- the separate add the
    backward once fell back to is unreachable, and the pass now refuses instead."""
    cfgs = [tiny_config(1), tiny_config(2), full_config()] + [fn() for fn, *_ in U.CONFIGS.values()]
    for cfg in cfgs:
        spec = build_spec(cfg)
        assert spec.input_blocks[0].layers[0].kind == "conv" and len(spec.input_blocks[0].layers) == 1
        for blk in spec.input_blocks[1:] + [spec.middle_block] + spec.output_blocks:
            assert blk.layers[0].kind == "res", blk.name
        # the stem is the only block that cannot take an addend, and nothing is owed to its input
        assert all(b.skip_ch > 0 for b in spec.output_blocks) and len(spec.output_blocks) == len(spec.input_blocks)
