"""tests/unet_ref.py on the CPU: the float64 restatement of the UNet agrees with the project's statement of it
(oracle/ref_cpu.UNetOracle), its hand-written per-block VJP equals autograd, every mutation of that VJP is far outside the bound
tests/test_gpu_backward_blocks.py asserts, the three configurations of that test reach every GroupNorm-backward route, and no
block can leave a skip gradient owed (csrc/backward.hip's former `pending` fall-back).  For tests/test_gpu_forward_blocks.py: the
forward's yardstick is fp16 rounding at every block, every mutation of the forward's composition is far outside that test's
bound, the head's split restatement meets the head's two conditions, and the forward configurations reach every launch form."""
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


# ------------------------------------------------------------------------------------------------------------ the forward, block by block
@pytest.fixture(scope="module")
def forwards():
    """per forward configuration, the rounded forward on the CPU once: (ref, ts, N, x16, acts, out, positions, per-position
    (statement, e_r whole batch, e_r per image)); the head's `out` is its split restatement"""
    out = {}
    for name, (_, _, N, ts) in U.FORWARD_CONFIGS.items():
        cfg, sd, x, ts = U.make_forward_inputs(name)
        ref = U.UNetRef(cfg, sd)
        emb = ref.emb(ts)
        _, acts = ref.forward(x, ts, rnd=True)
        head = ref.head_restatement(acts[(2, len(ref.spec.output_blocks) - 1)])
        pos = ref.forward_positions(U.f16r(x), acts, head)
        base = []
        for p in pos:
            st, e_r, _, _ = U.forward_position_errors(ref, p, emb)
            base.append((st, e_r[0], e_r[1]))
        out[name] = (ref, ts, N, U.f16r(x), acts, head, pos, base)
    return out


def _head_l2_bound(ref, p, st):
    """the GPU test's second head condition: one tenth of the error of the head with its lo products dropped"""
    return 0.1 * U.rel_l2(ref.head_restatement(p.x_in, lo=False), st)


@pytest.mark.parametrize("name", list(U.FORWARD_CONFIGS))
def test_forward_yardstick_is_fp16_rounding(forwards, name):
    """e_r of every block of every forward configuration, for the whole batch and for each image, lies in (1e-4, 1e-3): 2.1e-4 for
    the stem's single rounding, 3.0e-4 .. 6.1e-4 for the others.  No activation has saturated or sunk into fp16 subnormals, so
    FACTOR * e_r means a few fp16 roundings.  The head is fp32-grade and has a criterion of its own: its split restatement is
    3.2e-7 .. 5.5e-7 from the statement, the head without the lo products 3.0e-4 .. 3.2e-4 (an fp16 rounding)."""
    ref, ts, N, x16, acts, head, pos, base = forwards[name]
    for p, (st, e, e_img) in zip(pos, base):
        print(f"{name} {p.name:18s} {p.kind:30s} e_r {e:.2e}  per image {min(e_img):.2e} .. {max(e_img):.2e}")
        if p.blk is None:
            e_lo = 10.0 * _head_l2_bound(ref, p, st)
            print(f"{name} head without lo: {e_lo:.2e}")
            assert e < 1e-6 and 1e-4 < e_lo < 1e-3, (name, e, e_lo)
        else:
            assert all(1e-4 < v < 1e-3 for v in [e] + e_img), (name, p.name, e, e_img)


@pytest.mark.parametrize("name", list(U.FORWARD_CONFIGS))
def test_every_forward_mutation_is_far_outside_the_bound(forwards, name):
    """Each mistake the forward's composition could make (unet_ref.FORWARD_MUTATIONS) moves a position it applies to by more than
    ten times that position's bound in tests/test_gpu_forward_blocks.py: FACTOR * e_r for the whole batch or for one image
    (whichever ratio is larger -- the GPU test asserts both), for the head one tenth of the lo-dropped head's error.  On the 128^2
    configurations a mutation is evaluated until the first position that shows it (each evaluation is a float64 block at 128^2);
    elsewhere at every position it applies to.  Smallest .. largest ratio over the 6 configurations, in units of the bound:
        film_row               80 .. 153       film_dropped           71 .. 121       film_halves_swapped    44 .. 83
        emb_silu_dropped       65 .. 152       temb_sincos_swapped    78 .. 145       stats_other_image      21 .. 2071
        skip_identity_dropped 320 .. 810       pool_one_tap          515 .. 673       up_shifted            275 .. 414
        attn_residual_dropped 406 .. 650       attn_heads_new_order  131 .. 353       attn_scale             23 .. 111
        halves_swapped        415 .. 1214      seam_shifted          250 .. 641       skips_swapped         174 .. 278
        head_silu_dropped   30000 .. 36000     head_lo_dropped        10 (by construction: the bound IS a tenth of its error)
    Every mutation is above 10 at every position evaluated; the GPU test can see each of these mistakes wherever it can be made.
    (With two randn images of one scale at 128^2 the other image's GroupNorm statistics moved the first ResBlock by 4.4 bounds only:
    the forward-only configurations scale their images, unet_ref.IMAGE_SCALES.  attn_heads_new_order has no place in `top` /
    `top2`, whose attention has one head.)"""
    ref, ts, N, x16, acts, head, pos, base = forwards[name]
    emb = ref.emb(ts)
    first_hit = ref.cfg.image_size >= 128
    seen, best = set(), {}
    for mut in U.FORWARD_MUTATIONS:
        mpos = ref.forward_positions(x16, acts, head, mut)
        memb = ref.emb(ts, mut)
        for p, mp, (st, e, e_img) in zip(pos, mpos, base):
            if not ref.forward_applies(mut, p, N) or (first_hit and mut in seen):
                continue
            mv = ref.position_forward(mp, memb, rnd=False, mut=mut)
            if p.blk is None:
                ratio = U.rel_l2(mv, st) / _head_l2_bound(ref, p, st)
            else:
                ratio = max([U.rel_l2(mv, st) / (FACTOR * e)] + [m / (FACTOR * r) for m, r in zip(U.rel_l2_images(mv, st), e_img)])
            print(f"{name} {p.name:18s} {mut:22s} moves the result by {ratio:9.1f} x bound")
            best[mut] = max(best.get(mut, 0.0), ratio)
            if ratio > 10.0 or (mut == "head_lo_dropped" and ratio > 10.0 - 1e-9):
                seen.add(mut)
            assert ratio > 10.0 - 1e-9, (name, p.name, mut, ratio)
    layers = [l for p in pos if p.blk is not None for l in p.blk.layers]
    want = set(U.FORWARD_MUTATIONS)
    if N == 1:
        want -= {"film_row", "stats_other_image"}
    if not any(l.kind == "res" and l.up for l in layers):
        want.discard("up_shifted")
    if not any(l.kind == "res" and l.down for l in layers):
        want.discard("pool_one_tap")
    if not any(l.kind == "attn" for l in layers):
        want -= {"attn_residual_dropped", "attn_scale"}
    if not any(l.kind == "attn" and l.heads > 1 for l in layers):
        want.discard("attn_heads_new_order")
    if all(ref.forward_swap_partner(j) is None for j in range(len(ref.spec.input_blocks))):
        want.discard("skips_swapped")
    assert seen == want, (want ^ seen, best)
    assert name not in ("deep", "deep8") or seen == set(U.FORWARD_MUTATIONS)      # these have a place for every one of them


@pytest.mark.parametrize("name", list(U.FORWARD_CONFIGS))
def test_head_restatement_is_inside_the_head_bounds(forwards, name):
    """The head's hi/lo-split restatement (a_hi w_hi + a_lo w_hi + a_hi w_lo on fp32 statistics) at the rounded forward's last block
    output meets both head conditions of the GPU test -- every element inside conv(b_a, |w|) + ACC_REL (conv(|a|, |w|) + |bias|),
    relative L2 below a tenth of the lo-dropped head's error -- while the head without its lo products or without its SiLU is more
    than 10 times outside the second.  Measured: split 3.2e-7 .. 5.5e-7 relative L2 (worst element 0.007 .. 0.008 of its bound),
    lo dropped 3.0e-4 .. 3.2e-4 (worst element 3.9 .. 6.5 of its bound: the elementwise condition alone does not separate a plain
    fp16 head by an order of magnitude, the L2 condition does), SiLU dropped 0.97 .. 1.10."""
    ref, ts, N, x16, acts, head, pos, base = forwards[name]
    p, (st, e, _) = pos[-1], base[-1]
    assert p.blk is None
    bound = ref.head_bound(p.x_in)
    l2 = _head_l2_bound(ref, p, st)
    lo = ref.head_restatement(p.x_in, lo=False)
    nosilu = ref.head(p.x_in, "head_silu_dropped")
    worst = lambda t: float(((t - st).abs() / bound).max())
    print(f"{name}: split {e:.2e} (worst element {worst(head):.4f} of its bound), lo dropped {U.rel_l2(lo, st):.2e} "
          f"(worst element {worst(lo):.2f}), SiLU dropped {U.rel_l2(nosilu, st):.2e}; L2 bound {l2:.2e}")
    assert worst(head) <= 1.0 and e <= l2
    assert U.rel_l2(lo, st) >= 10.0 * l2 * (1 - 1e-12) and U.rel_l2(nosilu, st) > 10.0 * l2
    import tests.test_gpu_igemm_oracle as I
    assert U.ACC_REL == I.ACC_REL


def test_forward_configurations_reach_every_launch_form():
    """(HW, C, FiLM, SiLU, pool, split) of every GroupNorm forward and (M, cin, cout, taps, folded skip, upsampled input) of every
    convolution of the forward configurations (unet_ref.forward_sites), with what the planners give each (no GPU needed).
    GroupNorm, route x form -- reached:
        group-local (routes 2 / 3: deep, tiny2, deep8, wide)   SiLU | FiLM + SiLU | SiLU + 2x2 pool | plain (attention)
        full map (routes 1 / 4: top, top2)                     SiLU | FiLM + SiLU | SiLU + 2x2 pool | plain (attention) | hi/lo split
      not reachable: group-local x split -- csrc/unet.hip's gn_forward_op sends the head's split form down the full-map route on
      every map (`!split && local_gn`): deep, tiny2, deep8 and wide run the head's split form through the full-map kernels on 32^2
      and 16^2 maps.  Inputs still pending (the producer's K slices) reach the group-local route with and without FiLM.
    Convolutions -- reached: K split above 1 with the slices left pending (deep, tiny2, deep8, wide: conv1 in front of a group-local
      GroupNorm, conv2 with and without the folded 1x1 skip, splits 2 .. 8); K split above 1 reduced IN PLACE (wide only: conv2
      behind a separately launched 1x1 skip and the head, K = 2592, split 4); no split; 3x3 with an upsampled input; the folded
      and the separately launched 1x1 skip; qkv / proj_out GEMMs and the fused 8x8 attention (deep) beside the unfused one on the
      same map (deep8: 8 images x 4 heads x 12 parts exceed the 256 compute units the fused form may claim; tiny2, wide: heads of 32).
      In CONFIGS' three, top2, deep8 and in full_config itself NO forward launch is reduced in place: wherever K is long enough to
      split the map is small and the consumer adds the slices up, and where the forward does not ask for that (full maps, qkv,
      the separately launched skip) K stays below the 36 K-steps of the split policy or the grid fills the chip already."""
    from ishapediting_amd import _lib
    L = _lib.lib()
    gn_seen, conv_seen = set(), set()
    per_cfg_inplace = {}
    cfgs = {name: (fn(), N) for name, (fn, _, N, _) in U.FORWARD_CONFIGS.items()}
    cfgs["full_config"] = (full_config(), 1)
    for name, (cfg, N) in cfgs.items():
        gns, convs = U.forward_sites(build_spec(cfg), N)
        per_cfg_inplace[name] = 0
        for g in gns:
            side = int(round(g.HW ** 0.5))
            route, kern = C.c_int(), C.create_string_buffer(256)
            assert L.ishap_group_norm32_plan(N, side, side, g.C, 0, g.pending, g.film, g.act, g.pool, 0, 0, C.byref(route), *[None] * 7,
                                             kern, len(kern)) == 0, (name, g)
            local = route.value in (2, 3)
            assert local == (g.HW <= 1024), (name, g, route.value)          # forward_sites' `small map` is the planner's
            form = "split" if g.split else ("film" if g.film else ("pool" if g.pool else ("silu" if g.act else "plain")))
            where = "full" if g.split or not local else "local"             # gn_forward_op: the split form has no group-local kernel
            if name != "full_config":
                gn_seen.add((where, form))
                if g.pending and local:
                    gn_seen.add(("local-pending", form))
        for c in convs:
            ks, slot, kern = C.c_int(), C.c_int(), C.create_string_buffer(256)
            assert L.ishap_igemm_plan(c.M, c.cin, c.cout, c.taps, c.K2, c.H, c.W, 1, c.pending, c.sums, C.byref(ks), C.byref(slot), kern,
                                      len(kern)) == 0, (name, c)
            tags = ["pending" if ks.value > 1 and c.pending else ("in place" if ks.value > 1 else "no split")]
            if ks.value > 1 and not c.pending:
                per_cfg_inplace[name] += 1
            tags += ["ups"] * c.ups + ["folded skip"] * (c.K2 > 0) + ["skip 1x1"] * c.what.endswith("skip") + ["sums"] * c.sums
            tags += ["qkv"] * c.what.endswith("qkv")
            if name != "full_config":
                conv_seen.update(tags)
                print(f"{name:6s} {c.what:32s} M {c.M:6d} K {c.taps * c.cin + c.K2:5d} -> {c.cout:4d}  split {ks.value}  "
                      f"{' '.join(tags):24s} {kern.value.decode()}")
        n_attn = sum(1 for g in gns if g.what.endswith("norm"))
        n_unfused = sum(1 for c in convs if c.what.endswith("qkv"))
        if name != "full_config":
            conv_seen.update(["fused attention"] * (n_attn > n_unfused) + ["unfused attention"] * (n_unfused > 0))
    print(sorted(gn_seen), sorted(conv_seen), per_cfg_inplace)
    for where in ("local", "full"):
        for form in ("silu", "film", "pool", "plain"):
            assert (where, form) in gn_seen, (where, form)
    assert ("full", "split") in gn_seen and ("local", "split") not in gn_seen
    assert ("local-pending", "film") in gn_seen and ("local-pending", "silu") in gn_seen
    for tag in ("pending", "in place", "no split", "ups", "folded skip", "skip 1x1", "sums", "qkv", "fused attention", "unfused attention"):
        assert tag in conv_seen, tag
    assert [k for k, v in per_cfg_inplace.items() if v] == ["wide"], per_cfg_inplace
