"""The float64 drag oracle (tests/drag_ref.py) pinned on the CPU, and the input conditions of every case the device is checked
at (tests/test_gpu_drag_oracle.py): a seed that breaks a condition fails here, without a GPU."""
import numpy as np
import pytest
import torch

from tests import drag_ref as R

T = torch.from_numpy


def _tap_from_planes(feat):
    """[3,Cc,W,W] fp32 -> tap [W*W][ld] (fp32 values kept: G7's features are not fp16 numbers) + arange chmap."""
    P, Cc, W, _ = feat.shape
    ld = ((P * Cc + 31) // 32) * 32
    tap = torch.zeros(W * W, ld, dtype=torch.float32)
    tap[:, :P * Cc] = feat.reshape(P * Cc, W * W).t()
    return tap, np.arange(P * Cc, dtype=np.int32).reshape(P, Cc), ld


# ------------------------------------------------------------------------------------------------ the oracle itself
@pytest.mark.parametrize("loss_type", ["l2", "l1"])
@pytest.mark.parametrize("cof", [0.0, 0.4])
def test_oracle_agrees_with_the_g7_golden_gradients(gold, loss_type, cof):
    """The reference's own fp32 autograd gradient (G7), at the tolerance the suite uses for that fixture."""
    g = gold("g7_drag")
    edit, chmap, ld = _tap_from_planes(T(g["edit"]))
    orig, _, _ = _tap_from_planes(T(g["orig"]))
    res = R.drag_loss_grad64(edit, orig, chmap, g["sources"], g["targets"], int(g["r1"]), float(g["voxel_size"]), 16, cof, loss_type)
    got = res.grad[:, :60].t().reshape(3, 20, 16, 16)
    np.testing.assert_allclose(got.numpy(), g[f"{loss_type}_cof{cof}_grad"], rtol=1e-4, atol=1e-9)
    assert float(res.grad[:, 60:].abs().max()) == 0.0
    from oracle import ref_cpu as O
    lw = float(O.drag_loss(T(g["edit"]), T(g["orig"]), res.setup, cof, loss_type))
    assert abs(res.loss - lw) <= 1e-5 * abs(lw)


@pytest.mark.parametrize("case", R.CASES)
def test_explicit_bilinear_is_grid_sample_in_float64(case):
    """Four written-out corners against F.grid_sample(double) through autograd, loss and gradient: 1e-12 relative."""
    c = R.make_case(case)
    lt, cof = "l2", 0.4
    mine = R.oracle(case, lt, cof)
    gs = R.drag_loss_grad64(c.edit, c.orig, c.chmap, c.sources, c.targets, c.r, c.voxel, c.W, cof, lt, sampler=R.grid_sample64)
    assert abs(mine.loss - gs.loss) <= 1e-12 * abs(gs.loss)
    assert float((mine.grad - gs.grad).abs().max()) <= 1e-12 * float(gs.grad.abs().max())
    assert float((mine.d - gs.d).abs().max()) <= 1e-12 * float(gs.d.abs().max())
    assert float(gs.grad.abs().max()) > 0


def test_gradient_of_repeated_and_unmapped_channels():
    """Case H's map: the channel used twice in a plane and the one shared by two planes get the sum of their planes'
    gradients; channels absent from the map get exactly 0 (cof 0.4: the mask term reaches every mapped channel)."""
    c = R.make_case("H")
    res = R.oracle("H", "l2", 0.4)
    used = np.zeros(c.ld, bool)
    used[c.chmap.reshape(-1)] = True
    assert used.sum() == 16 and float(res.grad[:, ~used].abs().max()) == 0.0
    assert all(float(res.grad[:, ch].abs().max()) > 0 for ch in np.nonzero(used)[0])
    # finite difference on the doubly used channel 3 at the texel of its largest gradient
    i = int(res.grad[:, 3].abs().argmax())
    h = 1e-6
    e = c.edit.double().clone()
    e[i, 3] += h
    up = R.drag_loss_grad64(e, c.orig, c.chmap, c.sources, c.targets, c.r, c.voxel, c.W, 0.4, "l2").loss
    e[i, 3] -= 2 * h
    dn = R.drag_loss_grad64(e, c.orig, c.chmap, c.sources, c.targets, c.r, c.voxel, c.W, 0.4, "l2").loss
    assert abs((up - dn) / (2 * h) - float(res.grad[i, 3])) <= 1e-6 * abs(float(res.grad[i, 3]))


def test_loss_scale_reference():
    assert R.pick_scale_ref(1.0) == 256 and R.pick_scale_ref(1.5) == 128 and R.pick_scale_ref(256.0) == 1
    assert R.pick_scale_ref(0.0) == 1 and R.pick_scale_ref(np.inf) == 1 and R.pick_scale_ref(np.nan) == 1
    assert R.pick_scale_ref(2.0 ** -120) == 2.0 ** 99 and R.pick_scale_ref(2.0 ** 40) == 2.0 ** -20
    assert R.scaled_f16_ref([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11], 1.0).tolist() == [1.0, 1.0 + 2.0 ** -9]     # ties to even


# ------------------------------------------------------------------------------------------------ input conditions of the GPU cases
def _setups():
    out = [(n, R.make_case(n), R.oracle(n, *next((lt, cof) for c, lt, cof in R.COMBOS if c == n)).setup) for n in R.CASES]
    L = R.make_batch()
    for e in range(L.E):
        out.append((f"L{e}", None, R.oracle_batch("l2", False)[e][0].setup))
    return out


def test_no_lattice_texel_is_near_a_rounding_tie():
    """The mask sets round texel coordinates; the float32 reference's rounding is unambiguous when none is within 1e-4 of a
    half-integer."""
    for name, c, setup in _setups():
        W = c.W if c is not None else R.make_batch().W
        assert R.tie_margin(setup, W) >= R.TIE_MARGIN, (name, R.tie_margin(setup, W))


def test_mask_sets_are_not_empty_where_the_mask_term_is_on():
    for name, lt, cof in R.COMBOS:
        if cof > 0:
            assert R.oracle(name, lt, cof).nmask > 0, name
    assert all(o[0].nmask > 0 for o in R.oracle_batch("l2", False))


def test_l1_exclusion_stays_under_its_cap():
    """Elements whose L1 gradient hangs on an ambiguous sign: at most 1 % of the non-zero elements of g64."""
    for name, lt, cof in R.COMBOS:
        if lt != "l1":
            continue
        c, res = R.make_case(name), R.oracle(name, lt, cof)
        amb = R.l1_ambiguous_elements(res, c.edit, c.orig, c.chmap, c.W)
        assert int(amb.sum()) <= R.L1_EXCLUDED_CAP * int((res.grad != 0).sum()), (name, cof, int(amb.sum()))
    L = R.make_batch()
    for e, (res, _) in enumerate(R.oracle_batch("l1", False)):
        amb = R.l1_ambiguous_elements(res, L.edits[e], L.origs[e], L.chmap, L.W)
        assert int(amb.sum()) <= R.L1_EXCLUDED_CAP * int((res.grad != 0).sum()), (e, int(amb.sum()))


def test_case_b_has_a_tail_segment():
    c = R.make_case("B")
    assert c.side == 7 and R.tail_positions(c.side) == (2, 3)                  # positions 5, 6 live; 7, 8, 9 have i >= side
    assert (c.Cc + 63) // 64 == 2 and c.Cc - 64 == 6                           # two channel chunks, 6 live lanes in the second
    assert R.tail_positions(R.make_case("A").side) is None                     # A (G7's regime) has none
    assert R.make_case("C").side == 1 and R.make_case("C").Cc == 64
    j = R.make_case("J")
    assert j.Cc == 170 and j.Cc - 128 == 42 and j.side == 5 * R.DSEG and j.ld == 512


def test_case_d_jumps_and_leaves_the_map_on_every_side():
    c = R.make_case("D")
    setup = R.oracle("D", "l2", 0.0).setup
    steps = R.walk_columns(setup, c).diff(dim=-1)
    assert int(steps.min()) >= 2, steps                                        # the jump branch on every step
    ix, iy, x0, y0 = R.corners(setup.shift_grid.double(), c.W)
    W = c.W
    for v0 in (x0, y0):
        assert bool((v0 == -1).any()) and bool((v0 == W - 1).any())            # partly outside, low and high side
        assert bool((v0 < -1).any()) and bool((v0 >= W).any())                 # wholly outside, low and high side


def test_case_e_steps_by_exactly_one_texel():
    c = R.make_case("E")
    # W must be even (the kernels need 3 * W * W % 4 == 0), so 2 / (W - 1) is no fp32 number: the pitch is 1 to an ulp
    pitch = float(np.float32(c.voxel)) * (c.W - 1) / 2
    assert abs(pitch - 1.0) <= 2.0 ** -23
    steps = R.walk_columns(R.oracle("E", "l2", 0.0).setup, c).diff(dim=-1)
    assert bool((steps == 1).all()), steps                                     # the carry branch on every step


def test_case_a_never_jumps():
    """G7's regime: consecutive positions share a column or step by one."""
    steps = R.walk_columns(R.oracle("A", "l2", 0.0).setup, R.make_case("A")).diff(dim=-1)
    assert int(steps.min()) >= 0 and int(steps.max()) <= 1


def test_case_f_reaches_every_border_situation():
    c = R.make_case("F")
    setup = R.oracle("F", "l2", 0.0).setup
    W = c.W
    for grid in (setup.shift_grid, setup.patch_grid):                           # targets (edit, scatter) and sources (guidance)
        ix, iy, x0, y0 = R.corners(grid.double(), W)
        for t, t0, o0 in ((ix, x0, y0), (iy, y0, x0)):
            other_in = (o0 >= 0) & (o0 < W - 1)                                # the other axis inside: the sample is in the map
            assert bool(((t0 == -1) & (t > -1) & other_in).any())              # t in (-1, 0)
            assert bool(((t0 == W - 1) & (t > W - 1) & other_in).any())        # t in (W-1, W)
            assert bool(((t == W - 1) & other_in).any())                       # t = W-1 exactly
    _, _, x0, y0 = R.corners(setup.shift_grid.double(), W)
    out = (x0 < -1) | (x0 >= W) | (y0 < -1) | (y0 >= W)                        # [3, B, N]: all four corners outside
    assert bool(out[:, 1].all()) and not bool(out[:, 0].all())                 # handle 1's target: outside on every plane
    _, _, x0, y0 = R.corners(setup.patch_grid.double(), W)
    assert bool(((x0 < -1) | (x0 >= W) | (y0 < -1) | (y0 >= W))[:, 2].all())   # handle 2's source


def test_case_i_handles_overlap_and_one_stands_still():
    c = R.make_case("I")
    assert c.B == 4 and np.array_equal(c.targets[0], c.targets[1]) and np.array_equal(c.targets[2], c.sources[2])
    assert not np.array_equal(c.sources[0], c.sources[1])


def test_channel_maps_of_cases_g_and_h():
    g = R.make_case("G")
    used = np.unique(g.chmap)
    assert g.Cc == 20 and g.ld == 64 and len(used) < g.ld and used.max() < g.ld          # a gather that skips channels
    assert not np.array_equal(g.chmap.reshape(-1), np.arange(60))
    h = R.make_case("H")
    cnt = np.stack([np.bincount(h.chmap[p], minlength=h.ld) for p in range(3)])
    assert cnt[0, 3] == 2 and cnt[0, 5] == 1 and cnt[1, 5] == 1 and (cnt.sum(0) == 0).sum() == 16


def test_small_magnitude_cases_share_case_b():
    b = R.make_case("B")
    for name, k in (("K6", 6), ("K12", 12)):
        c = R.make_case(name)
        assert np.array_equal(c.sources, b.sources) and c.Cc == b.Cc and c.r == b.r
        assert 0.5 < float(c.edit.float().abs().max()) * 2.0 ** k / float(b.edit.float().abs().max()) < 2.0
