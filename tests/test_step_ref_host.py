"""tests/step_ref.py on the CPU: (a) the float64 statement of the diffusion step agrees with the committed golden of the
reference's own run and with oracle.ref_cpu.DiffusionOracle; (b) the reference's operation order in numpy float32 stays inside
half of FACTOR x bound at every element of every case the device test runs; (c) each of fourteen mistakes a kernel could make
leaves FACTOR x bound by ten times or more on a NAMED case of that table, so the table cannot be thinned without this file
noticing; (d) the inputs meet the conditions the cases exist for.

Mode 1 against mode 0 differs by rounding only (exp(logvar / 2) against sqrt(exp(logvar))): no bound can tell a kernel that
runs one for the other, and none here tries.  The two are told apart by the rejection rules of the ABI instead (a guided call
takes mode 0 only; tests/test_gpu_step_oracle.py::test_rejections).

The `nonzero` mistake in mode 3 cannot show at t = 0 of any schedule: abar_prev = 1 there, so the reference's sigma is exactly
0 and the noise term vanishes with or without the mask.  The case that catches it hands the kernel the coefficients of t = 20
with the `nonzero` field set to 0: the field is part of the ABI and must be honoured as given.
"""
from collections import defaultdict

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import step_ref as R


def _worst(ratios):
    return max(float(np.max(r)) for r in ratios)


# ------------------------------------------------------------------------------------------------ a. what the project trusts
def test_statement_agrees_with_reference_golden(gold):
    """g2_steps: p_sample_guidance (noise=, clip on and off, variance_noise=) and p_sample of the reference's own code, fp32
    torch.  Held to the UNIT bound, as the reference's own evaluation is in (b)."""
    g = gold("g2_steps")
    d = R.diffusion("40")
    x, mo, noise, vn = (g[k].reshape(1, g[k].shape[1], -1) for k in ("x", "model_output", "noise", "variance_noise"))
    pn = g["psample_noise"].reshape(x.shape)
    worst = 0.0
    for t in (0, 1, 17, 39):
        o = R.step(d._coefs(t, True, 0), x, mo, noise=noise)
        rs = [R.ratio(g[f"t{t}_{k}"], o[k]) for k in ("sample", "pred_xstart", "variance", "mean")]
        rs.append(R.ratio(g[f"t{t}_sample_noclip"], R.step(d._coefs(t, False, 0), x, mo, noise=noise)["sample"]))
        rs.append(R.ratio(g[f"t{t}_sample_vn"], R.step(d._coefs(t, True, 2), x, mo, noise=vn)["sample"]))
        rs.append(R.ratio(g[f"t{t}_psample"], R.step(d._coefs(t, True, 1), x, mo, noise=pn)["sample"]))
        worst = max(worst, _worst(rs))
        print(f"g2_steps t={t}: worst |golden - f64| / bound {_worst(rs):.3f}")
    assert worst <= 0.5 * R.FACTOR, worst


class _Fixed:
    def __init__(self, mo):
        self.mo = mo

    def forward(self, x, ts, feat_layer=-1, **kw):
        return (self.mo, None) if feat_layer >= 0 else self.mo


@pytest.mark.parametrize("resp,t", [("40", 0), ("40", 20), ("40", 39), ("ddim8", 0), ("ddim8", 7)])
def test_statement_agrees_with_diffusion_oracle(resp, t):
    """oracle.ref_cpu.DiffusionOracle (fp32 torch) on shape C: p_sample_guidance with and without variance= and
    variance_noise=, p_sample, ddim_sample at eta 0 and 1, clip on and off."""
    d, orc = R.diffusion(resp), O.DiffusionOracle(O.Tables(resp))
    o = R.operands("C", resp, t)
    N, C, HW = o.x.shape
    T4 = lambda a: torch.from_numpy(np.array(a)).reshape(N, -1, 16, 16)      # noqa: E731
    net, x4, nz4, vin4 = _Fixed(T4(o.model_out)), T4(o.x), T4(o.noise), T4(o.variance_in)
    worst = 0.0
    for clip in (True, False):
        pairs = []
        want = orc.p_sample_guidance(net, x4, t, noise=nz4, clip_denoised=clip)
        got = R.step(d._coefs(t, clip, 0), o.x, o.model_out, noise=o.noise)
        pairs += [(want[k], got[k]) for k in ("sample", "pred_xstart", "variance", "mean")]
        want = orc.p_sample_guidance(net, x4, t, noise=nz4, variance=vin4, clip_denoised=clip)
        got = R.step(d._coefs(t, clip, 0), o.x, o.model_out, noise=o.noise, variance_in=o.variance_in)
        pairs += [(want[k], got[k]) for k in ("sample", "pred_xstart", "mean")]
        assert torch.equal(want["variance"], vin4)         # the dict's variance is the caller's; the ABI's is the learned one
        want = orc.p_sample_guidance(net, x4, t, variance_noise=nz4, clip_denoised=clip)
        got = R.step(d._coefs(t, clip, 2), o.x, o.model_out, noise=o.noise)
        pairs += [(want[k], got[k]) for k in ("sample", "variance")]
        want = orc.p_sample(net, x4, t, nz4, clip_denoised=clip)
        got = R.step(d._coefs(t, clip, 1), o.x, o.model_out, noise=o.noise)
        pairs += [(want[k], got[k]) for k in ("sample", "pred_xstart")]
        for eta in (0.0, 1.0):
            want = orc.ddim_sample(net, x4, t, nz4, eta=eta, clip_denoised=clip)
            got = R.step(d._coefs(t, clip, 3, eta), o.x, o.model_out, noise=o.noise)
            pairs += [(want[k], got[k]) for k in ("sample", "pred_xstart")]
        w = _worst([R.ratio(a.numpy(), b) for a, b in pairs])
        print(f"DiffusionOracle {resp} t={t} clip={clip}: worst |oracle32 - f64| / bound {w:.3f}")
        worst = max(worst, w)
    assert worst <= 0.5 * R.FACTOR, worst


# ------------------------------------------------------------------------------------------------ b. the reference alone
def test_reference_fp32_stays_inside_half_the_bound():
    """Every element of every output of every case of the device table, plus guided_update and axpby at the four element
    counts.  Prints the worst ratio per (output, mode); the module docstring of test_gpu_step_oracle.py quotes them."""
    worst = defaultdict(float)
    for c in R.STEP_CASES + R.GUIDED_CASES:
        args, kw = R.call_args(c)
        f64, f32 = R.step(*args, **kw), R.step32(*args, **kw)
        for k in R.outputs_of(c):
            w = float(np.max(R.ratio(f32[k], f64[k])))
            assert w <= 0.5 * R.FACTOR, (c.name, k, w)
            worst[(k, c.mode)] = max(worst[(k, c.mode)], w)
    for s in "ABCD":
        e = R.elementwise_operands(s)
        for gm in (None, R.GRAD_MUL):
            w = float(np.max(R.ratio(R.guided_update32(e.sample, e.variance, e.grad, R.SCALAR_SCALE, gm),
                                     R.guided_update(e.sample, e.variance, e.grad, R.SCALAR_SCALE, gm))))
            worst[("guided_update", "-")] = max(worst[("guided_update", "-")], w)
        for a, b in R.AXPBY_COEFS:
            w = float(np.max(R.ratio(R.axpby32(e.sample, e.y, a, b), R.axpby(e.sample, e.y, a, b))))
            worst[("axpby", "-")] = max(worst[("axpby", "-")], w)
    for (k, m), w in sorted(worst.items(), key=str):
        print(f"reference fp32 / unit bound: {k:14s} mode {m}: {w:.3f}")
        assert w <= 0.5 * R.FACTOR, (k, m, w)


def test_median_bounds_are_the_sizes_the_scheme_promises():
    """The bound is no blanket tolerance: relative to the value its median is a few 1e-7 .. 1e-6 for mean and sample, a few
    1e-6 for variance, and of order 1e-5 only for pred_xstart where sqrt_recip x - sqrt_recipm1 eps cancels."""
    for name, lim in (("C-40-t20-m0-given", {"mean": 5e-6, "sample": 5e-6, "variance": 1e-5, "pred_xstart": 5e-5}),
                      ("C-40-t0-m0-given", {"mean": 5e-6, "sample": 5e-6, "variance": 1e-5, "pred_xstart": 5e-5})):
        args, kw = R.call_args(R.CASES[name])
        o = R.step(*args, **kw)
        for k, l in lim.items():
            med = float(np.median(o[k].e / np.abs(o[k].v)))
            print(f"{name}: median bound / |value| of {k}: {med:.2e}")
            assert 2.0 ** -24 <= med <= l, (name, k, med)


# ------------------------------------------------------------------------------------------------ c. mistakes
CAUGHT_BY = {
    "v_from_eps": ("C-40-t20-m0-clip-given",),
    "image_stride": ("B-40-t20-m0-clip-given",),
    "vin_ignored_in_guided": ("C-40-t20-m0-clip-vin-given-scales-gm",),
    "vin_ignored_in_sample": ("B-40-t20-m0-clip-vin-given",),
    "nonzero_ignored": ("B-40-t0-m0-clip-given", "B-40-t0-m1-clip-given", "B-40-t20-m3-clip-eta1-given-nonzero0"),
    "clip_dropped": ("A-40-t20-m0-clip-given",),
    "ddim_eps_unclipped": ("B-40-t20-m3-clip-eta0-given",),
    "grad_mul_dropped": ("B-40-t20-m0-clip-given-scalar-gm",),
    "scale_of_image0": ("C-40-t20-m0-clip-given-scales",),
    "coef1_coef2_swapped": ("B-40-t1-m0-clip-given",),
    "min_max_log_swapped": ("C-ddim8-t7-m1-clip-given",),
    "second_pass_unwritten": ("D-40-t20-m3-clip-eta0.5-given", "D-40-t20-m0-clip-drawn", "D-40-t20-m0-clip-vin-given-scales-gm"),
    "noise_index_per_image": ("B-40-t20-m0-clip-drawn",),
    "rng_offset_high_dropped": ("A-40-t20-m0-clip-drawn",),
}


def test_every_mutant_has_a_catching_case():
    assert set(CAUGHT_BY) == set(R.MUTANTS)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_bound_sees_the_mistake(mutant):
    """max |mutant - f64| / (FACTOR x bound) >= 10 on each named case (every mode the mistake applies to has its own)."""
    for name in CAUGHT_BY[mutant]:
        c = R.CASES[name]                  # KeyError: the case left the table
        args, kw = R.call_args(c)
        ref = R.step(*args, **kw)
        if mutant == "second_pass_unwritten":
            got = {}
            for k in R.outputs_of(c):
                got[k] = ref[k].v.copy().reshape(-1)
                assert got[k].size > 4 * R.CAP_VECS
                got[k][4 * R.CAP_VECS:] = R.SENTINEL
        elif mutant in ("noise_index_per_image", "rng_offset_high_dropped"):
            N, C, HW = R.SHAPES[c.shape]
            bad = R.philox_normals(N * C * HW // 4, R.RNG_SEED, R.RNG_OFFSET, mutant, C * HW // 4)
            good = R.philox_normals(N * C * HW // 4, R.RNG_SEED, R.RNG_OFFSET)
            rn = float(np.max(np.abs(bad - good))) / R.NOISE_ATOL
            print(f"{mutant} on {name}: noise off by {rn:.3g} x its tolerance")
            assert rn >= 10, (mutant, name, rn)
            kw = dict(kw, noise=bad.astype(np.float32).reshape(N, C, HW))
            got = {k: v.v for k, v in R.step(*args, **kw).items()}
        else:
            got = {k: v.v for k, v in R.step(*args, mutant=mutant, **kw).items()}
        per = {k: float(np.max(R.ratio(got[k], ref[k]))) / R.FACTOR for k in R.outputs_of(c)}
        k = max(per, key=per.get)
        print(f"{mutant} caught by {name}: {k} leaves FACTOR x bound by {per[k]:.3g} x")
        assert per[k] >= 10, (mutant, name, per)
    if mutant == "second_pass_unwritten":
        e = R.elementwise_operands("D")
        for tag, ref in (("guided_update-D", R.guided_update(e.sample, e.variance, e.grad, R.SCALAR_SCALE, R.GRAD_MUL)),
                         ("axpby-D", R.axpby(e.sample, e.y, *R.AXPBY_COEFS[1]))):
            got = ref.v.copy()
            got[4 * R.CAP_VECS:] = R.SENTINEL
            w = float(np.max(R.ratio(got, ref))) / R.FACTOR
            print(f"{mutant} caught by {tag}: {w:.3g} x")
            assert got.size - 4 * R.CAP_VECS == 4 * 259 and w >= 10


# ------------------------------------------------------------------------------------------------ d. conditions on the inputs
def test_inputs_meet_their_conditions():
    shares = []
    for c in R.STEP_CASES + R.GUIDED_CASES:
        args, kw = R.call_args(c)
        o = R.step(*args, **kw)
        if c.clip and not c.nonfinite:
            share = float(np.mean(np.abs(o["x0_unclipped"].v) > 1))
            shares.append(share)
            assert 0.10 <= share <= 0.90, (c.name, share)
        for k in R.outputs_of(c):
            fin = np.isfinite(o[k].v) & np.isfinite(o[k].e)
            if c.nonfinite:
                assert not fin.all() or k == "variance", (c.name, k)
                assert fin.sum() >= fin.size - len(R.NONFINITE_AT), (c.name, k)
            else:
                assert fin.all(), (c.name, k)
    print(f"share of |unclipped x0| > 1 over the clipped cases: {min(shares):.2f} .. {max(shares):.2f}")
    for s in "ABCD":
        for resp, t in R.TIMES if s != "D" else (("40", 20),):
            o = R.operands(s, resp, t)
            v = o.model_out[:, R.SHAPES[s][1]:]
            assert (o.variance_in >= 0).all() and (o.variance_in == 0).any()
            if s != "A":
                assert (v > 1).any() and (v < -1).any()
            else:
                assert (np.abs(v) > 1).any()
    # the planted values: NaN stays NaN everywhere it reaches; under clip +-inf in eps become -+1 in pred_xstart
    c = R.CASES["B-40-t20-m0-clip-given-nonfinite"]
    args, kw = R.call_args(c)
    o = R.step(*args, **kw)
    x0 = o["pred_xstart"].v.reshape(-1)
    for at, val in R.NONFINITE_AT:
        if np.isnan(val):
            assert all(np.isnan(o[k].v.reshape(-1)[at]) for k in ("pred_xstart", "mean", "sample"))
        else:
            assert x0[at] == -np.sign(val) and o["pred_xstart"].e.reshape(-1)[at] == 0 and np.isfinite(o["sample"].v.reshape(-1)[at])
    g = R.step(*R.call_args(R.CASES["B-40-t20-m0-clip-given-scalar-gm-nonfinite"])[0],
               **R.call_args(R.CASES["B-40-t20-m0-clip-given-scalar-gm-nonfinite"])[1])["guided"].v.reshape(-1)
    assert all(np.isnan(g[at]) == bool(np.isnan(val)) for at, val in R.NONFINITE_AT)
    # torch is the semantics the statement claims
    t = torch.tensor([float("nan"), float("inf"), float("-inf")]).clamp(-1, 1)
    assert bool(torch.isnan(t[0])) and t[1] == 1 and t[2] == -1


def test_uniforms_are_the_fp32_numbers_of_the_declaration():
    """Why philox_normals rounds (w >> 8) + 0.5 to fp32 as include/ishap.h states it: at shape D the exactly formed
    construction is more than the noise tolerance away at the one pair whose u0 is within 1e-6 of 1.  (Observed on the device before the oracle stated the rounding: 2 of 2 098 188 elements off by
    up to 5.5e-5.)  With fp32 uniforms u0 can be exactly 1: the radius and both normals are then 0, never infinite."""
    N, C, HW = R.SHAPES["D"]
    exact = R.philox_normals(N * C * HW // 4, R.RNG_SEED, R.RNG_OFFSET, exact_u=True)
    d = np.abs(exact - R.drawn_noise64("D"))
    far = d > R.NOISE_ATOL
    print(f"exact against fp32 uniforms at D: {int(far.sum())} elements beyond {R.NOISE_ATOL}, max {d.max():.2e}; the rest <= {d[~far].max():.2e}")
    assert 1 <= int(far.sum()) <= 4
    assert np.isfinite(R.drawn_noise64("D")).all()
