"""csrc/ddpm.hip launch by launch through the C ABI (ctypes) against the float64 statement of tests/step_ref.py:
ishap_ddpm_step, ishap_ddpm_step_guided, ishap_ddpm_step_guided_scales, ishap_guided_update and ishap_axpby, at every mode,
operand, output and tail.  The case table, the bound and its derivation are in tests/step_ref.py; tests/test_step_ref_host.py
pins the statement to the reference's golden, shows that the reference's own fp32 evaluation stays inside half of what is
allowed here, and names, for each of fourteen kernel mistakes, the case of this table that catches it.

Bound (not tuned to the device): every written output element within FACTOR x bound of the float64 value, FACTOR = 2, bound the
element's own first-order fp32 error of the reference's operation order.  Where the statement is NaN the device must give NaN,
where it is +-inf that infinity.  Drawn noise: 2e-5 absolute against the documented Philox / Box-Muller construction (the
tolerance of test_gpu_parity.py::test_step_draws_its_own_noise), and the step with drawn noise BITWISE the step with that noise
injected.

Shapes (N x C x HW): A 1x1x4 one vector; B 2x3x36 the image boundary inside a wave; C 3x6x256 the batched shape; D 3x4x174849
= 524 547 vectors, 259 beyond the 2048 x 256 grid cap and all in the last image (run for mode 0 guided with per-image scales,
mode 3, drawn noise, guided_update and axpby only).  On A to C: modes 0-3 x clip on / off x t in {0, 1, 20, 39} of "40", 999 of
"1000", {0, 7} of "ddim8" x eta {0, 0.5, 1} (mode 3) x variance_in absent / given (mode 0) x noise given / NULL / drawn; guided
calls with a scalar scale and per-image scales that include 0, grad_mul_dev NULL and a device 2^-9.  The output-pointer
combinations (all at once, each alone, guided alone) run at t = 20 of "40" for every shape, mode, clip, variance_in, scale kind
and grad_mul: which pointers are NULL does not depend on the timestep.

Memory discipline: 64 sentinel floats behind every output must survive; every input is bit-identical after the call; an
output that was not requested is passed as NULL and the others keep their bits.  No caller in the package passes an output
that aliases an input (ishap_axpby and ishap_guided_update write fresh tensors in gaussian_diffusion.py:388-408 and
drag_utils.py:970-976, :1274-1279; the step's outputs are torch.empty_like in SpacedDiffusion._step), so no aliased call is
made here.

ishap_x0_grad_to_cotangent (csrc/decode_bwd.hip) masks with comparisons (x0 < -1 || x0 > 1), not with fminf / fmaxf: a NaN x0
does not turn into a finite value there, and it can only see a NaN x0 when this step has already put NaN into the latent.  It
is left as it is.

MEASURED on an MI355X (worst |device - f64| / unit bound over all cases; allowed: 2; beside it the reference's own fp32
evaluation in numpy, test_step_ref_host.py, which must stay <= 1):

  output          mode   device   reference fp32
  pred_xstart     0-3    0.942    0.956
  mean            0-3    0.745    0.922
  variance        0-3    0.760    0.820
  sample          0      0.691    0.869
  sample          1      0.690    0.742
  sample          2      0.931    0.931
  sample          3      0.800    0.800
  guided          0      0.643    0.776
  guided_update   -      0.998    0.998
  axpby           -      0.968    0.981
  drawn noise: within 2e-5 of the construction at every element of every drawn case (A, B, C and the 2 098 188 of D)
  module run time: 3.9 s (19 tests; the slowest, shape D in mode 3, 0.5 s)

Findings:
  1. clip_denoised and NaN.  Before: test_nonfinite_operands[clip] failed -- at the planted NaN the device gave pred_xstart = -1
     and a finite mean / sample / guided (sample 1.3489 where the statement is NaN): fminf(fmaxf(NaN, -1), 1) is -1.  The
     kernel now clamps only when x0 == x0.  After: NaN at those elements of all four outputs, +-inf still clamp to -+1, and the
     module passes.  With the fix taken back exactly that one test fails.  Every finite case of the table (954 cases, 3921
     outputs) has the bits it had before the fix: the fused form of sqrt_recip x - sqrt_recipm1 eps that the compiler had
     chosen is now written out (fmaf), because with the extra compare it chose two roundings instead.
  2. Drawn noise near u0 = 1.  Before: at shape D 2 of 2 098 188 drawn values were 5.5e-5 from the construction formed in exact
     arithmetic (tolerance 2e-5).  The kernel forms u = ((w >> 8) + 0.5) 2^-24 in fp32, where + 0.5 rounds to even from 2^23
     on; 2^-25 in u is visible only where the radius sqrt(-2 log u0) goes to 0.  This is the intended construction: it is now
     stated at the declaration (include/ishap.h) and in step_ref.philox_normals, the tolerance is unchanged.  After: every
     drawn element within 2e-5.
  3. `variance` with variance_in.  The ABI's `variance` output is the learned variance also when variance_in is given (the
     reference's dict returns the caller's tensor, which the Python wrapper puts back).  Intended; stated at the declaration
     and in the statement.  `guided` and `sample` use variance_in, as the reference does (mutants 3 and 4 of the host file).
"""
import ctypes as C
import time
from collections import defaultdict
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ishapediting_amd import _lib
from tests import step_ref as R

pytestmark = pytest.mark.gpu

_WORST = defaultdict(float)          # (output, mode) -> worst ratio to the unit bound seen so far in this run


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).reshape(-1).view(np.int32)


class _In:
    """An input on the device with its host bits kept for the after-call comparison."""

    def __init__(self, a):
        self.host = np.array(a, dtype=np.float32).reshape(-1)
        self.t = torch.from_numpy(self.host.copy()).to(dev())

    @property
    def ptr(self):
        return self.t.data_ptr()

    def assert_untouched(self, tag):
        assert np.array_equal(_bits(self.t.cpu().numpy()), _bits(self.host)), f"{tag}: an input was written"


class _Out:
    """An output of n floats prefilled with the sentinel, 64 sentinel floats behind it."""

    def __init__(self, n):
        self.n = n
        self.t = torch.full((n + 64,), float(R.SENTINEL), dtype=torch.float32, device=dev())

    @property
    def ptr(self):
        return self.t.data_ptr()

    def read(self, tag):
        h = self.t.cpu().numpy()
        assert (_bits(h[self.n:]) == _bits(R.SENTINEL)[0]).all(), f"{tag}: wrote past the end of an output"
        return h[:self.n].copy()

    def assert_sentinel(self, tag):
        assert (_bits(self.t.cpu().numpy()) == _bits(R.SENTINEL)[0]).all(), f"{tag}: an output was written"


@lru_cache(maxsize=64)
def _inputs(shape, resp, t, nonfinite):
    c = R._case(shape, resp, t, 0, True, nonfinite=nonfinite)
    (_, x, mo), _ = R.call_args(c)
    o = R.operands(shape, resp, t)
    return SimpleNamespace(x=_In(x), model_out=_In(mo), noise=_In(o.noise), variance_in=_In(o.variance_in), grad=_In(o.grad),
                           scales=_In(np.array(R.SCALES[shape], np.float32)), gm=_In(np.array([R.GRAD_MUL], np.float32)))


def _call(c, want, noise="case", rng=None):
    """One launch of the case's ABI function with the outputs `want` requested (the others NULL).  noise: "case" = what the
    case says (drawn: NULL), or an _In to inject.  rng: an _Out that takes noise_out (sets k->rng = 1), or None.
    Returns {output: host array}; checks the return code, the sentinels and the inputs."""
    d = _inputs(c.shape, c.resp, c.t, c.nonfinite)
    N, Cn, HW = R.SHAPES[c.shape]
    k = R.coefs(c)
    if noise == "case":
        noise = d.noise if c.noise == "given" else None
    if rng is not None:
        k.rng, k.rng_seed, k.rng_offset, k.noise_out = 1, R.RNG_SEED, R.RNG_OFFSET, rng.ptr
    used = [d.x, d.model_out] + ([noise] if noise is not None else []) + ([d.variance_in] if c.vin else [])
    outs = {name: _Out(N * Cn * HW) for name in want}
    p = lambda name: outs[name].ptr if name in outs else None                      # noqa: E731
    head = (d.x.ptr, d.model_out.ptr, None if noise is None else noise.ptr, d.variance_in.ptr if c.vin else None, C.byref(k), N, Cn, HW)
    L, s = _lib.lib(), _lib.stream_ptr(dev())
    if c.guide:
        used += [d.grad] + ([d.gm] if c.gm else [])
        gm = d.gm.ptr if c.gm else None
        if c.guide == "scales":
            used.append(d.scales)
            rc = L.ishap_ddpm_step_guided_scales(*head, d.grad.ptr, d.scales.ptr, gm, p("guided"), p("sample"), p("variance"), s)
        else:
            rc = L.ishap_ddpm_step_guided(*head, d.grad.ptr, R.SCALAR_SCALE, gm, p("guided"), p("sample"), p("variance"), s)
    else:
        rc = L.ishap_ddpm_step(*head, p("sample"), p("pred_xstart"), p("variance"), p("mean"), s)
    _lib.check(rc)
    torch.cuda.synchronize()
    got = {name: o.read(f"{c.name} {name}") for name, o in outs.items()}
    for i in used:
        i.assert_untouched(c.name)
    return got


def _hold(c, got, drawn=None):
    """Every requested output of a case against the statement; records the worst ratio per (output, mode)."""
    args, kw = R.call_args(c, drawn=drawn)
    ref = R.step(*args, **kw)
    for name, g in got.items():
        r = R.ratio(g, ref[name])
        w = float(r.max())
        _WORST[(name, c.mode)] = max(_WORST[(name, c.mode)], w)
        assert w <= R.FACTOR, (c.name, name, w, int(r.argmax()), float(g[int(r.argmax())]), float(ref[name].v.reshape(-1)[int(r.argmax())]))


def _run(c):
    """A case with all its outputs requested at once.  A drawn case: the reported noise against the construction, the step
    bitwise the step with that noise injected (where the given noise wins over rng = 1 and noise_out is left alone)."""
    want = R.outputs_of(c)
    if c.noise != "drawn":
        got = _call(c, want)
        _hold(c, got)
        return got
    n = int(np.prod(R.SHAPES[c.shape]))
    nz = _Out(n)
    got = _call(c, want, rng=nz)
    noise = nz.read(f"{c.name} noise_out")
    np.testing.assert_allclose(noise, R.drawn_noise64(c.shape), rtol=0, atol=R.NOISE_ATOL, err_msg=c.name)
    untouched = _Out(n)
    again = _call(c, want, noise=_In(noise), rng=untouched)
    untouched.assert_sentinel(f"{c.name} noise_out with noise given")
    for name in want:
        assert np.array_equal(_bits(got[name]), _bits(again[name])), (c.name, name)
    _hold(c, got, drawn=noise.reshape(R.SHAPES[c.shape]))
    return got


def _report(tag, t0):
    rows = "  ".join(f"{k}/m{m} {w:.3f}" for (k, m), w in sorted(_WORST.items(), key=str))
    print(f"{tag}: {time.time() - t0:.2f} s; worst device / unit bound so far: {rows}")


# ------------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_step_against_float64(shape):
    t0, n = time.time(), 0
    for c in R.STEP_CASES:
        if c.shape == shape and not c.nonfinite:
            _run(c)
            n += 1
    assert n >= 7 * 2 * 19
    _report(f"step {shape} ({n} cases)", t0)


@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_guided_step_against_float64(shape):
    """ishap_ddpm_step_guided (scalar scale) and ishap_ddpm_step_guided_scales (per image, 0 among them), grad_mul_dev NULL
    and a device 2^-9, variance_in absent and given: guided, sample and variance all held to the statement -- not to each
    other, as tests/test_gpu_batched_drag.py does bitwise."""
    t0, n = time.time(), 0
    for c in R.GUIDED_CASES:
        if c.shape == shape and not c.nonfinite:
            _run(c)
            n += 1
    assert n >= 3 * 2 * 2 * 2 * 2 + 2
    _report(f"guided {shape} ({n} cases)", t0)


@pytest.mark.parametrize("name", [c.name for c in R.STEP_CASES + R.GUIDED_CASES if c.shape == "D"])
def test_second_grid_pass(name):
    """Shape D: vectors 524 288 .. 524 546 are written by the second trip of the grid-stride loop."""
    t0 = time.time()
    assert int(np.prod(R.SHAPES["D"])) // 4 - R.CAP_VECS == 259
    _run(R.CASES[name])
    _report(name, t0)


@pytest.mark.parametrize("shape", ["A", "B", "C"])
def test_output_pointers(shape):
    """An output has the same bits whichever other outputs were requested; what is not requested is NULL."""
    n = 0
    for c in R.STEP_CASES + R.GUIDED_CASES:
        if c.shape != shape or (c.resp, c.t) != ("40", 20) or c.noise != "given" or c.nonfinite or c.field:
            continue
        full = _call(c, R.outputs_of(c))
        _hold(c, full)
        subsets = [("guided",), ("guided", "sample"), ("guided", "variance")] if c.guide else [(k,) for k in R.outputs_of(c)]
        for want in subsets:
            part = _call(c, want)
            for k in want:
                assert np.array_equal(_bits(part[k]), _bits(full[k])), (c.name, want, k)
        n += 1
    assert n == 2 * 7 + 2 * 2 * 2 * 2


# ------------------------------------------------------------------------------------------------ non-finite operands
@pytest.mark.parametrize("clip", [True, False], ids=["clip", "noclip"])
def test_nonfinite_operands(clip):
    """NaN, +inf and -inf planted in eps at six elements of shape B, x and v finite there.  The reference (x.clamp(-1, 1)):
    NaN in gives NaN out for pred_xstart, mean, sample and guided; +-inf clamp to -+1 under clip and stay infinite (or turn
    NaN in mode 3's inf - inf) without it.  Every other element still meets its bound."""
    cases = [c for c in R.STEP_CASES + R.GUIDED_CASES if c.nonfinite and c.clip == clip]
    assert len(cases) == 3
    for c in cases:
        got = _run(c)
        nan_at = [at for at, val in R.NONFINITE_AT if np.isnan(val)]
        for k in set(got) - {"variance"}:
            assert np.isnan(got[k][nan_at]).all(), (c.name, k, got[k][nan_at])
        assert np.isfinite(got["variance"]).all()


# ------------------------------------------------------------------------------------------------ the two elementwise launches
@pytest.mark.parametrize("shape", ["A", "B", "C", "D"])
def test_guided_update_and_axpby(shape):
    e = R.elementwise_operands(shape)
    n = e.sample.size
    assert n == R.ELEMENTWISE_NUMEL[shape]
    sample, variance, grad, y, gm = _In(e.sample), _In(e.variance), _In(e.grad), _In(e.y), _In(np.array([R.GRAD_MUL], np.float32))
    L, s = _lib.lib(), _lib.stream_ptr(dev())
    for g in (None, gm):
        out = _Out(n)
        _lib.check(L.ishap_guided_update(sample.ptr, variance.ptr, grad.ptr, R.SCALAR_SCALE, None if g is None else g.ptr, n, out.ptr, s))
        torch.cuda.synchronize()
        r = R.ratio(out.read("guided_update"), R.guided_update(e.sample, e.variance, e.grad, R.SCALAR_SCALE, None if g is None else R.GRAD_MUL))
        _WORST[("guided_update", "-")] = max(_WORST[("guided_update", "-")], float(r.max()))
        assert float(r.max()) <= R.FACTOR, (shape, g is not None, float(r.max()), int(r.argmax()))
    for a, b in R.AXPBY_COEFS:
        out = _Out(n)
        _lib.check(L.ishap_axpby(sample.ptr, y.ptr, a, b, n, out.ptr, s))
        torch.cuda.synchronize()
        r = R.ratio(out.read("axpby"), R.axpby(e.sample, e.y, a, b))
        _WORST[("axpby", "-")] = max(_WORST[("axpby", "-")], float(r.max()))
        assert float(r.max()) <= R.FACTOR, (shape, a, b, float(r.max()), int(r.argmax()))
    for i in (sample, variance, grad, y, gm):
        i.assert_untouched(f"elementwise {shape}")
    print(f"{shape}: guided_update {_WORST[('guided_update', '-')]:.3f} axpby {_WORST[('axpby', '-')]:.3f} of the unit bound")


# ------------------------------------------------------------------------------------------------ rejections
def test_rejections():
    """Host-side checks that return before any launch: non-zero, ishap_last_error set, every output's sentinel intact.
    (Mode 1 cannot be told from mode 0 by a bound -- exp(logvar / 2) against sqrt(exp(logvar)) -- so that a guided call
    refuses every mode but 0 is what keeps the two apart.)"""
    L, s = _lib.lib(), _lib.stream_ptr(dev())
    d = _inputs("B", "40", 20, False)
    N, Cn, HW = R.SHAPES["B"]
    outs = [_Out(N * Cn * HW) for _ in range(4)]
    o = [b.ptr for b in outs]
    base = R.CASES["B-40-t20-m0-clip-given"]

    def k_of(mode):
        k = R.coefs(base)
        k.mode = mode
        return k

    def refused(rc, words):
        assert rc != 0, words
        msg = (L.ishap_last_error() or b"").decode()
        assert words in msg, (words, msg)
        torch.cuda.synchronize()
        for b in outs:
            b.assert_sentinel(words)

    x, mo, nz, gr, sc = d.x.ptr, d.model_out.ptr, d.noise.ptr, d.grad.ptr, d.scales.ptr
    refused(L.ishap_ddpm_step(x, mo, nz, None, C.byref(k_of(0)), 1, 1, 6, *o, s), "multiple of 4")
    refused(L.ishap_ddpm_step(x, mo, None, None, C.byref(k_of(2)), N, Cn, HW, *o, s), "mode 2 needs")
    for mode in (-1, 4, 7):
        refused(L.ishap_ddpm_step(x, mo, nz, None, C.byref(k_of(mode)), N, Cn, HW, *o, s), "k->mode >= 0 && k->mode <= 3")
    for mode in (1, 2, 3):
        refused(L.ishap_ddpm_step_guided(x, mo, nz, None, C.byref(k_of(mode)), N, Cn, HW, gr, 50.0, None, *o[:3], s), "k->mode == 0")
        refused(L.ishap_ddpm_step_guided_scales(x, mo, nz, None, C.byref(k_of(mode)), N, Cn, HW, gr, sc, None, *o[:3], s), "k->mode == 0")
    refused(L.ishap_ddpm_step_guided_scales(x, mo, nz, None, C.byref(k_of(0)), N, Cn, HW, gr, None, None, *o[:3], s), "&& scales &&")
    refused(L.ishap_guided_update(x, nz, gr, 50.0, None, 6, o[0], s), "n % 4 == 0")
    refused(L.ishap_axpby(x, nz, 1.0, -1.0, 6, o[0], s), "n % 4 == 0")
    for i in (d.x, d.model_out, d.noise, d.grad, d.scales):
        i.assert_untouched("rejections")
