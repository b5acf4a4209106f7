"""One reverse-diffusion step in float64 with a running fp32 error bound, and the case table of tests/test_gpu_step_oracle.py.

The statement is written from the reference's formulas, not from csrc/ddpm.hip:
  gaussian_diffusion.py:277-279  frac = (v + 1) / 2; log_variance = frac * max_log + (1 - frac) * min_log; variance = exp(.)
  :333-338, :299-300             pred_xstart = sqrt_recip * x - sqrt_recipm1 * eps, then x.clamp(-1, 1) under clip_denoised
  :216-219                       mean = coef1 * pred_xstart + coef2 * x
  :503 / :508                    mode 0: sample = mean + nonzero * sqrt(variance or the caller's `variance=`) * noise
  :443                           mode 1: sample = mean + nonzero * exp(0.5 * log_variance) * noise
  :498-499                       mode 2: sample = mean + variance_noise
  :350-354, :688-705             mode 3: eps' = (sqrt_recip * x - pred_xstart) / sqrt_recipm1;
                                         sample = pred_xstart * sqrt(abar_prev) + sqrt(1 - abar_prev - sigma^2) * eps'
                                                  + nonzero * sigma * noise
  drag_utils.py:385, :392        guided = sample + variance * (scale * grad), grad = grad_raw * grad_mul when a loss scale is undone
  gaussian_diffusion.py:522      axpby: a * x + b * y
The coefficients are the fp32 values of ishap_step_coefs as SpacedDiffusion._coefs builds them; the operands are fp32 values
widened to float64.  NaN and infinities follow torch: clamp keeps NaN, clamp(+-inf) = +-1.

What the C ABI calls `variance` is the LEARNED variance also when variance_in is given (include/ishap.h); the dict's "variance"
of the reference (the caller's own tensor then) is put back by the Python wrapper.  `variance` below is the ABI's.

Every value is a pair (value, bound): a first-order bound of what fp32 evaluation in the reference's operation order can be
off by.  u = 2^-24.  Each fp32 operation adds u |result| and carries its operands' bounds: a + b: e_a + e_b; a b: |a| e_b + |b|
e_a; a / b: (e_a + |a / b| e_b) / (|b| - e_b); clamp: unchanged (1-Lipschitz; exact at an infinite operand); exp: an absolute
bound e becomes the relative expm1(e), plus K_EXP ulp; sqrt: the larger one-sided change, plus K_SQRT ulp.  One ulp is taken as
2^-23 |result|, a whole spacing at the top of a binade.  K_EXP = K_SQRT = 1: the HIP math API reference of the ROCm
documentation ("HIP math API", table of single-precision functions) lists a maximum error of 1 ulp for expf and for sqrtf.

A device value passes when |device - value| <= FACTOR * bound, FACTOR = 2: the factor is the kernel's freedom to contract a
multiply and an add into one FMA (never worse than the two roundings it replaces, but another value) and to associate
scale * (grad * grad_mul) its own way.  It is not tuned to the device.
"""
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from tests.helpers import philox4x32_10

U = 2.0 ** -24
ULP = 2.0 ** -23
K_EXP = 1
K_SQRT = 1
FACTOR = 2.0
CAP_VECS = 2048 * 256            # float4 vectors one grid pass of the three kernels covers
SENTINEL = np.float32(-1.2345e33)
RNG_SEED = 0xC0FFEE123456789B    # bits above 2^32 in the seed ...
RNG_OFFSET = (3 << 32) + 8       # ... and in the offset


# ------------------------------------------------------------------------------------------------ value with bound
class V:
    """float64 value `v` with the bound `e` of its fp32 evaluation."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else e

    @staticmethod
    def of(a):
        return a if isinstance(a, V) else V(a)

    def _done(self, r, e):
        return V(r, e + U * np.abs(r))

    def __add__(self, o):
        o = V.of(o)
        return self._done(self.v + o.v, self.e + o.e)
    __radd__ = __add__

    def __sub__(self, o):
        o = V.of(o)
        return self._done(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        # 0 * inf is kept out of the bound (a bound of 0 times an infinite value is 0)
        ea = np.where(o.e == 0, 0.0, np.abs(self.v) * o.e)
        eb = np.where(self.e == 0, 0.0, np.abs(o.v) * self.e)
        return self._done(self.v * o.v, ea + eb)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        r = self.v / o.v
        return self._done(r, (self.e + np.where(o.e == 0, 0.0, np.abs(r) * o.e)) / (np.abs(o.v) - o.e))


def _exp(a):
    if not isinstance(a, V):
        return np.exp(a)
    r = np.exp(a.v)
    return V(r, r * np.expm1(a.e) + K_EXP * ULP * r)


def _sqrt(a):
    if not isinstance(a, V):
        return np.sqrt(a)
    r = np.sqrt(a.v)
    up = np.sqrt(a.v + a.e) - r
    down = r - np.sqrt(np.maximum(a.v - a.e, 0.0))
    return V(r, np.maximum(up, down) + K_SQRT * ULP * r)


def _clamp(a):
    """torch's x.clamp(-1, 1): NaN stays NaN (np.clip keeps it as well), +-inf become +-1."""
    if not isinstance(a, V):
        return np.clip(a, a.dtype.type(-1), a.dtype.type(1))
    return V(np.clip(a.v, -1.0, 1.0), np.where(np.isinf(a.v), 0.0, a.e))


# ------------------------------------------------------------------------------------------------ the statement
MUTANTS = ("v_from_eps", "image_stride", "vin_ignored_in_guided", "vin_ignored_in_sample", "nonzero_ignored", "clip_dropped",
           "ddim_eps_unclipped", "grad_mul_dropped", "scale_of_image0", "coef1_coef2_swapped", "min_max_log_swapped",
           "second_pass_unwritten", "noise_index_per_image", "rng_offset_high_dropped")


def _formulas(k, x, eps, v, nz, vin, grad, scale, gm, mutant):
    """The step on operands of one number type: V (float64 with bounds) or numpy float32 arrays.  `k`: the coefficients as
    Python floats (exact fp32 values); `scale`: None, or an array broadcastable against x."""
    min_log, max_log, coef1, coef2, nonzero = k.min_log, k.max_log, k.coef1, k.coef2, k.nonzero
    clip = bool(k.clip_denoised)
    if mutant == "coef1_coef2_swapped":
        coef1, coef2 = coef2, coef1
    if mutant == "min_max_log_swapped":
        min_log, max_log = max_log, min_log
    if mutant == "nonzero_ignored":
        nonzero = 1.0
    if mutant == "clip_dropped":
        clip = False
    frac = (v + 1.0) / 2.0
    logvar = frac * max_log + (1.0 - frac) * min_log
    var = _exp(logvar)
    x0u = k.sqrt_recip * x - k.sqrt_recipm1 * eps
    x0 = _clamp(x0u) if clip else x0u
    mean = coef1 * x0 + coef2 * x
    used = var if vin is None else vin
    if k.mode == 0:
        sample = mean + nonzero * _sqrt(var if mutant == "vin_ignored_in_sample" else used) * nz
    elif k.mode == 1:
        sample = mean + nonzero * _exp(0.5 * logvar) * nz
    elif k.mode == 2:
        sample = mean + nz
    elif k.mode == 3:
        eps2 = (k.sqrt_recip * x - (x0u if mutant == "ddim_eps_unclipped" else x0)) / k.sqrt_recipm1
        sample = (x0 * k.ddim_a + k.ddim_b * eps2) + nonzero * k.ddim_sigma * nz
    else:
        raise ValueError(k.mode)
    out = {"sample": sample, "pred_xstart": x0, "variance": var, "mean": mean, "x0_unclipped": x0u}
    if grad is not None:
        g = grad if (gm is None or mutant == "grad_mul_dropped") else grad * gm
        out["guided"] = sample + (var if mutant == "vin_ignored_in_guided" else used) * (scale * g)
    return out


def _coef_ns(k):
    return SimpleNamespace(**{f: getattr(k, f) for f in ("min_log", "max_log", "sqrt_recip", "sqrt_recipm1", "coef1", "coef2", "nonzero",
                                                       "clip_denoised", "mode", "ddim_a", "ddim_b", "ddim_sigma")})


def _operands(x, model_out, noise, variance_in, grad, scale, mutant, wrap):
    """Split model_out [N][2C][HW] into eps | v and give every operand the shape of x.  `wrap` lifts an fp32 array."""
    x = np.asarray(x, np.float32)
    N, C, HW = x.shape
    mo = np.asarray(model_out, np.float32).reshape(N, 2 * C, HW)
    eps, v = mo[:, :C], mo[:, C:]
    if mutant == "v_from_eps":
        v = eps
    if mutant == "image_stride":
        flat, per = mo.reshape(-1), C * HW
        eps = np.stack([flat[n * per:n * per + per] for n in range(N)]).reshape(N, C, HW)
        v = np.stack([flat[n * per + per:n * per + 2 * per] for n in range(N)]).reshape(N, C, HW)
    nz = np.zeros_like(x) if noise is None else np.asarray(noise, np.float32).reshape(x.shape)
    sc = None
    if grad is not None:
        sc = np.asarray(scale, np.float32).reshape(-1)
        assert sc.size in (1, N)
        if mutant == "scale_of_image0":
            sc = sc[:1]
        sc = wrap(np.broadcast_to(sc.reshape(-1, 1, 1), (N, 1, 1)))
    opt = lambda a: None if a is None else wrap(np.asarray(a, np.float32).reshape(x.shape))    # noqa: E731
    return wrap(x), wrap(eps), wrap(v), wrap(nz), opt(variance_in), opt(grad), sc


def step(k, x, model_out, noise=None, variance_in=None, grad=None, scale=None, grad_mul=None, mutant=None):
    """The float64 statement: dict of V for sample, pred_xstart, variance, mean (and guided when `grad` is given; x0_unclipped
    for the conditions on the inputs).  x [N][C][HW], model_out [N][2C][HW]; scale a number or N numbers."""
    with np.errstate(all="ignore"):
        ops = _operands(x, model_out, noise, variance_in, grad, scale, mutant, lambda a: V(a.astype(np.float64)))
        gm = None if grad_mul is None else float(np.float32(grad_mul))
        return _formulas(_coef_ns(k), *ops, gm, mutant)


def step32(k, x, model_out, noise=None, variance_in=None, grad=None, scale=None, grad_mul=None):
    """The same operations in the same order in numpy float32: the reference's own precision."""
    with np.errstate(all="ignore"):
        ops = _operands(x, model_out, noise, variance_in, grad, scale, None, lambda a: np.ascontiguousarray(a, np.float32))
        kk = _coef_ns(k)
        for f in ("min_log", "max_log", "sqrt_recip", "sqrt_recipm1", "coef1", "coef2", "nonzero", "ddim_a", "ddim_b", "ddim_sigma"):
            setattr(kk, f, np.float32(getattr(kk, f)))
        out = _formulas(kk, *ops, None if grad_mul is None else np.float32(grad_mul), None)
    assert all(o.dtype == np.float32 for o in out.values())
    return out


def guided_update(sample, variance, grad, scale, grad_mul=None):
    """drag_utils.py:385, :392 on its own: sample + variance * (scale * grad [* grad_mul])."""
    with np.errstate(all="ignore"):
        s, va, g = (V(np.asarray(a, np.float32).astype(np.float64)) for a in (sample, variance, grad))
        if grad_mul is not None:
            g = g * float(np.float32(grad_mul))
        return s + va * (float(np.float32(scale)) * g)


def guided_update32(sample, variance, grad, scale, grad_mul=None):
    s, va, g = (np.asarray(a, np.float32) for a in (sample, variance, grad))
    if grad_mul is not None:
        g = g * np.float32(grad_mul)
    return s + va * (np.float32(scale) * g)


def axpby(x, y, a, b):
    """gaussian_diffusion.py:522: a * x + b * y."""
    with np.errstate(all="ignore"):
        xv, yv = (V(np.asarray(t, np.float32).astype(np.float64)) for t in (x, y))
        return float(np.float32(a)) * xv + float(np.float32(b)) * yv


def axpby32(x, y, a, b):
    return np.float32(a) * np.asarray(x, np.float32) + np.float32(b) * np.asarray(y, np.float32)


def ratio(got, ref):
    """|got - value| / bound per element (the UNIT bound: a device value passes at <= FACTOR, the reference alone must stay
    <= 0.5 FACTOR).  Equal values give 0 whatever the bound; where the statement is NaN the value must be NaN, where it is
    infinite the value must be that infinity (ratio inf otherwise)."""
    got = np.asarray(got, np.float64).reshape(ref.v.shape)
    with np.errstate(all="ignore"):
        r = np.abs(got - ref.v) / ref.e
    same = (got == ref.v) | (np.isnan(got) & np.isnan(ref.v))
    r = np.where(same, 0.0, r)
    return np.where(np.isnan(r), np.inf, r)


# ------------------------------------------------------------------------------------------------ in-kernel noise
def philox_normals(nvec, seed, offset, mutant=None, vecs_per_image=None, exact_u=False):
    """include/ishap.h, ishap_step_coefs::rng, in float64: element 4 i + j takes normal j of vector i.  The uniforms are the
    fp32 numbers the declaration states: (w >> 8) + 0.5 needs 25 bits from 2^23 on and rounds to even there, which moves u by
    2^-25 at most.  That is far below the tolerance everywhere but at u0 -> 1, where the radius sqrt(-2 log u0) goes to 0 like
    sqrt(2 (1 - u0)): a pair with 1 - u0 < 1e-6 (one in a million; shape D has one) is 5e-5 off the exactly formed value.
    `exact_u` forms u without that rounding (what tests/test_gpu_parity.py compares with at its small shape)."""
    vec = np.arange(nvec, dtype=np.uint64)
    if mutant == "noise_index_per_image":
        vec = vec % np.uint64(vecs_per_image)
    if mutant == "rng_offset_high_dropped":
        offset &= 0xFFFFFFFF
    key = (seed ^ 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
    M = np.uint64(0xFFFFFFFF)
    w = philox4x32_10([vec & M, vec >> np.uint64(32), np.full(nvec, offset & 0xFFFFFFFF, np.uint64), np.full(nvec, offset >> 32, np.uint64)],
                      (key & 0xFFFFFFFF, key >> 32))
    u = [(t >> 8).astype(np.float64) + 0.5 for t in w]
    if not exact_u:
        u = [t.astype(np.float32).astype(np.float64) for t in u]
    u = [t * 2.0 ** -24 for t in u]
    out = np.empty((nvec, 4))
    for h in range(2):
        rad = np.sqrt(-2.0 * np.log(u[2 * h]))
        out[:, 2 * h] = rad * np.cos(2 * np.pi * u[2 * h + 1])
        out[:, 2 * h + 1] = rad * np.sin(2 * np.pi * u[2 * h + 1])
    return out.reshape(-1)


@lru_cache(maxsize=None)
def drawn_noise64(shape):
    """The noise a drawn case of this shape must report (float64), read-only."""
    N, C, HW = SHAPES[shape]
    a = philox_normals(N * C * HW // 4, RNG_SEED, RNG_OFFSET)
    a.setflags(write=False)
    return a


NOISE_ATOL = 2e-5      # fp32 log / sin / cos of the Box-Muller pair (tests/test_gpu_parity.py::test_step_draws_its_own_noise)


# ------------------------------------------------------------------------------------------------ cases
SHAPES = {"A": (1, 1, 4),           # one vector, one lane
          "B": (2, 3, 36),          # 54 vectors, the image boundary (vector 27) inside a wave
          "C": (3, 6, 256),         # the batched shape of test_gpu_batched_drag.py
          "D": (3, 4, 174849)}      # 524 547 vectors: 259 beyond one grid pass, all in the last image
TIMES = (("40", 0), ("40", 1), ("40", 20), ("40", 39), ("1000", 999), ("ddim8", 0), ("ddim8", 7))
SCALAR_SCALE = 50.0
SCALES = {"A": (1200.0,), "B": (0.0, 50.0), "C": (0.0, 50.0, 1200.0), "D": (50.0, 0.0, 1200.0)}
GRAD_MUL = 2.0 ** -9
AXPBY_COEFS = ((1.0, -1.0), (0.8125, -0.37))     # the inversion's exact +-1 (gaussian_diffusion.py:527-529) and a rounding pair
NONFINITE_AT = ((3, np.nan), (40, np.inf), (77, -np.inf), (110, np.nan), (150, np.inf), (215, -np.inf))   # flat in eps of B

Case = namedtuple("Case", "name shape resp t mode clip eta vin noise guide gm field nonfinite")


def _case(shape, resp, t, mode, clip, eta=0.0, vin=False, noise="given", guide=None, gm=False, field=None, nonfinite=False):
    name = f"{shape}-{resp}-t{t}-m{mode}{'-clip' if clip else ''}"
    if mode == 3:
        name += f"-eta{eta:g}"
    name += ("-vin" if vin else "") + f"-{noise}" + (f"-{guide}" if guide else "") + ("-gm" if gm else "")
    name += (f"-{field}" if field else "") + ("-nonfinite" if nonfinite else "")
    return Case(name, shape, resp, t, mode, bool(clip), float(eta), vin, noise, guide, gm, field, nonfinite)


def _build_cases():
    step_cases, guided_cases = [], []
    for shape in "ABC":
        for resp, t in TIMES:
            for clip in (True, False):
                for noise in ("given", "null", "drawn"):
                    for vin in (False, True):
                        step_cases.append(_case(shape, resp, t, 0, clip, vin=vin, noise=noise))
                    step_cases.append(_case(shape, resp, t, 1, clip, noise=noise))
                    for eta in (0.0, 0.5, 1.0):
                        step_cases.append(_case(shape, resp, t, 3, clip, eta=eta, noise=noise))
                step_cases.append(_case(shape, resp, t, 2, clip))
        for resp, t in (("40", 0), ("40", 20), ("1000", 999)):
            for clip in (True, False):
                for vin in (False, True):
                    for guide in ("scalar", "scales"):
                        for gm in (False, True):
                            guided_cases.append(_case(shape, resp, t, 0, clip, vin=vin, guide=guide, gm=gm))
        guided_cases.append(_case(shape, "40", 20, 0, True, vin=True, noise="drawn", guide="scales", gm=True))
        guided_cases.append(_case(shape, "40", 20, 0, True, noise="null", guide="scalar"))
    # the `nonzero` FIELD of the coefficients, away from t = 0: at t = 0 the reference's sigma is 0 (abar_prev = 1), so mode 3
    # cannot show there whether the field is honoured
    for mode in (0, 1, 3):
        step_cases.append(_case("B", "40", 20, mode, True, eta=1.0 if mode == 3 else 0.0, field="nonzero0"))
    for clip in (True, False):
        for mode in (0, 3):
            step_cases.append(_case("B", "40", 20, mode, clip, eta=0.5 if mode == 3 else 0.0, nonfinite=True))
        guided_cases.append(_case("B", "40", 20, 0, clip, guide="scalar", gm=True, nonfinite=True))
    step_cases.append(_case("D", "40", 20, 3, True, eta=0.5))
    step_cases.append(_case("D", "40", 20, 0, True, noise="drawn"))
    guided_cases.append(_case("D", "40", 20, 0, True, vin=True, guide="scales", gm=True))
    return tuple(step_cases), tuple(guided_cases)


STEP_CASES, GUIDED_CASES = _build_cases()
CASES = {c.name: c for c in STEP_CASES + GUIDED_CASES}
assert len(CASES) == len(STEP_CASES) + len(GUIDED_CASES)
ELEMENTWISE_NUMEL = {s: int(np.prod(SHAPES[s])) for s in "ABCD"}      # guided_update and axpby: the same element counts


@lru_cache(maxsize=None)
def diffusion(resp):
    from ishapediting_amd.gaussian_diffusion import create_gaussian_diffusion
    return create_gaussian_diffusion(timestep_respacing=resp)


def coefs(c):
    k = diffusion(c.resp)._coefs(c.t, c.clip, c.mode, c.eta)
    if c.field == "nonzero0":
        k.nonzero = 0.0
    assert all(np.isfinite(getattr(k, f)) for f in ("min_log", "max_log", "sqrt_recip", "sqrt_recipm1", "coef1", "coef2", "ddim_a",
                                                    "ddim_b", "ddim_sigma")), c.name
    return k


@lru_cache(maxsize=64)
def operands(shape, resp, t):
    """fp32 operands of one (shape, timestep), read-only.  x is a noised x0 of this timestep, x = sqrt(abar) x0 + sqrt(1 - abar)
    eps with x0 = 0.9 N(0, 1): the step's unclipped pred_xstart then falls outside [-1, 1] for about a quarter of the elements at
    EVERY t (standard-normal x and eps would put nearly all of them outside at large t), and sqrt_recip x - sqrt_recipm1 eps
    cancels as it does on the path.  v = 1.5 N(0, 1) takes frac out of [0, 1]; variance_in >= 0 with exact zeros."""
    N, C, HW = SHAPES[shape]
    r = np.random.default_rng([ord(shape), int(t), sum(map(ord, resp))])
    ab = diffusion(resp).alphas_cumprod[t]
    x0 = 0.9 * r.standard_normal((N, C, HW))
    if shape == "A":
        x0 = np.array([0.3, -1.7, 1.4, -0.6]).reshape(1, 1, 4)
    eps = r.standard_normal((N, C, HW))
    o = SimpleNamespace()
    o.x = (np.sqrt(ab) * x0 + np.sqrt(1 - ab) * eps).astype(np.float32)
    o.model_out = np.concatenate([eps, 1.5 * r.standard_normal((N, C, HW))], axis=1).astype(np.float32)
    o.noise = r.standard_normal((N, C, HW)).astype(np.float32)
    vin = np.abs(0.05 * r.standard_normal(N * C * HW))
    vin[::7] = 0.0
    o.variance_in = vin.reshape(N, C, HW).astype(np.float32)
    o.grad = (0.5 * r.standard_normal((N, C, HW))).astype(np.float32)
    o.drawn = drawn_noise64(shape).astype(np.float32).reshape(N, C, HW)
    for a in vars(o).values():
        a.setflags(write=False)
    return o


def call_args(c, drawn=None):
    """The arguments of step() / step32() for a case; `drawn`: the noise to use for a drawn case (default: the host's own
    construction rounded to fp32; the device test passes what the kernel reported)."""
    o = operands(c.shape, c.resp, c.t)
    mo = o.model_out
    if c.nonfinite:
        mo = mo.copy()
        C_, HW = SHAPES[c.shape][1:]
        for at, val in NONFINITE_AT:
            n, rem = divmod(at, C_ * HW)
            mo[n].reshape(-1)[rem] = val              # the eps half of image n
        mo.setflags(write=False)
    noise = {"given": o.noise, "null": None, "drawn": o.drawn if drawn is None else drawn}[c.noise]
    kw = dict(noise=noise, variance_in=o.variance_in if c.vin else None)
    if c.guide:
        kw.update(grad=o.grad, scale=SCALAR_SCALE if c.guide == "scalar" else np.array(SCALES[c.shape], np.float32),
                  grad_mul=GRAD_MUL if c.gm else None)
    return (coefs(c), o.x, mo), kw


def outputs_of(c):
    return ("guided", "sample", "variance") if c.guide else ("sample", "pred_xstart", "variance", "mean")


def elementwise_operands(shape):
    """Operands of the guided_update and axpby checks at the element count of a shape (flat)."""
    o = operands(shape, "40", 20)
    return SimpleNamespace(sample=o.x.reshape(-1), variance=o.variance_in.reshape(-1), grad=o.grad.reshape(-1), y=o.noise.reshape(-1))
