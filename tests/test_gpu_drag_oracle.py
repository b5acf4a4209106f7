"""The drag loss kernels (csrc/drag.hip) through DragKernels / BatchDragKernels against the float64 oracle of tests/drag_ref.py,
at every branch of the motion scatter: the tail segment, a second channel chunk with dead lanes, the carry and the jump of the
per-column register merge, every zero-padding situation, gather maps with skipped / repeated channels, overlapping footprints,
small magnitudes against the fixed-point quanta, the product's own shape, and a batch.  The case table and the conditions its
inputs must meet are in tests/drag_ref.py and tests/test_drag_ref_host.py.

Bounds (none is tuned to what the device gives):
  gradient  err(x) = max|x - g64| / max|g64| over the whole tap;  err_dev <= 8 * err_ref + q, err_ref the same metric of the
            reference's own float32 autograd on the same inputs (computed here, every run), q = 4 B side^2 * 2^-45 / max|g64|
            the fixed-point term (one add of a value rounded to 2^-44 per position at most, four (plane, channel) pairs per tap
            channel at most).  The 8 covers another summation order and fp32 weights from coordinates one ulp apart.
  L1        the same, without the tap elements in the 2x2 target footprint of a sample with 0 < |d64| < 1e-5 max|feature|.
  loss      |loss_dev - loss64| <= 8 |loss32 - loss64| + nblk 2^-25 / ntot + cof nblk_gather 2^-25 / (Cc nmask): every
            workgroup adds one partial sum rounded to 2^-24.
"""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import drag_ref as R

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _ids(combo):
    return f"{combo[0]}-{combo[1]}-cof{combo[2]}"


@lru_cache(maxsize=None)
def _device(name, loss_type, cof):
    """One solo run of a case (two calls on the same buffers), everything the tests look at copied to the host."""
    from ishapediting_amd.drag_utils import DragKernels
    c = R.make_case(name)
    dk = DragKernels(dev(), W=c.W, ld=c.ld, chmap=c.chmap, r=c.r, voxel=c.voxel, loss_type=loss_type)
    dk.setup(c.sources, c.targets, cof)
    e_d, o_d = c.edit.to(dev()).contiguous(), c.orig.to(dev()).contiguous()
    grad, loss = dk.loss_grad(e_d, o_d)
    torch.cuda.synchronize()
    out = SimpleNamespace(grad=grad.cpu().clone(), loss=float(loss.cpu()), touched=dk.touched.cpu().reshape(3, c.W, c.W).clone(),
                          nmask=int(dk.nmask.cpu()), scratch_max=max(int(dk.gfx.abs().max()), int(dk.acc.abs().max())))
    grad, loss = dk.loss_grad(e_d, o_d)
    torch.cuda.synchronize()
    out.again = bool(torch.equal(grad.cpu(), out.grad)) and float(loss.cpu()) == out.loss
    out.scratch_max = max(out.scratch_max, int(dk.gfx.abs().max()), int(dk.acc.abs().max()))
    return out


def _check_gradient(tag, got, res, ref32_grad, loss_type, B, side, ambiguous, l2_grad=None):
    """Assertions 1-3 on one edit: the gradient bound (L1: without the ambiguous elements) and the structural zeros.
    Structural: padding channels, channels absent from the map, texels outside every footprint and, with the mask term, inside
    the touched set -- the places where g64 == 0.  Under L1 a tap element's terms are +-weight * const, the weights are exact
    in float64 (products of float32 coordinates), and they can cancel to an exact 0 INSIDE a footprint (case B has two such
    elements; the float32 reference leaves 2^-44 there).  Those are no structural zeros: for an L1 run the set is where the
    L2 oracle of the same inputs (`l2_grad`) is 0 as well.  The error bound above covers the cancelled elements."""
    g64 = res.grad
    keep = torch.ones_like(g64, dtype=torch.bool) if ambiguous is None else ~ambiguous
    gmax = float(g64.abs().max())
    err_dev = float((got.double() - g64)[keep].abs().max()) / gmax
    err_ref = float((ref32_grad.double() - g64)[keep].abs().max()) / gmax
    q = 4 * B * side * side * 2.0 ** -45 / gmax
    print(f"{tag}: gradient err_ref {err_ref:.2e} err_dev {err_dev:.2e} q {q:.1e} max|g64| {gmax:.2e} excluded {int((~keep).sum())}")
    assert err_ref > 0
    assert err_dev <= 8 * err_ref + q, (tag, err_dev, err_ref, q)
    zero = g64 == 0
    if loss_type == "l1":
        print(f"{tag}: {int((zero & (l2_grad != 0)).sum())} element(s) cancel to 0 under L1 inside a footprint")
        zero = zero & (l2_grad == 0)
    assert int(zero.sum()) > 0 and bool((got[zero] == 0.0).all()), (tag, int((got[zero] != 0).sum()))


def _check_loss(tag, got, l64, l32, cof, B, r, Cc, W, ld, nmask):
    side = 2 * r + 1
    ntot = 3 * Cc * B * side ** 3
    bound = 8 * abs(l32 - l64) + R.terms_blocks(B, r, Cc) * 2.0 ** -25 / ntot
    if cof > 0:
        bound += cof * R.gather_blocks(W, ld) * 2.0 ** -25 / (Cc * nmask)
    print(f"{tag}: loss64 {l64:.6e} |dev - 64| {abs(got - l64):.2e} (rel {abs(got - l64) / abs(l64):.1e}) |ref32 - 64| "
          f"{abs(l32 - l64):.2e} bound {bound:.2e}")
    assert abs(got - l64) <= bound, (tag, got, l64, l32, bound)


# ------------------------------------------------------------------------------------------------ 1-3. gradient
@pytest.mark.parametrize("combo", R.COMBOS, ids=_ids)
def test_gradient_against_float64(combo):
    name, lt, cof = combo
    c, res, got = R.make_case(name), R.oracle(*combo), _device(*combo)
    amb = R.l1_ambiguous_elements(res, c.edit, c.orig, c.chmap, c.W) if lt == "l1" else None
    _check_gradient(_ids(combo), got.grad, res, R.reference32(*combo)[1], lt, c.B, c.side, amb, R.oracle(name, "l2", cof).grad)
    if name in ("G", "H"):            # channels absent from the map: exactly 0, mask term or not
        unused = np.ones(c.ld, bool)
        unused[c.chmap.reshape(-1)] = False
        assert unused.sum() > 0 and float(got.grad[:, unused].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 4. loss
@pytest.mark.parametrize("combo", R.COMBOS, ids=_ids)
def test_loss_against_float64(combo):
    """E-l1-cof0.4 is the sharp one: the float32 reference lands 2.2e-9 from loss64 there, so the bound (1.7e-8) is under half a
    unit in the last place of a float32 of that size and only the correctly rounded float passes.  With texel coordinates in
    float the device was 1.8e-7 off; with bilin_setup in double and the sums rounded once it is 2.2e-9 off."""
    name, lt, cof = combo
    c, res, got = R.make_case(name), R.oracle(*combo), _device(*combo)
    _check_loss(_ids(combo), got.loss, res.loss, R.reference32(*combo)[0], cof, c.B, c.r, c.Cc, c.W, c.ld, res.nmask)


# ------------------------------------------------------------------------------------------------ 5-6. mask sets, footprint, scratch
@pytest.mark.parametrize("combo", R.COMBOS, ids=_ids)
def test_mask_sets_footprint_and_scratch(combo):
    name, lt, cof = combo
    c, res, got = R.make_case(name), R.oracle(*combo), _device(*combo)
    for p in range(3):
        assert torch.equal((got.touched[p] & 1) == 0, res.setup.masks[p]), (name, p)
    assert got.nmask == res.nmask
    assert got.scratch_max == 0             # gfx and acc left zero by both calls
    assert got.again                        # the second call on the same buffers: the same bits
    # the gather reads the scatter buffer only under bit 1: every element the motion term reaches must lie under it
    motion = R.oracle(name, lt, 0.0).grad
    reached = (motion != 0).any(dim=1)
    marked = ((got.touched & 2) != 0).any(dim=0).reshape(-1)
    assert int(reached.sum()) > 0
    assert bool(marked[reached].all()), (name, int((reached & ~marked).sum()))


# ------------------------------------------------------------------------------------------------ 7. zero displacement
@pytest.mark.parametrize("loss_type", ["l2", "l1"])
@pytest.mark.parametrize("cof", [0.0, 0.4])
def test_zero_displacement_gives_exactly_zero(loss_type, cof):
    """Case I with edit == orig and every target on its source: shift and patch are the same fused multiply-adds of the same
    weights, so the loss is 0.0 and the gradient all zeros -- not merely small."""
    from ishapediting_amd.drag_utils import DragKernels
    c = R.make_case("I")
    dk = DragKernels(dev(), W=c.W, ld=c.ld, chmap=c.chmap, r=c.r, voxel=c.voxel, loss_type=loss_type)
    dk.setup(c.sources, c.sources.copy(), cof)
    e_d = c.edit.to(dev()).contiguous()
    o_d = e_d.clone()
    grad, loss = dk.loss_grad(e_d, o_d)
    torch.cuda.synchronize()
    assert float(loss.cpu()) == 0.0
    assert int((grad != 0).sum()) == 0
    assert int((dk.touched & 2).sum()) > 0 and int(dk.gfx.abs().max()) == 0


# ------------------------------------------------------------------------------------------------ L. a batch, each edit against the oracle
def _carve(bk, E, W, ld):
    """gfx, acc, nmask and touched inside the batch scratch (the carve rule of ishap_drag_batch_scratch_bytes: every part on a
    256-byte boundary)."""
    up = lambda v: (v + 255) // 256 * 256      # noqa: E731
    n_gfx = E * W * W * ld * 8
    o_acc = up(n_gfx)
    o_nmask = up(o_acc + 16 * E)
    o_touched = up(o_nmask + 4 * E)
    s = bk.scratch
    return (s[:n_gfx], s[o_acc:o_acc + 16 * E], s[o_nmask:o_nmask + 4 * E].view(torch.int32),
            s[o_touched:o_touched + E * 3 * W * W].reshape(E, 3, W, W))


@pytest.mark.parametrize("loss_type", ["l2", "l1"])
@pytest.mark.parametrize("shared", [False, True], ids=["stride", "shared"])
def test_every_edit_of_a_batch_against_float64(loss_type, shared):
    from ishapediting_amd.drag_utils import BatchDragKernels
    L = R.make_batch()
    bk = BatchDragKernels(dev(), L.E, W=L.W, ld=L.ld, chmap=L.chmap, r=L.r, voxel=L.voxel, loss_type=loss_type)
    bk.setup(L.sources, L.targets, list(L.cofs))
    e_d = L.edits.to(dev()).contiguous()
    o_d = (L.origs[:1] if shared else L.origs).to(dev()).contiguous()
    grad, loss = bk.loss_grad_ptr(e_d.data_ptr(), o_d.data_ptr(), 0 if shared else L.W * L.W * L.ld)
    torch.cuda.synchronize()
    grad, loss = grad.cpu().clone(), loss.cpu().clone()
    gfx, acc, nmask, touched = _carve(bk, L.E, L.W, L.ld)
    assert int(gfx.max()) == 0 and int(acc.max()) == 0
    nmask, touched = nmask.cpu(), touched.cpu()
    for e, (res, (l32, g32)) in enumerate(R.oracle_batch(loss_type, shared)):
        tag = f"L[{e}]-{loss_type}-{'shared' if shared else 'stride'}"
        B = len(L.sources[e])
        orig = L.origs[0 if shared else e]
        amb = R.l1_ambiguous_elements(res, L.edits[e], orig, L.chmap, L.W) if loss_type == "l1" else None
        _check_gradient(tag, grad[e], res, g32, loss_type, B, L.side, amb, R.oracle_batch("l2", shared)[e][0].grad)
        _check_loss(tag, float(loss[e]), res.loss, l32, L.cofs[e], B, L.r, L.Cc, L.W, L.ld, res.nmask)
        for p in range(3):
            assert torch.equal((touched[e, p] & 1) == 0, res.setup.masks[p]), (tag, p)
        assert int(nmask[e]) == res.nmask


# ------------------------------------------------------------------------------------------------ loss scale and cotangent
def _sweep():
    ks = list(range(-120, 41, 8))
    return [0.0, float("inf"), float("nan")] + [2.0 ** k for k in ks] + [1.5 * 2.0 ** k for k in ks]


def test_loss_scale_is_a_power_of_two_over_the_whole_range():
    """ishap_grad_to_scaled_f16 on a buffer that is zero except one element m, m swept over 2^k and 1.5 * 2^k, k = -120..40, and
    0 / inf / nan."""
    from ishapediting_amd.drag_utils import DragKernels
    c = R.make_case("A")
    dk = DragKernels(dev(), W=c.W, ld=c.ld, chmap=c.chmap, r=c.r, voxel=c.voxel)
    n = dk.grad.numel()
    bad = []
    for i, m in enumerate(_sweep()):
        host = np.zeros(n, np.float32)
        host[(n - 1, 0, n // 2 + 1)[i % 3]] = -m if i % 2 else m          # the sign and the place must not matter
        dk.grad.copy_(torch.from_numpy(host).reshape(dk.grad.shape))
        cot, scale2 = dk.scaled_cotangent()
        torch.cuda.synchronize()
        sc, inv = (float(v) for v in scale2.cpu())
        mant, _ = np.frexp(sc)
        want = float(R.pick_scale_ref(m))
        line = f"m {m:.4e}: scale {sc:.4e} (reference {want:.4e}) m * scale {m * sc if np.isfinite(m) else m}"
        print(line)
        ok = mant == 0.5 and inv == 1.0 / sc
        if not (m > 0 and np.isfinite(m)):
            ok = ok and sc == 1.0
        elif 2.0 ** -19 <= want <= 2.0 ** 98:                             # inside the unclamped range
            ok = ok and 64.0 <= m * sc <= 256.0                           # safe against fp16 overflow; no bit pattern claimed
        else:
            ok = ok and sc in (2.0 ** -20, 2.0 ** 99)
        if np.isfinite(m):
            ok = ok and np.array_equal(cot.cpu().numpy().reshape(-1).view(np.uint16), R.scaled_f16_ref(host, sc).view(np.uint16))
        if not ok:
            bad.append(line)
    assert not bad, bad


def test_cotangent_is_the_round_to_nearest_even_fp16_of_the_scaled_gradient():
    """A random buffer with magnitudes over thirty octaves (fp16 subnormals and zeros at the low end), and case A through the fused
    loss + cotangent call."""
    from ishapediting_amd.drag_utils import DragKernels
    c = R.make_case("A")
    dk = DragKernels(dev(), W=c.W, ld=c.ld, chmap=c.chmap, r=c.r, voxel=c.voxel)
    gen = torch.Generator().manual_seed(7)
    host = (torch.randn(dk.grad.shape, generator=gen) * torch.exp2(-30 * torch.rand(dk.grad.shape, generator=gen)) * 3e-5).numpy()
    dk.grad.copy_(torch.from_numpy(host))
    cot, scale2 = dk.scaled_cotangent()
    torch.cuda.synchronize()
    sc = float(scale2[0])
    assert sc == float(R.pick_scale_ref(np.abs(host).max())) or 64.0 <= float(np.abs(host).max()) * sc <= 256.0
    want = R.scaled_f16_ref(host, sc)
    assert int((want == 0).sum()) > 0 and int((np.abs(want) < 2.0 ** -14).sum()) > int((want == 0).sum())    # subnormals occur
    assert np.array_equal(cot.cpu().numpy().view(np.uint16), want.view(np.uint16))
    for lt, cof in (("l2", 0.4), ("l1", 0.0)):
        dk = DragKernels(dev(), W=c.W, ld=c.ld, chmap=c.chmap, r=c.r, voxel=c.voxel, loss_type=lt)
        dk.setup(c.sources, c.targets, cof)
        e_d, o_d = c.edit.to(dev()).contiguous(), c.orig.to(dev()).contiguous()
        cot, scale2 = dk.loss_cotangent_ptr(e_d.data_ptr(), o_d.data_ptr())
        torch.cuda.synchronize()
        g = dk.grad.cpu().numpy()
        sc, inv = (float(v) for v in scale2.cpu())
        assert np.frexp(sc)[0] == 0.5 and inv == 1.0 / sc
        assert 64.0 <= float(np.abs(g).max()) * sc <= 256.0
        assert np.array_equal(cot.cpu().numpy().view(np.uint16), R.scaled_f16_ref(g, sc).view(np.uint16))
        assert torch.equal(dk.grad.cpu(), _device("A", lt, cof).grad) and float(dk.loss.cpu()) == _device("A", lt, cof).loss
