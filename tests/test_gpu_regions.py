"""Region-constrained drag edits on the device: the weight maps of csrc/regions.hip against tests/regions_ref.py byte for byte, the
weighted gather pass of csrc/drag.hip against the weighted float64 oracle, a map of ones against the unweighted kernel bit for bit,
a batch that mixes edits with and without maps, and the keywords of DragStuff.training / training_batch on the tiny model.

Bounds (those tests/test_gpu_drag_oracle.py derives; none is tuned to what the device gives):
  gradient  err(x) = max|x - g64| / max|g64| over the whole tap;  err_dev <= 8 * err_ref + q, err_ref the same metric of the float32
            weighted yardstick (computed in the run), q = 4 B side^2 * 2^-45 / max|g64| the fixed-point term.  L1: without the
            ambiguous elements (drag_ref.l1_ambiguous_elements), capped on the host at drag_ref.L1_EXCLUDED_CAP.
  loss      |loss_dev - loss64| <= 8 |loss32 - loss64| + nblk 2^-25 / ntot + wmax cof nblk_gather 2^-25 / (Cc nmask): each
            workgroup's partial sum is rounded once to 2^-24, and a gather workgroup's sum carries weights up to wmax.
"""
from argparse import Namespace
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ishapediting_amd import _lib, synthetic
from ishapediting_amd.unet_spec import tiny_config
from tests import drag_ref as R
from tests import regions_ref as G

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ 1. weight maps
def _product_region(items):
    from ishapediting_amd.regions import Box, Sphere, Voxels
    out = []
    for it in items:
        if it[0] == "box":
            out.append(Box(it[1], it[2]))
        elif it[0] == "sphere":
            out.append(Sphere(it[1], it[2]))
        else:
            out.append(Voxels(torch.from_numpy(it[1])))
    return out


@pytest.mark.parametrize("dilate", G.MAP_DILATES)
@pytest.mark.parametrize("size", G.MAP_SIZES, ids=lambda s: f"D{s[0]}-W{s[1]}")
def test_device_maps_are_the_reference_maps_byte_for_byte(size, dilate):
    from ishapediting_amd.regions import plane_weights
    D, W = size
    for grids in G.MAP_GRIDS:
        keep, free = G.map_regions(D, grids)
        for kw, fw in G.MAP_WEIGHTS:
            want = G.plane_weights_ref(keep, free, W, kw, fw, dilate)
            got = plane_weights(keep=_product_region(keep), free=_product_region(free), W=W, keep_weight=kw, free_weight=fw,
                                dilate=dilate, device=dev())
            assert got.dtype == torch.float32 and got.shape == (3, W, W) and got.device.type == "cuda"
            got = got.cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
                (size, dilate, grids, kw, fw, np.argwhere(got != want)[:8].tolist())
    # one region alone, the other absent; and a region given as a single item
    keep, free = G.map_regions(D, "both")
    for k, f in ((keep, None), (None, free)):
        got = plane_weights(keep=_product_region(k) if k else None, free=_product_region(f) if f else None, W=W, dilate=dilate,
                            device=dev())
        assert np.array_equal(got.cpu().numpy(), G.plane_weights_ref(k, f, W, 4.0, 0.0, dilate))
    got = plane_weights(free=_product_region(free[:1])[0], W=W, dilate=dilate, device=dev())
    assert np.array_equal(got.cpu().numpy(), G.plane_weights_ref(None, free[:1], W, 4.0, 0.0, dilate))


def test_an_empty_shadow_raises_on_the_device_too():
    from ishapediting_amd.regions import Box, Sphere, Voxels, plane_weights
    box = Box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
    with pytest.raises(ValueError, match="keep region has an empty shadow"):
        plane_weights(keep=[Box((0.01, 0.01, 0.01), (0.03, 0.03, 0.03))], free=[box], W=16, device=dev())
    with pytest.raises(ValueError, match="free region has an empty shadow"):
        plane_weights(keep=[box], free=[Sphere((3.0, 3.0, 3.0), 0.5)], W=16, device=dev())
    with pytest.raises(ValueError, match="keep region has an empty shadow"):
        plane_weights(keep=[Voxels(torch.zeros(16, 16, 16, dtype=torch.bool))], W=16, device=dev())
    assert float(plane_weights(keep=[box], W=16, dilate=40, device=dev()).min()) == 4.0      # a dilation past the map covers it


def test_component_region_names_the_part_under_a_point():
    """Two balls in a 32^3 volume: the region of a point in one ball is that ball's voxels; a point outside raises."""
    from ishapediting_amd.regions import component_region, plane_weights
    D = 32
    ax = torch.linspace(-1, 1, D)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    a = 0.3 - torch.sqrt((x + 0.5) ** 2 + y ** 2 + z ** 2)
    b = 0.25 - torch.sqrt((x - 0.5) ** 2 + (y - 0.2) ** 2 + z ** 2)
    vol = torch.maximum(a, b).to(dev())
    reg = component_region(vol, (-0.5, 0.0, 0.0))
    assert torch.equal(reg.mask.cpu(), a > 0) and int(reg.mask.sum()) > 0
    assert torch.equal(component_region(vol, (0.5, 0.2, 0.0)).mask.cpu(), b > 0)
    with pytest.raises(ValueError, match="outside the shape"):
        component_region(vol, (0.0, -0.8, 0.8))
    w = plane_weights(keep=reg, W=16, device=dev()).cpu().numpy()
    assert np.array_equal(w, G.plane_weights_ref([("voxels", (a > 0).numpy())], None, 16))


# ------------------------------------------------------------------------------------------------ 2. against float64
def _ids(combo):
    return f"{combo[0]}-{combo[1]}"


@lru_cache(maxsize=None)
def _device(name, loss_type, weights="map"):
    """One solo run of a case (two calls on the same buffers) with the case's map, a map of ones or no map."""
    from ishapediting_amd.drag_utils import DragKernels
    c = R.make_case(name)
    w = {"map": G.weight_map(name), "ones": np.ones((3, c.W, c.W), np.float32), "none": None}[weights]
    dk = DragKernels(dev(), W=c.W, ld=c.ld, chmap=c.chmap, r=c.r, voxel=c.voxel, loss_type=loss_type)
    dk.setup(c.sources, c.targets, G.COF, weights=None if w is None else T(w))
    e_d, o_d = c.edit.to(dev()).contiguous(), c.orig.to(dev()).contiguous()
    grad, loss = dk.loss_grad(e_d, o_d)
    torch.cuda.synchronize()
    out = SimpleNamespace(grad=grad.cpu().clone(), loss=float(loss.cpu()), loss_bits=loss.cpu().clone(),
                          scratch_max=max(int(dk.gfx.abs().max()), int(dk.acc.abs().max())))
    grad, loss = dk.loss_grad(e_d, o_d)
    torch.cuda.synchronize()
    out.again = bool(torch.equal(grad.cpu(), out.grad)) and bool(torch.equal(loss.cpu(), out.loss_bits))
    out.scratch_max = max(out.scratch_max, int(dk.gfx.abs().max()), int(dk.acc.abs().max()))
    return out


@pytest.mark.parametrize("combo", G.COMBOS, ids=_ids)
def test_weighted_gradient_against_float64(combo):
    name, lt = combo
    c, res, got = R.make_case(name), G.oracle(*combo), _device(*combo)
    g64 = res.grad
    keep = ~R.l1_ambiguous_elements(res, c.edit, c.orig, c.chmap, c.W) if lt == "l1" else torch.ones_like(g64, dtype=torch.bool)
    gmax = float(g64.abs().max())
    err_dev = float((got.grad.double() - g64)[keep].abs().max()) / gmax
    err_ref = float((G.reference32(*combo)[1].double() - g64)[keep].abs().max()) / gmax
    q = 4 * c.B * c.side * c.side * 2.0 ** -45 / gmax
    print(f"{_ids(combo)}: gradient err_ref {err_ref:.2e} err_dev {err_dev:.2e} q {q:.1e} max|g64| {gmax:.2e} excluded {int((~keep).sum())}")
    assert err_ref > 0
    assert err_dev <= 8 * err_ref + q, (combo, err_dev, err_ref, q)
    # structural zeros, exact: wherever the oracle is 0 (L1: and the L2 oracle too -- an L1 element can cancel to 0 inside a
    # footprint, tests/test_gpu_drag_oracle.py), and the three classes by name
    zero = g64 == 0
    if lt == "l1":
        zero = zero & (G.oracle(name, "l2").grad == 0)
    assert int(zero.sum()) > 0 and bool((got.grad[zero] == 0.0).all()), (combo, int((got.grad[zero] != 0).sum()))
    for key, m in G.structural_zero(name).items():
        m = T(m)
        assert bool((got.grad[m] == 0.0).all()), (combo, key, int((got.grad[m] != 0).sum()))
    assert got.scratch_max == 0             # gfx and acc left zero by both calls
    assert got.again                        # the second call on the same buffers: the same bits


@pytest.mark.parametrize("combo", G.COMBOS, ids=_ids)
def test_weighted_loss_against_float64(combo):
    name, lt = combo
    c, res, got = R.make_case(name), G.oracle(*combo), _device(*combo)
    l64, l32 = res.loss, G.reference32(*combo)[0]
    wmax = float(G.weight_map(name).max())
    ntot = 3 * c.Cc * c.B * c.side ** 3
    bound = (8 * abs(l32 - l64) + R.terms_blocks(c.B, c.r, c.Cc) * 2.0 ** -25 / ntot
             + wmax * G.COF * R.gather_blocks(c.W, c.ld) * 2.0 ** -25 / (c.Cc * res.nmask))
    print(f"{_ids(combo)}: loss64 {l64:.6e} |dev - 64| {abs(got.loss - l64):.2e} |ref32 - 64| {abs(l32 - l64):.2e} bound {bound:.2e} "
          f"wmax {wmax}")
    assert wmax == 4.0
    assert abs(got.loss - l64) <= bound, (combo, got.loss, l64, l32, bound)
    assert got.loss != _device(name, lt, "none").loss          # the map is in use


# ------------------------------------------------------------------------------------------------ 3. ones == unweighted
@pytest.mark.parametrize("loss_type", ["l2", "l1"])
@pytest.mark.parametrize("name", ["B", "H"])
def test_a_map_of_ones_is_the_unweighted_kernel_bitwise(name, loss_type):
    a, b = _device(name, loss_type, "ones"), _device(name, loss_type, "none")
    assert torch.equal(a.loss_bits, b.loss_bits) and torch.equal(a.grad, b.grad)
    assert a.again and b.again and a.scratch_max == 0 and b.scratch_max == 0


# ------------------------------------------------------------------------------------------------ 4. batch
@pytest.mark.parametrize("loss_type", ["l2", "l1"])
@pytest.mark.parametrize("shared", [False, True], ids=["stride", "shared"])
def test_batch_with_and_without_maps_is_bitwise_the_solo_runs(loss_type, shared):
    from ishapediting_amd.drag_utils import BatchDragKernels, DragKernels
    L = R.make_batch()
    wmap, ones = T(G.batch_map()), torch.ones(3, L.W, L.W)
    maps = [None, wmap, ones]
    bk = BatchDragKernels(dev(), L.E, W=L.W, ld=L.ld, chmap=L.chmap, r=L.r, voxel=L.voxel, loss_type=loss_type)
    bk.setup(L.sources, L.targets, list(L.cofs), weights=maps)
    e_d = L.edits.to(dev()).contiguous()
    o_d = (L.origs[:1] if shared else L.origs).to(dev()).contiguous()
    stride = 0 if shared else L.W * L.W * L.ld
    grad, loss = bk.loss_grad_ptr(e_d.data_ptr(), o_d.data_ptr(), stride)
    torch.cuda.synchronize()
    grad, loss = grad.cpu().clone(), loss.cpu().clone()
    solo = []
    for e in range(L.E):
        dk = DragKernels(dev(), W=L.W, ld=L.ld, chmap=L.chmap, r=L.r, voxel=L.voxel, loss_type=loss_type)
        dk.setup(L.sources[e], L.targets[e], L.cofs[e], weights=maps[e] if e == 1 else None)      # 0 and 2: the unweighted run
        g, l = dk.loss_grad(e_d[e], o_d[0 if shared else e])
        torch.cuda.synchronize()
        solo.append((g.cpu().clone(), l.cpu().clone()))
        assert torch.equal(grad[e], solo[e][0]) and torch.equal(loss[e:e + 1], solo[e][1]), (e, loss_type, shared)
    # edit 1's map is in use: its solo run without one differs
    dk = DragKernels(dev(), W=L.W, ld=L.ld, chmap=L.chmap, r=L.r, voxel=L.voxel, loss_type=loss_type)
    dk.setup(L.sources[1], L.targets[1], L.cofs[1])
    g, l = dk.loss_grad(e_d[1], o_d[0 if shared else 1])
    assert not torch.equal(g.cpu(), solo[1][0])
    # the fused cotangent call: the same losses and gradients, and the fp16 cotangent of the gradient at the returned scale
    cot, scale2 = bk.loss_cotangent_ptr(e_d.data_ptr(), o_d.data_ptr(), stride)
    torch.cuda.synchronize()
    assert torch.equal(bk.grad.cpu(), grad) and torch.equal(bk.loss.cpu(), loss)
    sc, inv = (float(v) for v in scale2.cpu())
    assert np.frexp(sc)[0] == 0.5 and inv == 1.0 / sc
    assert np.array_equal(cot.cpu().numpy().view(np.uint16), R.scaled_f16_ref(grad.numpy(), sc).view(np.uint16))
    with pytest.raises(ValueError, match="cof"):                                    # edit 0 has cof 0: no map for it
        bk.setup(L.sources, L.targets, list(L.cofs), weights=[ones, None, None])
    with pytest.raises(ValueError, match="2 entries for 3 edits"):
        bk.setup(L.sources, L.targets, list(L.cofs), weights=[None, ones])
    bk.setup(L.sources, L.targets, list(L.cofs), weights=[None, None, None])        # all None: the unweighted launch
    assert bk.weights is None


# ------------------------------------------------------------------------------------------------ 5. end to end, tiny model
def _tiny(gold, max_edits=1):
    """The tiny DragStuff of tests/test_gpu_first_step_reuse.py (built for `max_edits`); get_mesh keeps the final latent only."""
    from ishapediting_amd.drag_utils import DragStuff
    g = gold("g8_g9_tiny_loops")
    Tn, w_time, feat_layer, r1, B = g["meta"].tolist()
    args = Namespace(clip_denoised=True, num_samples=1, batch_size=1, use_ddim=False, num_steps=Tn, image_size=16,
                     num_channels=32, num_res_blocks=1, num_heads=4, num_heads_upsample=-1, num_head_channels=32,
                     attention_resolutions="8", channel_mult="1,2", dropout=0.1, class_cond=False, shape_resolution=32,
                     use_checkpoint=False, use_scale_shift_norm=True, resblock_updown=True, use_fp16=True,
                     use_new_attention_order=False, in_out_channels=6, learn_sigma=True, diffusion_steps=1000,
                     noise_schedule="linear", timestep_respacing=str(Tn), w_time=w_time, feat_layer=feat_layer,
                     loss_type="l2", use_kl=False, predict_xstart=False, rescale_timesteps=False,
                     rescale_learned_sigmas=False, explicit_normalization=False)
    ds = DragStuff(dev(), args=args, max_edits=max_edits)
    ds.model.load_state_dict(synthetic.round_torso_to_fp16(synthetic.unet_state_dict(tiny_config(1), 101)))
    ds.set_offset1(r1)
    ds.voxel_size = 2.0 / 32

    def get_mesh(tri_feat=None, img=None, t=0):
        if tri_feat is None:
            tri_feat = ds._denoise(img, t)
        ds.tri_feat = tri_feat
    ds.get_mesh = get_mesh
    ns, dn = T(g["loop_noise_sampling"]).to(dev()), T(g["drag_noise"]).to(dev())
    ds.step_noise = lambda i: ns[Tn - 1 - i]
    ds.update_latent_params(img=g["loop_latent0"])
    ds.step_noise = lambda i: dn[w_time - 1 - i]
    return ds, g, dn, w_time


def _box():
    from ishapediting_amd.regions import Box
    return Box((-0.9, -0.9, -0.9), (0.15, 0.3, 0.1))


def _run(ds, g, **kw):
    prog = list(ds.training(g["drag_sources"], g["drag_targets"], scale=50.0, cof=0.4, **kw))
    torch.cuda.synchronize()
    assert len(prog) == len(ds.last_losses)
    return ds.tri_feat.clone(), [l.clone() for l in ds.last_losses]


def _same(a, b):
    return torch.equal(a[0], b[0]) and len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def test_training_with_regions_on_the_tiny_model(gold):
    from ishapediting_amd.drag_utils import DragKernels, feat_channel_map
    from ishapediting_amd.regions import plane_weights
    ds, g, dn, w_time = _tiny(gold)
    ch, width = ds.model.tap_shape(ds.args.feat_layer)
    plain = _run(ds, g)
    assert ds._first_step is not None                                     # the plain edit took the first-step snapshot
    ones = _run(ds, g, weights=torch.ones(3, width, width))
    assert _same(ones, plain)                                             # a map of ones: the plain edit, bit for bit
    kept = ds._first_step
    keep = _run(ds, g, keep=[_box()])                                     # after plain edits, on the restored first step
    assert ds._first_step is kept and ds._dk.weights is not None
    assert _same(_run(ds, g, keep=[_box()]), keep)                        # bitwise repeatable
    # in the first step the tap IS its guidance (nothing has moved yet): the preservation term is 0 and the map cannot show;
    # from the second step on it does
    assert not torch.equal(keep[0], plain[0]) and torch.equal(keep[1][0], plain[1][0]) and not torch.equal(keep[1][-1], plain[1][-1])
    # the first step's loss against a stand-alone DragKernels call on that step's tap (the snapshot) and guidance
    assert ds.model.snapshot_restore()
    dk = DragKernels(dev(), W=width, ld=ch, chmap=feat_channel_map(ch), r=ds.r1, voxel=ds.voxel_size, loss_type="l2")
    wmap = plane_weights(keep=[_box()], W=width, device=dev())
    assert float(wmap.max()) == 4.0 and float(wmap.min()) == 1.0
    dk.setup(g["drag_sources"], g["drag_targets"], 0.4, weights=wmap)
    _, loss = dk.loss_grad_ptr(ds.model.tap_ptr(), ds.feature_guidance[0].data_ptr())
    torch.cuda.synchronize()
    assert float(loss.cpu()) == float(keep[1][0].cpu())
    # the same call on a fresh object (no snapshot to restore: it runs its first forward)
    fresh, g2, _, _ = _tiny(gold)
    assert fresh._first_step is None
    assert _same(_run(fresh, g2, keep=[_box()]), keep)
    # the keywords are checked when the edit starts
    with pytest.raises(ValueError, match="cof"):
        list(ds.training(g["drag_sources"], g["drag_targets"], scale=50.0, cof=0.0, keep=[_box()]))
    with pytest.raises(ValueError, match="not both"):
        list(ds.training(g["drag_sources"], g["drag_targets"], scale=50.0, cof=0.4, keep=[_box()], weights=torch.ones(3, width, width)))
    assert int(_lib.lib().ishap_device_status()) == 0


def test_training_batch_with_a_region_on_one_edit(gold):
    """Two variants of one shape in one loop, keep = [None, [Box]]: edit 0 has the bits of the plain batched edit."""
    ds, g, dn, w_time = _tiny(gold, max_edits=2)
    ds.step_noise = lambda i: dn[w_time - 1 - i].repeat(2, 1, 1, 1)
    src, tgt = [g["drag_sources"]] * 2, [g["drag_targets"]] * 2

    def run(**kw):
        list(ds.training_batch(src, tgt, scale=50.0, cof=0.4, **kw))
        torch.cuda.synchronize()
        return ds.tri_feat_batch.clone(), torch.stack(ds.last_losses).clone()
    plain, plain_losses = run()
    assert torch.equal(plain[0], plain[1])                                # the same edit twice
    mixed, mixed_losses = run(keep=[None, [_box()]])
    assert ds._dk_batch.weights is not None and float(ds._dk_batch.weights[0].min()) == 1.0 == float(ds._dk_batch.weights[0].max())
    assert torch.equal(mixed[0], plain[0]) and torch.equal(mixed_losses[:, 0], plain_losses[:, 0])
    assert not torch.equal(mixed[1], plain[1]) and not torch.equal(mixed_losses[:, 1], plain_losses[:, 1])
    with pytest.raises(ValueError, match="3 entries for 2 edits"):
        list(ds.training_batch(src, tgt, scale=50.0, cof=0.4, keep=[None, [_box()], None]))
    assert int(_lib.lib().ishap_device_status()) == 0
