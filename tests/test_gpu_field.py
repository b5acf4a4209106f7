"""The decoder's field kernels (csrc/decode_field.hip) through their ABI calls, against the float64 statement of
tests/field_ref.py, and the mesh refinement built on them (mesh.OccupancyMesh(refine=...), DragStuff.refine).

Bounds (derived in tests/field_ref.py and tests/decoder_ref.py, none tuned to what the device gives; tests/test_field_ref_host.py
shows that the gradient bound passes an honest fp32 result and rejects every listed mutation):
  logits     |dev - ref64| <= decoder_ref.forward_bound with SIN_SOFT, on every point.
  gradients  |dev - ref64| <= 4 REL A + D per point and axis on the points that pass the kink filter and lie further than 2 u |ix|
             from every cell boundary; finite everywhere.  REL is measured on the CPU when the test runs.
  normals    the same bound carried through the normalisation (field_ref.normal_bound), at the returned points.
  projection per point, from the device's own numbers: |z_out| <= |z at x0|, |x_out - x0| <= max_move (1 + 4 u),
             accepted <= iterations, |normal| = 1 within 4 u or normal = 0 exactly.
Every output starts as a NaN bit pattern with 256 canary elements behind it; every call is made twice and must give the same bits.

Shapes: npts 1, 33, 1061 (a tail tile) and 65 575 (the launch's grid is 256 blocks x 4 waves x 32 points = 32 768 points a
pass, so this makes a second and the start of a third pass); S 2, 8 and 128; the seven coordinate families of decoder_ref.  The
float64 reference of a plane size is computed once: the 1- and 33-point cases are the first points of the 1061, the 65 575-point
case repeats them, so every point of every case is compared.

Measured on an MI355X (all 46 cases pass):
  field_grad  REL sits at its floor 2 u = 1.19e-7 in every case (A, all absolute values, is some 2 500 times the gradient, so
              the bound is about 0.2 % of it).  Worst error / bound: logits 0.003 (S = 2, 8), 0.036 (S = 128); gradients 0.001
              (S = 2), 0.003 (S = 8), 0.031 (S = 128: max |dev - ref64| 1.05e-3 at |grad| of order 10 .. 100), 0.042 in the fade
              band at S = 128.  The filter keeps 96.4 / 95.9 / 93.5 % of the uniform points at S = 2 / 8 / 128; in the centres and
              faces families (and far at S = 128) every point sits on a cell boundary, so only their logits are compared.
              Scaling the layers by 2^+-4 changes no bit of either output.
  project     z_out worst error / bound 0.004 (S = 8), 0.031 (S = 128); normals 0.002 and 0.029.  The 65 575 repeated points
              give 1 061 distinct results: a point's result does not depend on its lane.
  convergence |z| <= 1e-4 after 4 iterations on the 2 000 sign-change cell centres: float64 0.9080, device 0.9085; mean |z|
              0.119 -> 2.264e-3 (float64), 2.265e-3 (device); accepted steps per point 2.78 both.
  mesh        res 32: 9 729 vertices, 9 662 moved; |z| <= 1e-4 on 0.7 % of the smoothed vertices and 98.6 % of the refined ones,
              mean |z| 1.1e-2 -> 5.6e-5; analytic normals agree in sign with the triangle sum on 99.55 % (float64 and device).
  DragStuff   get_mesh at the default 256^3 on the small synthetic latent (a noise surface): 16 108 596 vertices, 16 064 362 moved,
              |z| <= 1e-4 on 0.1 % before and 83.2 % after, mean |z| 0.173 -> 6.9e-3; same triangles, volume unchanged.
"""
import ctypes as C
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import decoder_ref as D
from tests import field_ref as F
from tests.test_gpu_decoder_oracle import NAN_BITS, CANARY_BITS, NCANARY, Weights, L, dev, guarded, put, read

pytestmark = pytest.mark.gpu

U = D.U
GMIN = 1e-12
TOL = 1e-4
VOXEL = 2.0 / 31                    # the projections of this file move in voxels of a 32^3 grid
NBIG = 65575


def read_int(buf, n, tag):
    host = buf.view(torch.int32).cpu()
    assert bool((host[n:] == CANARY_BITS).all()), f"{tag}: a canary changed"
    assert not bool((host[:n] == NAN_BITS).any()), f"{tag}: element(s) not written"
    return host[:n].numpy().copy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def field_call(w, planes_d, S, coords):
    """two calls of ishap_triplane_field_grad on fresh guarded buffers -> (logits [n], grad [n,3]), asserted bitwise equal"""
    n = len(coords)
    c_d = put(coords)
    outs = []
    for _ in range(2):
        z, g = guarded(n), guarded(3 * n)
        L().check(L().lib().ishap_triplane_field_grad(planes_d.data_ptr(), S, C.byref(w.c), c_d.data_ptr(), n, z.data_ptr(), g.data_ptr(),
                                                      L().stream_ptr(dev())))
        torch.cuda.synchronize()
        outs.append((read(z, n, "logits"), read(g, 3 * n, "grad").reshape(n, 3)))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1]), "field_grad: a second call gave other bits"
    return outs[0]


def project_call(w, planes_d, S, coords, iterations, step_max=0.5 * VOXEL, max_move=VOXEL, tol=TOL, gmin=GMIN):
    """two calls of ishap_triplane_project -> SimpleNamespace(x, z, normal, accepted), asserted bitwise equal"""
    n = len(coords)
    c_d = put(coords)
    outs = []
    for _ in range(2):
        x, z, nr, ac = guarded(3 * n), guarded(n), guarded(3 * n), guarded(n)
        L().check(L().lib().ishap_triplane_project(planes_d.data_ptr(), S, C.byref(w.c), c_d.data_ptr(), n, iterations, step_max, max_move,
                                                   tol, gmin, x.data_ptr(), z.data_ptr(), nr.data_ptr(), ac.data_ptr(),
                                                   L().stream_ptr(dev())))
        torch.cuda.synchronize()
        outs.append(SimpleNamespace(x=read(x, 3 * n, "x_out").reshape(n, 3), z=read(z, n, "z_out"),
                                    normal=read(nr, 3 * n, "normal_out").reshape(n, 3), accepted=read_int(ac, n, "accepted_out")))
    a, b = outs
    assert same_bits(a.x, b.x) and same_bits(a.z, b.z) and same_bits(a.normal, b.normal) and np.array_equal(a.accepted, b.accepted), \
        "project: a second call gave other bits"
    return a


# ----------------------------------------------------------------------------------------------------------- references
@lru_cache(maxsize=None)
def setup(S, amp=D.AMP_BWD, k=0):
    sd, _ = D.synthetic_net()
    sd = D.scaled_state_dict(sd, k) if k else sd
    planes = D.make_planes(S, amp, S)
    return SimpleNamespace(S=S, net=D.net64(sd), planes=planes, w=Weights(sd), planes_d=put(planes))


def oracle(s, coords):
    """float64 logits and gradients of `coords` with their bounds, the filter and REL"""
    ref = F.field_grad(s.net, s.planes, coords)
    keep = F.gradient_filter(s.net, s.planes, coords)
    rel = F.measured_rel(s.net, s.planes, coords, ref, keep)
    fb = D.forward_bound(s.net, s.planes, ref.fw, sin_abs=D.SIN_SOFT).bound
    return SimpleNamespace(ref=ref, keep=keep, rel=rel, gb=F.grad_bound(ref, rel), fb=fb)


@lru_cache(maxsize=None)
def uniform_oracle(S, n=1061, k=0):
    s = setup(S, k=k)
    coords = D.coords_family("uniform", n, S, np.random.RandomState(100 + S))
    return s, coords, oracle(s, coords)


def check_field(tag, z, g, o, idx=None):
    """device logits / gradients against the oracle `o` (rows idx of it)"""
    idx = np.arange(len(z)) if idx is None else idx
    ez = np.abs(z - o.ref.logit[idx])
    worst_z = float((ez / o.fb[idx]).max())
    keep = o.keep[idx]
    eg, gb = np.abs(g - o.ref.grad[idx]), o.gb[idx]
    worst_g = float((eg[keep] / np.maximum(gb[keep], 1e-300) * (eg[keep] > 0)).max()) if keep.any() else 0.0
    print(f"{tag}: logits max err {ez.max():.2e} worst err / bound {worst_z:.3f}; gradients on {int(keep.sum())} of {len(z)} points, "
          f"REL {o.rel:.2e}, max err {eg[keep].max() if keep.any() else 0.0:.2e}, worst err / bound {worst_g:.3f}")
    assert np.isfinite(g).all()
    assert (ez <= o.fb[idx]).all(), f"{tag}: logit error / bound {worst_z}"
    assert (eg[keep] <= gb[keep]).all(), f"{tag}: gradient error / bound {worst_g}"


# ----------------------------------------------------------------------------------------------------------- field_grad
@pytest.mark.parametrize("npts", [1, 33, 1061, NBIG])
@pytest.mark.parametrize("S", [2, 8, 128])
def test_field_grad_uniform(S, npts):
    s, coords, o = uniform_oracle(S)
    assert 1.0 - o.keep.mean() <= 0.15, f"the filter leaves out {1.0 - o.keep.mean():.3f} of the uniform points"
    idx = np.arange(npts) % len(coords)
    z, g = field_call(s.w, s.planes_d, S, coords[idx])
    check_field(f"uniform S{S} n{npts}", z, g, o, idx)


@pytest.mark.parametrize("family", [f for f in D.FAMILIES if f != "uniform"])
@pytest.mark.parametrize("S", [2, 8, 128])
def test_field_grad_families(S, family):
    s = setup(S)
    coords = D.coords_family(family, 64, S, np.random.RandomState(7 * S + len(family)))
    o = oracle(s, coords)
    z, g = field_call(s.w, s.planes_d, S, coords)
    check_field(f"{family} S{S}", z, g, o)
    if family == "beyond":            # no tap of any plane in range: the decoder's value at zero features, and a field that is flat
        assert (g == 0).all()
        assert same_bits(z, np.full_like(z, z[0]))
        x1 = np.concatenate([np.zeros(64), np.ones(64)])[None, :]
        assert abs(float(z[0]) - float(D.mlp(s.net, x1)[4][0])) <= o.fb[0]


@pytest.mark.parametrize("k", [-4, 4])
def test_field_grad_scaled_layers(k):
    s, coords, o = uniform_oracle(8, 265, k)
    z, g = field_call(s.w, s.planes_d, 8, coords)
    check_field(f"scaled 2^{k}", z, g, o)
    z0, g0 = field_call(setup(8).w, setup(8).planes_d, 8, coords)
    print(f"scaled 2^{k}: against the unscaled network max |d logit| {np.abs(z - z0).max():.2e}, max |d grad| {np.abs(g - g0).max():.2e}")


# ----------------------------------------------------------------------------------------------------------- project
def check_projection(tag, s, coords, p, iterations, max_move, z_start, gmin=GMIN):
    """the per-point properties from the device's own numbers, then z_out and the normal against float64 at x_out"""
    n = len(coords)
    assert (np.abs(p.z) <= np.abs(z_start)).all(), f"{tag}: |z| grew"
    move = np.sqrt(((p.x.astype(np.float64) - coords.astype(np.float64)) ** 2).sum(1))
    assert (move <= max_move * (1 + 4 * U)).all(), f"{tag}: moved {move.max() / max_move} of max_move"
    assert (p.accepted >= 0).all() and (p.accepted <= iterations).all()
    nn = np.sqrt((p.normal.astype(np.float64) ** 2).sum(1))
    zero = (p.normal == 0).all(axis=1)
    assert (np.abs(nn[~zero] - 1) <= 4 * U).all(), f"{tag}: |normal| - 1 = {np.abs(nn[~zero] - 1).max() / U} u"
    assert same_bits(p.x[p.accepted == 0], coords[p.accepted == 0]), f"{tag}: a point without an accepted step moved"
    # float64 at the returned points; repeated inputs give repeated outputs, so only distinct rows are evaluated
    ux, inv = np.unique(p.x, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    o = oracle(s, ux)
    ez = np.abs(p.z - o.ref.logit[inv])
    assert (ez <= o.fb[inv]).all(), f"{tag}: z_out error / bound {(ez / o.fb[inv]).max()}"
    want = F.normal_of(o.ref.grad, gmin)
    nb = F.normal_bound(o.ref.grad, o.gb)
    g2 = (o.ref.grad ** 2).sum(1)
    cmp = (o.keep & (g2 > 4 * gmin))[inv] & ~zero            # a gradient AT gmin may fall on either side of the threshold
    en = np.abs(p.normal - want[inv])
    worst = float((en[cmp] / nb[inv][cmp]).max()) if cmp.any() else 0.0
    print(f"{tag}: {len(ux)} distinct of {n} points, moved {int((p.accepted > 0).sum())}, |z| <= tol before {np.mean(np.abs(z_start) <= TOL):.3f} "
          f"after {np.mean(np.abs(p.z) <= TOL):.3f}, mean |z| {np.abs(z_start).mean():.2e} -> {np.abs(p.z).mean():.2e}; z_out worst err / bound "
          f"{(ez / o.fb[inv]).max():.3f}; normals on {int(cmp.sum())} points, REL {o.rel:.2e}, worst err / bound {worst:.3f}")
    assert (en[cmp] <= nb[inv][cmp]).all(), f"{tag}: normal error / bound {worst}"


def test_project_zero_iterations_is_field_grad():
    s, coords, _ = uniform_oracle(8)
    z, g = field_call(s.w, s.planes_d, 8, coords)
    p = project_call(s.w, s.planes_d, 8, coords, 0)
    assert same_bits(p.x, coords) and same_bits(p.z, z) and (p.accepted == 0).all()
    check_projection("project it0", s, coords, p, 0, VOXEL, z)
    # the normal is the device's own gradient, normalised in double and rounded once
    want = F.normal_of(g.astype(np.float64), GMIN)
    assert (np.abs(p.normal - want) <= U * np.abs(want) + 1e-45).all()


@pytest.mark.parametrize("S,npts,iterations", [(8, 1061, 1), (8, 1061, 4), (8, 1, 4), (8, 33, 4), (8, NBIG, 1), (2, 265, 4), (128, 265, 4)])
def test_project(S, npts, iterations):
    s, base, _ = uniform_oracle(S)
    coords = base[np.arange(npts) % len(base)]
    z, _ = field_call(s.w, s.planes_d, S, coords)
    p = project_call(s.w, s.planes_d, S, coords, iterations)
    check_projection(f"project S{S} n{npts} it{iterations}", s, coords, p, iterations, VOXEL, z)


def test_project_clips_to_a_small_ball():
    """max_move far below step_max and below an ulp of some coordinates: the ball holds for the ROUNDED positions"""
    s, coords, _ = uniform_oracle(8)
    z, _ = field_call(s.w, s.planes_d, 8, coords)
    for mm in (3e-8, 1e-4):
        p = project_call(s.w, s.planes_d, 8, coords, 4, max_move=mm)
        move = np.sqrt(((p.x.astype(np.float64) - coords.astype(np.float64)) ** 2).sum(1))
        assert (move <= mm * (1 + 4 * U)).all() and (np.abs(p.z) <= np.abs(z)).all()


@lru_cache(maxsize=None)
def convergence_case():
    s = setup(8, D.AMP_FWD)
    pts = F.sign_change_points(s.net, s.planes, 32, 2000, 0)
    ref = F.project(s.net, s.planes, pts, 4, 0.5 * VOXEL, VOXEL, TOL, GMIN)
    return s, pts, ref


def test_project_converges_as_float64_does():
    """S = 8 planes at AMP_FWD, the centres of 2000 cells of a 32^3 grid whose float64 corner logits change sign, 4 iterations,
    steps of at most half a voxel, at most one voxel from the start: the share of points that end with |z| <= tol on the device
    is at least the share the float64 projection reaches, minus 0.02 (a trajectory that crosses a ReLU kink or a cell boundary
    may accept another step in fp32)."""
    s, pts, ref = convergence_case()
    p = project_call(s.w, s.planes_d, 8, pts, 4)
    share64, share = float(np.mean(np.abs(ref.z) <= TOL)), float(np.mean(np.abs(p.z) <= TOL))
    print(f"convergence: |z| <= {TOL} after 4 iterations: float64 {share64:.4f}, device {share:.4f}; mean |z| {np.abs(ref.z_start).mean():.3e} -> "
          f"float64 {np.abs(ref.z).mean():.3e}, device {np.abs(p.z).mean():.3e}; accepted steps float64 {ref.accepted.mean():.2f}, device {p.accepted.mean():.2f}")
    assert share >= share64 - 0.02


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing():
    s, coords, _ = uniform_oracle(8)
    c_d = put(coords[:33])
    n = 33
    bufs = [guarded(3 * n), guarded(n), guarded(3 * n), guarded(n)]
    x, z, nr, ac = bufs
    lib, st = L().lib(), L().stream_ptr(dev())
    fg = lambda S, npts, zp, gp: lib.ishap_triplane_field_grad(s.planes_d.data_ptr(), S, C.byref(s.w.c), c_d.data_ptr(), npts, zp, gp, st)      # noqa: E731
    pj = lambda S, npts, xp, zp, np_, ap: lib.ishap_triplane_project(s.planes_d.data_ptr(), S, C.byref(s.w.c), c_d.data_ptr(), npts, 4,      # noqa: E731
                                                                     0.5 * VOXEL, VOXEL, TOL, GMIN, xp, zp, np_, ap, st)
    P = lambda t: t.data_ptr()      # noqa: E731
    assert fg(1, n, P(z), P(x)) == -2 and fg(8, 0, P(z), P(x)) == -2 and fg(8, n, None, P(x)) == -2 and fg(8, n, P(z), None) == -2
    assert pj(1, n, P(x), P(z), P(nr), P(ac)) == -2 and pj(8, 0, P(x), P(z), P(nr), P(ac)) == -2
    assert pj(8, n, None, P(z), P(nr), P(ac)) == -2 and pj(8, n, P(x), None, P(nr), P(ac)) == -2
    assert pj(8, n, P(x), P(z), None, P(ac)) == -2 and pj(8, n, P(x), P(z), P(nr), None) == -2
    torch.cuda.synchronize()
    for b, m in zip(bufs, (3 * n, n, 3 * n, n)):
        host = b.view(torch.int32).cpu()
        assert bool((host[:m] == NAN_BITS).all()) and bool((host[m:] == CANARY_BITS).all())


# ----------------------------------------------------------------------------------------------------------- mesh level
MESH_RES = 32
# planes 0.005 * randn(seed 1) and the decoder's output bias lowered by the float64 median of the 32^3 logits, so that half the
# grid is inside (with the synthetic bias 1 % is: blobs of a few voxels that ten smoothing sweeps collapse).  Chosen on the
# float64 statement: seeds 0..5 at this amplitude give an orientation share of 0.9887 .. 0.9955 (this one 0.9955; the device
# gives the same 0.9955), 0.977 .. 0.990 at 0.01 * randn and 0.949 .. 0.966 at 0.02 * randn.
MESH_SEED, MESH_AMP = 1, 0.005


@lru_cache(maxsize=None)
def mesh_case():
    from ishapediting_amd.triplane_decoder import MultiTriplane, decode_planes_grid
    pl = D.make_planes(8, MESH_AMP, MESH_SEED)
    sd = {k: np.array(v, np.float32) for k, v in D.synthetic_net()[0].items()}
    grid = D.grid_coords(np.linspace(-1, 1, MESH_RES).astype(np.float32))
    sd["5.bias"] = (sd["5.bias"] - np.float32(np.median(D.forward(D.net64(sd), pl, grid).logit))).astype(np.float32)
    dec = MultiTriplane(1, device=dev())
    dec.net.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    planes = put(pl)
    vol = decode_planes_grid(dec, planes, MESH_RES)
    return dec, planes, vol, D.net64(sd)


def triangle_sum_slack(v, t):
    """[V,1]: how far two runs of mesh.vertex_normals may differ per component.  The face normals are elementwise fp32 (the same
    bits every run); their sum over a vertex's m incident triangles goes through float atomics in an order that changes from
    run to run: each order is within (m - 1) u sum |fn| of the exact sum, two orders within twice that, and normalising a vector
    s moves by at most 2 |ds| / |s|: 4 (m - 1) u |sum |fn|| / |s| + 4 u (the norm, the division, twice)."""
    v64, tl = v.double(), t.long()
    fn = torch.cross(v64[tl[:, 1]] - v64[tl[:, 0]], v64[tl[:, 2]] - v64[tl[:, 0]], dim=1)
    ssum, asum, cnt = torch.zeros_like(v64), torch.zeros_like(v64), torch.zeros_like(v64[:, :1])
    for k in range(3):
        ssum.index_add_(0, tl[:, k], fn)
        asum.index_add_(0, tl[:, k], fn.abs())
        cnt.index_add_(0, tl[:, k], torch.ones_like(fn[:, :1]))
    return 4 * (cnt - 1).clamp_min(0) * U * asum.norm(dim=1, keepdim=True) / ssum.norm(dim=1, keepdim=True).clamp_min(1e-300) + 4 * U


def test_plain_mesh_is_unchanged():
    """without refine the vertices are bit for bit what the public pieces give (extract, smooth, the vertex convention
    g / res * 2 - 1), as before this option existed, and the normals are mesh.vertex_normals of them: that sum goes through
    float atomics (index_add_), so two runs of it -- before this option as after -- agree to triangle_sum_slack in torch's
    default mode, and bit for bit under torch.use_deterministic_algorithms(True); both are asserted."""
    from ishapediting_amd import mesh as M
    _, _, vol, _ = mesh_case()
    m = M.OccupancyMesh(vol, MESH_RES)
    v, t = M.extract_surface(vol, 0.0)
    v = M.smooth_mesh(v, t, 10, box_max=float(MESH_RES - 1)) / MESH_RES * 2 - 1
    assert torch.equal(m.vertices, v) and torch.equal(m.triangles, t) and v.shape[0] > 100
    assert not m.has_vertex_normals()
    m.compute_vertex_normals()
    assert m._field_normals is None
    assert bool(((m._vnormals - M.vertex_normals(v, t)).abs() <= triangle_sum_slack(v, t)).all())
    # with torch's deterministic algorithms the sum has one order, and the two evaluations agree bit for bit
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a = M.OccupancyMesh(vol, MESH_RES).compute_vertex_normals()._vnormals
        b = M.vertex_normals(v, t)
    finally:
        torch.use_deterministic_algorithms(before)
    assert torch.equal(a, b)
    same = M.volume_to_mesh(vol, MESH_RES, refine=None)
    assert torch.equal(same.vertices, v) and same.refine is None and same.refinement is None


def test_refined_mesh():
    import copy
    from ishapediting_amd import mesh as M
    from ishapediting_amd.triplane_decoder import field_grad_planes
    dec, planes, vol, net = mesh_case()
    plain = M.OccupancyMesh(vol, MESH_RES)
    fine = M.OccupancyMesh(vol, MESH_RES, refine={"decoder": dec, "planes": planes, "iterations": 4, "max_move": 2.0 / (MESH_RES - 1)})
    assert torch.equal(fine.triangles, plain.triangles) and fine.vertices.shape == plain.vertices.shape
    # the smoothed vertices in decoder coordinates 2 g / (res - 1) - 1 (the rule the volume was sampled with) ...
    g = M.smooth_mesh(*M.extract_surface(vol, 0.0), 10, box_max=float(MESH_RES - 1))
    start, p = fine.refinement
    assert torch.equal(start, g * 2 / (MESH_RES - 1) - 1)
    # ... and the refined ones: the vertices are the projection's points mapped back to grid units and on to g / res * 2 - 1
    moved = (p.accepted > 0)[:, None]
    assert torch.equal(fine.vertices, torch.where(moved, (p.points + 1) * (MESH_RES - 1) / 2, g) / MESH_RES * 2 - 1)
    assert torch.equal(fine.vertices[~moved[:, 0]], plain.vertices[~moved[:, 0]])
    z0 = field_grad_planes(dec, planes, start).logits
    z1 = field_grad_planes(dec, planes, p.points).logits
    assert torch.equal(z1, p.logits)
    assert bool((z1.abs() <= z0.abs()).all())
    step = (p.points - start).double().norm(dim=1)
    assert bool((step <= 2.0 / (MESH_RES - 1) * (1 + 4 * U)).all())
    # analytic normals, the triangle sum where the field has none
    fine.compute_vertex_normals()
    tri = M.vertex_normals(fine.vertices, fine.triangles)
    has = (p.normals != 0).any(dim=1)
    assert torch.equal(fine._vnormals[has], p.normals[has])
    assert bool(((fine._vnormals - tri).abs() <= triangle_sum_slack(fine.vertices, fine.triangles))[~has].all())
    # normalized=False: still unit vectors throughout (the fallback is the normalised triangle sum)
    raw = copy.deepcopy(fine).compute_vertex_normals(normalized=False)._vnormals
    assert torch.equal(raw[has], p.normals[has]) and bool(((raw.double().norm(dim=1) - 1).abs() <= 1e-6).all())
    # orientation: the analytic normal (direction of decreasing logit) against the triangle sum of the same mesh, which
    # extract_surface orients outward; and the same share for the float64 statement at the same vertices
    n64 = F.normal_of(F.field_grad(net, planes.cpu().numpy(), p.points.cpu().numpy()).grad, GMIN)
    tri64 = tri.double().cpu().numpy()
    share64 = float(((n64 * tri64).sum(1) > 0).mean())
    share = float(((p.normals * tri).sum(1) > 0).float().mean())
    print(f"refined mesh: {fine.vertices.shape[0]} vertices, {int(moved.sum())} moved; |z| <= {TOL} {float((z0.abs() <= TOL).float().mean()):.3f} -> "
          f"{float((z1.abs() <= TOL).float().mean()):.3f}, mean |z| {float(z0.abs().mean()):.3e} -> {float(z1.abs().mean()):.3e}; "
          f"normals agreeing with the triangle sum: float64 {share64:.4f}, device {share:.4f}")
    assert share64 >= 0.98, "the plane seed was chosen for a float64 share of at least 0.98"
    assert share >= 0.90
    # deepcopy carries the option and the mesh; the open3d / third_party rules
    c = copy.deepcopy(fine)
    assert c.refine is fine.refine and torch.equal(c.vertices, fine.vertices)
    assert torch.equal(c.compute_vertex_normals()._vnormals[has], fine._vnormals[has])
    with pytest.raises(ValueError):
        M.volume_to_mesh(vol, MESH_RES, backend="third_party", refine=fine.refine)
    with pytest.raises(ValueError):
        M.OccupancyMesh(vol, MESH_RES, refine={"iterations": 4})


def test_dragstuff_refine():
    from ishapediting_amd import synthetic
    """get_mesh with and without DragStuff.refine at the DEFAULT shape_resolution (256): the decode, the surface, ten sweeps
    and the projection of every vertex (several grid-stride passes of the kernel), on the small synthetic latent"""
    from ishapediting_amd.drag_utils import DragStuff, get_args
    from ishapediting_amd.triplane_decoder import field_grad_planes
    from tests.helpers import small96_args, small96_config
    res = get_args([]).shape_resolution
    assert res == 256
    ds = DragStuff(dev(), args=small96_args(4, w_time=2, feat_layer=1, shape_resolution=res))
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(small96_config(), 202))
    ds.load_weights(sd, synthetic.decoder_state_dict(), -np.full(96, 1.5, np.float32), np.full(96, 0.5, np.float32))
    assert ds.refine is None
    feat = torch.randn((2, 96, 16, 16), generator=torch.Generator().manual_seed(5)).to(dev())
    plain = ds.get_mesh(tri_feat=feat[:1])
    vol = ds.volume.clone()
    assert plain.refine is None
    assert ds.args.shape_resolution == res and tuple(vol.shape) == (res, res, res)
    ds.refine = {"iterations": 4, "max_move": 2.0 / (res - 1)}
    fine = ds.get_mesh(tri_feat=feat[:1])
    assert torch.equal(ds.volume, vol) and fine.volume is ds.volume
    assert fine.triangles.shape == plain.triangles.shape and torch.equal(fine.triangles, plain.triangles)
    start, p = fine.refinement
    z0 = field_grad_planes(ds.decoder, fine.refine["planes"], start).logits
    assert start.shape[0] == plain.vertices.shape[0] and start.shape[0] > 32768      # more than one pass of the launch's grid
    assert bool((p.logits.abs() <= z0.abs()).all()) and bool((p.accepted > 0).any())
    assert torch.equal(field_grad_planes(ds.decoder, fine.refine["planes"], p.points).logits, p.logits)
    assert bool(((p.points - start).double().norm(dim=1) <= 2.0 / (res - 1) * (1 + 4 * U)).all())
    assert not torch.equal(fine.vertices, plain.vertices)
    print(f"DragStuff.refine at {res}^3: {start.shape[0]} vertices, {int((p.accepted > 0).sum())} moved, |z| <= {TOL} "
          f"{float((z0.abs() <= TOL).float().mean()):.3f} -> {float((p.logits.abs() <= TOL).float().mean()):.3f}, mean |z| "
          f"{float(z0.abs().mean()):.3e} -> {float(p.logits.abs().mean()):.3e}")
    both = ds.get_meshes(feat, t=0)
    assert len(both) == 2 and all(m.refine is not None for m in both) and torch.equal(both[0].vertices, fine.vertices)
    ds.refine = None
    assert torch.equal(ds.get_mesh(tri_feat=feat[:1]).vertices, plain.vertices)
