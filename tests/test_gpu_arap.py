"""As-rigid-as-possible deformation on the device (ishapediting_amd/deform.py, csrc/deform.hip: ishap_arap,
ishap_nearest_vertices) through the public functions.  Open3D is absent, so parity is pinned to the fp64 statement in
tests/arap_ref.py and to invariants of the method."""
import numpy as np
import pytest
import torch

from tests import arap_ref as R

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def diag(v):
    v = np.asarray(v, np.float64)
    return float(np.linalg.norm(v.max(axis=0) - v.min(axis=0)))


def smooth_field(res, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((1, 1, 5, 5, 5), generator=g)
    return torch.nn.functional.interpolate(f, size=(res, res, res), mode="trilinear", align_corners=True)[0, 0].contiguous()


def grid_mesh(vol, smooth=0):
    """marching-cubes mesh of a volume, vertices mapped to [-1, 1], optionally Laplacian-smoothed on the device"""
    from ishapediting_amd.mesh import extract_surface, smooth_mesh
    res = vol.shape[0]
    v, f = extract_surface(vol.to(dev()))
    v = (v / (res - 1) * 2 - 1).contiguous()
    if smooth:
        v = smooth_mesh(v, f, smooth).contiguous()
    return v, f


def far_static(v, handle_ids, dist):
    """vertices farther than `dist` from every handle vertex"""
    vt = torch.as_tensor(v, dtype=torch.float32)
    h = vt[torch.as_tensor(handle_ids, dtype=torch.long)]
    d = torch.cdist(vt.double(), h.double()).min(dim=1).values
    return torch.nonzero(d > dist).flatten().numpy()


def sphere_case():
    v, f = R.icosphere(3)                                      # 642 vertices
    order = np.argsort(v[:, 2])
    static, handles = order[:60], order[-5:]
    hp = v[handles] + np.array([0.2, -0.1, 0.15], np.float32)
    return v, f, static, handles, hp


def bar_case():
    v, f = R.bent_bar()                                        # 2 288 vertices
    static = np.nonzero(v[:, 0] < v[:, 0].min() + 0.1)[0]
    handles = np.nonzero(v[:, 0] > v[:, 0].max() - 0.03)[0]
    hp = v[handles] + np.array([0.0, 0.35, 0.1], np.float32)
    return v, f, static, handles, hp


def bar2048_case():
    """a bent bar of exactly 2 048 vertices: the scans of its nverts + 1 list lengths start a second block of one element"""
    v, f = R.bent_bar(n=(42, 12, 12))
    assert v.shape[0] == 2048
    static = np.nonzero(v[:, 0] < v[:, 0].min() + 0.1)[0]
    handles = np.nonzero(v[:, 0] > v[:, 0].max() - 0.03)[0]
    hp = v[handles] + np.array([0.0, 0.35, 0.1], np.float32)
    return v, f, static, handles, hp


def mc_case():
    v, f = grid_mesh(smooth_field(22, 11), smooth=5)
    v, f = v.cpu().numpy(), f.cpu().numpy()
    g = np.random.default_rng(5)
    handles = g.choice(v.shape[0], 3, replace=False)
    static = far_static(v, handles, 0.6)
    hp = v[handles] + np.array([0.06, 0.05, -0.04], np.float32)
    return v, f, static, handles, hp


CASES = {"icosphere": sphere_case, "bent_bar": bar_case, "marching_cubes": mc_case, "bar2048": bar2048_case}


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_fp64_statement(name):
    from ishapediting_amd.deform import deform_as_rigid_as_possible
    v, f, static, handles, hp = CASES[name]()
    if name == "marching_cubes":
        assert 1000 < v.shape[0] < 6000, v.shape
    ids = np.concatenate([static, handles])
    pos = np.concatenate([v[static], hp])
    scale = diag(v)
    for K in (1, 10, 50):
        x_ref, E_ref = R.arap(v, f, ids, pos, max_iter=K)
        out, info = deform_as_rigid_as_possible(torch.from_numpy(v).to(dev()), torch.from_numpy(f).to(dev()), ids, pos,
                                                max_iter=K, tol=1e-12)
        got = out.cpu().numpy().astype(np.float64)
        err = float(np.abs(got - x_ref).max())
        print(f"{name} K={K}: V={v.shape[0]} max dev {err:.2e} (diag {scale:.3f}), cg {info['cg_iters'].tolist()[:5]}...")
        assert err <= 1e-5 * scale, (K, err)
        np.testing.assert_allclose(info["energy"], E_ref, rtol=1e-6, atol=1e-12 * R.rest_energy_scale(v, f))
        assert info["converged"].all()
        assert np.array_equal(got[ids], pos.astype(np.float64))    # constraints bit for bit
    again, _ = deform_as_rigid_as_possible(torch.from_numpy(v).to(dev()), torch.from_numpy(f).to(dev()), ids, pos, max_iter=K, tol=1e-12)
    assert torch.equal(again, out)                                 # a repeat of the last call: the same bits


def test_invariants_exact_constraints_unconstrained_box_and_repeatability():
    from ishapediting_amd.deform import deform_as_rigid_as_possible
    v1, f1, static, handles, hp = sphere_case()
    v2, f2 = R.grid_box((5, 4, 6), (3.0, 3.0, 3.0), (3.5, 3.3, 3.6))
    v = np.concatenate([v1, v2])
    f = np.concatenate([f1, f2 + len(v1)])
    ids = np.concatenate([static, handles])
    pos = np.concatenate([v[static], hp])
    vt, ft = torch.from_numpy(v).to(dev()), torch.from_numpy(f).to(dev())
    a, ia = deform_as_rigid_as_possible(vt, ft, ids, pos, max_iter=20)
    b, ib = deform_as_rigid_as_possible(vt, ft, ids, pos, max_iter=20)
    assert torch.equal(a, b)
    assert np.array_equal(ia["energy"], ib["energy"]) and np.array_equal(ia["cg_iters"], ib["cg_iters"])
    assert torch.equal(a[len(v1):], vt[len(v1):])                   # the box holds no constraint: bit for bit at rest
    assert torch.equal(a[torch.from_numpy(ids).to(dev())], torch.from_numpy(pos).to(dev()))
    assert not torch.equal(a[:len(v1)], vt[:len(v1)])


def test_rigid_motion_equivariance():
    from ishapediting_amd.deform import deform_as_rigid_as_possible
    v, f, static, handles, hp = bar_case()
    ids = np.concatenate([static, handles])
    pos = np.concatenate([v[static], hp])
    Q, t = R.rigid(v, 12)
    vq = (v.astype(np.float64) @ Q.T + t).astype(np.float32)
    pq = (pos.astype(np.float64) @ Q.T + t).astype(np.float32)
    ft = torch.from_numpy(f).to(dev())
    a, _ = deform_as_rigid_as_possible(torch.from_numpy(v).to(dev()), ft, ids, pos, max_iter=10, tol=1e-12)
    b, _ = deform_as_rigid_as_possible(torch.from_numpy(vq).to(dev()), ft, ids, pq, max_iter=10, tol=1e-12)
    want = a.cpu().numpy().astype(np.float64) @ Q.T + t
    err = float(np.abs(b.cpu().numpy() - want).max())
    assert err <= 1e-5 * diag(v), err


def test_full_size_sphere():
    """The 256^3 sphere's marching-cubes mesh, four handles near the +z pole moved by 0.1, static beyond 0.5 of them, 50
    iterations at the default tol."""
    from ishapediting_amd.deform import deform_as_rigid_as_possible, nearest_vertices
    res, r = 256, 90.4
    ax = torch.arange(res, dtype=torch.float32) - (res - 1) / 2
    vol = r - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    v, f = grid_mesh(vol)
    assert v.shape[0] > 100_000
    picks = torch.tensor([[0.0, 0.0, 0.75], [0.25, 0.0, 0.7], [0.0, 0.25, 0.7], [-0.2, -0.2, 0.7]])
    handles = torch.unique(nearest_vertices((v, f), picks)).cpu().numpy()
    static = far_static(v.cpu(), handles, 0.5)
    ids = np.concatenate([static, handles])
    vc = v.cpu().numpy()
    pos = np.concatenate([vc[static], vc[handles] + np.array([0.1, 0.0, 0.0], np.float32)])
    out, info = deform_as_rigid_as_possible(v, f, ids, pos, max_iter=50)
    it, E = info["cg_iters"], info["energy"]
    free = v.shape[0] - len(ids)
    print(f"full size: V={v.shape[0]} F={f.shape[0]} free={free} cg/iter first {it[:3].tolist()} last {it[-3:].tolist()} "
          f"E {E[0]:.4e} -> {E[-1]:.4e}")
    assert info["converged"].all() and it.max() < 4 * free + 100
    assert np.all(E[1:] <= E[:-1] * (1 + 1e-6))
    assert E[-1] < E[0]
    assert torch.equal(out[torch.from_numpy(ids).to(dev())], torch.from_numpy(pos).to(dev()))
    assert torch.isfinite(out).all()


def test_nearest_vertices_against_brute_force_with_ties():
    from ishapediting_amd.deform import nearest_vertices
    g = torch.Generator().manual_seed(3)
    v = torch.rand((5000, 3), generator=g) * 2 - 1
    p = torch.rand((3000, 3), generator=g) * 2.4 - 1.2
    d = ((p.double()[:, None, :] - v.double()[None]) ** 2).sum(-1)
    want = d.argmin(dim=1)
    got = nearest_vertices((v.to(dev()), torch.zeros((1, 3), dtype=torch.int32, device=dev())), p.to(dev())).cpu()
    top2 = d.topk(2, dim=1, largest=False).values
    clear = (top2[:, 1] - top2[:, 0]) > 1e-12 * top2[:, 1]
    assert clear.sum() > 2900
    assert torch.equal(got[clear], want[clear])
    assert torch.equal(d[torch.arange(3000), got], d[torch.arange(3000), want])          # same distance everywhere
    # exact ties: integer lattice vertices (some listed twice), points at half-integers equidistant from several
    lat = torch.stack(torch.meshgrid(*[torch.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    vt = torch.cat([lat[torch.randperm(lat.shape[0], generator=g)], lat[:50]])
    pt = torch.cat([lat + 0.5, lat[:100], torch.randint(0, 11, (400, 3), generator=g).float() / 2])
    dt = ((pt.double()[:, None, :] - vt.double()[None]) ** 2).sum(-1)
    got = nearest_vertices((vt.to(dev()), torch.zeros((1, 3), dtype=torch.int32, device=dev())), pt.to(dev())).cpu()
    assert torch.equal(got, dt.argmin(dim=1))                  # torch.argmin: the first minimum, the lowest index


def test_drag_edit_comparison_flow(tmp_path):
    """get_mesh's decode and surface (drag_utils.py:453-455) on synthetic weights, handles from nearest_vertices of the drag
    sources moved to the targets, arap, then meshProcess's local distance between the two shapes."""
    from ishapediting_amd import synthetic
    from ishapediting_amd.deform import arap, nearest_vertices
    from ishapediting_amd.mesh import read_obj, volume_to_mesh
    from ishapediting_amd.metrics import calc_local_distance, device_mesh
    from ishapediting_amd.triplane_decoder import MultiTriplane, decode_volume
    res = 48
    dec = MultiTriplane(1, device=dev())
    dec.net.load_state_dict(synthetic.decoder_state_dict())
    lat = torch.from_numpy(synthetic.latent(0, size=64)) * 0.5
    vol = decode_volume(dec, lat.to(dev()), 1.0, 0.0, res)
    mesh = volume_to_mesh(vol, res, smooth_iterations=10)
    v, t = device_mesh(mesh)
    assert v.shape[0] > 100
    src, tgt = synthetic.handles(3, seed=7)
    hid = nearest_vertices(mesh, src).cpu().numpy()
    hid = np.unique(hid)
    hp = v[torch.from_numpy(hid).to(dev())].cpu().numpy() + (tgt - src)[:len(hid)]
    static = far_static(v.cpu(), hid, 0.5)
    path = str(tmp_path / "arap.obj")
    nv, nt = arap(mesh, static.tolist(), hid.tolist(), hp, max_iter=10, path=path)
    assert torch.equal(nt, t) and nv.shape == v.shape
    assert torch.equal(nv[torch.from_numpy(hid).to(dev())], torch.from_numpy(hp.astype(np.float32)).to(dev()))
    assert torch.equal(nv[torch.from_numpy(static).to(dev())], v[torch.from_numpy(static).to(dev())])
    rv, rt = read_obj(path)
    assert rv.shape == tuple(v.shape) and rt.shape == tuple(t.shape)
    ha = v[torch.from_numpy(hid).to(dev())]
    hb = nv[torch.from_numpy(hid).to(dev())]
    for metric in ("IoU", "L2"):
        val = calc_local_distance(mesh, (nv, nt), ha, hb, 0.1, 2000, metric)
        assert isinstance(val, float)
