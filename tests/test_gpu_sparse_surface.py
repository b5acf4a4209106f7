"""The sparse high-resolution surface on the device (csrc/sparse_surface.hip, the brick instantiation of csrc/decode.hip,
mesh.extract_surface_sparse / SparseOccupancyMesh, DragStuff.mesh_resolution) against the parent's dense path at the same
resolution: decode_planes_grid + extract_surface.  Everything is compared bit for bit -- the brick decode runs the dense decode's
arithmetic per point and both surfaces compile one header of rules -- so there is no tolerance anywhere in this file.
Fixture: mesh_case()'s decoder and S = 8 planes (tests/test_gpu_field.py), a blobby multi-component field with the median logit
at 0.  Fine grids R = 33 and 41 (R - 1 a multiple of 8: the last node plane is the last brick's local index 8) and R = 30
(29 intervals: the last brick is partial and its upper samples are clamped duplicates).
info.rounds is compared nowhere for equality: the number of growth rounds depends on how a round's workgroups were scheduled
(only its lower bound, the brick distance from the seed, is asserted); the arrays, info.bricks and info.points do not."""
import copy
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import sparse_surface_ref as R
from tests.test_gpu_decoder_oracle import dev
from tests.test_gpu_field import mesh_case

pytestmark = pytest.mark.gpu
RES = (33, 41, 30)
RC = 12


def M():
    from ishapediting_amd import mesh
    return mesh


@lru_cache(maxsize=None)
def dense(res):
    """the parent's path at `res`: volume, mesh (device and numpy), the vertices' component labels"""
    from ishapediting_amd.triplane_decoder import decode_planes_grid
    dec, planes, _, _ = mesh_case()
    vol = decode_planes_grid(dec, planes, res)
    v, t = M().extract_surface(vol, 0.0)
    vn, tn = v.cpu().numpy(), t.cpu().numpy()
    assert vn.shape[0] > 1000 and tn.shape[0] > 1000
    # every vertex lies strictly inside its edge, so "the bricks whose closed box holds the vertex" are the bricks with a cell on that edge
    assert int(((vn == np.floor(vn)).sum(axis=1) == 2).sum()) == vn.shape[0]
    return vol, v, t, vn, tn, R.vertex_components(vn.shape[0], tn)


def sparse(res, seeds, **kw):
    dec, planes, _, _ = mesh_case()
    return M().extract_surface_sparse(dec, planes, res, seeds, **kw)


def brick_mask(res, coords):
    nb = R.bricks_per_axis(res)
    m = np.zeros((nb,) * 3, bool)
    for b in np.asarray(coords).reshape(-1, 3):
        m[tuple(b)] = True
    return m


def expected_from(res, mask):
    """the components of the dense mesh that cut a cell of a brick of `mask`, as a mesh"""
    _, _, _, vn, tn, lab = dense(res)
    keep = set(np.unique(lab[R.in_bricks(vn, res, mask)]).tolist())
    return R.select_components(vn, tn, lab, keep), keep


def assert_same(v, t, vn, tn, tag):
    a, b = R.sorted_vertex_rows(v.cpu().numpy()), R.sorted_vertex_rows(vn)
    assert a.shape == b.shape and np.array_equal(a, b), f"{tag}: vertex multisets differ ({a.shape[0]} vs {b.shape[0]})"
    ca, cb = R.canonical_triangles(v.cpu().numpy(), t.cpu().numpy()), R.canonical_triangles(vn, tn)
    assert ca.shape == cb.shape and np.array_equal(ca, cb), f"{tag}: triangle sets differ ({ca.shape[0]} vs {cb.shape[0]})"


@lru_cache(maxsize=None)
def brick_components(res):
    """{brick (bx, by, bz): set of component labels that cut one of its cells} of the dense mesh, and the largest component"""
    _, _, _, vn, _, lab = dense(res)
    lo, hi = R.vertex_bricks(vn, res)
    out = {}
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                b = np.stack([np.where(dx, hi[:, 0], lo[:, 0]), np.where(dy, hi[:, 1], lo[:, 1]), np.where(dz, hi[:, 2], lo[:, 2])], 1)
                for key, l in zip(map(tuple, b.tolist()), lab.tolist()):
                    out.setdefault(key, set()).add(l)
    labels, sizes = np.unique(lab, return_counts=True)
    return out, int(labels[np.argmax(sizes)])


@lru_cache(maxsize=None)
def far_seed(res):
    """a brick of the largest component that is at least 3 bricks (Chebyshev) from another brick of it: growth from it alone
    cannot finish in fewer than 3 rounds, a round reaching one brick further at the most"""
    bc, big = brick_components(res)
    mine = np.asarray(sorted(b for b, s in bc.items() if big in s))
    d = np.abs(mine[:, None, :] - mine[None, :, :]).max(axis=2).max(axis=1)
    k = int(np.argmax(d))
    assert int(d[k]) >= 3, "the fixture's largest component spans fewer than 4 bricks"
    return tuple(int(x) for x in mine[k])


# ------------------------------------------------------------------------------------------------ 1. decode parity
@pytest.mark.parametrize("res", RES)
def test_decode_bricks_is_the_dense_decode(res):
    from ishapediting_amd.triplane_decoder import decode_bricks
    dec, planes, _, _ = mesh_case()
    vol = dense(res)[0]
    nb = R.bricks_per_axis(res)
    perm = np.random.RandomState(res).permutation(nb ** 3 - 1)
    # 1, 3, 37 bricks; at R = 41 also all 125: 2848 tiles of 32 points, more than the launch's 256 workgroups x 8 waves, so the tile loop wraps
    for n in (1, 3, 37) + ((nb ** 3,) if res == 41 else ()):
        assert (729 * n) % 32 != 0
        ids = np.concatenate([perm[:n - 1], [nb ** 3 - 1]]).astype(np.int64)       # the last (clamped) brick is always there
        got = decode_bricks(dec, planes, res, torch.as_tensor(ids))
        assert tuple(got.shape) == (n, 9, 9, 9)
        for k, i in enumerate(ids.tolist()):
            bx, by, bz = i // (nb * nb), (i // nb) % nb, i % nb
            ix, iy, iz = (torch.as_tensor(R.brick_nodes(res, b), device=vol.device) for b in (bx, by, bz))
            want = vol[ix[:, None, None], iy[None, :, None], iz[None, None, :]]
            assert torch.equal(got[k], want), (res, n, k, i)
    assert tuple(decode_bricks(dec, planes, res, torch.zeros(0, dtype=torch.int32)).shape) == (0, 9, 9, 9)
    with pytest.raises(ValueError):
        decode_bricks(dec, planes, res, torch.as_tensor([nb ** 3]))
    with pytest.raises(ValueError):
        decode_bricks(dec, planes, 8, torch.as_tensor([0]))


# ------------------------------------------------------------------------------------------------ 2. seeds="all" is the dense mesh
@pytest.mark.parametrize("res", RES)
def test_all_seeds_equal_dense(res):
    _, _, _, vn, tn, _ = dense(res)
    v, t, info = sparse(res, "all")
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and v.is_cuda and t.is_cuda
    assert_same(v, t, vn, tn, f"R = {res}, all seeds")
    nb = R.bricks_per_axis(res)
    assert info.bricks == nb ** 3 and info.points == 729 * nb ** 3 and info.rounds >= 1 and info.bytes > 729 * 4 * nb ** 3
    print(f"R = {res}: {info.bricks} bricks, {info.rounds} rounds, {v.shape[0]} vertices, {t.shape[0]} triangles, {info.bytes} bytes")


@pytest.mark.parametrize("res", RES)
@pytest.mark.parametrize("shift", (-1e3, 1e3))
def test_empty_and_full(res, shift):
    from ishapediting_amd.triplane_decoder import MultiTriplane
    dec, planes, _, _ = mesh_case()
    sd = {k: v.clone() for k, v in dec.net.state_dict().items()}
    sd["5.bias"] = sd["5.bias"] + shift
    other = MultiTriplane(1, device=dev())
    other.net.load_state_dict(sd)
    v, t, info = M().extract_surface_sparse(other, planes, res, "all")
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and v.dtype == torch.float32 and t.dtype == torch.int32
    assert info.rounds == 0
    coarse = torch.full((RC, RC, RC), float(shift), device=dev())
    v, t, info = M().extract_surface_sparse(other, planes, res, coarse)
    assert tuple(v.shape) == (0, 3) and tuple(t.shape) == (0, 3) and info.bricks == 0


# ------------------------------------------------------------------------------------------------ 3. coarse and explicit seeds
def closed_except_in_box_faces(v, t, res):
    vn, tn = v.cpu().numpy(), t.cpu().numpy().astype(np.int64)
    e = np.concatenate([tn[:, [0, 1]], tn[:, [1, 2]], tn[:, [2, 0]]])
    e.sort(axis=1)
    edges, cnt = np.unique(e, axis=0, return_counts=True)
    odd = edges[cnt != 2]
    assert bool((cnt[cnt != 2] == 1).all())
    a, b = vn[odd[:, 0]], vn[odd[:, 1]]
    in_face = (((a == 0) & (b == 0)) | ((a == res - 1) & (b == res - 1))).any(axis=1)
    assert bool(in_face.all()), f"{int((~in_face).sum())} open edges inside the box"
    return len(edges), len(odd)


@pytest.mark.parametrize("res", RES)
def test_coarse_seeds(res):
    from ishapediting_amd.triplane_decoder import decode_planes_grid
    dec, planes, _, _ = mesh_case()
    coarse = decode_planes_grid(dec, planes, RC)
    mask = R.seed_map(coarse.cpu().numpy(), 0.0, res)
    assert mask.any()
    (ve, te), keep = expected_from(res, mask)
    v, t, info = sparse(res, coarse)
    assert_same(v, t, ve, te, f"R = {res}, coarse seeds")
    assert info.bricks >= int(mask.sum())
    nedges, nopen = closed_except_in_box_faces(v, t, res)
    print(f"R = {res}: {int(mask.sum())} seeded of {mask.size} bricks, {info.bricks} active after {info.rounds} rounds; {len(keep)} of "
          f"{len(set(dense(res)[5].tolist()))} components, {v.shape[0]} vertices; {nedges} edges, {nopen} in box faces")


def test_single_seed_grows():
    res = 41
    seed = far_seed(res)
    (ve, te), keep = expected_from(res, brick_mask(res, [seed]))
    v, t, info = sparse(res, torch.as_tensor([seed]))
    assert info.rounds >= 3, info
    assert info.bricks > 1
    assert_same(v, t, ve, te, f"R = {res}, seed {seed}")
    closed_except_in_box_faces(v, t, res)
    ncomp = len(set(dense(res)[5].tolist()))
    print(f"seed {seed}: {info.bricks} of {R.bricks_per_axis(res) ** 3} bricks after {info.rounds} rounds, {len(keep)} of {ncomp} components")


# ------------------------------------------------------------------------------------------------ 4. order and repeatability
def test_order_and_repeatability():
    res = 41
    bc, big = brick_components(res)
    seed = far_seed(res)
    a = sparse(res, torch.as_tensor([seed]))
    b = sparse(res, torch.as_tensor([seed]))
    # the arrays, the brick set and the points are a fixed point of the field; the number of rounds depends on scheduling
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert (a[2].bricks, a[2].points) == (b[2].bricks, b[2].points)
    some = sorted(bc)[::7][:9]
    one = sparse(res, torch.as_tensor(some))
    two = sparse(res, torch.as_tensor(some[::-1] + some[:4] + some))
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    alone = [bk for bk in sorted(bc) if bc[bk] == {big}]
    assert len(alone) >= 3, "the fixture has fewer than 3 bricks that the largest component cuts alone"
    ref = sparse(res, torch.as_tensor([alone[0]]))
    lab = dense(res)[5]
    assert ref[0].shape[0] == int((lab == big).sum())
    for other in (alone[len(alone) // 2], alone[-1]):
        got = sparse(res, torch.as_tensor([other]))
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), other
    all_a, all_b = sparse(30, "all"), sparse(30, "all")
    assert torch.equal(all_a[0], all_b[0]) and torch.equal(all_a[1], all_b[1])


# ------------------------------------------------------------------------------------------------ 5. limits
def test_limits_raise_and_leave_the_device_usable():
    res = 41
    seed = torch.as_tensor([far_seed(res)])
    with pytest.raises(RuntimeError, match="max_bricks = 1"):
        sparse(res, seed, max_bricks=1)
    with pytest.raises(RuntimeError, match="max_rounds = 1"):
        sparse(res, seed, max_rounds=1)
    with pytest.raises(RuntimeError, match="max_bricks = 5"):
        sparse(res, "all", max_bricks=5)
    with pytest.raises(ValueError):
        sparse(res, "everything")
    with pytest.raises(ValueError):
        sparse(res, torch.as_tensor([[0, 0, R.bricks_per_axis(res)]]))
    with pytest.raises(ValueError):
        sparse(2049, "all")
    v, t, info = sparse(res, seed)
    assert v.shape[0] > 0 and t.shape[0] > 0 and info.rounds >= 3
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6. the public path
def test_sparse_occupancy_mesh():
    from ishapediting_amd.triplane_decoder import field_grad_planes
    dec, planes, vol32, _ = mesh_case()
    res = 41
    v_all, t_all, _ = sparse(res, "all")
    # seeded from the dense volume at the same resolution every crossing cell is seen: test 2's arrays, in the same order
    m = M().SparseOccupancyMesh(dec, planes, res, dense(res)[0], smooth_iterations=0)
    assert torch.equal(m.vertices, v_all / res * 2 - 1) and torch.equal(m.triangles, t_all)
    assert m.counts() == (v_all.shape[0], t_all.shape[0]) and m.info.bricks <= R.bricks_per_axis(res) ** 3
    # seeded from the 32^3 volume: what extract_surface_sparse gives for those seeds, smoothed with the fine grid's box
    v32, t32, _ = sparse(res, vol32)
    m32 = M().SparseOccupancyMesh(dec, planes, res, vol32)
    assert m32.volume is vol32 and isinstance(m32, M().OccupancyMesh)
    assert torch.equal(m32.triangles, t32)
    assert torch.equal(m32.vertices, M().smooth_mesh(v32, t32, 10, box_max=float(res - 1)) / res * 2 - 1)
    assert not m32.has_vertex_normals() and m32.compute_vertex_normals().has_vertex_normals()
    c = copy.deepcopy(m32)
    assert isinstance(c, M().SparseOccupancyMesh) and torch.equal(c.vertices, m32.vertices) and torch.equal(c.triangles, m32.triangles)
    assert c.volume is not m32.volume and c.info == m32.info
    # refine: the existing projection, at most one FINE voxel; no vertex's |logit| rises
    fine = M().SparseOccupancyMesh(dec, planes, res, vol32, refine={"iterations": 4})
    assert torch.equal(fine.triangles, m32.triangles)
    start, p = fine.refinement
    assert torch.equal(start, M().smooth_mesh(v32, t32, 10, box_max=float(res - 1)) * 2 / (res - 1) - 1)
    z0 = field_grad_planes(dec, planes, start).logits
    assert bool((p.logits.abs() <= z0.abs()).all()) and bool((p.accepted > 0).any())
    assert bool(((p.points - start).double().norm(dim=1) <= 2.0 / (res - 1) * (1 + 4 * 2.0 ** -24)).all())
    assert not torch.equal(fine.vertices, m32.vertices)
    fine.compute_vertex_normals()
    has = (p.normals != 0).any(dim=1)
    assert torch.equal(fine._vnormals[has], p.normals[has])
    with pytest.raises(ValueError):
        M().SparseOccupancyMesh(dec, planes, 4096, vol32)
    with pytest.raises(ValueError):
        M().sparse_volume_to_mesh(dec, planes, res, vol32, backend="third_party")


# ------------------------------------------------------------------------------------------------ 7. the mesh reaches a file
def test_sparse_mesh_is_written(tmp_path, monkeypatch):
    """write_mesh (DragStuff's save paths) on a sparse mesh: the whole mesh as streamed OBJ text or binary PLY, never the dense
    path's stub, and an error naming the limit above the text limit"""
    mesh = M()
    dec, planes, vol32, _ = mesh_case()
    res = 41
    m = mesh.SparseOccupancyMesh(dec, planes, res, vol32)
    v, t = m.vertices.cpu().numpy(), m.triangles.cpu().numpy()
    assert v.shape[0] > 10000
    monkeypatch.setattr(mesh, "MAX_OBJ_VERTICES", 10)          # the dense stub's limit does not apply to a sparse mesh
    monkeypatch.setattr(mesh, "EXPORT_CHUNK", 1000)            # several chunks, the last one partial
    assert v.shape[0] % 1000 and t.shape[0] % 1000
    mesh.write_mesh(str(tmp_path / "m.obj"), m)
    vo, fo = mesh.read_obj(str(tmp_path / "m.obj"))
    assert vo.shape == v.shape and np.array_equal(fo, t)
    assert float(np.abs(vo - v).max()) <= 0.5e-6 + 2.0 ** -24   # six decimals of coordinates in [-1, 1], then float32
    mesh.write_mesh(str(tmp_path / "m.ply"), m)
    vp, fp = mesh.read_ply(str(tmp_path / "m.ply"))
    assert np.array_equal(vp.view(np.uint32), v.view(np.uint32)) and np.array_equal(fp, t)
    # one piece or chunks: the same bytes
    monkeypatch.setattr(mesh, "EXPORT_CHUNK", 1 << 18)
    mesh.write_mesh(str(tmp_path / "whole.obj"), m)
    assert (tmp_path / "whole.obj").read_bytes() == (tmp_path / "m.obj").read_bytes()
    monkeypatch.setattr(mesh, "MAX_SPARSE_OBJ_VERTICES", 100)
    with pytest.raises(RuntimeError, match="MAX_SPARSE_OBJ_VERTICES = 100"):
        mesh.write_mesh(str(tmp_path / "big.obj"), m)
    assert not (tmp_path / "big.obj").exists()
    mesh.write_mesh(str(tmp_path / "big.ply"), m)
    assert mesh.read_ply(str(tmp_path / "big.ply"))[0].shape == v.shape
    # the dense mesh keeps its behaviour: above MAX_OBJ_VERTICES a one-line stub
    mesh.write_mesh(str(tmp_path / "dense.obj"), mesh.OccupancyMesh(vol32, 32))
    assert (tmp_path / "dense.obj").read_text().startswith("#")


def test_generate_writes_the_sparse_mesh(tmp_path, monkeypatch):
    """generate.py --mesh_resolution: the option reaches visualize.main as `mesh_res`, and the file it writes per shape is the
    sparse surface at that resolution seeded from the --shape_resolution volume, in create_obj's convention"""
    from argparse import Namespace
    from ishapediting_amd import generate, visualize
    mesh = M()
    dec, planes, vol32, _ = mesh_case()
    a = generate.build_parser().parse_args(["--shape_resolution", "32", "--mesh_resolution", "41"])
    assert a.mesh_resolution == 41 and generate.build_parser().parse_args([]).mesh_resolution is None
    np.save(tmp_path / "0.npy", planes.permute(0, 3, 1, 2).contiguous().cpu().numpy())          # [3,32,S,S], what generate saves
    monkeypatch.setattr(mesh, "MAX_OBJ_VERTICES", 10)
    sd = dec.net.state_dict()
    args = Namespace(input=str(tmp_path / "0.npy"), output=str(tmp_path / "0.obj"), model_path=None, res=a.shape_resolution,
                     mesh_res=a.mesh_resolution)
    visualize.main(args=args, state_dict=sd)                    # the call generate.main makes per shape
    vo, fo = mesh.read_obj(str(tmp_path / "0.obj"))
    v, t, _ = sparse(41, vol32)
    want = (v / 40 * 2 - 1).cpu().numpy()
    assert vo.shape == want.shape and vo.shape[0] > 10000 and np.array_equal(fo, t.cpu().numpy())
    assert float(np.abs(vo - want).max()) <= 0.5e-6 + 2.0 ** -24
    # without the option (or not above res): the dense create_obj, as before
    args = Namespace(input=str(tmp_path / "0.npy"), output=str(tmp_path / "d.obj"), model_path=None, res=32, mesh_res=None)
    monkeypatch.setattr(mesh, "MAX_OBJ_VERTICES", 4_000_000)
    visualize.main(args=args, state_dict=sd)
    vd, _ = mesh.read_obj(str(tmp_path / "d.obj"))
    assert vd.shape[0] == mesh.extract_surface(vol32, 0.0)[0].shape[0]


def test_dragstuff_mesh_resolution():
    from ishapediting_amd import synthetic
    from ishapediting_amd.drag_utils import DragStuff
    from tests.helpers import small96_args, small96_config
    ds = DragStuff(dev(), args=small96_args(4, w_time=2, feat_layer=1, shape_resolution=32))
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(small96_config(), 202))
    ds.load_weights(sd, synthetic.decoder_state_dict(), -np.full(96, 1.5, np.float32), np.full(96, 0.5, np.float32))
    assert ds.mesh_resolution is None
    feat = torch.randn((1, 96, 16, 16), generator=torch.Generator().manual_seed(5)).to(dev())
    plain = ds.get_mesh(tri_feat=feat)
    vol = ds.volume.clone()
    assert type(plain) is M().OccupancyMesh and tuple(vol.shape) == (32, 32, 32)
    today = M().volume_to_mesh(vol, 32, smooth_iterations=10)
    assert torch.equal(plain.vertices, today.vertices) and torch.equal(plain.triangles, today.triangles)
    ds.mesh_resolution = 32                      # not above shape_resolution: the dense path
    same = ds.get_mesh(tri_feat=feat)
    assert type(same) is M().OccupancyMesh and torch.equal(same.vertices, plain.vertices)
    ds.mesh_resolution = 64
    fine = ds.get_mesh(tri_feat=feat)
    assert isinstance(fine, M().SparseOccupancyMesh) and fine.res == 64
    assert torch.equal(ds.volume, vol) and tuple(ds.volume.shape) == (32, 32, 32) and fine.volume is ds.volume
    assert fine.vertices.shape[0] > plain.vertices.shape[0] and fine.triangles.shape[0] > plain.triangles.shape[0]
    assert float(fine.vertices.abs().max()) <= 1.0
    print(f"DragStuff.mesh_resolution 64 on a 32^3 volume: {plain.vertices.shape[0]} -> {fine.vertices.shape[0]} vertices, "
          f"{fine.info.bricks} bricks, {fine.info.rounds} rounds")
    ds.refine = {"iterations": 2}
    both = ds.get_mesh(tri_feat=feat)
    assert isinstance(both, M().SparseOccupancyMesh) and both.refine is not None and both.vertices.shape == fine.vertices.shape
    ds.refine = None
    for bad in (4096, 8.5, True, 64 * 31 + 2):           # the last: too fine for a 32^3 seed volume
        ds.mesh_resolution = bad
        with pytest.raises(ValueError):
            ds.get_mesh(tri_feat=feat)
    ds.mesh_resolution = None
    assert torch.equal(ds.get_mesh(tri_feat=feat).vertices, plain.vertices)
