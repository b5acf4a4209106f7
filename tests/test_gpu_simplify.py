"""Quadric vertex clustering on the device (csrc/simplify.hip, mesh.simplify_vertex_clustering, the `simplify` keyword of the mesh
classes, DragStuff.mesh_simplify) against the float64 numpy restatement of the rule (tests/simplify_ref.py).
Exact parts -- the cluster of every input vertex (the partition, return_clusters=True), the vertex map, the number of clusters,
the triangle array and SimplifyInfo -- are compared with ==.  Positions: contraction "average" within one
float32 ulp, singleton clusters bit for bit, quadric positions within the bound the reference derives per cluster (each of the
n_c rounded contributions off by at most one unit of 2^-36 moves x by at most 4 n_c 2^-36 (|x|_1 + 1) / (lambda tr) cell
units) plus one float32 ulp of the output coordinate; no cluster is excluded.
Fixture: max(torus, sphere, slab) on linspace(-1, 1, R)^3, R = 33 and 41, meshed by mesh.extract_surface at level 0."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import simplify_ref as R
from tests.test_gpu_decoder_oracle import dev, put

pytestmark = pytest.mark.gpu
CELLS = (0.75, 2, 3.3, 4, 8)
ODD = ((-0.37, 0.41, 1.23), 2.7)          # a non-zero origin that no voxel plane meets, and its cell size


def M():
    from ishapediting_amd import mesh
    return mesh


@lru_cache(maxsize=None)
def fixture(res):
    v, t = M().extract_surface(put(R.fixture_volume(res)), 0.0)
    assert v.shape[0] > 2000 and t.shape[0] > 5000
    return v, t, v.cpu().numpy(), t.cpu().numpy()


def grid_for(res, cell, origin):
    lo = np.asarray(origin, np.float64)
    return lo, [int(d) for d in np.floor(((res - 1) - lo) / cell).astype(np.int64) + 1]


def device_run(v, t, cell, contraction, lo, dims, **kw):
    return M().simplify_vertex_clustering(v, t, cell, contraction, origin=None if lo is None else tuple(lo), dims=dims,
                                          return_map=True, return_clusters=True, **kw)


@lru_cache(maxsize=None)
def case(res, cell, contraction, odd=False):
    """(device outputs as numpy + info, the reference) of one fixture / cell pair, computed once"""
    v, t, vn, tn = fixture(res)
    origin, h = (ODD[0], ODD[1]) if odd else ((0.0, 0.0, 0.0), cell)
    lo, dims = grid_for(res, h, origin)
    ov, ot, info, vmap, vclus = device_run(v, t, h, contraction, lo, dims)
    return (ov.cpu().numpy(), ot.cpu().numpy(), info, vmap.cpu().numpy(), vclus.cpu().numpy()), R.simplify(vn, tn, lo, h, dims, contraction), h


def assert_exact(got, ref, nv, nt, tag):
    ov, ot, info, vmap, vclus = got
    assert ot.dtype == np.int32 and vmap.dtype == np.int32 and ov.dtype == np.float32 and vclus.dtype == np.int32
    assert np.array_equal(vclus, ref.cluster), (tag, int((vclus != ref.cluster).sum()))       # the cluster partition itself
    assert info.clusters == len(ref.cells), (tag, info.clusters, len(ref.cells))
    assert (info.vertices_in, info.vertices_out, info.triangles_in, info.triangles_nondegenerate, info.triangles_out) == \
        (nv, ref.verts.shape[0], nt, ref.nondegenerate, ref.tris.shape[0]), (tag, info)
    assert info.bytes > 0 and ov.shape == ref.verts.shape and ot.shape == ref.tris.shape
    assert np.array_equal(vmap, ref.vertex_map), (tag, int((vmap != ref.vertex_map).sum()))
    assert np.array_equal(ot, ref.tris), (tag, int((ot != ref.tris).any(axis=1).sum()))


def assert_positions(got, ref, h, contraction, tag):
    ov = got[0]
    counts, bound = ref.counts[ref.referenced], ref.bound[ref.referenced]
    single = counts == 1
    assert np.array_equal(ov[single].view(np.uint32), ref.verts[single].view(np.uint32)), tag
    ulp = np.spacing(np.maximum(np.abs(ov), np.abs(ref.verts))).astype(np.float64)
    err = np.abs(ov.astype(np.float64) - ref.verts.astype(np.float64))
    allow = ulp if contraction == "average" else bound[:, None] * h + ulp
    worst = float((err / allow).max()) if len(err) else 0.0
    print(f"{tag}: {len(err)} vertices ({int(single.sum())} singletons), worst |dx| / allowed = {worst:.3f}, "
          f"largest bound {float(bound.max()) if len(bound) else 0:.2e} cell units")
    assert (err <= allow).all(), (tag, worst)


# ------------------------------------------------------------------------------------------------ 1, 2: exact parts and positions
@pytest.mark.parametrize("contraction", ["quadric", "average"])
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("res", [33, 41])
def test_fixture_matches_reference(res, cell, contraction):
    got, ref, h = case(res, cell, contraction)
    nv, nt = fixture(res)[2].shape[0], fixture(res)[3].shape[0]
    tag = f"R={res} cell={cell} {contraction}"
    assert_exact(got, ref, nv, nt, tag)
    assert_positions(got, ref, h, contraction, tag)
    if (res, cell) == (33, 4):                   # the unreferenced-cluster path: a cluster that no kept triangle touches
        assert got[2].clusters == got[2].vertices_out + 1 and int((got[3] < 0).sum()) > 0
    if cell == 0.75:                             # mostly singleton clusters
        assert int((ref.counts == 1).sum()) > len(ref.cells) // 2
    # a representative never leaves its cell
    g = grid_for(res, h, (0.0, 0.0, 0.0))[1][0]
    cc = np.stack([ref.cells // (g * g), (ref.cells // g) % g, ref.cells % g], 1)[ref.referenced].astype(np.float64)
    ulp = np.spacing(np.abs(got[0])).astype(np.float64)
    assert (got[0] >= cc * h - ulp).all() and (got[0] <= (cc + 1) * h + ulp).all()


@pytest.mark.parametrize("contraction", ["quadric", "average"])
@pytest.mark.parametrize("res", [33, 41])
def test_odd_origin_and_default_grid(res, contraction):
    got, ref, h = case(res, 0, contraction, odd=True)
    v, t, vn, tn = fixture(res)
    assert_exact(got, ref, vn.shape[0], tn.shape[0], f"R={res} odd origin {contraction}")
    assert_positions(got, ref, h, contraction, f"R={res} odd origin {contraction}")
    # origin and dims left to the default: the bounding box's low corner as float64, floor((max - lo) / cell) + 1 cells
    lo, dims = R.default_grid(vn, 2.5)
    ov, ot, info, vmap, vclus = device_run(v, t, 2.5, contraction, None, None)
    ref = R.simplify(vn, tn, lo, 2.5, dims, contraction)
    got = (ov.cpu().numpy(), ot.cpu().numpy(), info, vmap.cpu().numpy(), vclus.cpu().numpy())
    assert_exact(got, ref, vn.shape[0], tn.shape[0], f"R={res} default grid {contraction}")
    assert_positions(got, ref, 2.5, contraction, f"R={res} default grid {contraction}")


# ------------------------------------------------------------------------------------------------ 3: order independence
def rows_sorted(a):
    b = np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1) if a.dtype == np.float32 else np.asarray(a)
    return b[np.lexsort(b.T[::-1])]


@pytest.mark.parametrize("contraction", ["quadric", "average"])
def test_order_independence_and_repeatability(contraction):
    v, t, vn, tn = fixture(33)
    lo, dims = grid_for(33, 2.0, (0.0, 0.0, 0.0))
    base = device_run(v, t, 2.0, contraction, lo, dims)
    again = device_run(v, t, 2.0, contraction, lo, dims)
    for a, b in zip((base[0], base[1], base[3]), (again[0], again[1], again[3])):
        assert torch.equal(a, b)
    assert base[2] == again[2]
    g = torch.Generator().manual_seed(11)
    pt = torch.randperm(t.shape[0], generator=g).to(dev())
    tri_perm = device_run(v, t[pt].contiguous(), 2.0, contraction, lo, dims)
    pv = torch.randperm(v.shape[0], generator=g).to(dev())          # new vertex k is old vertex pv[k]
    inv = torch.empty_like(pv)
    inv[pv] = torch.arange(v.shape[0], device=dev())
    vert_perm = device_run(v[pv].contiguous(), inv[t.long()].to(torch.int32).contiguous(), 2.0, contraction, lo, dims)
    for name, other in (("triangles permuted", tri_perm), ("vertices permuted", vert_perm)):
        assert np.array_equal(rows_sorted(other[0].cpu().numpy()), rows_sorted(base[0].cpu().numpy())), name      # bitwise, as a multiset
        assert np.array_equal(rows_sorted(other[1].cpu().numpy()), rows_sorted(base[1].cpu().numpy())), name      # rotated triples, as a set
        assert other[2][:6] == base[2][:6], name
    assert torch.equal(tri_perm[3], base[3]) and torch.equal(vert_perm[3], base[3][pv])
    assert torch.equal(vert_perm[1], base[1])    # the same triangles in the same input order: the same array


# ------------------------------------------------------------------------------------------------ 4: duplicates and probing
def test_duplicates_and_probing():
    rng = np.random.default_rng(3)
    g, ndup, ndistinct = 12, 5000, 3000
    centres = np.stack(np.meshgrid(*[np.arange(g) + 0.5] * 3, indexing="ij"), -1).reshape(-1, 3)
    base = centres + rng.uniform(-0.45, 0.45, centres.shape)                       # vertex k lies in cell k
    A, B, C_ = 5, 700, 1300                                                       # the three cells of the repeated triple
    dup = np.concatenate([c + rng.uniform(-0.45, 0.45, (ndup, 3)) for c in (centres[A], centres[B], centres[C_])])
    verts = np.concatenate([base, dup]).astype(np.float32)
    n0 = len(base)
    k = np.arange(ndup)
    dup_t = np.stack([n0 + k, n0 + ndup + k, n0 + 2 * ndup + k], 1)
    dup_t = np.take_along_axis(dup_t, (rng.integers(0, 3, ndup)[:, None] + np.arange(3)[None]) % 3, 1)      # any rotation, one orientation
    rev_t = np.array([[n0 + 7, n0 + 2 * ndup + 9, n0 + ndup + 11]])                 # the same three cells the other way round
    others = np.stack([rng.permutation(g ** 3)[:3] for _ in range(ndistinct)])
    others = others[~np.isin(others, (A, B, C_)).all(axis=1)]
    tris = np.concatenate([dup_t, rev_t, others])
    tris = tris[rng.permutation(len(tris))]                                        # shuffled input order
    ref = R.simplify(verts, tris, (0, 0, 0), 1.0, (g, g, g), "average")
    ov, ot, info, vmap, vclus = device_run(put(verts), put(tris, torch.int32), 1.0, "average", (0.0, 0.0, 0.0), [g, g, g])
    got = (ov.cpu().numpy(), ot.cpu().numpy(), info, vmap.cpu().numpy(), vclus.cpu().numpy())
    assert_exact(got, ref, len(verts), len(tris), "duplicates")
    assert_positions(got, ref, 1.0, "average", "duplicates")
    ndistinct_keys = len(np.unique(R.rotate(ref.cluster[others]), axis=0))
    assert info.triangles_nondegenerate == len(tris) and info.triangles_out == ndistinct_keys + 2 and ndistinct_keys > 2900
    key = tuple(int(vmap[i]) for i in (n0, n0 + ndup, n0 + 2 * ndup))              # (A, B, C) as output vertices, A the smallest
    rows = [tuple(r) for r in got[1].tolist()]
    assert rows.count(key) == 1 and rows.count((key[0], key[2], key[1])) == 1
    # only the lowest input index of the 5000 survives: the output keeps the input order, so the triple stands where the first of
    # them stood among the survivors
    is_dup = (ref.cluster[tris] == np.array([A, B, C_])[None]).all(axis=1) | (ref.cluster[tris] == np.array([B, C_, A])[None]).all(axis=1) | \
        (ref.cluster[tris] == np.array([C_, A, B])[None]).all(axis=1)
    first = int(np.nonzero(is_dup)[0][0])
    assert rows.index(key) == len(set(tuple(r) for r in R.rotate(ref.cluster[tris[:first]]).tolist())), first


# ------------------------------------------------------------------------------------------------ 5: tails and limits
@pytest.mark.parametrize("V", [3, 63, 64, 65, 257])
def test_tails(V):
    rng = np.random.default_rng(100 + V)
    verts = rng.uniform(0.0, 3.0, (V, 3)).astype(np.float32)
    for F in (1, 255, 256, 257):
        tris = np.stack([rng.permutation(V)[:3] for _ in range(F)])
        for contraction in ("quadric", "average"):
            ref = R.simplify(verts, tris, (0, 0, 0), 1.0, (3, 3, 3), contraction)
            ov, ot, info, vmap, vclus = device_run(put(verts), put(tris, torch.int32), 1.0, contraction, (0.0, 0.0, 0.0), [3, 3, 3])
            got = (ov.cpu().numpy(), ot.cpu().numpy(), info, vmap.cpu().numpy(), vclus.cpu().numpy())
            assert_exact(got, ref, V, F, f"V={V} F={F} {contraction}")
            assert_positions(got, ref, 1.0, contraction, f"V={V} F={F} {contraction}")


@pytest.mark.parametrize("dims", [(41, 41, 41), (64, 64, 64), (65, 64, 64)])
def test_bitmap_words_across_scan_blocks(dims):
    """41^3 cells = 2154 words (crosses one scan block of 2048), 64^3 = 8192 words (fills four exactly), 65 x 64 x 64 = 8320"""
    v, t, vn, tn = fixture(41)
    h = 40.0 / 64 if dims[1] == 64 else 1.0
    ref = R.simplify(vn, tn, (0, 0, 0), h, dims, "quadric")
    ov, ot, info, vmap, vclus = device_run(v, t, h, "quadric", (0.0, 0.0, 0.0), list(dims))
    got = (ov.cpu().numpy(), ot.cpu().numpy(), info, vmap.cpu().numpy(), vclus.cpu().numpy())
    assert_exact(got, ref, vn.shape[0], tn.shape[0], f"dims {dims}")
    assert_positions(got, ref, h, "quadric", f"dims {dims}")


def test_cell_limit_and_empty():
    g = 1024                                     # 2^30 cells: the first and the last cell id
    verts = np.array([[0.2, 0.3, 0.4], [1023.5, 1023.25, 1023.75], [511.5, 3.5, 900.25], [0.7, 0.6, 0.1], [1023.1, 1023.9, 1023.2],
                      [2000.0, 1500.0, 1023.5], [-5.0, 0.5, 0.5]], np.float32)
    tris = np.array([[0, 1, 2], [3, 4, 2], [0, 2, 1], [5, 6, 2], [0, 3, 2]])
    for contraction in ("quadric", "average"):
        ref = R.simplify(verts, tris, (0, 0, 0), 1.0, (g, g, g), contraction)
        assert ref.cells[0] == 0 and ref.cells[-1] == (1 << 30) - 1 and ref.tris.shape[0] == 2
        ov, ot, info, vmap, vclus = device_run(put(verts), put(tris, torch.int32), 1.0, contraction, (0.0, 0.0, 0.0), [g, g, g])
        got = (ov.cpu().numpy(), ot.cpu().numpy(), info, vmap.cpu().numpy(), vclus.cpu().numpy())
        assert_exact(got, ref, len(verts), len(tris), f"1024^3 {contraction}")
        assert_positions(got, ref, 1.0, contraction, f"1024^3 {contraction}")
    with pytest.raises(ValueError):
        device_run(put(verts), put(tris, torch.int32), 1.0, "quadric", (0.0, 0.0, 0.0), [1025, 1024, 1024])
    # all vertices in one cell: an empty mesh
    v, t, vn, tn = fixture(33)
    ov, ot, info, vmap, vclus = device_run(v, t, 64.0, "quadric", (0.0, 0.0, 0.0), [1, 1, 1])
    assert ov.shape == (0, 3) and ot.shape == (0, 3) and bool((vmap == -1).all()) and vmap.shape[0] == vn.shape[0]
    assert (info.clusters, info.vertices_out, info.triangles_nondegenerate, info.triangles_out) == (1, 0, 0, 0)
    assert bool((vclus == 0).all()) and vclus.shape[0] == vn.shape[0]
    # no triangles, no vertices
    ov, ot, info, vmap, vclus = device_run(v, t[:0], 2.0, "quadric", None, None)
    assert ov.shape == (0, 3) and ot.shape == (0, 3) and bool((vmap == -1).all()) and info.triangles_in == 0
    assert bool((vclus == -1).all()) and vclus.shape[0] == vn.shape[0]       # nothing ran: no partition either
    ov, ot, info, vmap, vclus = device_run(v[:0], t[:0], 2.0, "quadric", None, None)
    assert ov.shape == (0, 3) and vmap.shape == (0,)


# ------------------------------------------------------------------------------------------------ 6: the overflow guard
def test_guard():
    """a fan through one vertex of cell 0 whose sum ceil(w) is 2^26 - 1: seven triangles of w = 2^23 and one of w = 2^23 - 1 (legs
    4096 and 4096 - 2^-11 cell units, all exact in float32); one more triangle of ceil(w) = 1 reaches 2^26 and the call raises"""
    S = 4096.0
    verts = [[0.5, 0.5, 0.5]]
    tris = []
    for k in range(8):
        leg = S - (2.0 ** -11 if k == 7 else 0.0)
        verts += [[0.5 + S, 0.5 + 0.01 * k, 0.5], [0.5, 0.5 + leg, 0.5 + 0.0]]
        tris.append([0, 1 + 2 * k, 2 + 2 * k])
    verts, tris = np.array(verts, np.float32), np.array(tris)
    # the far vertices of triangle k differ, its area does not: (S, 0.01 k, 0) x (0, leg, 0) = (0, 0, S leg), exact in float64
    ref = R.simplify(verts, tris, (0, 0, 0), 1.0, (2, 2, 2), "quadric")
    total = int(ref.sums[0, 15])
    assert ref.referenced[0] and (1 << 26) - 64 <= total < 1 << 26, total
    # top the fan up to exactly 2^26 - 1 with small triangles of ceil(w) = 1 through the same vertex (legs 1 x 1: w = 0.5)
    small_v, small_t = [], []
    for k in range((1 << 26) - 1 - total + 1):
        n = len(verts) + len(small_v)
        small_v += [[1.5, 0.5 + 0.001 * k, 0.5], [0.5, 1.5, 0.5 + 0.001 * k]]
        small_t.append([0, n, n + 1])
    below_v = np.concatenate([verts, np.array(small_v[:-2], np.float32).reshape(-1, 3)])
    below_t = np.concatenate([tris, np.array(small_t[:-1], np.int64).reshape(-1, 3)])
    ref = R.simplify(below_v, below_t, (0, 0, 0), 1.0, (2, 2, 2), "quadric")
    assert int(ref.sums[0, 15]) == (1 << 26) - 1
    ov, ot, info, vmap, vclus = device_run(put(below_v), put(below_t, torch.int32), 1.0, "quadric", (0.0, 0.0, 0.0), [2, 2, 2])
    got = (ov.cpu().numpy(), ot.cpu().numpy(), info, vmap.cpu().numpy(), vclus.cpu().numpy())
    assert_exact(got, ref, len(below_v), len(below_t), "guard, just below")
    assert_positions(got, ref, 1.0, "quadric", "guard, just below")
    over_v = np.concatenate([verts, np.array(small_v, np.float32)])
    over_t = np.concatenate([tris, np.array(small_t, np.int64)])
    with pytest.raises(R.Overflow):
        R.simplify(over_v, over_t, (0, 0, 0), 1.0, (2, 2, 2), "quadric")
    with pytest.raises(RuntimeError, match="overflow"):
        device_run(put(over_v), put(over_t, torch.int32), 1.0, "quadric", (0.0, 0.0, 0.0), [2, 2, 2])
    # the same mesh has no quadric to overflow with the average
    ref = R.simplify(over_v, over_t, (0, 0, 0), 1.0, (2, 2, 2), "average")
    ov, ot, info, vmap, vclus = device_run(put(over_v), put(over_t, torch.int32), 1.0, "average", (0.0, 0.0, 0.0), [2, 2, 2])
    assert_exact((ov.cpu().numpy(), ot.cpu().numpy(), info, vmap.cpu().numpy(), vclus.cpu().numpy()), ref, len(over_v), len(over_t), "guard, average")


# ------------------------------------------------------------------------------------------------ 7: integration
def test_occupancy_mesh_simplify():
    import copy
    from ishapediting_amd.triplane_decoder import field_grad_planes
    from tests.test_gpu_field import mesh_case
    dec, planes, vol, _ = mesh_case()
    res = int(vol.shape[0])
    plain = M().OccupancyMesh(vol, res)
    off = M().OccupancyMesh(vol, res, simplify=None)
    assert torch.equal(off.vertices, plain.vertices) and torch.equal(off.triangles, plain.triangles) and off.simplification is None
    same = M().volume_to_mesh(vol, res, simplify=None)
    assert torch.equal(same.vertices, plain.vertices) and torch.equal(same.triangles, plain.triangles)
    # {"cell": 2}: the smoothed mesh in grid units, origin 0, cells of two voxels
    sv, st = M().extract_surface(vol, 0.0)
    sv = M().smooth_mesh(sv, st, 10, box_max=float(res - 1))
    g = (res - 1) // 2 + 1
    ref = R.simplify(sv.cpu().numpy(), st.cpu().numpy(), (0, 0, 0), 2.0, (g, g, g), "quadric")
    m = M().OccupancyMesh(vol, res, simplify={"cell": 2})
    assert m.vertices.shape[0] == ref.verts.shape[0] and m.triangles.shape[0] == ref.tris.shape[0]
    assert 0 < m.vertices.shape[0] < plain.vertices.shape[0]
    info = m.simplification
    assert (info.clusters, info.vertices_in, info.triangles_in, info.triangles_nondegenerate) == \
        (len(ref.cells), sv.shape[0], st.shape[0], ref.nondegenerate)
    assert np.array_equal(m.triangles.cpu().numpy(), ref.tris)
    ov, ot, _, vmap = M().simplify_vertex_clustering(sv, st, 2.0, origin=(0.0, 0.0, 0.0), dims=[g, g, g], return_map=True)
    assert torch.equal(m.vertices, ov / res * 2 - 1) and torch.equal(m.triangles, ot)
    has = vmap >= 0
    gap = (sv[has].double() - ov[vmap[has].long()].double()).abs()
    ulp = torch.from_numpy(np.spacing(ov.cpu().numpy())).to(dev()).double()[vmap[has].long()]
    assert bool((gap <= 2.0 + ulp).all()), float(gap.max())
    assert np.array_equal(vmap.cpu().numpy(), ref.vertex_map)
    c = copy.deepcopy(m)
    assert c.simplify == {"cell": 2.0} and c.simplification == info and torch.equal(c.vertices, m.vertices)
    via = M().volume_to_mesh(vol, res, simplify=2)
    assert torch.equal(via.vertices, m.vertices) and torch.equal(via.triangles, m.triangles)
    with pytest.raises(ValueError):
        M().volume_to_mesh(vol, res, backend="third_party", simplify=2)
    # with refine as well: the fewer, moved vertices go back on the level set; no |logit| rises; normals per output vertex
    fine = M().OccupancyMesh(vol, res, refine={"decoder": dec, "planes": planes, "iterations": 4}, simplify={"cell": 2})
    assert torch.equal(fine.triangles, m.triangles)
    start, p = fine.refinement
    assert torch.equal(start, ov * 2 / (res - 1) - 1)
    z0 = field_grad_planes(dec, planes, start).logits
    assert bool((p.logits.abs() <= z0.abs()).all()) and bool((p.accepted > 0).any())
    assert float(p.logits.abs().mean()) < float(z0.abs().mean())
    fine.compute_vertex_normals()
    assert fine._vnormals.shape == fine.vertices.shape
    # the sparse mesh takes the same keyword, cells in FINE voxels
    sp = M().SparseOccupancyMesh(dec, planes, 41, vol, simplify={"cell": 2, "contraction": "average"})
    full = M().SparseOccupancyMesh(dec, planes, 41, vol)
    assert 0 < sp.vertices.shape[0] < full.vertices.shape[0] and sp.simplification.vertices_in == full.vertices.shape[0]
    assert copy.deepcopy(sp).simplify == sp.simplify


def test_dragstuff_mesh_simplify():
    from ishapediting_amd import synthetic
    from ishapediting_amd.drag_utils import DragStuff
    from tests.helpers import small96_args, small96_config
    ds = DragStuff(dev(), args=small96_args(4, w_time=2, feat_layer=1, shape_resolution=32))
    sd = synthetic.round_torso_to_fp16(synthetic.unet_state_dict(small96_config(), 202))
    ds.load_weights(sd, synthetic.decoder_state_dict(), -np.full(96, 1.5, np.float32), np.full(96, 0.5, np.float32))
    assert ds.mesh_simplify is None
    feat = torch.randn((1, 96, 16, 16), generator=torch.Generator().manual_seed(5)).to(dev())
    plain = ds.get_mesh(tri_feat=feat)
    assert plain.simplify is None and plain.simplification is None
    ds.mesh_simplify = 2
    small = ds.get_mesh(tri_feat=feat)
    direct = M().volume_to_mesh(ds.volume, 32, smooth_iterations=10, simplify={"cell": 2})
    assert small.simplify == {"cell": 2.0} and torch.equal(small.vertices, direct.vertices) and torch.equal(small.triangles, direct.triangles)
    assert 0 < small.vertices.shape[0] < plain.vertices.shape[0] and small.simplification.vertices_in == plain.vertices.shape[0]
    ds.mesh_resolution = 64
    fine = ds.get_mesh(tri_feat=feat)
    assert isinstance(fine, M().SparseOccupancyMesh) and fine.simplify == {"cell": 2.0} and fine.simplification is None
    nfine = fine.vertices.shape[0]               # the mesh is built on first use
    assert fine.simplification.vertices_out == nfine and fine.simplification.vertices_in > small.simplification.vertices_in
    ds.mesh_resolution, ds.mesh_simplify = None, None
    back = ds.get_mesh(tri_feat=feat)
    assert torch.equal(back.vertices, plain.vertices) and torch.equal(back.triangles, plain.triangles)


def test_generate_writes_the_simplified_mesh(tmp_path):
    """generate.py --mesh_simplify: the option reaches visualize.main as `mesh_simplify`, and the file it writes per shape is the
    clustered surface -- of the dense volume (create_obj_simplified) and, with --mesh_resolution, of the sparse surface
    (create_obj_sparse) -- in create_obj's vertex convention"""
    from argparse import Namespace
    from ishapediting_amd import generate, visualize
    from tests.test_gpu_field import mesh_case
    mesh = M()
    dec, planes, vol32, _ = mesh_case()
    a = generate.build_parser().parse_args(["--shape_resolution", "32", "--mesh_resolution", "41", "--mesh_simplify", "2"])
    assert a.mesh_simplify == 2.0
    np.save(tmp_path / "0.npy", planes.permute(0, 3, 1, 2).contiguous().cpu().numpy())          # [3,32,S,S], what generate saves
    sd = dec.net.state_dict()

    def written(name, **kw):
        args = Namespace(input=str(tmp_path / "0.npy"), output=str(tmp_path / name), model_path=None, res=a.shape_resolution, **kw)
        visualize.main(args=args, state_dict=sd)                # the call generate.main makes per shape
        return mesh.read_obj(str(tmp_path / name))

    def same(got, v, t, scale):
        want = (v / scale * 2 - 1).cpu().numpy()
        assert got[0].shape == want.shape and want.shape[0] > 100 and np.array_equal(got[1], t.cpu().numpy())
        assert float(np.abs(got[0] - want).max()) <= 0.5e-6 + 2.0 ** -24       # six decimals of coordinates in [-1, 1], then float32

    # the dense volume's surface, cells of two voxels from origin 0
    dv, dt = mesh.extract_surface(vol32, 0.0)
    v, t, info = mesh.simplify_vertex_clustering(dv, dt, 2.0, origin=(0.0, 0.0, 0.0), dims=[16, 16, 16])
    assert 0 < v.shape[0] < dv.shape[0]
    same(written("dense.obj", mesh_res=None, mesh_simplify=a.mesh_simplify), v, t, 255.0)
    # the sparse surface at 41, cells of two FINE voxels
    sv, st, _ = mesh.extract_surface_sparse(dec, planes, 41, vol32)
    v, t, info = mesh.simplify_vertex_clustering(sv, st, 2.0, origin=(0.0, 0.0, 0.0), dims=[21, 21, 21])
    assert 0 < v.shape[0] < sv.shape[0]
    same(written("sparse.obj", mesh_res=a.mesh_resolution, mesh_simplify=a.mesh_simplify), v, t, 40.0)
    # without the option: the mesh as cut
    plain = written("plain.obj", mesh_res=None, mesh_simplify=None)
    assert plain[0].shape[0] == dv.shape[0]
