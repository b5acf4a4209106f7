"""The headless renderer (ishapediting_amd/render.py, csrc/render.hip) through its public functions, against the fp64
statement in tests/render_ref.py and against analytic shapes.  Open3D is absent: parity with its pictures is unpinned."""
import functools

import numpy as np
import pytest
import torch

from tests import render_ref as R

pytestmark = pytest.mark.gpu

W1, H1 = 150, 117            # not a multiple of any tile
GREY, TAN = (0.7, 0.7, 0.7), (0.8, 0.6, 0.3)


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def cam1():
    from ishapediting_amd.render import Camera
    return Camera(eye=(0.4, 0.3, 2.5), centre=(0, 0, 0), fov=60, near=0.1, far=10)


def host_normals(v, f):
    """mesh.vertex_normals in fp64: area-weighted sum of the face normals, normalised"""
    v64, f = v.astype(np.float64), f.astype(np.int64)
    fn = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
    n = np.zeros_like(v64)
    for k in range(3):
        np.add.at(n, f[:, k], fn)
    return n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)


def concat(parts):
    """what render_mesh hands the library for a list of (mesh, colour, lit) parts, as host arrays"""
    vs, fs, ns, ids, table, base = [], [], [], [], [], 0
    for k, ((v, f), colour, lit) in enumerate(parts):
        vs.append(v); fs.append(f + base); ids.append(np.full(len(f), k))
        ns.append(host_normals(v, f) if lit else np.zeros(v.shape))
        table.append([*colour, 1.0 if lit else 0.0])
        base += len(v)
    return (np.concatenate(vs), np.concatenate(fs).astype(np.int32), np.concatenate(ns).astype(np.float32), np.concatenate(ids),
            np.asarray(table, np.float32))


def scene1_parts():
    return [(R.uv_sphere(0.6, 48, 32), GREY, True), (R.box_mesh((-0.9, -0.25, 0.1), (0.1, 0.2, 0.9)), TAN, True)]


@functools.lru_cache(maxsize=None)
def scene1():
    """the shared scene, its fp64 picture (computed once, never modified) and the device picture"""
    from ishapediting_amd.render import render_mesh
    parts = scene1_parts()
    v, f, n, ids, table = concat(parts)
    ref = R.render(v, f, cam1(), W1, H1, normals=n, tri_part=ids, parts=table)
    for a in ref.values():
        a.setflags(write=False)
    out = render_mesh(parts, cam1(), W1, H1, device=dev())
    return v, f, ref, out


def test_visibility_matches_the_fp64_statement():
    v, f, ref, out = scene1()
    assert out.rgb.shape == (H1, W1, 3) and out.rgb.dtype == torch.uint8 and out.rgb.is_cuda
    assert out.depth.shape == (H1, W1) and out.depth.dtype == torch.float32
    assert out.tri_id.shape == (H1, W1) and out.tri_id.dtype == torch.int32
    amb = ref["ambiguous"]
    hit = ref["tri_id"] >= 0
    print(f"ambiguous {amb.mean():.4%}, coverage {hit.mean():.2%}, visible triangles {np.unique(ref['tri_id'][hit]).size}")
    assert amb.mean() <= 0.01
    assert hit.mean() >= 0.10
    assert (ref["tri_id"][hit] >= 2 * 48 * 31).any() and (ref["tri_id"][hit] < 2 * 48 * 31).any()      # box and sphere both show
    ok = ~amb
    tid, depth, rgb = out.tri_id.cpu().numpy(), out.depth.cpu().numpy(), out.rgb.cpu().numpy()
    wrong = (tid != ref["tri_id"]) & ok
    derr = np.abs(depth.astype(np.float64) - ref["depth"])[ok].max()
    cerr = np.abs(rgb.astype(np.int64) - ref["rgb"].astype(np.int64))[ok].max()
    print(f"wrong ids {wrong.sum()}, max depth error {derr:.3e}, max colour error {cerr}")
    assert not wrong.any()
    assert np.array_equal((tid < 0)[ok], ~hit[ok])
    assert (depth[ok & ~hit] == 1.0).all() and (depth[ok & hit] < 1.0).all()
    assert derr <= 2e-6
    assert cerr <= 1
    assert (rgb[(tid < 0)] == 0).all()


@pytest.mark.parametrize("nx,ny", [(1, 1), (37, 29)])
def test_fill_rule_leaves_no_hole_and_no_double_hit(nx, ny):
    """A rectangle that covers the picture, as 2 triangles and as a 37 x 29 grid of cells: every pixel is drawn, at the
    rectangle's depth, by the triangle the statement names."""
    from ishapediting_amd.render import Camera, render_mesh
    cam = Camera(eye=(0, 0, 2), centre=(0, 0, 0), fov=60, near=0.1, far=10)
    v, f = R.grid_quad((-2.03, -1.51), (2.01, 1.57), 0.0, nx, ny)
    out = render_mesh((v, f), cam, 64, 48, device=dev())
    tid, depth = out.tri_id.cpu().numpy(), out.depth.cpu().numpy()
    assert (tid >= 0).all() and (tid < len(f)).all()
    want = R.depth_of(cam, 2.0)
    assert float(np.abs(depth.astype(np.float64) - want).max()) <= 2e-6
    ref = R.render(v, f, cam, 64, 48)
    assert (ref["tri_id"] >= 0).all()
    ok = ~ref["ambiguous"]                   # only one triangle covers a pixel, so this is the distance-to-edge flag alone
    assert not ref["tie"].any() and ok.mean() > 0.9
    assert np.array_equal(tid[ok], ref["tri_id"][ok])


def segment_distance(a, b, w, h):
    """[H, W]: distance of every pixel centre to the nearest of the 2-D segments a[i] .. b[i]"""
    xs, ys = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
    c = np.stack([xs, ys], axis=-1)[:, :, None, :]
    ab = (b - a)[None, None]
    t = np.clip(((c - a[None, None]) * ab).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300), 0, 1)
    return np.linalg.norm(c - (a[None, None] + t[..., None] * ab), axis=-1).min(axis=-1)


def test_exact_cube_depth():
    from ishapediting_amd.render import Camera, render_mesh, unproject
    cam = Camera(eye=(1.2, 0.9, 2.0), centre=(0, 0, 0), fov=60, near=0.1, far=10)
    w, h = 160, 120
    lo, hi = (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)
    v, f = R.box_mesh(lo, hi)
    out = render_mesh((v, f), cam, w, h, device=dev())
    depth = out.depth.cpu().numpy()
    eye, dirs = R.pixel_rays(cam, w, h)
    t = R.ray_box(eye, dirs, lo, hi)
    xw, yw, _ = R.project(cam, v, w, h)
    p = np.stack([xw, yw], axis=1)
    cube_edges = np.array([(a, b) for a in range(8) for b in range(a + 1, 8) if bin(a ^ b).count("1") == 1])
    clear = segment_distance(p[cube_edges[:, 0]], p[cube_edges[:, 1]], w, h) > 1.0
    hit = ~np.isnan(t)
    assert (hit & clear).mean() > 0.1
    assert np.array_equal((depth < 1.0)[clear], hit[clear])
    zv = (t[..., None] * dirs) @ R.camera_basis(cam)[3]
    exact = R.depth_of(cam, zv)
    assert float(np.abs(depth.astype(np.float64) - exact)[hit & clear].max()) <= 1e-5
    # and the unprojected points lie on the cube
    ys, xs = np.nonzero(hit & clear)
    pts = unproject(cam, xs, ys, depth[ys, xs], w, h).cpu().numpy().astype(np.float64)
    assert float(np.abs(np.abs(pts).max(axis=1) - 0.5).max()) <= 1e-4


def test_repeatable_and_independent_of_triangle_order():
    from ishapediting_amd.render import render_mesh
    v, f, ref, out = scene1()
    again = render_mesh(scene1_parts(), cam1(), W1, H1, device=dev())
    assert torch.equal(again.rgb, out.rgb) and torch.equal(again.depth, out.depth) and torch.equal(again.tri_id, out.tri_id)
    perm = np.random.default_rng(7).permutation(len(f))
    shuffled = render_mesh((v, f[perm]), cam1(), W1, H1, device=dev())
    assert torch.equal(shuffled.depth, out.depth)
    sid, tid = shuffled.tri_id.cpu().numpy(), out.tri_id.cpu().numpy()
    assert np.array_equal(sid < 0, tid < 0)
    ok = (tid >= 0) & ~ref["tie"]
    assert ok.sum() > 1000 and np.array_equal(perm[sid[ok]], tid[ok])


def test_skipped_geometry_draws_nothing():
    """Triangles behind the eye, across the near plane, of zero area and wholly off-screen change no bit of the picture."""
    from ishapediting_amd.render import render_mesh
    v, f, ref, out = scene1()
    cam = cam1()
    eye, r, u, fwd = R.camera_basis(cam)

    def at(x, y, z):
        return eye + x * r + y * u + z * fwd
    extra_v = np.array([at(-0.3, -0.2, -1.0), at(0.3, -0.2, -1.0), at(0.0, 0.3, -1.0),        # behind the eye
                        at(0.0, 0.0, 0.05), at(-0.3, 0.1, 1.0), at(0.3, 0.1, 1.0),            # one vertex nearer than near
                        at(-0.3, 0.1, 0.5), at(0.2, -0.1, 0.5), at(0.2, -0.1, 0.5),           # two coincident vertices
                        at(5.0, 0.0, 1.0), at(6.0, 0.0, 1.0), at(5.5, 0.5, 1.0),              # right of the picture
                        at(0.0, -9.0, 1.0), at(0.5, -8.0, 1.0), at(-0.5, -8.0, 1.0)], np.float32)   # below it
    b = len(v)
    extra_f = np.array([(b, b + 1, b + 2), (b + 3, b + 4, b + 5), (b + 6, b + 7, b + 8), (b + 6, b + 6, b + 7),
                        (b + 9, b + 10, b + 11), (b + 12, b + 13, b + 14)], np.int32)
    # (the crossing triangle would cover the middle of the picture if its far part were drawn)
    sphere, box = scene1_parts()
    more = render_mesh([sphere, box, ((extra_v, extra_f - b), (0.0, 1.0, 0.0), False)], cam, W1, H1, device=dev())
    assert torch.equal(more.rgb, out.rgb) and torch.equal(more.depth, out.depth) and torch.equal(more.tri_id, out.tri_id)
    alone = render_mesh((extra_v, extra_f - b), cam, W1, H1, device=dev())
    assert bool((alone.tri_id == -1).all()) and bool((alone.depth == 1.0).all()) and bool((alone.rgb == 0).all())


def test_empty_mesh_and_one_pixel_picture():
    from ishapediting_amd.render import render_mesh
    empty = render_mesh((np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)), cam1(), 33, 17, device=dev())
    assert empty.depth.shape == (17, 33)
    assert bool((empty.tri_id == -1).all()) and bool((empty.depth == 1.0).all()) and bool((empty.rgb == 0).all())
    v, f, _, _ = scene1()
    from ishapediting_amd.render import Camera
    cam = Camera(eye=(0.4, 0.3, 2.5), centre=(0.13, 0.07, 0), fov=60, near=0.1, far=10)     # the one centre is clear of every edge
    one = render_mesh((v, f), cam, 1, 1, device=dev())
    ref = R.render(v, f, cam, 1, 1)
    assert not ref["ambiguous"][0, 0] and ref["tri_id"][0, 0] >= 0
    assert int(one.tri_id[0, 0]) == int(ref["tri_id"][0, 0])
    assert abs(float(one.depth[0, 0]) - ref["depth"][0, 0]) <= 2e-6


def test_full_size_mesh_at_1024():
    """The 256^3 sphere mesh (~300 k triangles of a few pixels each) at 1024 x 1024 against the ray-sphere hit: no hole inside
    the silhouette, and 2 px inside it the drawn surface point is within the polyhedral bound the surface tests use."""
    from ishapediting_amd.mesh import extract_surface
    from ishapediting_amd.render import render_mesh, unproject
    res, r, side = 256, 90.4, 1024
    ax = torch.arange(res, dtype=torch.float32) - (res - 1) / 2
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v, f = extract_surface((r - torch.sqrt(x * x + y * y + z * z)).to(dev()))
    v = (v / (res - 1) * 2 - 1).contiguous()
    rad = r / (res - 1) * 2
    assert f.shape[0] > 250_000
    cam = cam1()
    out = render_mesh((v, f), cam, side, side)
    eye, dirs = R.pixel_rays(cam, side, side)
    t = R.ray_sphere(eye, dirs, rad)
    inside = torch.from_numpy(~np.isnan(t))
    # erode the analytic silhouette by 2 pixels
    core = (torch.nn.functional.max_pool2d((~inside).float()[None, None], 5, stride=1, padding=2)[0, 0] == 0).numpy()
    depth = out.depth.cpu().numpy()
    tid = out.tri_id.cpu().numpy()
    assert core.mean() > 0.15            # the silhouette's radius is f * rad / sqrt(|eye|^2 - rad^2) = 257 px: 0.197 of the picture
    assert (depth[core] < 1.0).all() and (tid[core] >= 0).all() and tid.max() < f.shape[0]
    outside = (torch.nn.functional.max_pool2d(inside.float()[None, None], 5, stride=1, padding=2)[0, 0] == 0).numpy()
    assert (depth[outside] == 1.0).all()
    ys, xs = np.nonzero(core)
    drawn = unproject(cam, xs, ys, depth[ys, xs], side, side).cpu().numpy().astype(np.float64)
    exact = eye + t[ys, xs, None] * dirs[ys, xs]
    err = float(np.linalg.norm(drawn - exact, axis=1).max())
    print(f"{f.shape[0]} triangles, max surface-point error {err:.3e}")
    assert err < 0.03


def test_picking():
    """main.py:496-509 on 50 surface pixels: the unprojected point against the fp64 ray-triangle hit, the vertex against a
    brute-force search; a background pixel gives None, or the point at the source's depth."""
    from ishapediting_amd.render import pick, unproject
    v, f, ref, out = scene1()
    cam = cam1()
    g = np.random.default_rng(11)
    ys, xs = np.nonzero((ref["tri_id"] >= 0) & ~ref["ambiguous"])
    sel = g.choice(len(ys), 50, replace=False)
    eye, dirs = R.pixel_rays(cam, W1, H1)
    v64 = v.astype(np.float64)
    mesh = (torch.from_numpy(v).to(dev()), torch.from_numpy(f).to(dev()))
    worst = 0.0
    for y, x in zip(ys[sel], xs[sel]):
        a, b, c = v64[f[ref["tri_id"][y, x]]]
        exact = R.ray_triangle(eye, dirs[y, x], a, b, c)
        d = float(out.depth[y, x])
        world = unproject(cam, int(x), int(y), d, W1, H1).cpu().numpy().astype(np.float64)
        worst = max(worst, float(np.linalg.norm(world - exact)))
        pos, idx, got_depth = pick(mesh, cam, out.depth, int(x), int(y))
        assert got_depth == d
        dist = np.sort(((v64 - world) ** 2).sum(axis=1))
        nearest = int(np.argmin(((v64 - world) ** 2).sum(axis=1)))
        if np.sqrt(dist[1]) - np.sqrt(dist[0]) >= 1e-5:
            assert idx == nearest
        assert np.array_equal(pos, v[idx])
    print(f"max picked-point error {worst:.3e}")
    assert worst <= 1e-4
    by, bx = np.argwhere((ref["tri_id"] < 0) & ~ref["ambiguous"])[0]
    assert pick(mesh, cam, out.depth, int(bx), int(by)) is None
    p = pick(mesh, cam, out.depth, int(bx), int(by), source_depth=0.93)
    assert float(np.abs(p - R.unproject(cam, bx, by, np.float64(np.float32(0.93)), W1, H1)).max()) <= 1e-5
    # arrays of pixels unproject in one call
    many = unproject(cam, xs[sel], ys[sel], out.depth.cpu().numpy()[ys[sel], xs[sel]], W1, H1)
    assert many.shape == (50, 3)


def test_unlit_part_keeps_its_colour():
    """An unlit red sphere in front of the lit mesh is exactly (255, 0, 0); the lit mesh behind it is shaded."""
    from ishapediting_amd.render import marker_sphere, render_mesh
    sphere = R.uv_sphere(0.6, 48, 32)
    red = marker_sphere((0.1, 0.05, 0.9), radius=0.2)
    parts = [(sphere, GREY, True), (red, (1.0, 0.0, 0.0), False)]
    v, f, n, ids, table = concat(parts)
    ref = R.render(v, f, cam1(), W1, H1, normals=n, tri_part=ids, parts=table)
    out = render_mesh(parts, cam1(), W1, H1, device=dev())
    rgb, tid = out.rgb.cpu().numpy(), out.tri_id.cpu().numpy()
    on_red = (ref["tri_id"] >= len(sphere[1])) & ~ref["ambiguous"]
    on_grey = (ref["tri_id"] >= 0) & (ref["tri_id"] < len(sphere[1])) & ~ref["ambiguous"]
    assert on_red.sum() > 200 and on_grey.sum() > 1000
    assert np.array_equal(tid[on_red], ref["tri_id"][on_red])
    assert (rgb[on_red] == np.array([255, 0, 0], np.uint8)).all()
    assert np.abs(rgb[on_grey].astype(int) - ref["rgb"][on_grey].astype(int)).max() <= 1
    assert (rgb[on_grey][:, 0] == rgb[on_grey][:, 1]).all() and rgb[on_grey].min() >= 44 and rgb[on_grey].max() <= 179
