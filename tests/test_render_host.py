"""Host side of the headless renderer (ishapediting_amd/render.py) and the fp64 statement it is tested against
(tests/render_ref.py): no GPU needed."""
import os
import re
import struct
import zlib

import numpy as np
import pytest

from tests import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_symbols_and_version():
    from ishapediting_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ishap.h")).read()
    declared = set(re.findall(r"\b(ishap_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ishap_render_scratch_bytes", "ishap_render_mesh", "ishap_unproject"):
        assert name in declared and name in _lib.SYMBOLS
    L = _lib.lib()
    assert L.ishap_version() >= 11
    # 8 bytes of visibility per pixel (rounded up to 16) + 16 per vertex + 16 per triangle + 16
    assert L.ishap_render_scratch_bytes(0, 0, 1, 1) == 16 + 16
    assert L.ishap_render_scratch_bytes(10, 20, 150, 117) == 150 * 117 * 8 + 16 * 10 + 16 * 20 + 16
    assert L.ishap_render_scratch_bytes(-1, 0, 4, 4) == -1 and L.ishap_render_scratch_bytes(0, 0, 0, 4) == -1
    assert L.ishap_render_scratch_bytes(0, 0, 4, 16385) == -1 and L.ishap_render_scratch_bytes(0, 1 << 31, 4, 4) == -1


def test_render_kernels_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_meta
    ks = kernel_meta.kernels(os.path.join(ROOT, "ishapediting_amd", "libishap_hip.so"))
    for want in ("render_clear_kernel", "render_vertex_kernel", "render_small_kernel", "render_large_kernel",
                 "render_resolve_kernel", "render_unproject_kernel"):
        found = [n for n in ks if want in n]
        assert len(found) == 1, (want, found)
        assert ks[found[0]].get(".private_segment_fixed_size", 0) == 0, (want, ks[found[0]])


def test_camera_struct_matches_the_header():
    import ctypes as C
    from ishapediting_amd import _lib
    from ishapediting_amd.render import Camera
    assert C.sizeof(_lib.CameraC) == 12 * 4
    c = Camera(eye=(1, 2, 3), centre=(4, 5, 6), up=(0, 0, 1), fov=45, near=0.5, far=7)._c()
    assert list(c.eye) == [1, 2, 3] and list(c.centre) == [4, 5, 6] and list(c.up) == [0, 0, 1]
    assert (c.fov_y_deg, c.near, c.far) == (45.0, 0.5, 7.0)


@pytest.mark.parametrize("w,h", [(150, 117), (1, 1), (1024, 768)])
def test_unproject_inverts_project_in_fp64(w, h):
    from ishapediting_amd.render import Camera
    cam = Camera(eye=(0.4, 0.3, 2.5), centre=(0, 0, 0), fov=60, near=0.1, far=10)
    g = np.random.default_rng(w)
    pts = g.uniform(-1, 1, (500, 3))
    xw, yw, zv = R.project(cam, pts, w, h)
    assert (zv > 0.1).all()
    d = R.depth_of(cam, zv)
    assert ((d > 0) & (d < 1)).all()
    back = R.unproject_window(cam, xw, yw, d, w, h)
    assert float(np.abs(back - pts).max()) <= 1e-12
    # the pixel form names the pixel centre
    p = R.unproject(cam, 3, 5, 0.9, 150, 117)
    assert float(np.abs(p - R.unproject_window(cam, 3.5, 5.5, 0.9, 150, 117)).max()) == 0
    x2, y2, z2 = R.project(cam, p[None], 150, 117)
    assert abs(x2[0] - 3.5) <= 1e-9 and abs(y2[0] - 5.5) <= 1e-9 and abs(R.depth_of(cam, z2)[0] - 0.9) <= 1e-12


@pytest.mark.parametrize("lo,hi,wh", [((-0.6, -0.45, -0.5), (0.6, 0.45, 0.5), (640, 480)),
                                      ((-1, -1, -1), (1, 1, 1), (256, 256)),            # a cube: the eye has to move back
                                      ((0.2, 0.1, -3.0), (0.5, 2.1, 0.3), (117, 150)),
                                      ((-0.3, -0.2, -0.9), (0.3, 0.2, 0.9), (512, 512))])
def test_camera_fit_frames_the_bounds(lo, hi, wh):
    from ishapediting_amd.render import Camera
    w, h = wh
    cam = Camera.fit(lo, hi, fov=60, aspect=w / h)
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    centre, ext = (lo + hi) / 2, hi - lo
    assert np.allclose(cam.centre, centre) and cam.up == (0.0, 1.0, 0.0) and cam.fov == 60.0
    eye = np.asarray(cam.eye)
    assert np.allclose(eye[:2], centre[:2]) and eye[2] - centre[2] >= 1.25 * ext.max() - 1e-12
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    xw, yw, zv = R.project(cam, corners, w, h)
    assert (xw > 0).all() and (xw < w).all() and (yw > 0).all() and (yw < h).all()
    assert (zv > cam.near).all() and (zv < cam.far).all()
    # the whole bounding sphere lies strictly between near and far
    dist, radius = np.linalg.norm(eye - centre), np.linalg.norm(ext) / 2
    assert cam.near < dist - radius and dist + radius < cam.far and cam.near > 0
    # Open3D's placement wherever it frames the box
    flat = Camera.fit((-0.6, -0.3, -0.5), (0.6, 0.3, 0.5), fov=60, aspect=4 / 3)
    assert abs(flat.eye[2] - 1.25 * 1.2) <= 1e-12


def test_markers_are_closed_meshes():
    from ishapediting_amd.render import edit_parts, marker_arrow, marker_sphere
    v, f = marker_sphere((0.1, -0.2, 0.3))
    assert v.dtype == np.float32 and f.dtype == np.int32 and R.closed_edges(f)
    assert np.allclose(np.linalg.norm(v - np.float32([0.1, -0.2, 0.3]), axis=1), 0.04, atol=1e-6)      # main.py:541
    assert f.min() == 0 and f.max() == v.shape[0] - 1
    for start, end in (((0, 0, 0), (0.5, 0.2, -0.1)), ((0.1, 0.1, 0.1), (0.1, 0.1, 0.15)), ((1, 0, 0), (-1, 0, 0)),
                       ((0, 0, 0), (0, 0, -0.3))):
        v, f = marker_arrow(start, end)
        assert R.closed_edges(f) and f.min() == 0 and f.max() == v.shape[0] - 1
        s, e = np.asarray(start, float), np.asarray(end, float)
        length = np.linalg.norm(e - s)
        axis = (e - s) / length
        along = (v - s) @ axis
        radial = np.linalg.norm((v - s) - along[:, None] * axis, axis=1)
        cone = min(0.1, 0.5 * length)                                                                    # main.py:576
        assert abs(along.min()) <= 1e-6 and abs(along.max() - length) <= 1e-6
        assert abs(radial.max() - 0.04) <= 1e-6                                                          # cone radius, main.py:581
        assert np.allclose(radial[np.abs(along) <= 1e-6][1:], 0.02, atol=1e-6)                           # shaft radius, main.py:583
        assert np.allclose(along[np.abs(radial - 0.04) <= 1e-6], length - cone, atol=1e-6)
        assert np.allclose(v[-1], e, atol=1e-6)
    with pytest.raises(ValueError):
        marker_arrow((1, 2, 3), (1, 2, 3))
    mesh = R.uv_sphere(0.5, 12, 8)
    parts = edit_parts(mesh, [(0.5, 0, 0), (0, 0.5, 0)], [(0.7, 0, 0), (0, 0.8, 0)])
    assert len(parts) == 1 + 2 + 2 + 2
    assert [p[2] for p in parts] == [True, False, False, False, False, True, True]
    assert parts[1][1] == (1.0, 0.0, 0.0) and parts[3][1] == (0.0, 0.0, 1.0) and parts[5][1] == (0.0, 1.0, 0.0)


def _decode_png(data: bytes):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        pos += 12 + n
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    w, h, bits, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (bits, colour, comp, filt, lace) == (8, 2, 0, 0, 0)
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(h, w, 3)


def test_save_picture_writes_a_png_with_white_background(tmp_path):
    from ishapediting_amd.render import save_picture
    g = np.random.default_rng(0)
    rgb = g.integers(0, 256, (29, 37, 3), dtype=np.uint8)
    depth = g.uniform(0, 0.99, (29, 37)).astype(np.float32)
    depth[g.uniform(size=depth.shape) < 0.3] = 1.0
    import torch
    out = save_picture(str(tmp_path / "p.png"), (torch.from_numpy(rgb), torch.from_numpy(depth)))
    img = _decode_png(open(tmp_path / "p.png", "rb").read())
    assert np.array_equal(img, out)
    assert (img[depth == 1.0] == 255).all() and np.array_equal(img[depth != 1.0], rgb[depth != 1.0])
    assert (rgb[depth == 1.0] != 255).any()                     # the input itself was not white there
    with pytest.raises(ValueError):
        save_picture(str(tmp_path / "q.png"), (rgb, depth[:5]))


def test_reference_renderer_draws_an_analytic_sphere():
    """The fp64 statement on a latitude / longitude sphere against the ray-sphere hit: inside the silhouette the drawn point
    is within the polyhedral bound the surface tests use (0.03), nothing is missing there, and nothing is drawn outside."""
    from ishapediting_amd.render import Camera
    cam = Camera(eye=(0.4, 0.3, 2.5), centre=(0, 0, 0), fov=60, near=0.1, far=10)
    w, h, rad = 96, 80, 0.6
    v, f = R.uv_sphere(rad, 48, 32)
    assert R.closed_edges(f) and f.shape[0] == 2 * 48 * 31
    out = R.render(v, f, cam, w, h)
    eye, dirs = R.pixel_rays(cam, w, h)
    t = R.ray_sphere(eye, dirs, rad)
    t_in = R.ray_sphere(eye, dirs, rad - 0.03)              # rays that clear the polyhedron's sagitta
    hit = out["tri_id"] >= 0
    assert not hit[np.isnan(t)].any() and hit[~np.isnan(t_in)].all() and hit.mean() > 0.1
    ys, xs = np.nonzero(~np.isnan(t_in))
    drawn = R.unproject(cam, xs, ys, out["depth"][ys, xs], w, h)
    exact = eye + t[ys, xs, None] * dirs[ys, xs]
    assert float(np.linalg.norm(drawn - exact, axis=1).max()) < 0.03
    assert (out["depth"][~hit] == 1.0).all() and (out["rgb"][~hit] == 0).all()
    # lit grey: the centre of the disc faces the eye (|n . v| ~ 1), the rim does not
    cy, cx = np.unravel_index(np.argmin(np.where(hit, out["depth"], 2)), hit.shape)
    assert out["rgb"][cy, cx, 0] >= 170 and out["rgb"][hit].min() >= 44      # 255 * 0.7 * (0.25 .. 1)
    assert out["ambiguous"].mean() < 0.05
