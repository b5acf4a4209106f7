"""The renderer's statement in fp64 numpy (what csrc/render.hip is tested against; Open3D cannot run here).

Camera: looks from `eye` at `centre`, z_view > 0 in front; square pixels, f = (H/2) / tan(fov/2);
x_win = W/2 + f x_v / z_v, y_win = H/2 - f y_v / z_v (row 0 on top).  Coverage at pixel centres (x + 0.5, y + 0.5), top-left
rule; depth d = far/(far-near) (1 - near/z_v) from 1/z interpolated with the screen barycentrics, pixels with d >= 1 dropped,
the lowest triangle id on exact ties; triangles with a vertex nearer than `near`, of zero screen area or with no pixel centre
of the picture in their bounding box draw nothing.  Shading: colour * (0.25 + 0.75 |n . v|) for lit parts.

The camera's numbers are rounded to fp32 first (the C ABI carries floats), then everything is fp64.
"""
import numpy as np

EDGE_EPS = 1e-3      # |min barycentric| * sqrt(|doubled screen area|) below this: the centre is within rounding reach of an edge
DEPTH_EPS = 1e-5     # the two nearest covering depths closer than this: the winner may legitimately differ


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def camera_basis(cam):
    eye, centre, up = _f32(cam.eye), _f32(cam.centre), _f32(cam.up)
    f = centre - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    return eye, r, np.cross(r, f), f


def focal(cam, height):
    return 0.5 * height / np.tan(0.5 * np.deg2rad(float(np.float32(cam.fov))))


def project(cam, pts, width, height):
    """(x_win, y_win, z_view) of world points [n, 3]"""
    eye, r, u, f = camera_basis(cam)
    d = np.asarray(pts, np.float64).reshape(-1, 3) - eye
    zv = d @ f
    fl = focal(cam, height)
    return 0.5 * width + fl * (d @ r) / zv, 0.5 * height - fl * (d @ u) / zv, zv


def depth_of(cam, zv):
    near, far = float(np.float32(cam.near)), float(np.float32(cam.far))
    return far / (far - near) * (1.0 - near / zv)


def unproject_window(cam, xw, yw, depth, width, height):
    """world point of the WINDOW position (xw, yw) at `depth`"""
    eye, r, u, f = camera_basis(cam)
    near, far = float(np.float32(cam.near)), float(np.float32(cam.far))
    xw, yw, depth = (np.asarray(a, np.float64) for a in (xw, yw, depth))
    zv = near / (1.0 - depth * (far - near) / far)
    fl = focal(cam, height)
    xv, yv = (xw - 0.5 * width) * zv / fl, -(yw - 0.5 * height) * zv / fl
    return eye + xv[..., None] * r + yv[..., None] * u + zv[..., None] * f


def unproject(cam, x, y, depth, width, height):
    """camera.unproject of PIXEL (x, y): its centre"""
    return unproject_window(cam, np.asarray(x, np.float64) + 0.5, np.asarray(y, np.float64) + 0.5, depth, width, height)


def pixel_rays(cam, width, height):
    """(origin [3], unit directions [H, W, 3]) of the rays through the pixel centres"""
    eye, r, u, f = camera_basis(cam)
    fl = focal(cam, height)
    xs, ys = np.meshgrid(np.arange(width) + 0.5, np.arange(height) + 0.5)
    d = ((xs - 0.5 * width) / fl)[..., None] * r - ((ys - 0.5 * height) / fl)[..., None] * u + f
    return eye, d / np.linalg.norm(d, axis=-1, keepdims=True)


def _edge_in(e, dx, dy):
    # top-left: E rises by -dy per step in x and by dx per step in y
    return (e > 0) | ((e == 0) & ((dy < 0) | ((dy == 0) & (dx > 0))))


def render(verts, tris, cam, width, height, normals=None, tri_part=None, parts=None):
    """dict: depth [H,W] fp64 (background 1), tri_id [H,W] (background -1), rgb [H,W,3] uint8, ambiguous [H,W] bool,
    tie [H,W] bool (the depth half of ambiguous), bary [H,W,3] screen barycentrics of the winner."""
    V = np.asarray(verts, np.float32).astype(np.float64).reshape(-1, 3)
    T = np.asarray(tris, np.int64).reshape(-1, 3)
    W, H = int(width), int(height)
    near, far = float(np.float32(cam.near)), float(np.float32(cam.far))
    kf = far / (far - near)
    if V.shape[0]:
        xw, yw, zv = project(cam, V, W, H)
    depth = np.ones((H, W))
    second = np.full((H, W), np.inf)
    tid = np.full((H, W), -1, np.int64)
    bary = np.zeros((H, W, 3))
    amb = np.zeros((H, W), bool)
    for t, (i0, i1, i2) in enumerate(T):
        z = zv[[i0, i1, i2]]
        if not (z >= near).all():
            continue
        X, Y = xw[[i0, i1, i2]], yw[[i0, i1, i2]]
        area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
        if area == 0:
            continue
        x0, x1 = int(np.ceil(X.min() - 0.5)), int(np.floor(X.max() - 0.5))
        y0, y1 = int(np.ceil(Y.min() - 0.5)), int(np.floor(Y.max() - 0.5))
        # one pixel of margin: a centre just outside the box can still be within rounding reach of an edge
        x0, x1, y0, y1 = max(x0 - 1, 0), min(x1 + 1, W - 1), max(y0 - 1, 0), min(y1 + 1, H - 1)
        if x0 > x1 or y0 > y1:
            continue
        s = 1.0 if area > 0 else -1.0
        px, py = np.meshgrid(np.arange(x0, x1 + 1) + 0.5, np.arange(y0, y1 + 1) + 0.5)
        b, inside = [], np.ones(px.shape, bool)
        for a_, b_ in ((1, 2), (2, 0), (0, 1)):                       # edge i is opposite vertex i
            dx, dy = s * (X[b_] - X[a_]), s * (Y[b_] - Y[a_])
            e = dx * (py - Y[a_]) - dy * (px - X[a_])
            inside &= _edge_in(e, dx, dy)
            b.append(e / (s * area))
        b = np.stack(b, axis=-1)
        sl = (slice(y0, y1 + 1), slice(x0, x1 + 1))
        amb[sl] |= np.abs(b.min(axis=-1)) * np.sqrt(abs(area)) < EDGE_EPS
        d = kf * (1.0 - near * (b @ (1.0 / z)))
        inside &= d < 1.0
        if not inside.any():
            continue
        d = np.where(inside, np.maximum(d, 0.0), np.inf)
        cur, cid = depth[sl], tid[sl]
        win = inside & ((d < cur) | ((d == cur) & (cid >= 0) & (t < cid)))
        second[sl] = np.where(win, np.where(cid >= 0, cur, second[sl]), np.minimum(second[sl], d))
        depth[sl] = np.where(win, d, cur)
        tid[sl] = np.where(win, t, cid)
        bary[sl] = np.where(win[..., None], b, bary[sl])
    tie = (tid >= 0) & (second - depth < DEPTH_EPS)
    amb |= tie
    # ---- shading
    rgb = np.zeros((H, W, 3))
    hit = tid >= 0
    if hit.any():
        eye = camera_basis(cam)[0]
        table = np.asarray([[0.7, 0.7, 0.7, 1.0]] if parts is None else parts, np.float32).astype(np.float64).reshape(-1, 4)
        ids = tid[hit]
        tri = T[ids]
        q = bary[hit] / zv[tri]
        g = q / q.sum(axis=1, keepdims=True)
        P = (g[..., None] * V[tri]).sum(axis=1)
        if normals is not None:
            N = np.asarray(normals, np.float32).astype(np.float64).reshape(-1, 3)
            n = (g[..., None] * N[tri]).sum(axis=1)
        else:
            n = np.cross(V[tri[:, 1]] - V[tri[:, 0]], V[tri[:, 2]] - V[tri[:, 0]])
        v = eye - P
        nn, vv = np.linalg.norm(n, axis=1), np.linalg.norm(v, axis=1)
        c = np.where((nn > 0) & (vv > 0), np.abs((n * v).sum(axis=1)) / np.maximum(nn * vv, 1e-300), 0.0)
        part = np.zeros(len(ids), np.int64) if tri_part is None else np.asarray(tri_part, np.int64)[ids]
        row = table[part]
        shade = np.where(row[:, 3] != 0, 0.25 + 0.75 * np.minimum(c, 1.0), 1.0)
        rgb[hit] = np.clip(row[:, :3] * shade[:, None], 0, 1) * 255.0
    return {"depth": depth, "tri_id": tid, "rgb": np.rint(rgb).astype(np.uint8), "rgb_exact": rgb, "ambiguous": amb, "tie": tie,
            "bary": bary}


# ---------------------------------------------------------------- shapes
def uv_sphere(radius, n_lon, n_lat, centre=(0, 0, 0)):
    """closed latitude / longitude sphere: (vertices [V,3] float32, triangles [F,3] int32), 2 n_lon (n_lat - 1) triangles"""
    theta = np.pi * np.arange(1, n_lat) / n_lat
    phi = 2 * np.pi * np.arange(n_lon) / n_lon
    ring = np.stack([np.outer(np.sin(theta), np.cos(phi)), np.outer(np.cos(theta), np.ones(n_lon)),
                     np.outer(np.sin(theta), np.sin(phi))], axis=-1).reshape(-1, 3)
    v = np.concatenate([[[0, 1.0, 0]], ring, [[0, -1.0, 0]]]) * radius + np.asarray(centre, np.float64)
    south = 1 + (n_lat - 1) * n_lon
    f = []
    for j in range(n_lon):
        k = (j + 1) % n_lon
        f.append((0, 1 + k, 1 + j))
        for i in range(n_lat - 2):
            a, b = 1 + i * n_lon, 1 + (i + 1) * n_lon
            f += [(a + j, b + k, b + j), (a + j, a + k, b + k)]
        last = 1 + (n_lat - 2) * n_lon
        f.append((south, last + j, last + k))
    return v.astype(np.float32), np.asarray(f, np.int32)


def box_mesh(lo, hi):
    """axis-aligned box as 12 triangles, outward winding"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    v = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
         (1, 5, 7), (1, 7, 3)]
    return v.astype(np.float32), np.asarray(f, np.int32)


def grid_quad(lo, hi, z, nx, ny):
    """the rectangle [lo, hi] at height z as an nx x ny grid of cells, two triangles each"""
    xs, ys = np.linspace(lo[0], hi[0], nx + 1), np.linspace(lo[1], hi[1], ny + 1)
    gx, gy = np.meshgrid(xs, ys)
    v = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, float(z))], axis=1)
    f = []
    for j in range(ny):
        for i in range(nx):
            a = j * (nx + 1) + i
            f += [(a, a + 1, a + nx + 2), (a, a + nx + 2, a + nx + 1)]
    return v.astype(np.float32), np.asarray(f, np.int32)


def closed_edges(tris):
    """True when every undirected edge is shared by exactly two triangles"""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
    _, counts = np.unique(e, axis=0, return_counts=True)
    return bool((counts == 2).all())


def ray_sphere(origin, dirs, radius, centre=(0, 0, 0)):
    """distance along each unit ray to the sphere's first hit, nan where it misses"""
    oc = np.asarray(origin, np.float64) - np.asarray(centre, np.float64)
    b = dirs @ oc
    disc = b * b - (oc @ oc - radius * radius)
    with np.errstate(invalid="ignore"):
        return np.where(disc >= 0, -b - np.sqrt(np.maximum(disc, 0)), np.nan)


def ray_box(origin, dirs, lo, hi):
    """distance along each ray to the box's first hit (slab method), nan where it misses"""
    o, lo, hi = np.asarray(origin, np.float64), np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / dirs, (hi - o) / dirs
    tn, tf = np.minimum(t0, t1).max(axis=-1), np.maximum(t0, t1).min(axis=-1)
    return np.where((tn <= tf) & (tn > 0), tn, np.nan)


def ray_triangle(origin, d, a, b, c):
    """the point where the ray meets the triangle's plane"""
    n = np.cross(b - a, c - a)
    return origin + d * ((a - origin) @ n) / (d @ n)
