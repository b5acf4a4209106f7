"""A drag edit without a window: generate a shape, pick handles by pixel, edit, save before / after pictures.

What the reference's GUI does with Open3D's scene widget (main.py:345-360, 492-517, 539-590, 611-612), with every stage on the
device: a synthetic-weight DragStuff denoises a latent (update_latent_params), the camera is fitted to the mesh, K handle
sources are picked by pixel from the depth picture (render.pick: unproject + nearest vertex), the targets are the sources
moved by --offset, training() runs the guided loop, and before.png / after.png show the mesh with the red / blue handle
spheres and green arrows.  With synthetic weights the decoded shape is noise; the path is the point.

  python tools/headless_edit.py --out /tmp/edit [--handles 3] [--num_steps 6] [--w_time 3] [--res 64] [--size 512] [--clean largest]
                                [--refine 4] [--mesh-resolution 512] [--simplify 2]

--mesh-resolution R (above --res) cuts every mesh at R from bricks near the surface only (DragStuff.mesh_resolution).
--simplify CELL reduces every mesh by quadric vertex clustering with cells of CELL voxels of the mesh's grid (DragStuff.mesh_simplify).
--clean largest keeps only the largest connected component of every decoded volume (DragStuff.clean, volume.clean_volume).
--refine N puts every mesh's smoothed vertices back on the decoder's zero level set with N projection steps of at most one voxel
in all (DragStuff.refine) and shades the pictures with the field's analytic normals.

Regions (repeatable): --keep-box x0 y0 z0 x1 y1 z1, --keep-sphere cx cy cz r hold a part of the shape, --free-box / --free-sphere
release one (ishapediting_amd.regions; --keep-weight, --free-weight, --region-dilate as DragStuff.training).  The boxes are drawn
into both pictures as wire frames (amber keep, teal free).  With regions the edit runs twice, without and with them, and the tool
prints for every region the fraction of the voxels inside it whose occupancy sign changed in each run: a report, not a check --
on synthetic weights the direction is not guaranteed.

A part edit: --part-box x0 y0 z0 x1 y1 z1 / --part-sphere cx cy cz r select the part (the shape inside them; --part-at x,y,z keeps
only the connected piece at that point), --rotate ax,ay,az,deg --pivot x,y,z --translate x,y,z move it rigidly, and --handles n
handles are spread over the part instead of picked by pixel (DragStuff.training_part; --offset is not used; write a list that
starts with a minus sign with an equals sign, --pivot=-0.2,0,0).  The part and the
place it moves to are the free regions; --keep-* still apply.  The pictures show the handles, their targets and the selecting
boxes.  Each handle's lattice only translates, so a rotation is approximated by the handles' different displacements; with
synthetic weights nobody can judge how good the result looks.  --neck V (with --part-at) cuts the selection at necks thinner
than 2 V voxels and keeps the piece on the point's side; --margin V also frees what lies within V voxels of the part and of its
new place; the voxel counts before and after are printed.  --region-falloff T feathers the edges of every region's weights over
T texels of the planes instead of a jump.

--track [R,rp,every] (default 4,2,1) re-finds every handle in feature space after every `every`-th guided step
(DragStuff.training(track=...), HandleTracker: search radius R, patch radius rp, in voxels of the handle lattice), prints for each
handle where it ended up -- offset in voxels, distance to its target in voxels, share of the requested move covered -- writes the
table and the whole track to track.json next to the pictures, and marks each handle's last tracked position in after.png with a
yellow sphere.  A handle that has not moved keeps its mark inside the red source sphere; with synthetic weights the features are
noise and that is the usual outcome.

--closed-loop STEP [--arrive A] [--stop] closes the loop (DragStuff.training(closed_loop=...)): after every tracked
step the loss is re-aimed at a goal STEP voxels from each handle's tracked position towards its target; --arrive A (default 1) is
the distance, in voxels, at which a handle counts as arrived, and with --stop the edit finishes unguided once all have.  It turns
--track on; the table gains each handle's remaining distance in voxels (after the last tracked step) and whether it has arrived,
and track.json the goals and remaining distances of every tracked step.

--keep3d-box / --carve-box / --fill-box X0 Y0 Z0 X1 Y1 Z1 (each may repeat) [--volume-scale V] constrain boxes in the VOLUME,
through the decoder (DragStuff.training(volume_keep=, carve=, fill=)): keep the decoded occupancy of the box,
empty it, or fill it.  With a part edit, --solid makes the place the part moves to fill and the place it leaves clear
(training_part(solid=True)).  Either costs one more full-depth backward per guided step.

--time instead measures the renderer alone (device events around `--repeat` calls after a warm-up, medians):
  the 256^3 sphere mesh (~300 k triangles of a few pixels each) at 1024 x 1024, and 2 picture-filling triangles at 1024 x 1024
  (the second shows that large triangles do not serialise on one lane), next to the bytes each call has to move
  (vertices + triangles + 8 B per pixel of visibility + the three outputs).  Written to profiles/render_times.json.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pick_sources(mesh, camera, depth, k, seed):
    """k distinct surface pixels (seeded) -> [(vertex position, vertex index, depth, (x, y))]"""
    from ishapediting_amd.render import pick
    ys, xs = np.nonzero(depth.cpu().numpy() < 1.0)
    if len(ys) < k:
        raise RuntimeError(f"only {len(ys)} surface pixels for {k} handles")
    out, seen = [], set()
    for j in np.random.default_rng(seed).permutation(len(ys)):
        pos, idx, d = pick(mesh, camera, depth, int(xs[j]), int(ys[j]))
        if idx not in seen:
            seen.add(idx)
            out.append((pos, idx, d, (int(xs[j]), int(ys[j]))))
        if len(out) == k:
            break
    return out


def regions_of(a):
    """the command line's regions -> (keep list, free list, frames for edit_parts, [(name, inside(x, y, z) -> bool array)])"""
    from ishapediting_amd.regions import Box, Sphere
    from ishapediting_amd.render import FREE_COLOUR, KEEP_COLOUR, marker_box
    keep, free, frames, named = [], [], [], []
    for role, dst, colour, boxes, spheres in (("keep", keep, KEEP_COLOUR, a.keep_box, a.keep_sphere),
                                              ("free", free, FREE_COLOUR, a.free_box, a.free_sphere)):
        for b in boxes or []:
            lo, hi = np.asarray(b[:3], np.float64), np.asarray(b[3:], np.float64)
            dst.append(Box(lo, hi))
            frames.append((marker_box(lo, hi), colour))
            named.append((f"{role}-box {b}", lambda x, y, z, lo=lo, hi=hi: (x >= lo[0]) & (x <= hi[0]) & (y >= lo[1]) & (y <= hi[1])
                          & (z >= lo[2]) & (z <= hi[2])))
        for sp in spheres or []:
            c, r = np.asarray(sp[:3], np.float64), float(sp[3])
            dst.append(Sphere(c, r))
            named.append((f"{role}-sphere {sp}", lambda x, y, z, c=c, r=r: (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r * r))
    return keep, free, frames, named


def _csv(text, n, what):
    try:
        v = [float(x) for x in text.split(",")]
    except ValueError:
        v = []
    if len(v) != n:
        raise SystemExit(f"{what}: {n} comma-separated numbers expected, got {text!r}")
    return v


def part_of(a, volume):
    """the command line's part edit -> (part Voxels, Rigid, frames of the selecting boxes), or None without --part-box / --part-sphere"""
    from ishapediting_amd.regions import Box, Rigid, Sphere, select_part
    from ishapediting_amd.render import FREE_COLOUR, marker_box
    if not (a.part_box or a.part_sphere):
        if a.part_at or a.rotate or a.pivot or a.translate:
            raise SystemExit("--part-at / --rotate / --pivot / --translate describe a part edit: give --part-box or --part-sphere")
        return None
    if a.free_box or a.free_sphere:
        raise SystemExit("a part edit frees the part and the place it moves to: --free-box / --free-sphere do not go with it")
    within, frames = [], []
    for b in a.part_box or []:
        within.append(Box(b[:3], b[3:]))
        frames.append((marker_box(np.asarray(b[:3], np.float64), np.asarray(b[3:], np.float64)), FREE_COLOUR))
    for sp in a.part_sphere or []:
        within.append(Sphere(sp[:3], sp[3]))
    at = _csv(a.part_at, 3, "--part-at") if a.part_at else None
    if a.neck and at is None:
        raise SystemExit("--neck cuts the selection at necks on the way from a point: give --part-at")
    part = select_part(volume, within, point=at, neck=a.neck)
    if a.neck:
        print(f"part: {int(select_part(volume, within, point=at).mask.sum())} voxels connected to --part-at, "
              f"{int(part.mask.sum())} after cutting necks thinner than {2 * a.neck:g} voxels")
    rot = _csv(a.rotate, 4, "--rotate") if a.rotate else None
    rigid = Rigid(rotation=(rot[:3], rot[3]) if rot else None, pivot=_csv(a.pivot, 3, "--pivot") if a.pivot else (0.0, 0.0, 0.0),
                  translation=_csv(a.translate, 3, "--translate") if a.translate else (0.0, 0.0, 0.0))
    return part, rigid, frames


TRACK_COLOUR = (1.0, 1.0, 0.0)       # yellow: a handle's last tracked position


def track_of(a):
    """--track -> the `track` keyword of DragStuff.training (None without it)"""
    if a.track is None:
        return None
    R, rp, every = (int(v) for v in _csv(a.track, 3, "--track"))
    return {"radius": R, "patch": rp, "every": every}


def closed_loop_of(a):
    """--closed-loop / --arrive / --stop -> the `closed_loop` keyword of DragStuff.training (None without --closed-loop)"""
    if a.closed_loop is None:
        if a.arrive is not None or a.stop:
            raise SystemExit("--arrive / --stop belong to --closed-loop STEP")
        return None
    return {"step": a.closed_loop, "arrive": 1.0 if a.arrive is None else a.arrive, "stop": bool(a.stop)}


def track_report(ds, sources, targets):
    """the per-handle table of the last tracked edit (printed) and the JSON that goes next to the pictures"""
    tr, err = ds.last_track, ds.handle_error()
    closed = "goals" in tr
    last, pos = tr["offsets"][-1].cpu().tolist(), tr["positions"][-1].cpu().tolist()
    rows = [{"handle": b, "source": [float(v) for v in sources[b]], "target": [float(v) for v in targets[b]], "offset_voxels": last[b],
             "position": pos[b], "error_voxels": float(err["error"][b]), "fraction": float(err["fraction"][b]),
             "dist": float(tr["dist"][-1, b]), "dist0": float(tr["dist0"][-1, b])} for b in range(len(last))]
    if closed:
        for b, r in enumerate(rows):
            r.update(remaining_voxels=float(tr["remaining_after"][b]), arrived=bool(tr["arrived_after"][b]))
    print("handle  offset (voxels)      error (voxels)  covered   D(k*) / D(0)" + ("      remaining (voxels)" if closed else ""))
    for r in rows:
        print(f"{r['handle']:6d}  {str(r['offset_voxels']):19s}  {r['error_voxels']:14.2f}  {100 * r['fraction']:6.1f} %  "
              f"{r['dist']:.4g} / {r['dist0']:.4g}" + (f"  {r['remaining_voxels']:10.3f}{' arrived' if r['arrived'] else ''}" if closed else ""))
    out = {"radius": tr["radius"], "patch": tr["patch"], "steps": tr["steps"], "voxel": ds.voxel_size, "handles": rows,
           "offsets": tr["offsets"].cpu().tolist(), "dist": tr["dist"].cpu().tolist(), "dist0": tr["dist0"].cpu().tolist()}
    if closed:
        print(f"closed loop: lead {tr['step']} voxels, arrival within {tr['arrive']}, "
              + ("ran every guided step" if ds.last_stop is None else f"stopped before guided step {ds.last_stop}"))
        out.update(step=tr["step"], arrive=tr["arrive"], stopped_before=ds.last_stop, goals=tr["goals"].cpu().tolist(),
                   remaining=tr["remaining"].cpu().tolist(), arrived=tr["arrived"].cpu().tolist())
    return out


def changed_fraction(before, after, inside):
    """share of the voxels selected by `inside` (a bool grid) whose occupancy sign differs between two decoded volumes"""
    n = int(inside.sum())
    return float(((before > 0) != (after > 0))[inside].float().mean()) if n else float("nan")


def edit(a):
    from ishapediting_amd import synthetic
    from ishapediting_amd.drag_utils import DragStuff, get_args
    from ishapediting_amd.render import Camera, edit_parts, marker_sphere, render_mesh, save_picture
    from ishapediting_amd.unet_spec import full_config
    dev = torch.device("cuda", 0)
    os.makedirs(a.out, exist_ok=True)
    args = get_args(["--w_time", str(a.w_time), "--num_steps", str(a.num_steps), "--shape_resolution", str(a.res)])
    ds = DragStuff(dev, args=args)
    if a.clean is not None:
        ds.clean = {"keep": "largest" if a.clean == "largest" else int(a.clean)}
    if a.refine is not None:
        ds.refine = {"iterations": a.refine, "max_move": 2.0 / (a.res - 1)}
    ds.mesh_resolution = a.mesh_resolution
    ds.mesh_simplify = a.simplify
    ds.load_weights(synthetic.round_torso_to_fp16(synthetic.unet_state_dict(full_config(), 1234)), synthetic.decoder_state_dict(4321),
                    -0.05 * np.ones(96, np.float32), 0.05 * np.ones(96, np.float32))
    ds.update_latent_params(img=synthetic.latent(0))
    before = ds.mesh0
    if a.refine is not None:          # the renderer shades with a mesh's stored normals: the field's own
        before.compute_vertex_normals()
    v = before.vertices
    if v.shape[0] == 0:
        raise RuntimeError("the decoded volume has no surface")
    cam = Camera.fit(v.min(dim=0).values.cpu().numpy(), v.max(dim=0).values.cpu().numpy(), fov=60, aspect=1.0)   # main.py:611-612
    keep, free, frames, named = regions_of(a)
    volume0 = ds.volume.clone()
    part_edit = part_of(a, volume0)
    report, part_report = {}, None
    track, closed = track_of(a), closed_loop_of(a)
    tkw = {} if track is None else {"track": track}
    if closed is not None:
        tkw["closed_loop"] = closed
    # volume constraints: boxes constrained in the volume itself, through the decoder
    from ishapediting_amd.regions import Box
    vkw = {role: [Box(b[:3], b[3:]) for b in getattr(a, flag)]
           for role, flag in (("volume_keep", "keep3d_box"), ("carve", "carve_box"), ("fill", "fill_box")) if getattr(a, flag)}
    if a.solid and part_edit is None:
        raise SystemExit("--solid belongs to a part edit (--part-box / --part-sphere)")
    if vkw and part_edit is not None:
        raise SystemExit("--keep3d-box / --carve-box / --fill-box go with a handle edit; a part edit takes --solid")
    if vkw:
        print(f"volume constraints: {({k: len(v) for k, v in vkw.items()})} box(es), volume_scale "
              f"{a.volume_scale if a.volume_scale is not None else a.scale}")
        vkw["volume_res"] = min(a.res, 128)
        if a.volume_scale is not None:
            vkw["volume_scale"] = a.volume_scale
        tkw.update(vkw)
    if part_edit is not None:     # handles and targets come from the part and its motion; the plan is made when the edit is created
        part, rigid, part_frames = part_edit
        frames = frames + part_frames
        final = ds.training_part(part, rigid, handles=a.handles, scale=a.scale, cof=a.cof, keep=keep or None, keep_weight=a.keep_weight,
                                 free_weight=a.free_weight, region_dilate=a.region_dilate, margin=a.margin,
                                 region_falloff=a.region_falloff, **tkw,
                                 **({"solid": True, **({"volume_scale": a.volume_scale} if a.volume_scale is not None else {})} if a.solid else {}))
        plan = ds.part_plan
        sources, targets = plan.sources, plan.targets
        part_report = {"voxels": int(part.mask.sum()), "moved_voxels": int(plan.moved.mask.sum()), "margin": a.margin,
                       "free_voxels": [int(r.mask.sum()) for r in plan.free], "handles": int(sources.shape[0]),
                       "spacing": plan.spacing, "spacing_in_voxels": plan.spacing / ds.voxel_size, "r1": int(ds.r1),
                       "rotation": rigid.matrix.tolist(), "pivot": list(rigid.pivot), "translation": list(rigid.translation)}
        print(f"part: {part_report}")
        for s, t in zip(sources, targets):
            print(f"handle {s.tolist()} -> {t.tolist()}")
    else:
        first = render_mesh(before, cam, a.size, a.size)
        picked = pick_sources(before, cam, first.depth, a.handles, a.seed)
        sources = np.stack([p[0] for p in picked])
        targets = sources + np.asarray(a.offset, np.float32)
        for pos, idx, d, px in picked:
            print(f"pick pixel {px}: vertex {idx} at {pos.tolist()}, depth {d:.6f}")
        final = ds.training(sources, targets, scale=a.scale, cof=a.cof, keep=keep or None, free=free or None,
                            keep_weight=a.keep_weight, free_weight=a.free_weight, region_dilate=a.region_dilate,
                            **({"region_falloff": a.region_falloff} if (keep or free) else {}), **tkw)
    save_picture(os.path.join(a.out, "before.png"), render_mesh(edit_parts(before, sources, targets, boxes=frames), cam, a.size, a.size))
    if named:                # the same edit without the regions first: what they change is the difference of the two runs
        for _ in ds.training(sources, targets, scale=a.scale, cof=a.cof):
            pass
        plain = ds.volume.clone()
    for _ in final:
        pass
    if named:
        ax = torch.linspace(-1, 1, a.res, device=dev, dtype=torch.float64)
        x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
        for name, inside in named:
            m = inside(x, y, z)
            report[name] = {"voxels": int(m.sum()), "changed_without_regions": changed_fraction(volume0, plain, m),
                            "changed_with_regions": changed_fraction(volume0, ds.volume, m)}
            print(f"{name}: {report[name]}")
    if a.refine is not None:
        ds.mesh.compute_vertex_normals()
    after = edit_parts(ds.mesh, sources, targets, boxes=frames)
    tracked = None
    if track is not None or closed is not None:
        tracked = track_report(ds, np.asarray(sources), np.asarray(targets))
        with open(os.path.join(a.out, "track.json"), "w") as fh:
            json.dump(tracked, fh, indent=1)
            fh.write("\n")
        after += [(marker_sphere(np.asarray(r["position"], np.float64), radius=0.03), TRACK_COLOUR, False) for r in tracked["handles"]]
    save_picture(os.path.join(a.out, "after.png"), render_mesh(after, cam, a.size, a.size))
    torch.cuda.synchronize()
    print(json.dumps({"out": a.out, "handles": a.handles, "regions": report, "part": part_report,
                      "track": None if tracked is None else tracked["handles"], "before_triangles": int(before.triangles.shape[0]),
                      "after_triangles": int(ds.mesh.triangles.shape[0]), "camera": {"eye": list(cam.eye), "near": cam.near, "far": cam.far}}))


def timed(fn, warmup, repeat):
    """median and spread, in ms, of `repeat` calls after `warmup`, each between two device events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms[0]), "p90_ms": float(ms[int(0.9 * (len(ms) - 1))]), "calls": repeat}


def time_renderer(a):
    from ishapediting_amd.mesh import extract_surface
    from ishapediting_amd.render import Camera, render_arrays
    dev = torch.device("cuda", 0)
    side, res, r = 1024, 256, 90.4
    ax = torch.arange(res, dtype=torch.float32) - (res - 1) / 2
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    v, f = extract_surface((r - torch.sqrt(x * x + y * y + z * z)).to(dev))
    v = (v / (res - 1) * 2 - 1).contiguous()
    cam = Camera(eye=(0.4, 0.3, 2.5), centre=(0, 0, 0), fov=60, near=0.1, far=10)
    quad_v = torch.tensor([[-3, -3, 0], [3, -3, 0], [3, 3, 0], [-3, 3, 0]], dtype=torch.float32, device=dev)
    quad_f = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32, device=dev)

    def floor_bytes(nv, nt):        # vertices + triangles + visibility + rgb, depth, tri_id
        return 12 * nv + 12 * nt + side * side * (8 + 3 + 4 + 4)
    out = {"picture": [side, side], "method": "device events around one render_arrays call (scratch and output allocation included), "
           f"median of {a.repeat} after {a.warmup} warm-up calls", "device": torch.cuda.get_device_name(0)}
    covered = render_arrays(v, f, cam, side, side)
    out["mesh"] = {"triangles": int(f.shape[0]), "vertices": int(v.shape[0]), "coverage": float((covered.tri_id >= 0).float().mean()),
                   "floor_bytes": floor_bytes(v.shape[0], f.shape[0]), **timed(lambda: render_arrays(v, f, cam, side, side), a.warmup, a.repeat)}
    covered = render_arrays(quad_v, quad_f, cam, side, side)
    out["full_screen_quad"] = {"triangles": 2, "coverage": float((covered.tri_id >= 0).float().mean()), "floor_bytes": floor_bytes(4, 2),
                               **timed(lambda: render_arrays(quad_v, quad_f, cam, side, side), a.warmup, a.repeat)}
    path = a.time_out or os.path.join(ROOT, "profiles", "render_times.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


def build_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default="headless_edit_out")
    p.add_argument("--handles", type=int, default=3)
    p.add_argument("--offset", type=float, nargs=3, default=(0.0, 0.15, 0.0))
    p.add_argument("--num_steps", type=int, default=6)
    p.add_argument("--w_time", type=int, default=3)
    p.add_argument("--res", type=int, default=64)
    p.add_argument("--size", type=int, default=512)
    p.add_argument("--scale", type=float, default=1200.0)
    p.add_argument("--cof", type=float, default=0.4)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--clean", default=None, metavar="largest|K",
                   help="keep only the largest (or the K largest) connected components of each decoded volume")
    p.add_argument("--mesh-resolution", type=int, default=None, metavar="R",
                   help="above --res (up to 2048): every mesh at this resolution, cut from bricks near the surface only "
                        "(DragStuff.mesh_resolution); the volume, the metrics and the parts stay at --res")
    p.add_argument("--simplify", type=float, default=None, metavar="CELL",
                   help="reduce every mesh by quadric vertex clustering, cells of CELL voxels of the mesh's grid (DragStuff.mesh_simplify)")
    p.add_argument("--refine", type=int, default=None, metavar="N",
                   help="project the mesh vertices back onto the decoder's level set with N steps (DragStuff.refine)")
    for role in ("keep", "free"):
        p.add_argument(f"--{role}-box", type=float, nargs=6, action="append", metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                       help=f"a {role} region: the box x0 y0 z0 x1 y1 z1 in [-1, 1]^3 (repeatable)")
        p.add_argument(f"--{role}-sphere", type=float, nargs=4, action="append", metavar=("CX", "CY", "CZ", "R"),
                       help=f"a {role} region: the sphere cx cy cz r (repeatable)")
    p.add_argument("--part-box", type=float, nargs=6, action="append", metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                   help="a part edit: the part is the shape inside this box (repeatable, with --part-sphere: their union)")
    p.add_argument("--part-sphere", type=float, nargs=4, action="append", metavar=("CX", "CY", "CZ", "R"),
                   help="a part edit: the part is the shape inside this sphere (repeatable)")
    p.add_argument("--part-at", default=None, metavar="X,Y,Z", help="only the connected piece of the selection at this point")
    p.add_argument("--rotate", default=None, metavar="AX,AY,AZ,DEG", help="rotate the part by DEG degrees about the axis (AX, AY, AZ)")
    p.add_argument("--pivot", default=None, metavar="X,Y,Z", help="the point the rotation turns about (default: the origin)")
    p.add_argument("--translate", default=None, metavar="X,Y,Z", help="then move the part by this vector")
    for flag, what in (("keep3d", "keep the decoded occupancy of this box as it is"), ("carve", "this box must end up empty"),
                       ("fill", "this box must end up solid")):
        p.add_argument(f"--{flag}-box", type=float, nargs=6, action="append", metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                       help=f"volume constraint: {what} (constrained in 3-D through the decoder; one more full-depth backward per step)")
    p.add_argument("--volume-scale", type=float, default=None, metavar="V", help="guidance scale of the volume constraints (default: --scale)")
    p.add_argument("--solid", action="store_true", help="with a part edit: the place the part moves to must fill, the place it leaves must clear")
    p.add_argument("--keep-weight", type=float, default=4.0)
    p.add_argument("--free-weight", type=float, default=0.0)
    p.add_argument("--region-dilate", type=int, default=0)
    p.add_argument("--region-falloff", type=float, default=0.0, metavar="T",
                   help="feather the edges of the region weights over T texels of the planes (at most 64) instead of a jump")
    p.add_argument("--margin", type=float, default=0.0, metavar="V",
                   help="part edit: also free what lies within V voxels of the part and of the place it moves to")
    p.add_argument("--neck", type=float, default=0.0, metavar="V",
                   help="with --part-at: cut the selection at necks thinner than 2 V voxels, keep the piece on the point's side")
    p.add_argument("--track", nargs="?", const="4,2,1", default=None, metavar="R,RP,EVERY",
                   help="track the handles in feature space (search radius, patch radius, every n-th step; default 4,2,1)")
    p.add_argument("--closed-loop", type=float, default=None, metavar="STEP",
                   help="re-aim the loss STEP voxels ahead of each tracked handle after every tracked step (turns --track on)")
    p.add_argument("--arrive", type=float, default=None, metavar="A", help="with --closed-loop: a handle has arrived within A voxels (default 1)")
    p.add_argument("--stop", action="store_true", help="with --closed-loop: finish unguided once every handle has arrived")
    p.add_argument("--time", action="store_true", help="measure the renderer instead of running an edit")
    p.add_argument("--time_out", default=None, help="where --time writes its JSON (default profiles/render_times.json)")
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--repeat", type=int, default=200)
    return p


def main():
    a = build_parser().parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("headless_edit needs the GPU: rendering has no CPU fallback")
    (time_renderer if a.time else edit)(a)


if __name__ == "__main__":
    main()
