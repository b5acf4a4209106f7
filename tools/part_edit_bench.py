"""Times of the part-edit step on the device: regions.select_part, sample_handles (n = 16 and 64) and transform_region at D = 256.

The shape is the one bench.py edits on rank 0 (bench.make_dragstuff: UNet seed 1234, decoder seed 4321, synthetic.latent(0), 200
DDPM steps) decoded at 256^3; the part is what of it lies in a box around the origin.  Each call is timed between two device events
after warm-up calls (medians; the calls include their scratch and output allocations and their one read-back of a count).

For comparison only, with no bar: the same farthest-point loop written with torch device ops -- torch.minimum + argmax per round
over the candidates' coordinates, no host synchronisation between rounds.  (argmax names the first maximum, which is the lowest
linear index here, so its picks are compared with the kernel's.)

    python tools/part_edit_bench.py [--out profiles/part_edit_bench.txt] [--res 256] [--warmup 3] [--repeat 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, repeat):
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
    return float(np.median(ms)), float(ms[0]), float(ms[-1])


def torch_fps(mask, n):
    """The farthest-point loop in torch device ops: int64 coordinates [M, 3] in ascending linear index, first pick farthest from
    the centre of the bounding box, then minimum + argmax per round.  -> voxels int64 [n, 3] on the device"""
    coords = torch.nonzero(mask)                                     # the compaction (synchronises: the size is data dependent)
    lo, hi = coords.min(dim=0).values, coords.max(dim=0).values
    k = torch.argmax(((2 * coords - (lo + hi)) ** 2).sum(dim=1))
    picks = [coords[k]]
    mind = torch.full((coords.shape[0],), torch.iinfo(torch.int64).max, dtype=torch.int64, device=mask.device)
    for _ in range(1, n):
        mind = torch.minimum(mind, ((coords - picks[-1]) ** 2).sum(dim=1))
        picks.append(coords[torch.argmax(mind)])
    return torch.stack(picks)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "part_edit_bench.txt"))
    p.add_argument("--res", type=int, default=256)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeat", type=int, default=20)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("part_edit_bench needs the GPU: nothing here has a CPU path")
    import bench
    from ishapediting_amd import synthetic
    from ishapediting_amd.regions import Box, Rigid, sample_handles, select_part, transform_region
    dev = torch.device("cuda", 0)
    bench.RES = a.res
    ds = bench.make_dragstuff(dev, 1234)                             # rank 0 of bench.py: its weights, its 200 steps, its latent
    ds.update_latent_params(img=synthetic.latent(0))
    vol = ds.volume
    D = int(vol.shape[0])
    within = Box((-0.6, -0.6, -0.6), (0.6, 0.6, 0.6))
    rigid = Rigid(rotation=((0.2, -0.3, 1.0), 20.0), pivot=(0.1, -0.1, 0.0), translation=(0.04, 0.02, -0.03))
    part = select_part(vol, within)                                  # raises if the shape has nothing in the box
    M, inside = int(part.mask.sum()), int((vol > 0).sum())
    lines = [f"part edit step at D = {D} on {torch.cuda.get_device_name(0)}: {inside} voxels inside the shape, {M} in the part (box +-0.6)",
             f"device events around each call, median (min .. max) of {a.repeat} after {a.warmup} warm-up calls", ""]
    rows = [("select_part (box)", lambda: select_part(vol, within)),
            ("select_part (box, point: + label_volume)", None),
            ("sample_handles n = 16", lambda: sample_handles(part, 16)),
            ("sample_handles n = 64", lambda: sample_handles(part, 64)),
            ("transform_region", lambda: transform_region(part, rigid)),
            ("torch loop n = 16 (comparison)", lambda: torch_fps(part.mask, 16)),
            ("torch loop n = 64 (comparison)", lambda: torch_fps(part.mask, 64))]
    at = sample_handles(part, 1).points[0].cpu().numpy()             # a point of the part, for the labelled selection
    rows[1] = (rows[1][0], lambda: select_part(vol, within, point=at))
    for name, fn in rows:
        med, lo, hi = timed(fn, a.warmup, a.repeat)
        lines.append(f"{name:44s} {med:9.3f} ms  ({lo:.3f} .. {hi:.3f})")
    for n in (16, 64):
        same = bool(torch.equal(torch_fps(part.mask, n), sample_handles(part, n).voxels.to(torch.int64)))
        lines.append(f"torch loop and kernel pick the same {n} voxels: {same}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
