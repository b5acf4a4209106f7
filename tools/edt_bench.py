"""Times of the exact distance transform (csrc/edt.hip) and of what is built on it, on the device.

The shape is the one bench.py edits on rank 0 (bench.make_dragstuff: UNet seed 1234, decoder seed 4321, synthetic.latent(0), 200
DDPM steps) decoded at 256^3; the part is what of it lies in a box around the origin.  Each call is timed between two device
events after warm-up calls (medians; the Python calls include their scratch and output allocations).  One more call, timed once,
shows that the limit runs: 1024^3 voxels with eight seeds.

    python tools/edt_bench.py [--out profiles/edt_bench.txt] [--res 256] [--warmup 3] [--repeat 20] [--big 1024]
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


def edt_call(seeds, invert):
    """ishap_edt alone on a uint8 [n0, n1, n2] device tensor, its buffers allocated once: -> (call, dist2)"""
    from ishapediting_amd import _lib
    L = _lib.lib()
    n0, n1, n2 = seeds.shape
    nbytes = int(L.ishap_edt_scratch_bytes(n0, n1, n2, 7))
    out = torch.empty((n0, n1, n2), dtype=torch.int32, device=seeds.device)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=seeds.device)

    def call():
        _lib.check(L.ishap_edt(seeds.data_ptr(), n0, n1, n2, 7, invert, out.data_ptr(), scratch.data_ptr(), nbytes,
                               _lib.stream_ptr(seeds.device)))
    return call, out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "edt_bench.txt"))
    p.add_argument("--res", type=int, default=256)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--repeat", type=int, default=20)
    p.add_argument("--big", type=int, default=1024, help="side of the one large call (0: skip it)")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("edt_bench needs the GPU: nothing here has a CPU path")
    import bench
    from ishapediting_amd import synthetic
    from ishapediting_amd.regions import Box, grow, plane_weights, select_part
    from ishapediting_amd.volume import EDT_INF, signed_distance
    dev = torch.device("cuda", 0)
    bench.RES = a.res
    ds = bench.make_dragstuff(dev, 1234)                             # rank 0 of bench.py: its weights, its 200 steps, its latent
    ds.update_latent_params(img=synthetic.latent(0))
    vol = ds.volume
    D = int(vol.shape[0])
    inside = (vol > 0).contiguous().view(torch.uint8)
    part = select_part(vol, Box((-0.6, -0.6, -0.6), (0.6, 0.6, 0.6)))
    n_in, n_part = int(inside.sum()), int(part.mask.sum())
    in_call, d_in = edt_call(inside, 0)
    out_call, d_out = edt_call(inside, 1)
    in_call(), out_call()
    lines = [f"distance transform at D = {D} on {torch.cuda.get_device_name(0)}: {n_in} voxels inside the shape, {n_part} in the part (box +-0.6)",
             f"largest distance to the shape {float(d_in.max()) ** 0.5:.2f} voxels, largest depth inside it {float(d_out.max()) ** 0.5:.2f} voxels",
             f"device events around each call, median (min .. max) of {a.repeat} after {a.warmup} warm-up calls", ""]
    rows = [("ishap_edt, seeds = inside voxels", in_call),
            ("ishap_edt, seeds = outside voxels (invert)", out_call),
            ("signed_distance", lambda: signed_distance(vol)),
            ("grow(part, 4)", lambda: grow(part, 4)),
            ("plane_weights W = 128, free = part, hard", lambda: plane_weights(free=part, W=128, device=dev)),
            ("plane_weights W = 128, free = part, falloff 8", lambda: plane_weights(free=part, W=128, device=dev, falloff=8))]
    for name, fn in rows:
        med, lo, hi = timed(fn, a.warmup, a.repeat)
        lines.append(f"{name:48s} {med:9.3f} ms  ({lo:.3f} .. {hi:.3f})")
    if a.big:
        del d_in, d_out, in_call, out_call
        torch.cuda.empty_cache()
        B = a.big
        seeds = torch.zeros((B, B, B), dtype=torch.uint8, device=dev)
        picks = np.random.default_rng(B).integers(0, B, size=(8, 3))
        for s in picks:
            seeds[tuple(int(v) for v in s)] = 1
        call, out = edt_call(seeds, 0)
        med, _, _ = timed(call, 0, 1)
        probe = np.random.default_rng(1).integers(0, B, size=(4096, 3))
        want = ((probe[:, None, :] - picks[None, :, :]) ** 2).sum(-1).min(1)
        idx = torch.from_numpy(probe).to(dev)
        got = out[idx[:, 0], idx[:, 1], idx[:, 2]].cpu().numpy()
        lines += ["", f"one call at {B}^3 with 8 seeds (the limit: {4 * B ** 3 / 2 ** 30:.0f} GiB of distances, as much scratch): {med:.1f} ms; "
                      f"4096 probed voxels equal min over seeds: {bool(np.array_equal(got, want))}; no voxel at EDT_INF: {bool(out.max() < EDT_INF)}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
