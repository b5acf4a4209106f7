#!/usr/bin/env python3
"""Timing of the volume connected-components pass (ishapediting_amd/volume.py, csrc/components.hip; not part of bench.py) at
256^3 on three volumes:
  decoded    a smooth synthetic triplane through the synthetic-weight decoder, cut at its median (a shape-like level set)
  bernoulli  independent voxels, inside with probability 0.31 (near the 6-connectivity percolation threshold)
  ball       a solid ball of radius 100
For each: ishap_volume_label (connectivity 6 and 26, inside phase), the component table (count + emit with its one host
read-back), ishap_volume_flip of every component but the largest, and clean_volume(keep="largest") end to end, in
milliseconds (median of --reps after one warm-up; host clock around calls that end in a device synchronise), next to the
triplane decode and the surface extraction of the same volume.  Where scipy is importable, scipy.ndimage.label of the same mask
on the host is printed as context.  One JSON line.

    python tools/components_bench.py [--reps 5] [--res 256]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def decoded_volume(res, dev):
    """(volume - its median, the decode call): tools/parity_report.py's shape-like field"""
    import torch
    from ishapediting_amd import synthetic
    from ishapediting_amd.triplane_decoder import MultiTriplane, decode_volume
    S = 128
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, S), torch.linspace(-1, 1, S), indexing="ij")
    g = torch.Generator().manual_seed(17)
    lat = torch.zeros(1, 96, S, S)
    for c in range(96):
        a, b, p, q = torch.randn(4, generator=g)
        lat[0, c] = 0.005 * (a * torch.cos(1.5 * xx + p) + b * torch.cos(1.5 * yy + q))
    dec = MultiTriplane(1, device=dev)
    dec.net.load_state_dict(synthetic.decoder_state_dict(4321))
    lat = lat.to(dev)

    def decode():
        return decode_volume(dec, lat, 1.0, 0.0, res)
    vol = decode()
    return (vol - vol.median()).contiguous(), decode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--res", type=int, default=256)
    a = ap.parse_args()
    import torch
    from ishapediting_amd import volume as V
    from ishapediting_amd.mesh import extract_surface
    dev = torch.device("cuda", 0)
    res = a.res
    out = {"res": res, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    decoded, decode = decoded_volume(res, dev)
    out["decode_ms"] = timed(decode, a.reps)
    g = torch.Generator().manual_seed(31)
    bern = torch.where(torch.rand((res, res, res), generator=g) < 0.31, 1.0, -1.0).to(dev)
    ax = torch.arange(res, dtype=torch.float32, device=dev) - (res - 1) / 2
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    ball = (100.0 / 256 * res - torch.sqrt(x * x + y * y + z * z)).contiguous()
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    for name, vol in (("decoded", decoded), ("bernoulli", bern), ("ball", ball)):
        r = {"inside_voxels": int((vol > 0).sum())}
        scratch = V._scratch(vol)
        for conn in (6, 26):
            r[f"label_c{conn}_ms"] = timed(lambda: V._label(vol, 0.0, "inside", conn), a.reps)
        labels = V._label(vol, 0.0, "inside", 6)
        r["table_ms"] = timed(lambda: V._table(labels, scratch), a.reps)
        table = V._table(labels, scratch)
        r["components"] = int(table.shape[0])
        rest = table[:, 0][table[:, 1] != table[:, 1].max()].contiguous()
        flipped = torch.empty_like(vol)
        r["flip_ms"] = timed(lambda: V._flip(vol, flipped, labels, 0.0, rest, scratch), a.reps)
        r["clean_largest_ms"] = timed(lambda: V.clean_volume(vol, keep="largest"), a.reps)
        r["clean_largest_fill_ms"] = timed(lambda: V.clean_volume(vol, keep="largest", fill_cavities=True), a.reps)
        r["surface_ms"] = timed(lambda: extract_surface(vol, 0.0), a.reps)
        r["label_plus_flip_over_decode"] = (r["label_c6_ms"] + r["flip_ms"]) / out["decode_ms"]
        if ndimage is not None:
            mask = (vol > 0).cpu().numpy()
            t0 = time.perf_counter()
            _, count = ndimage.label(mask)
            r["scipy_ndimage_label_host_ms"] = (time.perf_counter() - t0) * 1e3
            r["scipy_components"] = int(count)
        out[name] = r

    def rnd(v):
        if isinstance(v, dict):
            return {k: rnd(w) for k, w in v.items()}
        return round(v, 4) if isinstance(v, float) else v
    print(json.dumps(rnd(out)))


if __name__ == "__main__":
    main()
