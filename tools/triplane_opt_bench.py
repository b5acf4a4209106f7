#!/usr/bin/env python3
"""Full-size direct triplane fit (drag_utils.py:473-550, train_triplane_opt) on one GPU: S = 128, 200 000 occupancy samples
of a sphere mesh (device sampling), 20 epochs x 5 batches of 40 000, synthetic decoder weights.  Prints one JSON line:
the fit time (median of --reps after a warm-up), ms per step, the sampling time and the final loss.

    python tools/triplane_opt_bench.py [--reps 5] [--epochs 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--batch", type=int, default=40000)
    a = ap.parse_args()
    import torch
    from ishapediting_amd import mesh as mesh_backend, synthetic
    from ishapediting_amd.triplane_decoder import MultiTriplane, fit_triplanes, total_loss
    dev = torch.device("cuda", 0)
    dec = MultiTriplane(1, device=dev)
    dec.net.load_state_dict(synthetic.decoder_state_dict(4321))
    ax = torch.arange(64, dtype=torch.float32, device=dev) - 31.5
    sph = 20.0 - torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    v, f = mesh_backend.extract_surface(sph)
    mesh = (v / 63 * 2 - 1, f)

    def sample():
        return mesh_backend.sample_occupancy(mesh, None, True, a.points, 0.5, device=dev,
                                             generator=torch.Generator().manual_seed(0))
    sample()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pts, occ = sample()
    torch.cuda.synchronize()
    t_sample = time.perf_counter() - t0
    g = torch.Generator(device=dev).manual_seed(1)
    init = torch.randn((1, 96, 128, 128), generator=g, device=dev) * 0.3
    fit_triplanes(dec, pts, occ, init, epochs=1, batch_size=a.batch, generator=g)        # warm-up
    times = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        planes, losses = fit_triplanes(dec, pts, occ, init, epochs=a.epochs, batch_size=a.batch, generator=g)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    times.sort()
    fit = times[len(times) // 2]
    tot = total_loss(losses)
    print(json.dumps({"metric": "triplane_opt_fit", "S": 128, "points": a.points, "steps": int(losses.shape[0]),
                      "fit_s": round(fit, 5), "fit_s_min": round(times[0], 5),
                      "ms_per_step": round(fit * 1e3 / losses.shape[0], 4), "sampling_s": round(t_sample, 5),
                      "loss_first": float(tot[0]), "loss_last": float(tot[-1]),
                      "finite": bool(torch.isfinite(planes).all())}))


if __name__ == "__main__":
    main()
