#!/usr/bin/env python3
"""What the volume constraints cost: the per-step loss call against the call it extends, and a constrained C3 edit against the
plain one.

  python tools/constrain_bench.py [--reps 4] [--warmup 1] [--call-reps 200] [--skip-edit] [--out profiles/constrain_bench.txt]

Call.  ishap_constraint_loss_grad (MultiTriplane.constraint_loss_grad: the point pass and the gather pass) at M = 16384 points,
S = 128, against ishap_triplane_points_loss_grad (MultiTriplane.points_loss_grad, the float-atomic scatter with its two
memsets) at the same M and S, same planes, weights, points and targets, alternating, each between two device events: median,
minimum and maximum of `call-reps` calls after 10 warm-up calls.  Two point sets: `box`, the voxel centres of a 26^3 box of a
128^3 grid cut to 16384 (what an edit's builder makes: rows of up to ~100 entries), and `uniform` points in the cube.  Next to
them ishap_constraint_setup, once per edit.  The two calls' dplanes are compared (max |difference| over max |value|).
Edit.  bench.py's C3 shape, weights and handles; one warm-up of each kind, then `reps` timed edits of each kind, interleaved
(plain, constrained, plain, ...), a device synchronise before each clock reading.  `constrained` carves one box and fills
another at the default 16384 points per role on a 128^3 grid, volume_scale = scale.  The plain edits restore the first-step
snapshot (from the second on), the constrained ones cannot: ms per step added = (constrained - plain) / guided steps counts that
forward too.  Writes the JSON (one line) and a readable table to --out and prints the JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from track_bench import event_ms  # noqa: E402  (tools/ is this script's own directory)

M, S = 16384, 128
CARVE, FILL = ((-0.6, -0.5, -0.5), (-0.2, 0.0, 0.0)), ((0.2, 0.0, 0.0), (0.6, 0.5, 0.5))


def point_sets(device):
    gen = torch.Generator().manual_seed(3)
    ax = 2.0 * torch.arange(128, dtype=torch.float64) / 127 - 1.0
    i = torch.arange(40, 66)
    g = torch.stack(torch.meshgrid(ax[i], ax[i], ax[i], indexing="ij"), dim=-1).reshape(-1, 3)[:M].float()
    return {"box": g.to(device), "uniform": (torch.rand(M, 3, generator=gen) * 2 - 1).to(device)}


def call_times(device, reps):
    import ctypes as C
    from ishapediting_amd import _lib, synthetic
    from ishapediting_amd.triplane_decoder import MultiTriplane
    dec = MultiTriplane(1, device=device)
    dec.net.load_state_dict(synthetic.decoder_state_dict())
    gen = torch.Generator().manual_seed(4)
    planes = (torch.randn(3, S, S, 32, generator=gen) * 0.02).to(device)
    gt = (torch.rand(M, generator=gen) < 0.5).float().to(device)
    ones = torch.ones(M, device=device)
    out = {"M": M, "S": S, "sets": {}}
    for name, pts in point_sets(device).items():
        setup = event_ms(lambda: dec.constraint_setup(pts, gt, ones, S), 3, 20)
        st = dec.constraint_setup(pts, gt, ones, S)
        dpl, loss = torch.empty_like(planes), torch.empty(1, device=device)
        # the C call alone, as the new one is timed: the transposed weight copies and the outputs made once
        sd, wc = dec.net.sd, dec.net.weights_c()
        w1t, w2t = sd["1.weight"].t().contiguous(), sd["3.weight"].t().contiguous()
        odpl, oloss, ologits = torch.empty_like(planes), torch.empty(1, device=device), torch.empty(M, device=device)

        def old_call(pts=pts):
            _lib.check(_lib.lib().ishap_triplane_points_loss_grad(planes.data_ptr(), S, C.byref(wc), w1t.data_ptr(), w2t.data_ptr(),
                                                                  pts.data_ptr(), gt.data_ptr(), M, odpl.data_ptr(), oloss.data_ptr(),
                                                                  ologits.data_ptr(), _lib.stream_ptr(device)))
        new, old = [], []
        for _ in range(5):                                    # alternate the two calls in blocks
            new.append(event_ms(lambda: dec.constraint_loss_grad(planes, st, dplanes=dpl, loss=loss), 10, reps // 5))
            old.append(event_ms(old_call, 10, reps // 5))
        fold = lambda rs: {"median_ms": round(float(np.median([r["median_ms"] for r in rs])), 4),      # noqa: E731
                           "min_ms": min(r["min_ms"] for r in rs), "max_ms": max(r["max_ms"] for r in rs),
                           "block_medians_ms": [r["median_ms"] for r in rs], "calls": sum(r["calls"] for r in rs)}
        ref = dec.points_loss_grad(planes, pts, gt)
        lg = torch.empty(M, device=device)
        dec.constraint_loss_grad(planes, st, dplanes=dpl, loss=loss, logits=lg)
        diff = float((dpl - ref[1]).abs().max() / ref[1].abs().max())
        # a point next to a ReLU kink may take the other branch in the other kernel (other sin / cos, other summation order): its
        # whole footprint, 12 texels x 32 channels, then differs by a finite amount.  Count the texels such differences sit on.
        off = ((dpl - ref[1]).abs() > 1e-4 * ref[1].abs().max()).any(dim=-1)
        rows = torch.diff(st.row_start)
        out["sets"][name] = {"constraint_loss_grad": fold(new), "points_loss_grad": fold(old), "constraint_setup": setup,
                             "entries": int(st.row_start[-1]), "longest_row": int(rows.max()), "rows_used": int((rows > 0).sum()),
                             "dplanes_rel_diff": diff, "texels_off_by_1e-4": int(off.sum()), "logits_max_diff": float((ologits - lg).abs().max()),
                             "loss_diff": abs(float(loss) - float(ref[0]))}
    return out


def edit_times(device, reps, warmup):
    from ishapediting_amd import synthetic
    from ishapediting_amd.regions import Box
    ds = bench.make_dragstuff(device, 1234)
    ds.update_latent_params(img=synthetic.latent(0))
    src, tgt = synthetic.handles(bench.HANDLES, seed=7)
    kinds = (("plain", {}), ("constrained", {"carve": Box(*CARVE), "fill": Box(*FILL)}))
    points = {}

    def edit(kind, kw):
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in ds.training(src, tgt, scale=1200, cof=0.4, **kw):       # bench.one_edit's arguments
            pass
        torch.cuda.synchronize()
        points[kind] = len(ds.last_volume_losses)
        return time.time() - t0
    for _ in range(warmup):
        for kind, kw in kinds:
            edit(kind, kw)
    times = {kind: [] for kind, _ in kinds}
    for _ in range(reps):
        for kind, kw in kinds:
            times[kind].append(edit(kind, kw))
    lv = [float(v) for v in ds.last_volume_losses]
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"guided_steps": bench.GUIDED_STEPS, "res": bench.RES, "handles": bench.HANDLES, "reps": reps, "warmup": warmup,
            **{f"{k}_s": [round(t, 4) for t in v] for k, v in times.items()}, **{f"{k}_median_s": round(m, 4) for k, m in med.items()},
            "added_ms_per_step": round(1e3 * (med["constrained"] - med["plain"]) / bench.GUIDED_STEPS, 3),
            "volume_loss_steps": points["constrained"], "L_vol_first": round(lv[0], 5), "L_vol_last": round(lv[-1], 5)}


def table(res):
    lines = [f"volume constraints on {res['device']}", ""]
    c = res["call"]
    lines.append(f"per-step loss call, M = {c['M']} points, S = {c['S']} (ms between device events: median [min .. max] of n calls)")
    for name, s in c["sets"].items():
        for key in ("constraint_loss_grad", "points_loss_grad", "constraint_setup"):
            t = s[key]
            lines.append(f"  {name:8s} {key:22s} {t['median_ms']:8.4f} [{t['min_ms']:.4f} .. {t['max_ms']:.4f}] n = {t['calls']}"
                         + (f"  block medians {t['block_medians_ms']}" if "block_medians_ms" in t else ""))
        lines.append(f"  {name:8s} entries {s['entries']}, rows used {s['rows_used']}, longest row {s['longest_row']}; "
                     f"dplanes max |new - old| / max |old| {s['dplanes_rel_diff']:.2e} ({s['texels_off_by_1e-4']} of {3 * c['S'] ** 2} texels "
                     f"differ by more than 1e-4 of the maximum: footprints of points at a ReLU kink), max |logit new - old| "
                     f"{s['logits_max_diff']:.2e}, |loss new - old| {s['loss_diff']:.2e}")
    if "edit" in res:
        e = res["edit"]
        lines += ["", f"C3 edit ({e['guided_steps']} guided steps, {e['res']}^3, {e['handles']} handles), seconds per shape, {e['reps']} interleaved repeats "
                  f"after {e['warmup']} warm-up", f"  plain        {e['plain_s']}  median {e['plain_median_s']}",
                  f"  constrained  {e['constrained_s']}  median {e['constrained_median_s']}",
                  f"  added per guided step: {e['added_ms_per_step']} ms (a full-depth backward, the loss call, and the first step's forward "
                  "that a plain edit restores)", f"  L_vol step 0 -> last: {e['L_vol_first']} -> {e['L_vol_last']}"]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--call-reps", type=int, default=200)
    ap.add_argument("--skip-edit", action="store_true", help="time the stand-alone calls only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrain_bench.txt"))
    a = ap.parse_args()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    torch.manual_seed(bench.RNG_SEED)
    np.random.seed(bench.RNG_SEED)
    res = {"metric": "volume constraints", "device": torch.cuda.get_device_name(device), "call": call_times(device, a.call_reps)}
    if not a.skip_edit:
        res["edit"] = edit_times(device, a.reps, a.warmup)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(table(res) + "\n" + line + "\n")
    print(line)


if __name__ == "__main__":
    main()
