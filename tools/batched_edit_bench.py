#!/usr/bin/env python3
"""Per-shape time of batched C3 drag edits (DragStuff.training_batch) at K = 1, 2, 3, 4 (and 8) on one GPU.

  python tools/batched_edit_bench.py [--ks 1,2,3,4,8] [--reps 2] [--warmup 1] [--no-overlap-ab]

One batched step = K shapes edited in one guided loop: 40 guided iterations at batch K + K 256^3 decodes and surfaces (what
bench.py's step is for one shape).  bench.py's weights (make_dragstuff, seed 1234), generator seeds, latents
(synthetic.latent(k) for shape k) and handles (synthetic.handles(3, seed=7 + k)); the context is built with max_edits = K.
Timing as in bench.py: warm-up steps, then `reps` timed steps with a device synchronise before the clock stops.
For K > 1 the overlapped forward tail is timed on and off (the faster is reported as the K's figure) and the two are checked
bit for bit on one seeded edit.  Prints ONE JSON line.  Kernel statistics: run it under
`rocprofv3 --kernel-trace --stats -d DIR -o k4 -- python tools/batched_edit_bench.py --ks 4 --reps 1 --no-overlap-ab` on its
own, then `python tools/batched_edit_bench.py --trace-db DIR/.../k4_results.db` (no GPU) prints launches and kernel time per
guided step (the dispatches between two consecutive drag_batch_terms_kernel launches; steps that hold a decode are left out).
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


def make_batched(device, K):
    """bench.make_dragstuff with the model context built for K edits."""
    from ishapediting_amd import drag_utils as du
    base = du.DragStuff

    class DragStuffK(base):
        def __init__(self, *a, **kw):
            super().__init__(*a, max_edits=K, **kw)

    du.DragStuff = DragStuffK
    try:
        return bench.make_dragstuff(device, 1234)
    finally:
        du.DragStuff = base


def summarize_trace(db):
    """Per guided step of a rocprofv3 kernel-trace database: median launches, kernel time, span, and time by kernel class."""
    import collections
    import sqlite3
    import statistics as st
    rows = list(sqlite3.connect(db).execute("select name, start, end from kernels order by start"))
    marks = [i for i, r in enumerate(rows) if r[0].startswith("drag_batch_terms_kernel")]
    steps = [rows[a:b] for a, b in zip(marks, marks[1:])]
    span = [(s[-1][2] - s[0][1]) / 1e6 for s in steps]
    med = st.median(span)
    steps = [s for s, w in zip(steps, span) if w < 1.5 * med]
    classes = collections.defaultdict(lambda: [0, 0.0])
    for s in steps:
        for name, t0, t1 in s:
            k = ("drag" if "drag" in name else "ddpm step" if "ddpm" in name else "conv/gemm" if "igemm" in name
                 else "groupnorm" if "gn_" in name else "attention" if "att" in name else "other")
            classes[k][0] += 1
            classes[k][1] += (t1 - t0) / 1e6
    n = len(steps)
    return {"guided_steps": n, "launches_per_step": st.median(len(s) for s in steps),
            "kernel_ms_per_step": round(st.median(sum(r[2] - r[1] for r in s) / 1e6 for s in steps), 3),
            "span_ms_per_step": round(st.median((s[-1][2] - s[0][1]) / 1e6 for s in steps), 3),
            "by_class": {k: {"launches": round(v[0] / n, 1), "ms": round(v[1] / n, 3)} for k, v in classes.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace-db", default=None, help="summarise a rocprofv3 kernel-trace database of this tool and exit")
    ap.add_argument("--ks", default="1,2,3,4,8")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-overlap-ab", action="store_true", help="time the default tail setting only")
    a = ap.parse_args()
    if a.trace_db:
        print(json.dumps(summarize_trace(a.trace_db)))
        return
    from ishapediting_amd import synthetic
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    torch.manual_seed(bench.RNG_SEED)
    np.random.seed(bench.RNG_SEED)
    rows = {}
    for K in [int(k) for k in a.ks.split(",")]:
        try:
            ds = make_batched(device, K)
            lat = np.concatenate([synthetic.latent(k) for k in range(K)])
            hs = [synthetic.handles(bench.HANDLES, seed=7 + k) for k in range(K)]
            src, tgt = [h[0] for h in hs], [h[1] for h in hs]
            torch.cuda.synchronize()
            t0 = time.time()
            ds.update_latent_params_batch(lat)
            torch.cuda.synchronize()
            t_setup = time.time() - t0
        except torch.cuda.OutOfMemoryError as e:          # K = 8 "if memory allows"
            rows[str(K)] = {"error": f"out of memory: {e}"[:200]}
            continue

        def step():
            for _ in ds.training_batch(src, tgt, scale=1200, cof=0.4):       # bench.one_edit's arguments
                pass

        def timed(overlap):
            ds.overlap_tail = overlap
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.time()
            for _ in range(a.reps):
                step()
            torch.cuda.synchronize()
            return (time.time() - t0) / (a.reps * K)

        row = {"setup_s": round(t_setup, 3)}
        if K > 1 and not a.no_overlap_ab:
            finals = []
            for ov in (True, False):
                torch.cuda.manual_seed(bench.RNG_SEED)         # the same drawn step noise for both
                ds.overlap_tail = ov
                step()
                torch.cuda.synchronize()
                finals.append((ds.tri_feat_batch.clone(), torch.stack(ds.volumes).clone()))
            row["overlap_bitwise"] = bool(torch.equal(finals[0][0], finals[1][0]) and torch.equal(finals[0][1], finals[1][1]))
            del finals
            row["s_per_shape_overlap_on"] = round(timed(True), 4)
            row["s_per_shape_overlap_off"] = round(timed(False), 4)
            row["s_per_shape"] = min(row["s_per_shape_overlap_on"], row["s_per_shape_overlap_off"])
        else:
            row["s_per_shape"] = round(timed(None), 4)
        row["losses_finite"] = bool(all(bool(torch.isfinite(l).all()) for l in ds.last_losses))
        rows[str(K)] = row
        del ds
        torch.cuda.empty_cache()
    base = rows.get("1", {}).get("s_per_shape")
    for r in rows.values():
        if base and "s_per_shape" in r:
            r["speedup_per_shape_vs_k1"] = round(base / r["s_per_shape"], 3)
    print(json.dumps({"metric": "batched C3 drag edits: wall-clock per shape (s)", "unit": "s/shape",
                      "guided_steps": bench.GUIDED_STEPS, "res": bench.RES, "reps": a.reps, "warmup": a.warmup,
                      "device": torch.cuda.get_device_name(device), "by_k": rows}))


if __name__ == "__main__":
    main()
