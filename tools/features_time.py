#!/usr/bin/env python3
"""What the first-hit feature buffers cost: rtx_features (both planes) on the
C2 frame (1920x1080, 486 spheres) or the C5 frame (100k spheres), timed by
device events on the context's stream (a torch stream; `--reps` calls between
two events, `--rounds` windows after a warm-up), beside the 1-spp cost pass of
the same configuration (rtx_debug_pixel_cost(1)), which traces at least one
segment per pixel through the same scans. The cost pass is a synchronous call
with an allocation and a readback in it, so its own kernel time comes from a
kernel trace of this tool:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python tools/features_time.py --config c2 --out OUT/events_c2.json
    python tools/features_time.py --merge OUT/events_c2.json --kernel-stats OUT/.../run_kernel_stats.csv

The merge step needs no GPU: it adds the trace's mean kernel times of
k_features and of the cost pass (k_render<false, true, ...>) to the record.

C2 only: one masked step of 10 samples over the three big spheres' pixels
(ids 1, 2, 3, grow 1) after refine 10 + 10, beside the uniform carried step
before it, both by the library's HIP events (rtx_get_stats).
Prints one JSON line (and writes it to --out).
"""
import argparse
import csv
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytrace-we-gpu_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=["c2", "c5"], default="c2")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20, help="rtx_features calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--out", default="")
ap.add_argument("--merge", default="", help="a record of an earlier run: add --kernel-stats to it (no GPU)")
ap.add_argument("--kernel-stats", default="", help="rocprofv3's kernel stats CSV of that run")
a = ap.parse_args()


def emit(rec):
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if a.merge:
    rec = json.load(open(a.merge))
    found = {}
    with open(a.kernel_stats, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            key = "k_features" if re.search(r"\bk_features\b", name) else \
                "cost_pass" if re.search(r"\bk_render<false, true", name) else None
            if key:
                found[key] = {"kernel": name, "calls": int(row["Calls"]), "mean_ms": float(row["AverageNs"]) * 1e-6,
                              "min_ms": float(row["MinNs"]) * 1e-6, "max_ms": float(row["MaxNs"]) * 1e-6}
    rec["kernel_trace"] = found
    emit(rec)
    sys.exit(0 if len(found) == 2 else 1)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtx  # noqa: E402

if a.config == "c2":
    world = rtx.random_world(11, depth=50, spp=100)
else:
    world = rtx.random_world(159, capacity=100000, depth=50, spp=16)
frame = rtx.camera_look_at(a.width, a.height, aspect=a.width / a.height)
px = a.width * a.height
stream = torch.cuda.Stream()
rec = {"tool": "features_time", "config": a.config, "width": a.width, "height": a.height, "spheres": world.count,
       "rounds": a.rounds, "reps": a.reps, "build": rtx.build_info()}
with rtx.Context(0, stream=stream.cuda_stream) as ctx:
    ctx.upload_world(world)
    ctx.set_frame(frame)
    rec["kernels"] = ctx.scene_info()["kernels"]
    geom, surf = ctx.alloc((a.height, a.width, 4)), ctx.alloc((a.height, a.width, 4))
    for _ in range(3):  # warm-up
        ctx.features_rows(1, 0, 1, geom.ptr, surf.ptr)
    ctx.debug_pixel_cost(1)
    ctx.sync()
    feat, cost_wall = [], []
    for _ in range(a.rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            ctx.features_rows(1, 0, 1, geom.ptr, surf.ptr)
        e1.record(stream)
        e1.synchronize()
        feat.append(e0.elapsed_time(e1) / a.reps)
        t0 = time.perf_counter()
        cost = ctx.debug_pixel_cost(1)  # synchronous: allocation, kernel, readback
        cost_wall.append((time.perf_counter() - t0) * 1e3)
    s = surf.numpy()[..., 3]
    rec["features_ms"] = {"mean": round(float(np.mean(feat)), 4), "min": round(min(feat), 4), "max": round(max(feat), 4)}
    rec["cost_pass_call_wall_ms"] = {"mean": round(float(np.mean(cost_wall)), 4), "min": round(min(cost_wall), 4),
                                     "max": round(max(cost_wall), 4)}
    rec["cost_pass_segments_per_pixel"] = round(float(cost.mean()), 4)
    rec["miss_share"] = round(float((s < 0).mean()), 4)
    rec["distinct_ids"] = int(len(np.unique(s[s >= 0])))
    if a.config == "c2":
        ctx.set_refine_keys("carried")
        mask, covered = ctx.mask_from_ids(surf, (1, 2, 3), 1)
        carried, masked, active = [], [], 0
        for r in range(a.rounds + 1):  # round 0: warm-up
            ctx.refine(10, reset=True)
            ctx.stats_reset()
            ctx.refine(10)
            c_ms = ctx.stats().kernel_ms
            ctx.stats_reset()
            active = ctx.refine_masked(10, mask)
            m_ms = ctx.stats().kernel_ms
            if r:
                carried.append(c_ms)
                masked.append(m_ms)
        rec["masked_step"] = {"samples": 10, "ids": [1, 2, 3], "grow": 1, "mask_share": round(covered / px, 4),
                              "active": active,
                              "masked_ms": {"mean": round(float(np.mean(masked)), 4), "min": round(min(masked), 4),
                                            "max": round(max(masked), 4)},
                              "uniform_carried_ms": {"mean": round(float(np.mean(carried)), 4),
                                                     "min": round(min(carried), 4), "max": round(max(carried), 4)}}
        mask.free()
    geom.free()
    surf.free()
emit(rec)
