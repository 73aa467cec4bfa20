#!/usr/bin/env python3
"""What a refine step costs per part of a row split: the C2 frame (1920x1080,
486 spheres, depth 50) to --spp samples per pixel as --steps equal steps of
rtx_refine_rows, for R = 1, 2, 4, 8 members. The box has one GPU, so this is
the rehearsal tools/part_scaling.py runs for the plain render: each part of an
R-way split (tiles of --tile-rows rows) is refined ALONE on the one GPU, every
step timed by the library's HIP events (rtx_get_stats), each part after a
warm-up run of its own, `--rounds` timed runs. On R GPUs the parts would run
side by side, so the step time of a group is PROJECTED as its slowest
("critical") part's step time; the gather and the de-interleave are not in it,
and nothing here measures scaling. RCCL has only ever run with one rank and
peer copies have never run.

Prints one JSON line; --out FILE also writes it there.

    python tools/refine_group_steps.py [--rounds 2] [--keys carried] [--out profiles/refine_group_c2.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytrace-we-gpu_amd"))
import numpy as np  # noqa: E402
import rtx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--spp", type=int, default=100)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--tile-rows", type=int, default=5)
ap.add_argument("--members", default="1,2,4,8")
ap.add_argument("--keys", choices=["prepass", "carried"], default="prepass")
ap.add_argument("--out", default="")
a = ap.parse_args()
if a.steps < 1 or a.spp % a.steps != 0:
    sys.exit("--spp must be a multiple of --steps")
s = a.spp // a.steps
world = rtx.random_world(11, depth=50, spp=a.spp)
frame = rtx.camera_look_at(a.width, a.height, aspect=a.width / a.height)
T = a.tile_rows


def run(ctx, out, part, R):
    """One part through all steps from a reset: per-step kernel ms, and its segments."""
    ms, segs = [], 0
    for k in range(a.steps):
        ctx.stats_reset()
        ctx.refine_rows(T, part, R, s, reset=(k == 0), d_out=out.ptr)
        st = ctx.stats()
        ms.append(st.kernel_ms)
        segs += st.segments
    return ms, segs


result = {}
with rtx.Context(0) as ctx:
    ctx.upload_world(world)
    ctx.set_frame(frame)
    ctx.set_refine_keys(a.keys)
    out = ctx.alloc((a.height, a.width, 4))
    whole_segs = None
    for R in [int(r) for r in a.members.split(",") if r]:
        parts, total_segs = [], 0
        for part in range(R):
            rows = rtx.part_rows(a.height, T, part, R)
            if rows == 0:
                parts.append({"part": part, "rows": 0})
                continue
            _, segs = run(ctx, out, part, R)  # warm-up (and the buffers sized for this part)
            t = np.array([run(ctx, out, part, R)[0] for _ in range(a.rounds)])  # [round][step]
            total_segs += segs
            parts.append({"part": part, "rows": rows, "segments": segs,
                          "first_step_ms": round(float(t[:, 0].mean()), 3),
                          "step_ms_mean": round(float(t[:, 1:].mean()), 3) if a.steps > 1 else None,
                          "step_ms_min": round(float(t[:, 1:].min()), 3) if a.steps > 1 else None,
                          "step_ms_max": round(float(t[:, 1:].max()), 3) if a.steps > 1 else None,
                          "total_ms_mean": round(float(t.sum(axis=1).mean()), 3)})
        if whole_segs is None:
            whole_segs = total_segs
        live = [p for p in parts if p["rows"]]
        crit = max(live, key=lambda p: p["total_ms_mean"])
        result[str(R)] = {"parts": parts, "segments": total_segs, "segments_equal_whole": total_segs == whole_segs,
                          "sum_of_parts_total_ms": round(sum(p["total_ms_mean"] for p in live), 3),
                          "projected_critical_part": crit["part"],
                          "projected_step_ms": crit["step_ms_mean"],
                          "projected_first_step_ms": crit["first_step_ms"],
                          "projected_total_ms": crit["total_ms_mean"]}
    out.free()
doc = {"tool": "refine_group_steps", "width": a.width, "height": a.height, "spheres": world.count,
       "depth": world.depth, "spp": a.spp, "steps": a.steps, "step_samples": s, "tile_rows": T, "keys": a.keys,
       "rounds": a.rounds, "build": rtx.build_info(),
       "note": "each part timed alone on one GPU; projected_* is the slowest part's time, a projection, not a "
               "measurement of R GPUs; gather and de-interleave not included",
       "members": result}
line = json.dumps(doc)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if all(r["segments_equal_whole"] for r in result.values()) else 1)
