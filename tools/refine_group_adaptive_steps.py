#!/usr/bin/env python3
"""What an adaptive refine step costs per part of a row split: the C2 frame
(1920x1080, 486 spheres, depth 50) in --steps steps of --samples samples
through rtx_refine_adaptive_rows at each of --thresholds, for R = 2, 4, 8
members, beside rtx_refine_adaptive on the whole frame. The box has one GPU,
so this is tools/refine_group_steps.py's rehearsal: each part of an R-way split
(tiles of --tile-rows rows) is driven ALONE on the one GPU with its true halos,
each part after a warm-up run of its own. The parts of a frame hold the
whole-frame maps bit for bit, so a part's true halo before step k is rows of
the whole-frame err map after step k - 1, which the whole-frame run records.

Per step and part: kernel_ms, the launch's HIP-event time (rtx_get_stats: the
sort, the render, the unpermute); edges_ms and mask_ms, host clock around
rtx_refine_edges + rtx_sync and around rtx_refine_pending_rows (the mask kernel
and its 4-byte readback); call_ms, host clock around rtx_refine_adaptive_rows +
rtx_sync, which holds a second mask, the image pass over the pixels the call
does not trace, and the launch; rest_ms = call_ms - kernel_ms - mask_ms, an
upper bound of the image pass. On R GPUs the parts would run side by side, so
a group's step is PROJECTED as the slowest part's edges + mask + call; the
halo exchange, the gather and the de-interleave are not measured, and nothing
here measures scaling. RCCL has only ever run with one rank and peer copies
have never run.

Prints one JSON line; --out FILE also writes it there.

    python tools/refine_group_adaptive_steps.py [--out profiles/refine_group_adaptive_c2.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytrace-we-gpu_amd"))
import numpy as np  # noqa: E402
import rtx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--samples", type=int, default=10)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--tile-rows", type=int, default=5)
ap.add_argument("--members", default="2,4,8")
ap.add_argument("--thresholds", default="0.05,0.1")
ap.add_argument("--repeats", type=int, default=5, help="timed whole-frame runs per threshold")
ap.add_argument("--out", default="")
a = ap.parse_args()
world = rtx.random_world(11, depth=50, spp=a.samples * a.steps)
frame = rtx.camera_look_at(a.width, a.height, aspect=a.width / a.height)
W, H, T, S = a.width, a.height, a.tile_rows, a.samples


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def whole(ctx, thr, keep_err):
    """The whole frame through all steps from a reset: per step (kernel ms, call ms, active), and the err
    map after each step."""
    rows, errs = [], []
    for k in range(a.steps):
        ctx.stats_reset()

        def call():
            n = ctx.refine_adaptive(S, thr, reset=(k == 0))
            ctx.sync()
            return n
        n, ms = clock(call)
        rows.append((ctx.stats().kernel_ms, ms, n))
        if keep_err:
            errs.append(ctx.refine_error())
    return rows, errs


def halo_of(err, part, R, tiles):
    """Part `part`'s halo before a step, from the whole-frame err map after the step before."""
    halo = np.full((2, tiles, W), np.nan, np.float32)
    ntiles = -(-H // T)
    for j in range(tiles):
        k = part + j * R
        if k > 0:
            halo[0, j] = err[k * T - 1]
        if k + 1 < ntiles:
            halo[1, j] = err[(k + 1) * T]
    return halo


def part_run(ctx, out, edges, halo, thr, errs, part, R, tiles):
    """One part through all steps from a reset: per step a dict of times."""
    steps = []
    for k in range(a.steps):
        first = k == 0
        if not first:
            halo.upload(halo_of(errs[k - 1], part, R, tiles))
        ctx.sync()
        _, edges_ms = (None, 0.0) if first else clock(lambda: (ctx.refine_edges(edges.ptr), ctx.sync()))
        # (a fresh start traces every pixel: no exchange, and nothing to ask before the reset)
        _, mask_ms = (None, 0.0) if first else clock(lambda: ctx.refine_pending_rows(T, part, R, S, thr,
                                                                                     d_halo=halo.ptr))
        ctx.stats_reset()

        def call():
            n = ctx.refine_adaptive_rows(T, part, R, S, thr, reset=first, d_halo=0 if first else halo.ptr,
                                         d_out=out.ptr)
            ctx.sync()
            return n
        n, call_ms = clock(call)
        st = ctx.stats()
        steps.append({"active": n, "kernel_ms": st.kernel_ms, "edges_ms": edges_ms, "mask_ms": mask_ms,
                      "call_ms": call_ms, "segments": st.segments})
    return steps


def r3(x):
    return round(float(x), 3)


doc_thr = {}
with rtx.Context(0) as ctx:
    ctx.upload_world(world)
    ctx.set_frame(frame)
    out = ctx.alloc((H, W, 4))
    for thr in [float(t) for t in a.thresholds.split(",") if t]:
        whole(ctx, thr, False)  # warm-up
        runs = [whole(ctx, thr, r == 0) for r in range(a.repeats)]
        errs = runs[0][1]
        k_ms = np.array([[s[0] for s in r[0]] for r in runs])  # [repeat][step]
        c_ms = np.array([[s[1] for s in r[0]] for r in runs])
        active = [s[2] for s in runs[0][0]]
        whole_doc = {"active": active, "step_kernel_ms": [r3(v) for v in k_ms.mean(axis=0)],
                     "step_call_ms": [r3(v) for v in c_ms.mean(axis=0)],
                     "total_kernel_ms": [r3(v) for v in k_ms.sum(axis=1)],
                     "total_call_ms": [r3(v) for v in c_ms.sum(axis=1)]}
        members = {}
        for R in [int(r) for r in a.members.split(",") if r]:
            parts = []
            for part in range(R):
                rows = rtx.part_rows(H, T, part, R)
                if rows == 0:
                    parts.append({"part": part, "rows": 0})
                    continue
                tiles = -(-rows // T)
                edges, halo = ctx.alloc((2, tiles, W)), ctx.alloc((2, tiles, W))
                part_run(ctx, out, edges, halo, thr, errs, part, R, tiles)  # warm-up
                steps = part_run(ctx, out, edges, halo, thr, errs, part, R, tiles)
                edges.free()
                halo.free()
                parts.append({"part": part, "rows": rows, "steps": steps})
            live = [p for p in parts if p["rows"]]
            per_step = []
            for k in range(a.steps):
                def cost(p):
                    s = p["steps"][k]
                    return s["edges_ms"] + s["mask_ms"] + s["call_ms"]
                crit = max(live, key=cost)
                s = crit["steps"][k]
                per_step.append({"critical_part": crit["part"], "projected_step_ms": r3(cost(crit)),
                                 "kernel_ms": r3(s["kernel_ms"]), "edges_ms": r3(s["edges_ms"]),
                                 "mask_ms": r3(s["mask_ms"]), "call_ms": r3(s["call_ms"]),
                                 "rest_ms": r3(s["call_ms"] - s["kernel_ms"] - s["mask_ms"]),
                                 "active": sum(p["steps"][k]["active"] for p in live)})
            members[str(R)] = {"per_step": per_step,
                               "active_equal_whole": [s["active"] for s in per_step] == active,
                               "projected_total_ms": r3(sum(s["projected_step_ms"] for s in per_step)),
                               "slowest_kernel_total_ms": r3(sum(max(p["steps"][k]["kernel_ms"] for p in live)
                                                                 for k in range(a.steps))),
                               "segments": sum(s["segments"] for p in live for s in p["steps"])}
        doc_thr[str(thr)] = {"whole_frame": whole_doc, "members": members}
    out.free()
doc = {"tool": "refine_group_adaptive_steps", "width": W, "height": H, "spheres": world.count, "depth": world.depth,
       "steps": a.steps, "step_samples": S, "tile_rows": T, "repeats": a.repeats, "build": rtx.build_info(),
       "note": "each part driven alone on one GPU with its true halos; projected_* is the slowest part's edges + mask "
               "+ call per step, a projection, not a measurement of R GPUs; the halo exchange, the gather and the "
               "de-interleave are not included; host-clock figures include launch and synchronisation overhead",
       "thresholds": doc_thr}
line = json.dumps(doc)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
ok = all(m["active_equal_whole"] for t in doc_thr.values() for m in t["members"].values())
sys.exit(0 if ok else 1)
