#!/usr/bin/env python3
"""What refining in steps costs: the C2 frame (1920x1080, 486 spheres, depth
50) to 100 samples per pixel three ways — one rtx_render at spp 100,
rtx_refine as 4 x 25, and rtx_refine as 10 x 10 — timed by the library's HIP
events (rtx_get_stats), each shape after a warm-up run of its own, `--rounds`
timed runs interleaved. Every final image must equal the one-shot's bit for
bit. Prints one JSON line. A step pays the cost pre-pass's sort and the state
store (16 B per pixel) each time; this figure says how much that is.

--keys prepass|carried|both: what orders a scheduled step's pixel queue
(rtx_refine_set_keys): a pre-pass per step, the previous step's cost map, or
every refine shape in each mode ("refine_4x25" and "refine_4x25_carried"),
interleaved in the same rounds.

Another scene: --grid / --max-spheres / --spp / --splits, e.g. the bench's C5
frame (100k spheres) to 16 samples as 2 x 8:

    python tools/refine_steps.py [--rounds 3] [--width 1920] [--height 1080] [--keys both]
    python tools/refine_steps.py --grid 159 --max-spheres 100000 --spp 16 --splits 2 --rounds 1 --keys both

--adaptive T1[,T2...]: the adaptive shape instead (rtx_refine_adaptive): the
frame in --steps steps of --spp / --steps samples, each step timed on its own
by the library's HIP events, the rounds interleaved:
  carried      rtx_refine with carried keys (the uniform reference; from
               --baseline-lib when given: another build of the library, e.g.
               the parent commit's from tools/build_commit_variant.sh)
  adaptive_T   rtx_refine_adaptive at threshold T, max_samples = --spp, until
               nothing is active or --steps steps ran: per step the active
               share and the time
Steps 1 and 2 of an adaptive run trace every pixel: the gate compares them
with the carried steps of the same size (the mean over the reference's carried
steps), allowing the reference's own min-to-max spread plus 3 %. Also timed:
the call that only builds the mask and reads the count back (rtx_refine_pending).

    python tools/refine_steps.py --adaptive 0.05,0.1 --steps 10 --baseline-lib raytrace-we-gpu_amd/lib/variants/librtx_parent.so
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--spp", type=int, default=100)
ap.add_argument("--keys", choices=["prepass", "carried", "both"], default="prepass")
ap.add_argument("--grid", type=int, default=11, help="random_world grid half extent (159 with --max-spheres 100000: C5)")
ap.add_argument("--max-spheres", type=int, default=0)
ap.add_argument("--splits", default="4,10", help="step counts: the spp in this many equal refine steps each")
ap.add_argument("--adaptive", default="", help="thresholds of the adaptive shape (comma separated)")
ap.add_argument("--steps", type=int, default=10, help="adaptive shape: steps of spp / steps samples")
ap.add_argument("--baseline-lib", default="", help="adaptive shape: the library the carried reference runs on")
a = ap.parse_args()

splits = [int(s) for s in a.splits.split(",") if s]
if any(k < 1 or a.spp % k != 0 for k in splits):
    sys.exit("--spp must be a multiple of every entry of --splits")
world = rtx.random_world(a.grid, capacity=a.max_spheres or None, depth=50, spp=a.spp)
frame = rtx.camera_look_at(a.width, a.height, aspect=a.width / a.height)
modes = ["prepass", "carried"] if a.keys == "both" else [a.keys]
# name -> (steps, key mode); the one-shot first: the image the others must equal
shapes = {"render_1x%d" % a.spp: (None, "prepass")}
for k in splits:
    for m in modes:
        shapes["refine_%dx%d%s" % (k, a.spp // k, "_carried" if m == "carried" else "")] = ([a.spp // k] * k, m)


def adaptive_shape():
    s = a.spp // a.steps
    if s < 1 or a.spp % a.steps != 0:
        sys.exit("--spp must be a multiple of --steps")
    thresholds = [float(t) for t in a.adaptive.split(",") if t]
    px = a.width * a.height

    def timed(ctx, call):
        ctx.stats_reset()
        r = call()
        return r, ctx.stats().kernel_ms

    def carried(ctx):
        ctx.set_refine_keys("carried")
        return [timed(ctx, lambda k=k: ctx.refine(s, reset=(k == 0)))[1] for k in range(a.steps)]

    def adaptive(ctx, thr):
        out = []
        for k in range(a.steps):
            n, ms = timed(ctx, lambda k=k: ctx.refine_adaptive(s, thr, a.spp, reset=(k == 0)))
            if n == 0:
                break
            out.append((n / px, ms))
        return out

    base_lib = rtx.load_library(os.path.abspath(a.baseline_lib)) if a.baseline_lib else None
    with rtx.Context(0) as ctx, rtx.Context(0, lib=base_lib) as base:
        for c in (ctx, base):
            c.upload_world(world)
            c.set_frame(frame)
        carried(base)  # warm-up of each shape
        for t in thresholds:
            adaptive(ctx, t)
        ref, runs = [], {t: [] for t in thresholds}
        for _ in range(a.rounds):
            ref.append(carried(base))
            for t in thresholds:
                runs[t].append(adaptive(ctx, t))
        # the mask-and-readback call alone, wall clock around a synchronous call
        ctx.refine_adaptive(s, 0.0, 0, reset=True)
        ctx.refine_adaptive(s, 0.0, 0)
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(50):
            ctx.refine_pending(s, thresholds[0], 0)
        pending_ms = (time.perf_counter() - t0) * 1e3 / 50
        counts_max = {}
        for t in thresholds:
            adaptive(ctx, t)
            counts_max[t] = int(ctx.refine_counts().max())
    ref = np.array(ref)  # [round][step]; step 0 takes the pre-pass, the rest are carried
    car = ref[:, 1:]
    car_mean, car_min, car_max = float(car.mean()), float(car.min()), float(car.max())
    limit = car_mean + (car_max - car_min) + 0.03 * car_mean
    out = {"tool": "refine_steps", "shape": "adaptive", "width": a.width, "height": a.height, "spheres": world.count,
           "depth": world.depth, "spp": a.spp, "steps": a.steps, "step_samples": s, "rounds": a.rounds,
           "build": rtx.build_info(), "baseline_build": rtx.build_info(base_lib) if base_lib else rtx.build_info(),
           "carried_step_ms": {"mean": round(car_mean, 3), "min": round(car_min, 3), "max": round(car_max, 3),
                               "first_step_prepass_mean": round(float(ref[:, 0].mean()), 3),
                               "total_mean": round(float(ref.sum(axis=1).mean()), 3)},
           "gate_limit_ms": round(limit, 3), "pending_call_ms": round(pending_ms, 4), "adaptive": {}}
    ok = True
    for t in thresholds:
        n = min(len(r) for r in runs[t])
        share = [round(runs[t][0][k][0], 4) for k in range(n)]
        ms = np.array([[r[k][1] for k in range(n)] for r in runs[t]])
        full = [round(float(ms[:, k].mean()), 3) for k in range(min(2, n))]
        passed = [m <= limit for m in full]
        ok = ok and all(passed)
        out["adaptive"]["%g" % t] = {"steps_run": n, "active_share": share,
                                     "step_ms_mean": [round(float(v), 3) for v in ms.mean(axis=0)],
                                     "step_ms_min": [round(float(v), 3) for v in ms.min(axis=0)],
                                     "step_ms_max": [round(float(v), 3) for v in ms.max(axis=0)],
                                     "total_ms_mean": round(float(ms.sum(axis=1).mean()), 3),
                                     "largest_count": counts_max[t], "full_steps_ms": full, "gate_passed": passed}
    out["gate"] = "passed" if ok else "failed"
    print(json.dumps(out))
    sys.exit(0)


if a.adaptive:
    adaptive_shape()


def run(ctx, steps, mode):
    """One image at a.spp samples per pixel; (summed kernel ms, segments, what each step was keyed by)."""
    ctx.set_refine_keys(mode)
    ctx.stats_reset()
    keyed = []
    if steps is None:
        ctx.render()
    else:
        for k, s in enumerate(steps):
            ctx.refine(s, reset=(k == 0))
            keyed.append(ctx.refine_last_keys)
    st = ctx.stats()
    return st.kernel_ms, st.segments, keyed


with rtx.Context(0) as ctx:
    ctx.upload_world(world)
    ctx.set_frame(frame)
    times = {n: [] for n in shapes}
    segs, ref, equal, keyed = {}, None, {}, {}
    for n, (steps, mode) in shapes.items():  # warm-up of each shape, and its image
        _, segs[n], keyed[n] = run(ctx, steps, mode)
        img = ctx.download()
        if ref is None:
            ref = img
        equal[n] = bool(((img.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(img) & np.isnan(ref))).all())
    for _ in range(a.rounds):
        for n, (steps, mode) in shapes.items():
            times[n].append(run(ctx, steps, mode)[0])
out = {"tool": "refine_steps", "width": a.width, "height": a.height, "spheres": world.count, "depth": world.depth,
       "spp": a.spp, "rounds": a.rounds, "keys": a.keys, "build": rtx.build_info(),
       "kernel_ms": {n: {"mean": round(float(np.mean(t)), 3), "min": round(float(min(t)), 3),
                         "max": round(float(max(t)), 3)} for n, t in times.items()},
       "keyed_by": {n: k for n, k in keyed.items() if k},
       "segments": segs, "images_equal_one_shot": equal}
print(json.dumps(out))
sys.exit(0 if all(equal.values()) and len(set(segs.values())) == 1 else 1)
