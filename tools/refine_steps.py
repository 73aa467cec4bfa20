#!/usr/bin/env python3
"""What refining in steps costs: the C2 frame (1920x1080, 486 spheres, depth
50) to 100 samples per pixel three ways — one rtx_render at spp 100,
rtx_refine as 4 x 25, and rtx_refine as 10 x 10 — timed by the library's HIP
events (rtx_get_stats), each shape after a warm-up run of its own, `--rounds`
timed runs interleaved. Every final image must equal the one-shot's bit for
bit. Prints one JSON line. A step pays the cost pre-pass's sort and the state
store (16 B per pixel) each time; this figure says how much that is.

    python tools/refine_steps.py [--rounds 3] [--width 1920] [--height 1080]
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
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--spp", type=int, default=100)
a = ap.parse_args()

world = rtx.random_world(11, depth=50, spp=a.spp)
frame = rtx.camera_look_at(a.width, a.height, aspect=a.width / a.height)
shapes = {"render_1x%d" % a.spp: None, "refine_4x%d" % (a.spp // 4): [a.spp // 4] * 4,
          "refine_10x%d" % (a.spp // 10): [a.spp // 10] * 10}
if a.spp % 20 != 0:
    sys.exit("--spp must be a multiple of 20")


def run(ctx, steps):
    """One image at a.spp samples per pixel; (summed kernel ms, segments)."""
    ctx.stats_reset()
    if steps is None:
        ctx.render()
    else:
        for k, s in enumerate(steps):
            ctx.refine(s, reset=(k == 0))
    st = ctx.stats()
    return st.kernel_ms, st.segments


with rtx.Context(0) as ctx:
    ctx.upload_world(world)
    ctx.set_frame(frame)
    times = {n: [] for n in shapes}
    segs, ref, equal = {}, None, {}
    for n, steps in shapes.items():  # warm-up of each shape, and its image
        _, segs[n] = run(ctx, steps)
        img = ctx.download()
        if ref is None:
            ref = img
        equal[n] = bool(((img.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(img) & np.isnan(ref))).all())
    for _ in range(a.rounds):
        for n, steps in shapes.items():
            times[n].append(run(ctx, steps)[0])
out = {"tool": "refine_steps", "width": a.width, "height": a.height, "spheres": world.count, "depth": world.depth,
       "spp": a.spp, "rounds": a.rounds, "build": rtx.build_info(),
       "kernel_ms": {n: {"mean": round(float(np.mean(t)), 3), "min": round(float(min(t)), 3),
                         "max": round(float(max(t)), 3)} for n, t in times.items()},
       "segments": segs, "images_equal_one_shot": equal}
print(json.dumps(out))
sys.exit(0 if all(equal.values()) and len(set(segs.values())) == 1 else 1)
