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
ap.add_argument("--keys", choices=["prepass", "carried", "both"], default="prepass")
ap.add_argument("--grid", type=int, default=11, help="random_world grid half extent (159 with --max-spheres 100000: C5)")
ap.add_argument("--max-spheres", type=int, default=0)
ap.add_argument("--splits", default="4,10", help="step counts: the spp in this many equal refine steps each")
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
