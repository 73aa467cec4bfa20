#!/usr/bin/env python3
"""What rtx_trace_film costs, on the C2 frame's scene (486 spheres) or the C5
scene (100k spheres), at --width x --height and the world's spp:

    frame       film_from_frame of the whole frame through rtx_trace_film in
                the given and in the cost order, beside rtx_render_sum of the
                same frame (the same arithmetic bit for bit, checked) and
                rtx_trace_paths of the same pixels' centre rays with their
                pixels' seeds (the zero-film twins' queries)
    zero        the zero-footprint film batch (H = V = 0, L = o + d of those
                queries) against rtx_trace_paths on the same queries: the same
                records (checked), so the ratio is what the longer record and
                the restated sample start cost
    equirect    rtx_film_camera's equirectangular records of the same number of
                pixels from the frame's camera position

timed by device events on the context's stream (a torch stream; `--reps` calls
between two events, `--rounds` windows after a warm-up, the configurations'
windows alternating within a round). Prints one JSON line (and writes it to
--out); progress goes to stderr.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytrace-we-gpu_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=["c2", "c5"], default="c2")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=2, help="calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--spp", type=int, default=0, help="samples (0: the benchmark's, 100 / 16)")
ap.add_argument("--out", default="")
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtx  # noqa: E402

f32, u32 = np.float32, np.uint32


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def stat(ms):
    return {"mean": round(sum(ms) / len(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, f32), np.ascontiguousarray(y, f32)
    return bool(((x.view(u32) == y.view(u32)) | (np.isnan(x) & np.isnan(y))).all())


spp = a.spp or (100 if a.config == "c2" else 16)
if a.config == "c2":
    world = rtx.random_world(11, depth=50, spp=spp)
else:
    world = rtx.random_world(159, capacity=100000, depth=50, spp=spp)
W, H = a.width, a.height
n = W * H
frame = rtx.camera_look_at(W, H, aspect=W / H)
ys, xs = np.divmod(np.arange(n), W)
film, img_w, img_h = rtx.film_from_frame(frame, xs, ys)
film = np.ascontiguousarray(film).view(f32).reshape(n, 16)

# the pixel-centre rays with the pixels' seeds (tools/paths_time.py's camera batch), and their zero-footprint records
u = ((np.arange(W, dtype=f32) + f32(0.5)) / (f32(frame.img_w) - f32(1.0))).astype(f32)
v = ((np.arange(H, dtype=f32) + f32(0.5)) / (f32(frame.img_h) - f32(1.0))).astype(f32)
org, hor, ver, llc = (np.array(x[:3], f32) for x in (frame.origin, frame.horizontal, frame.vertical, frame.lower_left))
d = (llc[None, None, :] + u[None, :, None] * hor[None, None, :]).astype(f32)
d = ((d + v[:, None, None] * ver[None, None, :]).astype(f32) - org[None, None, :]).astype(f32).reshape(-1, 3)
paths = np.zeros((n, 8), f32)
zero = np.zeros((n, 16), f32)
zero[:, 0:3], zero[:, 3] = org, film[:, 3]
zero[:, 4:7] = (org[None, :] + d).astype(f32)
paths[:, 0:3], paths[:, 3] = org, film[:, 3]
paths[:, 4:7] = (zero[:, 4:7] - org[None, :]).astype(f32)  # fl(L - o): the twin's ray of the zero-footprint record
equi = np.ascontiguousarray(rtx.film_camera("equirect", W, H, look_from=tuple(org))).view(f32).reshape(n, 16)

stream = torch.cuda.Stream()
rec = {"tool": "film_time", "config": a.config, "width": W, "height": H, "spheres": world.count, "spp": spp,
       "rounds": a.rounds, "reps": a.reps, "build": rtx.build_info()}
ok = True
with rtx.Context(0, stream=stream.cuda_stream) as ctx:
    def window(fn, reps=a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    ctx.upload_world(world)
    ctx.set_frame(frame)
    rec["kernels"] = ctx.scene_info()["kernels"]
    dev = {}
    for k, host in (("film", film), ("zero", zero), ("equirect", equi), ("paths", paths)):
        dev[k] = ctx.alloc(host.shape)
        dev[k].upload(host)
    d_r, d_s, d_sum = ctx.alloc((n, 4)), ctx.alloc((n,), np.uint32), ctx.alloc((n, 4))
    calls = {
        "render_sum": lambda: ctx.render_sum(0, d_sum.ptr),
        "film/given": lambda: ctx.trace_film(dev["film"], spp, img_w, img_h, order="given", results=d_r, segments=d_s, n=n),
        "film/cost": lambda: ctx.trace_film(dev["film"], spp, img_w, img_h, order="cost", results=d_r, segments=d_s, n=n),
        "paths/given": lambda: ctx.trace_paths(dev["paths"], spp, order="given", results=d_r, segments=d_s, n=n),
        "zero/given": lambda: ctx.trace_film(dev["zero"], spp, img_w, img_h, order="given", results=d_r, segments=d_s, n=n),
        "equirect/given": lambda: ctx.trace_film(dev["equirect"], spp, 2, 2, order="given", results=d_r, segments=d_s, n=n),
        "equirect/cost": lambda: ctx.trace_film(dev["equirect"], spp, 2, 2, order="cost", results=d_r, segments=d_s, n=n),
    }
    res, segs = {}, {}
    for k, fn in calls.items():  # warm-up, and the records
        fn()
        ctx.sync()
        res[k] = d_sum.numpy() if k == "render_sum" else d_r.numpy()
        segs[k] = None if k == "render_sum" else int(d_s.numpy().astype(np.uint64).sum())
        note(f"warm-up {k}: segments {segs[k]}")
    agree = {"film_given_is_render_sum": same_bits(res["film/given"][:, :3], res["render_sum"][:, :3]),
             "film_cost_is_film_given": same_bits(res["film/cost"], res["film/given"]) and segs["film/cost"] == segs["film/given"],
             "zero_is_paths": same_bits(res["zero/given"], res["paths/given"]) and segs["zero/given"] == segs["paths/given"],
             "equirect_cost_is_given": same_bits(res["equirect/cost"], res["equirect/given"])}
    ok = all(agree.values())
    rec["agree"] = agree
    rec["segments"] = segs
    ms = {k: [] for k in calls}
    for r in range(a.rounds):
        for k, fn in calls.items():
            ms[k].append(window(fn))
        note(f"round {r}: " + ", ".join(f"{k} {v[-1]:.2f}" for k, v in ms.items()))
    rec["ms"] = {k: stat(v) for k, v in ms.items()}
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    rec["ratios"] = {"film_given_over_render_sum": round(mean["film/given"] / mean["render_sum"], 3),
                     "film_cost_over_film_given": round(mean["film/cost"] / mean["film/given"], 3),
                     "film_given_over_paths_given": round(mean["film/given"] / mean["paths/given"], 3),
                     "zero_over_paths": round(mean["zero/given"] / mean["paths/given"], 3),
                     "equirect_cost_over_given": round(mean["equirect/cost"] / mean["equirect/given"], 3)}
    rec["gsegs_per_s"] = {k: round(segs[k] / mean[k] * 1e-6, 3) for k in calls if segs[k]}
    for x in list(dev.values()) + [d_r, d_s, d_sum]:
        x.free()
line = json.dumps(rec)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if ok else 1)
