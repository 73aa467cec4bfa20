#!/usr/bin/env python3
"""What rtx_trace_paths costs against the scheduled render, on the C2 frame's
scene (486 spheres) or the C5 scene (100k spheres):

    twin        one ray's --twin x --twin zero-film twin frame through
                rtx_render_sum against the same queries (that ray, the pixels'
                seeds) through rtx_trace_paths: the same arithmetic bit for bit
                (checked), so the ratio is what the render's schedule gains
                over the exact grid
    camera      the frame's pixel-centre rays with their pixels' seeds at the
                world's spp: segments per second (the sum of d_segments over
                the call's time) beside rtx_render's (rtx_stats.segments over
                kernel_ms) on the same build
    orders      "given" against "coherent" for the camera batch and for a
                seeded shuffle of it

timed by device events on the context's stream (a torch stream; `--reps` calls
between two events, `--rounds` windows after a warm-up, the render's windows
alternating with the queries'). "auto": whether COHERENT's mean lies below
GIVEN's by more than three times GIVEN's own window spread (max - min), the
bar rtx_cast.h's AUTO rule was set by. Prints one JSON line (and writes it to
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
ap.add_argument("--reps", type=int, default=3, help="calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--twin-reps", type=int, default=40, help="calls per timed window of the twin comparison")
ap.add_argument("--twin", type=int, default=512, help="the twin frame's side")
ap.add_argument("--twin-spp", type=int, default=0, help="samples of the twin comparison (0: 16 for c2, 4 for c5)")
ap.add_argument("--spp", type=int, default=0, help="samples of the camera batch (0: the benchmark's, 100 / 16)")
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


def base_hash(px, py):
    px, py = px.astype(u32), py.astype(u32)
    k = u32(1103515245)
    qx, qy = k * ((px >> u32(1)) ^ py), k * ((py >> u32(1)) ^ px)
    h = k * (qx ^ (qy >> u32(3)))
    return h ^ (h >> u32(16))


def pixel_seeds(w, h):
    """rtx_path_seed(x, y, 0) of every pixel, row-major."""
    y, x = np.divmod(np.arange(w * h, dtype=np.int64), w)
    s = (base_hash(x, y).astype(f32) / f32(4294967296.0)).astype(f32)
    assert s[w + 2] == rtx.path_seed(2, 1) and s[0] == rtx.path_seed(0, 0)
    return s


def queries_of(o, d, seeds):
    q = np.zeros((len(seeds), 8), f32)
    q[:, 0:3], q[:, 4:7], q[:, 3] = o, d, seeds
    return q


spp = a.spp or (100 if a.config == "c2" else 16)
twin_spp = a.twin_spp or (16 if a.config == "c2" else 4)
if a.config == "c2":
    world = rtx.random_world(11, depth=50, spp=spp)
else:
    world = rtx.random_world(159, capacity=100000, depth=50, spp=spp)
W, H, T = a.width, a.height, a.twin
frame = rtx.camera_look_at(W, H, aspect=W / H)


def centre_rays():
    """The pixel-centre rays, (H * W, 6) float32, with rtx_features' operations."""
    u = ((np.arange(W, dtype=f32) + f32(0.5)) / (f32(frame.img_w) - f32(1.0))).astype(f32)
    v = ((np.arange(H, dtype=f32) + f32(0.5)) / (f32(frame.img_h) - f32(1.0))).astype(f32)
    org, hor, ver, llc = (np.array(x[:3], f32) for x in (frame.origin, frame.horizontal, frame.vertical, frame.lower_left))
    d = (llc[None, None, :] + u[None, :, None] * hor[None, None, :]).astype(f32)
    d = ((d + v[:, None, None] * ver[None, None, :]).astype(f32) - org[None, None, :]).astype(f32).reshape(-1, 3)
    return np.ascontiguousarray(np.c_[np.broadcast_to(org, d.shape), d], f32)


def twin_frame(o, L):
    f = rtx.camera_look_at(T, T, aspect=1.0)
    for k in range(3):
        f.origin[k], f.lower_left[k] = float(o[k]), float(L[k])
        f.horizontal[k] = f.vertical[k] = 0.0
    f.img_w = f.img_h = float(T)
    f.rng_mode, f.frame_index, f.flags = 0, 0, 0
    f.lens_u[3] = 0.0
    return f


stream = torch.cuda.Stream()
rec = {"tool": "paths_time", "config": a.config, "width": W, "height": H, "twin": T, "spheres": world.count, "spp": spp,
       "twin_spp": twin_spp, "rounds": a.rounds, "reps": a.reps, "twin_reps": a.twin_reps, "build": rtx.build_info()}
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

    # ---- twin: the same work through the render and through the exact grid ----
    world_t = rtx.World(world.spheres, world.mat_types, world.mat_values, 50, twin_spp)
    ctx.upload_world(world_t)
    rec["kernels"] = ctx.scene_info()["kernels"]
    r6 = centre_rays()
    mid = r6[(H // 2) * W + W // 2]  # the frame's centre ray
    o, L = mid[0:3].copy(), (mid[0:3] + mid[3:6]).astype(f32)
    L = (L + f32(0.0)).astype(f32)
    d = (L - o).astype(f32)
    ctx.set_frame(twin_frame(o, L))
    d_sum = ctx.alloc((T * T, 4))
    q_t = queries_of(o, d, pixel_seeds(T, T))
    d_q, d_r, d_s = ctx.alloc(q_t.shape), ctx.alloc((T * T, 4)), ctx.alloc((T * T,), np.uint32)
    d_q.upload(q_t)

    def render_twin():
        ctx.render_sum(0, d_sum.ptr)

    def paths_twin():
        ctx.trace_paths(d_q, twin_spp, order="given", results=d_r, segments=d_s, n=T * T)

    for _ in range(2):
        render_twin()
        paths_twin()
    ctx.sync()
    want, got = d_sum.numpy()[:, :3], d_r.numpy()[:, :3]
    same = bool(((want.view(u32) == got.view(u32)) | (np.isnan(want) & np.isnan(got))).all())
    ok = ok and same
    segs_t = int(d_s.numpy().astype(np.uint64).sum())
    note(f"twin: equal bits {same}, {segs_t} segments")
    ms_r, ms_p = [], []
    for _ in range(a.rounds):
        ms_r.append(window(render_twin, a.twin_reps))
        ms_p.append(window(paths_twin, a.twin_reps))
    rec["twin_run"] = {"queries": T * T, "equal_bits": same, "segments": segs_t, "render_sum_ms": stat(ms_r),
                       "trace_paths_ms": stat(ms_p),
                       "paths_over_render": round(sum(ms_p) / sum(ms_r), 3)}
    note(f"twin: render_sum {stat(ms_r)} trace_paths {stat(ms_p)}")
    for x in (d_sum, d_q, d_r, d_s):
        x.free()

    # ---- camera: the frame's centre rays with their pixels' seeds --------------
    ctx.upload_world(world)
    ctx.set_frame(frame)
    seeds = pixel_seeds(W, H)
    rng = np.random.default_rng(20261021)
    perm = rng.permutation(W * H)
    host = {"camera": queries_of(r6[:, 0:3], r6[:, 3:6], seeds)}
    host["shuffle"] = np.ascontiguousarray(host["camera"][perm])
    dev = {}
    for k, v in host.items():
        dev[k] = ctx.alloc(v.shape)
        dev[k].upload(v)
    n = W * H
    d_r, d_s = ctx.alloc((n, 4)), ctx.alloc((n,), np.uint32)
    configs = [(b, o_) for b in host for o_ in ("given", "coherent")]

    def call(b, o_):
        ctx.trace_paths(dev[b], spp, order=o_, results=d_r, segments=d_s, n=n)

    def render():
        ctx.render()

    res = {}
    for c in configs:  # warm-up, and: the records do not depend on the order or on the neighbours
        call(*c)
        ctx.sync()
        res[c] = (d_r.numpy().tobytes(), d_s.numpy())
        note(f"warm-up {c}")
    segs_c = int(res[("camera", "given")][1].astype(np.uint64).sum())
    agree = {b: res[(b, "given")][0] == res[(b, "coherent")][0] for b in host}
    cam = np.frombuffer(res[("camera", "given")][0], f32).reshape(n, 4)
    shf = np.frombuffer(res[("shuffle", "given")][0], f32).reshape(n, 4)
    agree["shuffle_is_camera_permuted"] = bool((cam[perm].view(u32) == shf.view(u32)).all())
    ok = ok and all(agree.values())
    rec["orders_agree"] = agree
    render()
    ctx.sync()
    ms = {c: [] for c in configs}
    rend_ms, rend_kernel, rend_segs = [], [], []
    for r in range(a.rounds):
        for c in configs:  # the render's windows alternate with the queries'
            ctx.stats_reset()
            rend_ms.append(window(render))
            st = ctx.stats()
            rend_kernel.append(st.kernel_ms / a.reps)
            rend_segs.append(st.segments // a.reps)
            ms[c].append(window(lambda: call(*c)))
        note(f"round {r}: " + ", ".join(f"{'/'.join(c)} {ms[c][-1]:.2f}" for c in configs) + f", render {rend_ms[-1]:.2f}")
    rec["camera_run"] = {
        "queries": n, "path_segments": segs_c, "render_segments": int(rend_segs[0]),
        "render_ms": stat(rend_ms), "render_kernel_ms": stat(rend_kernel),
        "trace_paths_ms": {"/".join(c): stat(v) for c, v in ms.items()},
        "render_gsegs_per_s": round(rend_segs[0] / (sum(rend_kernel) / len(rend_kernel)) * 1e-6, 3),
        "paths_gsegs_per_s": {"/".join(c): round(segs_c / (sum(v) / len(v)) * 1e-6, 3) for c, v in ms.items()}}
    auto = {}
    for b in host:
        g, s = rec["camera_run"]["trace_paths_ms"][f"{b}/given"], rec["camera_run"]["trace_paths_ms"][f"{b}/coherent"]
        bar = g["mean"] - 3.0 * (g["max"] - g["min"])
        auto[b] = {"given_mean": g["mean"], "given_spread": round(g["max"] - g["min"], 4), "coherent_mean": s["mean"],
                   "bar": round(bar, 4), "coherent_wins": s["mean"] < bar}
    rec["auto"] = auto
    for x in list(dev.values()) + [d_r, d_s]:
        x.free()
line = json.dumps(rec)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if ok else 1)
