#!/usr/bin/env python3
"""What the cost order of rtx_trace_paths_keyed buys, on the C2 frame's scene
(486 spheres, spp 100) or the C5 scene (100k spheres, spp 16), depth 50: the
camera's 1920 x 1080 pixel-centre queries with their pixels' seeds, once in
pixel order and once in a fixed shuffle, through

    given       rtx_trace_paths, RTX_CAST_ORDER_GIVEN
    coherent    rtx_trace_paths, RTX_CAST_ORDER_COHERENT
    probed      rtx_trace_paths_keyed, d_keys NULL, the default probe
    exact       rtx_trace_paths_keyed with d_keys = the d_segments of a full
                earlier call: the best any key can do on this grid, so an
                upper bound on what a better probe could buy
    parent      "given" on a library built from the parent commit
                (tools/build_commit_variant.sh <commit> parent), to show that
                the old path is unchanged

timed by device events on the contexts' common stream (a torch stream; `--reps`
calls between two events, `--rounds` windows after a warm-up of every shape,
the legs alternating within a window). Every leg's records are checked equal,
bit for bit, to "given"'s at full size in the same run. Each leg is reported
against "given": a difference counts when it exceeds three times "given"'s
own window spread (max - min). Prints one JSON line (and writes it to --out);
progress goes to stderr.
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
ap.add_argument("--reps", type=int, default=0, help="calls per timed window (0: 3 for c2, 1 for c5)")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--spp", type=int, default=0, help="samples per query (0: the benchmark's, 100 / 16)")
ap.add_argument("--parent", default="parent", help="the parent commit's build, lib/variants/librtx_<name>.so")
ap.add_argument("--out", default="")
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtx  # noqa: E402

f32, u32 = np.float32, np.uint32
PARENT = os.path.join(ROOT, "raytrace-we-gpu_amd", "lib", "variants", f"librtx_{a.parent}.so")
if not os.path.exists(PARENT):
    sys.exit(f"{PARENT} is missing: tools/build_commit_variant.sh <parent commit> {a.parent}")


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


spp = a.spp or (100 if a.config == "c2" else 16)
reps = a.reps or (3 if a.config == "c2" else 1)
if a.config == "c2":
    world = rtx.random_world(11, depth=50, spp=spp)
else:
    world = rtx.random_world(159, capacity=100000, depth=50, spp=spp)
W, H = a.width, a.height
n = W * H
frame = rtx.camera_look_at(W, H, aspect=W / H)


def camera_queries():
    """The pixel-centre rays (rtx_features' operations) with rtx_path_seed(x, y, 0), row-major."""
    u = ((np.arange(W, dtype=f32) + f32(0.5)) / (f32(frame.img_w) - f32(1.0))).astype(f32)
    v = ((np.arange(H, dtype=f32) + f32(0.5)) / (f32(frame.img_h) - f32(1.0))).astype(f32)
    org, hor, ver, llc = (np.array(x[:3], f32) for x in (frame.origin, frame.horizontal, frame.vertical, frame.lower_left))
    d = (llc[None, None, :] + u[None, :, None] * hor[None, None, :]).astype(f32)
    d = ((d + v[:, None, None] * ver[None, None, :]).astype(f32) - org[None, None, :]).astype(f32).reshape(-1, 3)
    y, x = np.divmod(np.arange(n, dtype=np.int64), W)
    seeds = (base_hash(x, y).astype(f32) / f32(4294967296.0)).astype(f32)
    assert seeds[W + 2] == rtx.path_seed(2, 1) and seeds[0] == rtx.path_seed(0, 0)
    q = np.zeros((n, 8), f32)
    q[:, 0:3], q[:, 4:7], q[:, 3] = org, d, seeds
    return q


LEGS = ("given", "coherent", "probed", "exact", "parent")
stream = torch.cuda.Stream()
rec = {"tool": "paths_order_time", "config": a.config, "width": W, "height": H, "queries": n, "spheres": world.count,
       "spp": spp, "depth": 50, "rounds": a.rounds, "reps": reps, "build": rtx.build_info()}
ok = True
with rtx.Context(0, stream=stream.cuda_stream) as ctx, \
        rtx.Context(0, stream=stream.cuda_stream, lib=rtx.load_library(PARENT)) as old:
    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / reps

    assert not hasattr(old._lib, "rtx_trace_paths_keyed"), "the parent build has the new entry point"
    for c in (ctx, old):
        c.upload_world(world)
    info = ctx.scene_info()
    rec["kernels"], rec["probe"] = info["kernels"], 1 if info["n_pad"] > 1024 else 2
    host = {"camera": camera_queries()}
    perm = np.random.default_rng(20261021).permutation(n)
    host["shuffle"] = np.ascontiguousarray(host["camera"][perm])
    dev, keys = {}, {}
    for b, v in host.items():
        dev[b] = ctx.alloc(v.shape)
        dev[b].upload(v)
        keys[b] = ctx.alloc((n,), u32)
    d_r, d_s = ctx.alloc((n, 4)), ctx.alloc((n,), u32)

    def call(b, leg, seg=None):
        seg = d_s if seg is None else seg
        if leg == "parent":
            old.trace_paths(dev[b], spp, order="given", results=d_r, segments=seg, n=n)
        elif leg in ("given", "coherent"):
            ctx.trace_paths(dev[b], spp, order=leg, results=d_r, segments=seg, n=n)
        else:
            ctx.trace_paths_keyed(dev[b], spp, keys=keys[b] if leg == "exact" else None, results=d_r, segments=seg, n=n)

    # warm-up of every shape, and: the records do not depend on the leg
    want, agree, ran = {}, {}, {}
    for b in host:
        call(b, "given", keys[b])  # the exact keys: a full call's own segment counts
        ctx.sync()
        for leg in LEGS:
            d_r.upload(np.full((n, 4), np.nan, f32))
            call(b, leg)
            ctx.sync()
            old.sync()
            got = (d_r.numpy().tobytes(), d_s.numpy().tobytes())
            if leg == "given":
                want[b] = got
                assert got[1] == keys[b].numpy().tobytes()
            agree[f"{b}/{leg}"] = got == want[b]
            ran[f"{b}/{leg}"] = (old if leg == "parent" else ctx).paths_last_order()
            note(f"warm-up {b}/{leg}: equal bits {agree[f'{b}/{leg}']}, ran {ran[f'{b}/{leg}']}")
    cam = np.frombuffer(want["camera"][0], f32).reshape(n, 4)
    shf = np.frombuffer(want["shuffle"][0], f32).reshape(n, 4)
    agree["shuffle_is_camera_permuted"] = bool((cam[perm].view(u32) == shf.view(u32)).all())
    ok = ok and all(agree.values())
    seg = np.frombuffer(want["camera"][1], u32)
    rec["records_agree"], rec["ran"] = agree, ran
    rec["segments"] = int(seg.astype(np.uint64).sum())
    rec["segments_per_query"] = {"mean": round(float(seg.mean()), 2), "max": int(seg.max()),
                                 "p50": int(np.percentile(seg, 50)), "p99": int(np.percentile(seg, 99))}
    ctx.trace_paths(dev["camera"], rec["probe"], order="given", results=d_r, segments=d_s, n=n)
    ctx.sync()
    rec["probe_distinct_keys"] = int(len(np.unique(np.minimum(d_s.numpy(), 65535))))

    ms = {f"{b}/{leg}": [] for b in host for leg in LEGS}
    for r in range(a.rounds):
        for b in host:
            for leg in LEGS:  # the legs alternate within a window
                ms[f"{b}/{leg}"].append(window(lambda: call(b, leg)))
        note(f"round {r}: " + ", ".join(f"{k} {v[-1]:.2f}" for k, v in ms.items()))
    rec["ms"] = {k: stat(v) for k, v in ms.items()}
    rec["windows_ms"] = {k: [round(x, 4) for x in v] for k, v in ms.items()}
    verdict = {}
    for b in host:
        g = rec["ms"][f"{b}/given"]
        spread = g["max"] - g["min"]
        for leg in LEGS[1:]:
            m = rec["ms"][f"{b}/{leg}"]["mean"]
            diff = m - g["mean"]
            verdict[f"{b}/{leg}"] = {"given_mean": g["mean"], "given_spread": round(spread, 4), "mean": m,
                                     "diff_ms": round(diff, 4), "diff_percent": round(100.0 * diff / g["mean"], 2),
                                     "outcome": "no difference" if abs(diff) <= 3.0 * spread
                                     else ("faster" if diff < 0 else "slower")}
    rec["against_given"] = verdict
    for x in list(dev.values()) + list(keys.values()) + [d_r, d_s]:
        x.free()
line = json.dumps(rec)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
sys.exit(0 if ok else 1)
