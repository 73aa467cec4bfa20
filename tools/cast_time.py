#!/usr/bin/env python3
"""What rtx_cast_rays costs, and whether sorting the rays pays: the C2 frame's
scene (486 spheres) or the C5 scene (100k spheres), four batches on the device

    row_major   the 1920x1080 pixel-centre rays, row by row
    patch       the same rays in rtx_features' 8 x 8 patch order
    shuffle     the same rays in a seeded shuffle
    ao          4 seeded cosine-weighted rays per first hit, built from the
                feature planes, t_max = 1

each under "given" and "coherent", bytes only and hit records, timed by device
events on the context's stream (a torch stream; `--reps` calls between two
events, `--rounds` windows after a warm-up). rtx_features, the kernel this
change does not touch, is timed in the same run, its windows alternating with
the casts': patch / given against it is the price of reading rays from memory.

The COHERENT call is the key passes and the cast together; their split comes
from a kernel trace of this tool, in a run of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python tools/cast_time.py --config c2 --rounds 2 --reps 10 --out OUT/traced_c2.json
    python tools/cast_time.py --merge OUT/traced_c2.json --kernel-trace OUT/.../run_kernel_trace.csv

The merge step needs no GPU: the record lists the calls in the order they were
made ("plan"), and the trace's k_cast dispatches are dealt to them in that
order, each with the key-pass kernels that ran since the one before.

"auto": for the shuffled and the AO batch, whether COHERENT's mean (key passes
included) lies below GIVEN's by more than three times GIVEN's own window
spread (max - min) — the bar rtx_cast.h's AUTO rule is set by.
Prints one JSON line (and writes it to --out).
"""
import argparse
import csv
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "raytrace-we-gpu_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--config", choices=["c2", "c5"], default="c2")
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
ap.add_argument("--width", type=int, default=1920)
ap.add_argument("--height", type=int, default=1080)
ap.add_argument("--out", default="")
ap.add_argument("--merge", default="", help="a record of an earlier run: add --kernel-trace to it (no GPU)")
ap.add_argument("--kernel-trace", default="", help="rocprofv3's per-dispatch kernel trace CSV of that run")
a = ap.parse_args()


def emit(rec):
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


def stat(ms):
    return {"mean": round(sum(ms) / len(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


if a.merge:
    rec = json.load(open(a.merge))
    rows = []
    with open(a.kernel_trace, newline="") as f:
        for row in csv.DictReader(f):
            rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"]))
    rows.sort()
    labels = [label for label, calls in rec["plan"] for _ in range(calls)]
    split, passes, k, feat = {}, 0, 0, []
    for t0, t1, name in rows:
        if re.search(r"\bk_cast_(keys|prefix|scatter)\b", name):
            passes += t1 - t0
        elif re.search(r"\bk_cast\b", name):
            if k < len(labels):
                s = split.setdefault(labels[k], {"calls": 0, "cast_ns": 0, "key_passes_ns": 0})
                s["calls"] += 1
                s["cast_ns"] += t1 - t0
                s["key_passes_ns"] += passes
            k += 1
            passes = 0
        elif re.search(r"\bk_features\b", name):
            feat.append(t1 - t0)
    out = {label: {"calls": s["calls"], "cast_ms": round(s["cast_ns"] / s["calls"] * 1e-6, 4),
                   "key_passes_ms": round(s["key_passes_ns"] / s["calls"] * 1e-6, 4)}
           for label, s in split.items() if label != "warm-up"}
    rec["kernel_trace"] = {"k_cast_dispatches": k, "planned": len(labels), "per_call": out,
                           "k_features_ms": stat([v * 1e-6 for v in feat]) if feat else None}
    emit(rec)
    sys.exit(0 if k == len(labels) and k > 0 else 1)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rtx  # noqa: E402

f32 = np.float32
if a.config == "c2":
    world = rtx.random_world(11, depth=50, spp=100)
else:
    world = rtx.random_world(159, capacity=100000, depth=50, spp=16)
W, H = a.width, a.height
frame = rtx.camera_look_at(W, H, aspect=W / H)


def centre_rays():
    """The pixel-centre rays, (H * W, 6) float32, with rtx_features' operations."""
    u = ((np.arange(W, dtype=f32) + f32(0.5)) / (f32(frame.img_w) - f32(1.0))).astype(f32)
    v = ((np.arange(H, dtype=f32) + f32(0.5)) / (f32(frame.img_h) - f32(1.0))).astype(f32)
    org, hor, ver, llc = (np.array(x[:3], f32) for x in (frame.origin, frame.horizontal, frame.vertical, frame.lower_left))
    d = (llc[None, None, :] + u[None, :, None] * hor[None, None, :]).astype(f32)
    d = ((d + v[:, None, None] * ver[None, None, :]).astype(f32) - org[None, None, :]).astype(f32).reshape(-1, 3)
    return np.ascontiguousarray(np.c_[np.broadcast_to(org, d.shape), d], f32)


def rows8(r6, t_max):
    out = np.zeros((len(r6), 8), f32)
    out[:, 0:3], out[:, 4:7], out[:, 3] = r6[:, 0:3], r6[:, 3:6], t_max
    return out


def patch_order():
    """Pixel indices in k_features' order: 8 x 8 patches row by row, a patch's pixels row by row."""
    y, x = np.divmod(np.arange(H * W), W)
    key = ((y // 8) * ((W + 7) // 8) + x // 8) * 64 + (y % 8) * 8 + x % 8
    return np.argsort(key, kind="stable")


def ao_rays(geom, r6, rng, per=4):
    """`per` cosine-weighted directions about the normal of every pixel that hit something, from its hit point."""
    g = geom.reshape(-1, 4)
    hit = np.isfinite(g[:, 3])
    d = r6[hit, 3:6].astype(np.float64)
    p = r6[hit, 0:3] + g[hit, 3:4] * d / np.linalg.norm(d, axis=1, keepdims=True)
    n = np.repeat(g[hit, :3].astype(np.float64), per, 0)
    s = rng.normal(size=n.shape)
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    w = n + s
    w /= np.maximum(np.linalg.norm(w, axis=1, keepdims=True), 1e-12)
    return np.ascontiguousarray(np.c_[np.repeat(p, per, 0), w], f32), float(hit.mean())


stream = torch.cuda.Stream()
rec = {"tool": "cast_time", "config": a.config, "width": W, "height": H, "spheres": world.count,
       "rounds": a.rounds, "reps": a.reps, "build": rtx.build_info(), "plan": []}
with rtx.Context(0, stream=stream.cuda_stream) as ctx:
    ctx.upload_world(world)
    ctx.set_frame(frame)
    rec["kernels"] = ctx.scene_info()["kernels"]
    geom, surf = ctx.alloc((H, W, 4)), ctx.alloc((H, W, 4))
    ctx.features_rows(1, 0, 1, geom.ptr, surf.ptr)
    rng = np.random.default_rng(20261020)
    r6 = centre_rays()
    ao6, hit_share = ao_rays(geom.numpy(), r6, rng)
    host = {"row_major": rows8(r6, np.inf), "patch": rows8(r6[patch_order()], np.inf),
            "shuffle": rows8(r6[rng.permutation(len(r6))], np.inf), "ao": rows8(ao6, 1.0)}
    rec["rays"] = {k: len(v) for k, v in host.items()}
    rec["first_hit_share"] = round(hit_share, 4)
    dev = {}
    for k, v in host.items():
        dev[k] = ctx.alloc(v.shape)
        dev[k].upload(v)
    n_max = max(len(v) for v in host.values())
    d_hits, d_occ = ctx.alloc((n_max,), rtx.RAY_HIT_DTYPE), ctx.alloc((n_max,), np.uint8)
    configs = [(b, o, out) for b in host for o in ("given", "coherent") for out in ("bytes", "hits")]

    def call(b, o, out):
        ctx.cast(dev[b], order=o, hits=d_hits if out == "hits" else False, occluded=d_occ if out == "bytes" else False,
                 n=len(host[b]))

    def window(fn, label):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.reps):
            fn()
        e1.record(stream)
        e1.synchronize()
        if label:
            rec["plan"].append([label, a.reps])
        return e0.elapsed_time(e1) / a.reps

    for c in configs:  # warm-up: every shape the windows use, and the sort's scratch at its final size
        call(*c)
        call(*c)
        rec["plan"].append(["warm-up", 2])
    for _ in range(3):
        ctx.features_rows(1, 0, 1, geom.ptr, surf.ptr)
    ctx.sync()
    ms = {c: [] for c in configs}
    feat = []
    for _ in range(a.rounds):
        for c in configs:  # the yardstick's windows alternate with the casts'
            feat.append(window(lambda: ctx.features_rows(1, 0, 1, geom.ptr, surf.ptr), ""))
            ms[c].append(window(lambda: call(*c), "/".join(c)))
    # the records do not depend on the order (the tests' claim, here at full size)
    same = {}
    for b in host:
        got = []
        for o in ("given", "coherent"):
            ctx.cast(dev[b], order=o, hits=d_hits, occluded=d_occ, n=len(host[b]))
            rec["plan"].append(["warm-up", 1])
            ctx.sync()
            got.append((d_hits.numpy()[:len(host[b])].tobytes(), d_occ.numpy()[:len(host[b])].tobytes()))
        same[b] = got[0] == got[1]
        occ = np.frombuffer(got[0][1], np.uint8)
        rec.setdefault("occluded_share", {})[b] = round(float(occ.mean()), 4)
    rec["orders_agree"] = same
    rec["features_ms"] = stat(feat)
    rec["cast_ms"] = {"/".join(c): stat(v) for c, v in ms.items()}
    auto = {}
    for b in ("shuffle", "ao"):
        for out in ("bytes", "hits"):
            g, s = rec["cast_ms"][f"{b}/given/{out}"], rec["cast_ms"][f"{b}/coherent/{out}"]
            bar = g["mean"] - 3.0 * (g["max"] - g["min"])
            auto[f"{b}/{out}"] = {"given_mean": g["mean"], "given_spread": round(g["max"] - g["min"], 4),
                                  "coherent_mean": s["mean"], "bar": round(bar, 4), "coherent_wins": s["mean"] < bar}
    rec["auto"] = auto
    for d in list(dev.values()) + [d_hits, d_occ, geom, surf]:
        d.free()
emit(rec)
sys.exit(0 if all(same.values()) else 1)
