#!/usr/bin/env python3
"""Flat blocks the layer grid marks per ray and per wave, by block order.

Builds tools/layout_blocks.cpp (the project's own grid and layout headers)
and runs it: one JSON line for scene order and for each candidate order of
the layer's spheres (rtx_layout.h). This is the tool that chose the order
rtx_upload_world uses.

    python tools/layout_blocks.py [--ext 11] [--rays SAMPLE.npz] [--waves 4000] [--seed 1]

--rays: a sample of real lane-mode rays taken on the GPU by tools/ray_sample.py
(the `rays` diagnostic build): its scene and its waves of 64 lanes are used.
Without it the tool falls back to its seeded synthetic ray family.
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--ext", type=int, default=11)
ap.add_argument("--rays", default="")
ap.add_argument("--waves", type=int, default=4000)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()

with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "layout_blocks")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma", "-o", exe,
                    os.path.join(ROOT, "tools", "layout_blocks.cpp"),
                    os.path.join(ROOT, "raytrace-we-gpu_amd", "csrc", "rtx_host.cpp")], check=True)
    cmd = [exe, "--ext", str(a.ext), "--waves", str(a.waves), "--seed", str(a.seed)]
    if a.rays:
        import numpy as np

        z = np.load(a.rays)
        scene, rays = os.path.join(tmp, "scene.f32"), os.path.join(tmp, "rays.f32")
        np.ascontiguousarray(z["spheres"], np.float32).reshape(-1, 4).tofile(scene)
        rec = np.concatenate([z["o"], z["d"], z["live"][..., None].astype(np.float32)], -1)  # [records][64][7]
        np.ascontiguousarray(rec, np.float32).tofile(rays)
        cmd += ["--scene", scene, "--rays", rays]
    sys.exit(subprocess.run(cmd).returncode)
