"""Waves for the walk's item prefix, chosen on the CPU by every ray's item
count (rtx_grid.h grid_stretch, through tests/walk_items_check.cpp, which
builds the world's layout and grid with the headers' own code). Shared by
test_walk_prefix.py (the CPU conditions on the inputs) and
test_gpu_walk_prefix.py (the same batches through rtx_debug_hit_world). Only
numpy, the oracle's worlds and g++.

A batch is one full wave of its shape and then, for 1 and 17 lanes, a partial
wave of the same shape: rtx_debug_hit_world gives ray i to thread i, so the
last wave of a batch of 64 + k rays has k active lanes.

Worlds: `strip` (a 64 x 8 grid: a ray along x inside the slab has up to 64
columns, so counts of exactly 48, the walk's limit, exist) and `rtiow11` (the
benchmark's world, 486 spheres; its grid is too small for 48, its largest
count that 40 rays of the pool reach is used there).
"""
import os
import subprocess

import numpy as np

import regime_cases as rc
from test_gpu_grid_coop import _rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "walk_items_check.cpp"),
        os.path.join(ROOT, "raytrace-we-gpu_amd", "csrc", "rtx_host.cpp")]
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"]
LANES = (1, 17, 64)  # active lanes of a batch's last wave
WORLDS = ("strip", "rtiow11")
MAX_ITEMS = 48  # kGridMaxSteps
POOL = {"strip": 40000, "rtiow11": 12000}


def _pool(name, rng):
    """Candidate rays of world `name`: above the slab and leaving (no items),
    dropping steeply through it (few), and inside the slab at a small slope in
    y (many: the slope decides after how many columns the ray leaves it)."""
    sph = rc.world(name).spheres[1:]
    ex, ez = float(np.abs(sph[:, 0]).max()), float(np.abs(sph[:, 2]).max())
    scale = np.array([ex / 11, 1.0, ez / 11, ex / 11, 1.0, ez / 11], np.float32)
    n = POOL[name]
    k = n // 8
    out = [_rays("none", k, rng) * scale, _rays("short", 2 * k, rng) * scale]
    m = n - 3 * k
    along_x = ex > 4 * ez  # the strip: only x has room for long stretches
    ang = np.where(rng.random(m) < 0.5, 0.0, np.pi) + rng.normal(scale=0.02, size=m) if along_x \
        else rng.uniform(0, 2 * np.pi, m)
    o = np.c_[rng.uniform(-ex, ex, m), rng.uniform(0.05, 0.35, m), rng.uniform(-ez, ez, m)]
    d = np.c_[np.cos(ang), rng.normal(scale=0.006, size=m), np.sin(ang)] * rng.uniform(0.5, 2, (m, 1))
    out.append(np.c_[o, d])
    return np.ascontiguousarray(np.concatenate(out), np.float32)


def classify(name, rays, workdir):
    """(items [nrays] int32, -1: gives up; mask [nrays] uint64; perm; flat_lo, flat_hi) of `rays` on world `name`."""
    exe = os.path.join(str(workdir), "walk_items_check")
    if not os.path.exists(exe):
        subprocess.run(GXX + ["-o", exe] + SRCS, check=True)
    w = rc.world(name)
    src, dst = os.path.join(str(workdir), f"{name}.bin"), os.path.join(str(workdir), f"{name}.out")
    with open(src, "wb") as f:
        f.write(np.array([w.count, len(rays), 0, 0], np.uint32).tobytes())
        f.write(w.spheres.tobytes())
        f.write(np.ascontiguousarray(rays, np.float32).tobytes())
    res = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.stdout, res.stderr[-2000:])
    raw = open(dst, "rb").read()
    flat_lo, flat_hi, npos, nrays = np.frombuffer(raw, np.uint32, 4)
    assert nrays == len(rays)
    perm = np.frombuffer(raw, np.uint32, npos, 16)
    items = np.frombuffer(raw, np.int32, nrays, 16 + 4 * npos)
    mask = np.frombuffer(raw, np.uint64, nrays, 16 + 4 * npos + 4 * nrays)
    return items, mask, perm, int(flat_lo), int(flat_hi)


class Cases:
    """The batches of one world: name -> (rays, items, mask), and the layout's
    position map and flat run. `big` is the largest item count used: 48 on the
    strip."""

    def __init__(self, name, workdir):
        rng = np.random.default_rng(4100 + len(name))
        pool = _pool(name, rng)
        items, mask, self.perm, self.flat_lo, self.flat_hi = classify(name, pool, workdir)
        self.pool_items = items
        # 48 on the strip; elsewhere the largest count that 40 rays of the pool have
        counts = np.bincount(items[items >= 0], minlength=MAX_ITEMS + 1)
        self.big = MAX_ITEMS if name == "strip" else int(np.flatnonzero(counts >= 40).max())
        by = lambda cond: np.flatnonzero(cond)  # noqa: E731
        zero, big = by(items == 0), by(items == self.big)
        low, seven, eight = by((items >= 1) & (items <= 7)), by(items == 7), by(items == 8)
        high, gave_up = by(items >= 8), by(items == -1)
        self.available = dict(zero=len(zero), big=len(big), low=len(low), seven=len(seven), eight=len(eight),
                              high=len(high), gave_up=len(gave_up))

        def take(ids, k):
            return rng.choice(ids, k, replace=len(ids) < k)

        def wave(shape, k):
            if shape == "all 0":
                return take(zero, k)
            if shape == "one lane big, the rest 0":
                ids = take(zero, k)
                ids[rng.integers(0, k)] = take(big, 1)[0]
                return ids
            if shape == "every lane big":
                return take(big, k)
            if shape == "every lane 1..7":
                return take(low, k)
            if shape == "7 and 8":
                ids = take(seven, k)
                ids[::3] = take(eight, len(ids[::3]))
                return ids
            ids = take(np.concatenate([zero, low, high]), k)  # "mixed"
            ids[0] = take(high, 1)[0]
            return ids

        self.batches = {}
        for shape in ("all 0", "one lane big, the rest 0", "every lane big", "every lane 1..7", "7 and 8", "mixed"):
            for lanes in LANES:
                ids = wave(shape, 64)
                if lanes < 64:
                    ids = np.concatenate([ids, wave(shape, lanes)])
                self.batches[f"{shape}, {lanes} lanes"] = (np.ascontiguousarray(pool[ids]), items[ids], mask[ids])

    def check_shapes(self):
        """Every wave of every batch has the item counts its name says."""
        for key, (rays, items, _) in self.batches.items():
            shape = key.rsplit(",", 1)[0]
            for w in range(0, len(items), 64):
                n = items[w:w + 64]
                assert (n >= 0).all(), key  # no lane gives up: the prefix runs
                if shape == "all 0":
                    assert (n == 0).all(), key
                elif shape == "one lane big, the rest 0":
                    assert (n == self.big).sum() == 1 and (n == 0).sum() == len(n) - 1, key
                elif shape == "every lane big":
                    assert (n == self.big).all(), key
                elif shape == "every lane 1..7":
                    assert (n >= 1).all() and (n <= 7).all(), key  # the prefix's high bits are skipped
                elif shape == "7 and 8":
                    assert set(n.tolist()) <= {7, 8} and (n == 8).any(), key
                    assert len(n) < 3 or (n == 7).any(), key
                else:
                    assert (n >= 8).any(), key

    def check_hits_in_masks(self, key, want):
        """Every hit of the oracle on a sphere of the layer lies in a block of
        the hitting ray's own mask (bit j: block flat_lo + j), so the wave's
        union must hold it: an item the prefix hands to no slot, in a wave
        where no other lane marks that block, loses the hit. Returns the
        number of such hits."""
        _, items, mask = self.batches[key]
        idx = want[:, 9].astype(np.int64)
        found = 0
        for r in np.flatnonzero(want[:, 0] == 1):
            blocks = np.unique(np.flatnonzero(self.perm == idx[r]) // 8)
            blocks = blocks[(blocks >= self.flat_lo) & (blocks < self.flat_hi)]
            if len(blocks) == 0:
                continue  # off the layer: scanned whatever the mask says
            bits = [(int(mask[r]) >> int(b - self.flat_lo)) & 1 for b in blocks]
            assert any(bits), (key, int(r), int(idx[r]), int(items[r]), hex(int(mask[r])))
            found += 1
        return found


_CASES = {}


def cases(name, workdir):
    if name not in _CASES:
        _CASES[name] = Cases(name, workdir)
    return _CASES[name]
