"""GPU side of the wave-cooperative layer-grid walk (rtx_kernels.hip
grid_wave_mask; CPU side: test_grid_coop.py) on the 486-sphere world: hand
built waves through rtx_debug_hit_world, and a small frame whole and as a
share whose waves hold fewer pixels than lanes. Everything is bit for bit the
linear scan's and the fp32 oracle's.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def assert_bits_equal(a, b, what=""):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} values differ; first at {np.argwhere(~same)[:5].tolist()}"


@pytest.fixture(scope="module")
def world(rtx):
    return rtx.random_world(11, depth=50, spp=4)


def _rays(kind, n, rng):
    """Rays over the 486-sphere world's layer (y = 0.2, x and z in -11..11) by
    the number of grid columns they cross: "none" misses the slab, "short"
    drops steeply through it (1-2 items), "long" grazes it across the grid
    (tens of items), "far" starts beyond the grid's origin range and "range"
    is outside the prefilter's safe range (both scan every block)."""
    o = np.empty((n, 3))
    d = np.empty((n, 3))
    xz = rng.uniform(-10, 10, (n, 2))
    if kind == "none":
        o[:] = np.c_[xz[:, 0], rng.uniform(2, 5, n), xz[:, 1]]
        d[:] = np.c_[rng.normal(size=n), rng.uniform(0.1, 1, n), rng.normal(size=n)]
    elif kind == "short":
        o[:] = np.c_[xz[:, 0], rng.uniform(1, 4, n), xz[:, 1]]
        d[:] = np.c_[rng.normal(scale=0.05, size=n), -rng.uniform(0.5, 1, n), rng.normal(scale=0.05, size=n)]
    elif kind == "long":
        ang = rng.uniform(0, 2 * np.pi, n)
        o[:] = np.c_[-9 * np.cos(ang), rng.uniform(0.05, 0.35, n), -9 * np.sin(ang)]
        d[:] = np.c_[np.cos(ang), rng.normal(scale=2e-3, size=n), np.sin(ang)] * rng.uniform(0.5, 2, (n, 1))
    elif kind == "far":
        o[:] = np.c_[xz[:, 0] + 70, rng.uniform(1, 4, n), xz[:, 1]]
        d[:] = np.c_[-rng.uniform(0.5, 1, n), -rng.uniform(0.01, 0.05, n), rng.normal(scale=0.05, size=n)]
    else:  # "range": a direction too long for the line test
        o[:] = np.c_[xz[:, 0], rng.uniform(1, 4, n), xz[:, 1]]
        d[:] = np.c_[rng.normal(size=n), -rng.uniform(0.5, 1, n), rng.normal(size=n)] * 1e7
    return np.c_[o, d].astype(np.float32)


def _waves(rng):
    """Batches of 64, 65 and 128 rays, each shaping its waves as one of the
    host emulation's cases (tests/grid_coop_check.cpp)."""
    out = {}
    out["64 without items"] = _rays("none", 64, rng)
    w = _rays("none", 64, rng)
    w[37] = _rays("long", 1, rng)[0]
    out["64, one lane holds every item"] = w
    out["64 short"] = _rays("short", 64, rng)
    w = _rays("short", 65, rng)
    out["65: a second wave with a single live lane"] = w
    w = _rays("long", 65, rng)
    out["65 long: one lane's items over its own rounds"] = w
    out["128 short"] = _rays("short", 128, rng)
    w = _rays("short", 128, rng)
    w[::2] = _rays("none", 64, rng)
    w[5] = _rays("long", 1, rng)[0]
    w[64 + 63] = _rays("long", 1, rng)[0]
    out["128 mixed: lanes without items in between"] = w
    out["128 long: many rounds"] = _rays("long", 128, rng)
    w = _rays("short", 64, rng)
    w[17] = _rays("far", 1, rng)[0]
    out["64, a far-origin lane among normal ones"] = w
    w = _rays("long", 128, rng)
    w[3] = _rays("range", 1, rng)[0]
    w[64 + 40] = _rays("far", 1, rng)[0]
    out["128, give-up lanes among long ones"] = w
    return out


def test_hit_world_hand_built_waves(gpu_ctx, oracle, rtx, world):
    rng = np.random.default_rng(2024)
    waves = _waves(rng)
    got = {}
    try:
        for mode in ("linear", "auto"):
            gpu_ctx.set_scan_mode(mode)
            gpu_ctx.upload_world(world)
            got[mode] = {k: gpu_ctx.debug_hit_world(r) for k, r in waves.items()}
    finally:
        gpu_ctx.set_scan_mode("auto")
        gpu_ctx.upload_world(world)
    hits = 0
    for k, r in waves.items():
        want = oracle.hit_world_f32(world, r)
        assert_bits_equal(got["auto"][k], want, f"{k}: grid vs oracle")
        assert_bits_equal(got["auto"][k], got["linear"][k], f"{k}: grid vs linear")
        hits += int((want[:, 0] == 1).sum())
    assert hits > 200  # the batches do hit the layer


def test_small_frame_whole_and_share(gpu_ctx, oracle, rtx, world):
    """160x90 spp 4, whole and as part 3 of an 8-way row split with 5-row
    tiles (10 rows: its waves hold fewer pixels than lanes)."""
    W, H, T, R, part = 160, 90, 5, 8, 3
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    want, segs = oracle.render_rows(world, frame, np.arange(H), nthreads=min(8, os.cpu_count() or 1))
    ids = rtx.part_row_ids(H, T, part, R)
    got = {}
    try:
        for mode in ("linear", "auto"):
            gpu_ctx.set_scan_mode(mode)
            gpu_ctx.upload_world(world)
            gpu_ctx.set_frame(frame)
            gpu_ctx.stats_reset()
            img = gpu_ctx.render_image()
            assert gpu_ctx.stats().segments == segs, mode
            buf = gpu_ctx.alloc((len(ids), W, 4))
            gpu_ctx.render_rows(T, part, R, buf.ptr)
            got[mode] = (img, buf.numpy())
            buf.free()
    finally:
        gpu_ctx.set_scan_mode("auto")
        gpu_ctx.upload_world(world)
    assert_bits_equal(got["auto"][0], want, "whole frame vs oracle")
    assert_bits_equal(got["auto"][1], want[ids], "part 3 of 8 vs oracle rows")
    assert_bits_equal(got["auto"][0], got["linear"][0], "whole frame vs linear")
    assert_bits_equal(got["auto"][1], got["linear"][1], "part 3 of 8 vs linear")
