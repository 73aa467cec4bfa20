"""rtx_features, rtx_pick and rtx_mask_from_ids: what a pixel shows.

The expectation is built on the CPU alone: oracle.hit_world_f32 on the
pixel-centre rays of regime_cases.primary_rays gives every pixel's record; the
geom plane is its normal and depth = t * sqrt((dx dx + dy dy) + dz dz) restated
in numpy float32 (each operation rounds to fp32), the surf plane the hit
sphere's albedo from the world arrays and its index. Both planes are compared
bit for bit, on the three scan paths (layout and layer grid, culled, linear),
on partial 8 x 8 patches, on row parts, and on the stress build. The id mask
is compared with a numpy restatement of its rule.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import regime_cases as rc
from test_gpu_refine import ROOT, assert_bits_equal, read_pfm, stress_ctx  # noqa: F401

pytestmark = pytest.mark.gpu

RTX_ERR_INVALID, RTX_ERR_STATE = -1, -3
f32 = np.float32

_WANT = {}


def expected(oracle, key, world, frame):
    """(geom, surf, rec) of a world and frame from the oracle alone; rec is the
    oracle's record per pixel, (H, W, 10). Computed once per key, read-only."""
    if key in _WANT:
        return _WANT[key]
    H, W = frame.height, frame.width
    rays = rc.primary_rays(frame)
    rec = oracle.hit_world_f32(world, rays)
    hit = rec[:, 0] != 0
    idx = np.where(hit, rec[:, 9], -1).astype(np.int64)
    d = rays[:, 3:6]
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    length = np.sqrt(((xx + yy).astype(f32) + zz).astype(f32)).astype(f32)
    with np.errstate(invalid="ignore"):
        depth = (rec[:, 1] * length).astype(f32)
    geom = np.zeros((H * W, 4), f32)
    geom[:, :3] = rec[:, 5:8]
    geom[:, 3] = depth
    geom[~hit] = (0.0, 0.0, 0.0, np.inf)
    mv = np.ascontiguousarray(world.mat_values, f32).reshape(-1, 4)
    surf = np.zeros((H * W, 4), f32)
    surf[hit, :3] = mv[idx[hit], :3]
    surf[:, 3] = idx.astype(f32)
    out = (geom.reshape(H, W, 4), surf.reshape(H, W, 4), rec.reshape(H, W, 10))
    for a in out:
        a.setflags(write=False)
    _WANT[key] = out
    return out


def rtx_world(rtx, case, spp=1):
    return rtx.World(case.spheres, case.mat_types, case.mat_values, case.depth, spp)


def frame_of(rtx, camera, twins=False):
    f = rtx.camera_look_at(**rc.camera_args(camera))
    return rc.in_plane(f) if twins else f


def check_planes(ctx, want, what):
    geom, surf = ctx.features()
    assert_bits_equal(geom, want[0], f"{what}: geom plane")
    assert_bits_equal(surf, want[1], f"{what}: surf plane")
    return geom, surf


CASES = [("rtiow11", "default"), ("rtiow11", "grazing"), ("rtiow11", "top_down"), ("rtiow11", "in_slab"),
         ("two_layers", "default"), ("no_layer", "default"), ("r3_full", "default"), ("strip", "default"),
         ("strip", "grazing"), ("twins", "in_plane")]


@pytest.mark.parametrize("name,camera", CASES, ids=[f"{n}-{c}" for n, c in CASES])
def test_planes_small_scenes(gpu_ctx, oracle, rtx, name, camera):
    """The layout and layer-grid path, 64 x 36, every regime's world."""
    world = rtx_world(rtx, rc.world(name))
    frame = frame_of(rtx, "default", twins=True) if camera == "in_plane" else frame_of(rtx, camera)
    want = expected(oracle, (name, camera), world, frame)
    idx = want[1][..., 3]
    if (name, camera) == ("rtiow11", "default"):
        assert (idx < 0).mean() >= 0.05 and len(np.unique(idx[idx >= 0])) >= 50, "inputs: too few misses or ids"
    if (name, camera) == ("rtiow11", "in_slab"):
        hits = want[2][..., 0] != 0
        assert (want[2][..., 8][hits] == 0).mean() >= 0.5, "inputs: fewer than half the hits are back faces"
    assert (idx >= 0).any()
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    assert gpu_ctx.scene_info()["kernels"] == 0
    check_planes(gpu_ctx, want, f"{name}/{camera}")


@pytest.mark.parametrize("mode,kernels", [("auto", 1), ("linear", 2)])
def test_planes_large_scene(gpu_ctx, oracle, rtx, mode, kernels):
    """1,157 spheres: the culled scan under AUTO, the linear one under
    RTX_SCAN_LINEAR; the path is asserted through rtx_debug_scene_info."""
    world = rtx.random_world(17, depth=50, spp=1)
    assert world.count == 1157
    frame = rtx.camera_look_at(rc.W, rc.H, aspect=rc.W / rc.H)
    want = expected(oracle, "rw17", world, frame)
    idx = want[1][..., 3]
    assert len(np.unique(idx[idx >= 0])) >= 100, "inputs: too few distinct ids"
    try:
        gpu_ctx.set_scan_mode(mode)
        gpu_ctx.upload_world(world)
        gpu_ctx.set_frame(frame)
        assert gpu_ctx.scene_info()["kernels"] == kernels
        check_planes(gpu_ctx, want, f"random_world(17) {mode}")
    finally:
        gpu_ctx.set_scan_mode("auto")


def test_planes_small_scene_linear(gpu_ctx, oracle, rtx):
    """A small scene under RTX_SCAN_LINEAR: no layout, scene-order blocks."""
    world = rtx_world(rtx, rc.world("rtiow11"))
    frame = frame_of(rtx, "default")
    want = expected(oracle, ("rtiow11", "default"), world, frame)
    try:
        gpu_ctx.set_scan_mode("linear")
        gpu_ctx.upload_world(world)
        gpu_ctx.set_frame(frame)
        assert gpu_ctx.scene_info()["layout"] == 0
        check_planes(gpu_ctx, want, "rtiow11/default linear")
    finally:
        gpu_ctx.set_scan_mode("auto")


def test_planes_stress_build(stress_ctx, oracle, rtx):
    """Candidate lists of one entry: every overflow and resolve round."""
    world = rtx_world(rtx, rc.world("rtiow11"))
    frame = frame_of(rtx, "default")
    want = expected(oracle, ("rtiow11", "default"), world, frame)
    stress_ctx.set_scan_mode("auto")
    stress_ctx.upload_world(world)
    stress_ctx.set_frame(frame)
    check_planes(stress_ctx, want, "rtiow11/default stress")


@pytest.mark.parametrize("W,H", [(2, 2), (67, 35), (130, 3)])
def test_partial_patches(gpu_ctx, oracle, rtx, W, H):
    """Sizes that are no multiple of the 8 x 8 patch, smaller than one patch
    and wider than a workgroup's four patches."""
    world = rtx_world(rtx, rc.world("rtiow11"))
    frame = rtx.camera_look_at(W, H, aspect=W / H, **rc.CAMERAS["default"])
    want = expected(oracle, ("rtiow11", W, H), world, frame)
    assert (want[1][..., 3] >= 0).any()
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    check_planes(gpu_ctx, want, f"{W} x {H}")


@pytest.mark.parametrize("tile_rows,nparts", [(5, 3), (1, 4), (8, 2)])
def test_row_parts(gpu_ctx, oracle, rtx, tile_rows, nparts):
    """The parts of a frame, put back together, are the whole-frame planes; one
    plane at a time works (the other pointer NULL)."""
    world = rtx_world(rtx, rc.world("rtiow11"))
    frame = frame_of(rtx, "default")
    want = expected(oracle, ("rtiow11", "default"), world, frame)
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    geom, surf = np.full((rc.H, rc.W, 4), np.nan, f32), np.full((rc.H, rc.W, 4), np.nan, f32)
    for part in range(nparts):
        ids = rtx.part_row_ids(rc.H, tile_rows, part, nparts)
        assert len(ids) == rtx.part_rows(rc.H, tile_rows, part, nparts) > 0
        g, s = gpu_ctx.alloc((len(ids), rc.W, 4)), gpu_ctx.alloc((len(ids), rc.W, 4))
        if part % 2:
            gpu_ctx.features_rows(tile_rows, part, nparts, g.ptr, s.ptr)
        else:
            gpu_ctx.features_rows(tile_rows, part, nparts, g.ptr, 0)
            gpu_ctx.features_rows(tile_rows, part, nparts, 0, s.ptr)
        geom[ids], surf[ids] = g.numpy(), s.numpy()
        g.free()
        s.free()
    assert_bits_equal(geom, want[0], f"parts ({tile_rows}, {nparts}): geom")
    assert_bits_equal(surf, want[1], f"parts ({tile_rows}, {nparts}): surf")


def test_empty_part_and_refusals(gpu_ctx, rtx):
    lib, h = gpu_ctx._lib, gpu_ctx._h
    world = rtx_world(rtx, rc.world("rtiow11"))
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame_of(rtx, "default"))
    # 36 rows in tiles of 8: 5 tiles, so parts 5 and 6 of 7 own nothing
    assert rtx.part_rows(rc.H, 8, 6, 7) == 0
    buf = gpu_ctx.alloc((4, 4), np.float32)
    buf.upload(np.full((4, 4), 7.0, f32))
    gpu_ctx.features_rows(8, 6, 7, buf.ptr, buf.ptr)
    gpu_ctx.sync()
    assert (buf.numpy() == 7.0).all()
    one = C.c_void_p(buf.ptr)
    assert lib.rtx_features(h, None, None) == RTX_ERR_INVALID
    assert lib.rtx_features_rows(h, 0, 0, 1, one, one) == RTX_ERR_INVALID
    assert lib.rtx_features_rows(h, 1, 0, 0, one, one) == RTX_ERR_INVALID
    assert lib.rtx_features_rows(h, 1, 2, 2, one, one) == RTX_ERR_INVALID
    assert (buf.numpy() == 7.0).all()
    with rtx.Context(0) as fresh:
        assert lib.rtx_features(fresh._h, one, one) == RTX_ERR_STATE  # no world
        fresh.upload_world(world)
        assert lib.rtx_features(fresh._h, one, one) == RTX_ERR_STATE  # no frame
        hit = rtx.rtx_hit()
        assert lib.rtx_pick(fresh._h, 0, 0, C.byref(hit)) == RTX_ERR_STATE
    buf.free()


def test_frame_options_do_not_enter(gpu_ctx, oracle, rtx):
    """A lens radius, the per-sample RNG and a frame_index give the pinhole
    frame's planes."""
    world = rtx_world(rtx, rc.world("rtiow11"))
    want = expected(oracle, ("rtiow11", "default"), world, frame_of(rtx, "default"))
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.upload_world(world)
    lens = rtx.set_aperture(frame_of(rtx, "default"), 0.2)
    assert lens.lens_u[3] > 0
    ps = frame_of(rtx, "default")
    ps.rng_mode = rtx.RNG_PER_SAMPLE
    seven = frame_of(rtx, "default")
    seven.frame_index = 7
    for what, frame in (("lens", lens), ("per-sample", ps), ("frame_index 7", seven)):
        gpu_ctx.set_frame(frame)
        check_planes(gpu_ctx, want, what)


def test_nothing_else_changes(gpu_ctx, oracle, rtx):
    """The framebuffer, the stats and a chain state of 8 samples are bitwise
    what they were after rtx_features and rtx_pick."""
    world = rtx.random_world(11, depth=20, spp=4)
    frame = rtx.camera_look_at(rc.W, rc.H, aspect=rc.W / rc.H)
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    gpu_ctx.stats_reset()
    gpu_ctx.refine(8, reset=True)
    before = (gpu_ctx.download(), gpu_ctx.refine_export(), gpu_ctx.refine_cost()[0], gpu_ctx.stats())
    gpu_ctx.features()
    gpu_ctx.pick(10, 10)
    gpu_ctx.pick(0, rc.H - 1)
    after = (gpu_ctx.download(), gpu_ctx.refine_export(), gpu_ctx.refine_cost()[0], gpu_ctx.stats())
    assert_bits_equal(after[0], before[0], "framebuffer")
    assert_bits_equal(after[1], before[1], "chain state")
    assert (after[2] == before[2]).all()
    for field in ("kernel_ms", "launches", "samples", "segments", "sphere_tests"):
        assert getattr(after[3], field) == getattr(before[3], field), field
    assert gpu_ctx.refined_samples == 8 and gpu_ctx.refine(8) == 16  # the chain goes on


def test_pick(gpu_ctx, oracle, rtx):
    """rtx_pick at 20 pixels, a miss among them: the planes' entries, with p, t,
    front_face, the material and its parameter from the oracle's record and the
    world arrays."""
    lib, h = gpu_ctx._lib, gpu_ctx._h
    case = rc.world("rtiow11")
    world = rtx_world(rtx, case)
    frame = frame_of(rtx, "default")
    geom, surf, rec = expected(oracle, ("rtiow11", "default"), world, frame)
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    rng = np.random.default_rng(3)
    pixels = [(int(rng.integers(rc.W)), int(rng.integers(rc.H))) for _ in range(18)] + [(0, 0), (rc.W - 1, rc.H - 1)]
    misses = np.argwhere(surf[..., 3] < 0)
    assert len(misses), "inputs: no miss"
    pixels[0] = (int(misses[0][1]), int(misses[0][0]))
    mt = np.asarray(case.mat_types).reshape(-1)
    mv = np.ascontiguousarray(case.mat_values, f32).reshape(-1, 4)
    seen_hit = False
    for x, y in pixels:
        got = gpu_ctx.pick(x, y)
        r, i = rec[y, x], int(surf[y, x, 3])
        assert got["index"] == i and got["hit"] == (i >= 0), (x, y)
        assert_bits_equal(got["depth"], geom[y, x, 3], f"pick {x},{y}: depth")
        if i < 0:
            assert got["depth"] == np.inf and not got["front_face"] and got["material"] == 0 and got["t"] == 0
            assert not got["p"].any() and not got["normal"].any() and not got["albedo"].any() and got["mat_param"] == 0
            continue
        seen_hit = True
        assert_bits_equal(got["normal"], geom[y, x, :3], f"pick {x},{y}: normal")
        assert_bits_equal(got["albedo"], surf[y, x, :3], f"pick {x},{y}: albedo")
        assert_bits_equal(got["p"], r[2:5], f"pick {x},{y}: p")
        assert_bits_equal(got["t"], r[1], f"pick {x},{y}: t")
        assert got["front_face"] == bool(r[8]) and got["material"] == int(mt[i])
        assert_bits_equal(got["mat_param"], mv[i, 3], f"pick {x},{y}: mat_param")
    assert seen_hit
    hit = rtx.rtx_hit()
    assert lib.rtx_pick(h, rc.W, 0, C.byref(hit)) == RTX_ERR_INVALID
    assert lib.rtx_pick(h, 0, rc.H, C.byref(hit)) == RTX_ERR_INVALID
    assert lib.rtx_pick(h, 0, 0, None) == RTX_ERR_INVALID


# ---- the id mask --------------------------------------------------------------
def grow_mask(listed, grow):
    """Some pixel within Chebyshev distance `grow`, inside the image, is listed."""
    H, W = listed.shape
    p = np.zeros((H + 2 * grow, W + 2 * grow), bool)
    p[grow:grow + H, grow:grow + W] = listed
    out = np.zeros_like(listed)
    for dy in range(2 * grow + 1):
        for dx in range(2 * grow + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def expected_id_mask(surf, ids, grow):
    idx = surf[..., 3]
    return grow_mask((idx >= 0) & np.isin(idx.astype(np.int64), np.asarray(ids, np.int64)), grow)


def test_mask_from_ids(gpu_ctx, oracle, rtx):
    """ids (1, 2, 3), the three big spheres of random_world(11), at grow 0, 1
    and 3; an id nobody sees sets nothing; the argument rules."""
    lib, h = gpu_ctx._lib, gpu_ctx._h
    world = rtx.random_world(11, depth=20, spp=1)
    frame = rtx.camera_look_at(rc.W, rc.H, aspect=rc.W / rc.H)
    want = expected(oracle, "rw11", world, frame)
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    surf = gpu_ctx.alloc((rc.H, rc.W, 4))
    gpu_ctx.features_rows(1, 0, 1, 0, surf.ptr)
    assert_bits_equal(surf.numpy(), want[1], "surf plane on the device")
    sizes = []
    for grow in (0, 1, 3):
        m = expected_id_mask(want[1], (1, 2, 3), grow)
        mask, n = gpu_ctx.mask_from_ids(surf, (1, 2, 3), grow)
        assert n == int(m.sum()) and (mask.numpy() == m.astype(np.uint8)).all(), grow
        sizes.append(n)
        mask.free()
    assert 0 < sizes[0] < sizes[1] < sizes[2] < rc.W * rc.H
    seen = set(np.unique(want[1][..., 3]).astype(int).tolist())
    unseen = next(i for i in range(world.count) if i not in seen)
    mask, n = gpu_ctx.mask_from_ids(surf, (unseen, 0xFFFFFFFF), 3)
    assert n == 0 and not mask.numpy().any()
    ids = (C.c_uint32 * 2)(1, 2)
    cnt = C.c_uint32(77)
    dm, ds = C.c_void_p(mask.ptr), C.c_void_p(surf.ptr)
    assert lib.rtx_mask_from_ids(h, ds, ids, 0, 0, dm, C.byref(cnt)) == RTX_ERR_INVALID
    assert lib.rtx_mask_from_ids(h, ds, ids, 257, 0, dm, C.byref(cnt)) == RTX_ERR_INVALID
    assert lib.rtx_mask_from_ids(h, ds, ids, 2, 9, dm, C.byref(cnt)) == RTX_ERR_INVALID
    assert lib.rtx_mask_from_ids(h, None, ids, 2, 0, dm, C.byref(cnt)) == RTX_ERR_INVALID
    assert lib.rtx_mask_from_ids(h, ds, None, 2, 0, dm, C.byref(cnt)) == RTX_ERR_INVALID
    assert lib.rtx_mask_from_ids(h, ds, ids, 2, 0, None, C.byref(cnt)) == RTX_ERR_INVALID
    assert cnt.value == 77 and not mask.numpy().any()
    # without `set` the call is asynchronous and writes the same mask
    assert lib.rtx_mask_from_ids(h, ds, ids, 2, 8, dm, None) == 0
    gpu_ctx.sync()
    assert (mask.numpy() == expected_id_mask(want[1], (1, 2), 8).astype(np.uint8)).all()
    mask.free()
    surf.free()


# ---- rtx_cli -------------------------------------------------------------------
CLI = os.path.join(ROOT, "raytrace-we-gpu_amd", "bin", "rtx_cli")
CLI_BASE = [CLI, "--width", str(rc.W), "--height", str(rc.H), "--depth", "20", "--scene", "rtiow11"]


def _json_lines(out):
    rep = {}
    for line in out.stdout.strip().splitlines():
        rep.update(json.loads(line))
    return rep


def test_cli_aov_and_pick(tmp_path, gpu_ctx, oracle, rtx):
    """--aov writes the four planes (scalars in three channels, row 0 at the
    bottom) and --pick adds what rtx_pick reports to the JSON line."""
    world = rtx.random_world(11, depth=20, spp=1)
    frame = rtx.camera_look_at(rc.W, rc.H, aspect=rc.W / rc.H)
    geom, surf, _ = expected(oracle, "rw11", world, frame)
    hits = np.argwhere(surf[..., 3] >= 0)
    y, x = (int(v) for v in hits[len(hits) // 2])
    prefix = str(tmp_path / "f")
    out = subprocess.run(CLI_BASE + ["--spp", "1", "--aov", prefix, "--pick", f"{x},{y}"], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert_bits_equal(read_pfm(prefix + "_normal.pfm"), geom[..., :3], "--aov normal")
    assert_bits_equal(read_pfm(prefix + "_albedo.pfm"), surf[..., :3], "--aov albedo")
    for name, plane in (("depth", geom[..., 3]), ("id", surf[..., 3])):
        got = read_pfm(f"{prefix}_{name}.pfm")
        for c in range(3):
            assert_bits_equal(got[..., c], plane, f"--aov {name}, channel {c}")
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    want, got = gpu_ctx.pick(x, y), _json_lines(out)["pick"]
    assert want["hit"] and got["hit"] == 1 and (got["x"], got["y"]) == (x, y)
    assert got["index"] == want["index"] == int(surf[y, x, 3])
    assert got["front_face"] == int(want["front_face"]) and got["material"] == want["material"]
    for k in ("t", "depth", "mat_param"):
        assert_bits_equal(f32(got[k]), want[k], f"--pick {k}")
    for k in ("p", "normal", "albedo"):
        assert_bits_equal(np.array(got[k], f32), want[k], f"--pick {k}")
    # a miss: depth is null, the index -1
    my, mx = (int(v) for v in np.argwhere(surf[..., 3] < 0)[0])
    out = subprocess.run(CLI_BASE + ["--spp", "1", "--pick", f"{mx},{my}"], capture_output=True, text=True, timeout=120)
    got = _json_lines(out)["pick"]
    assert out.returncode == 0 and got["hit"] == 0 and got["index"] == -1 and got["depth"] is None
    out = subprocess.run(CLI_BASE + ["--spp", "1", "--pick", f"{rc.W},0"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "rtx_pick" in out.stderr


def test_cli_focus_at(tmp_path, oracle, rtx):
    """--focus-at on a hit: the image is the oracle's for the frame built with
    the reported focus distance and the aperture; on a miss it exits nonzero;
    without --aperture it is refused."""
    world = rtx.random_world(11, depth=20, spp=4)
    frame = rtx.camera_look_at(rc.W, rc.H, aspect=rc.W / rc.H)
    _, surf, rec = expected(oracle, "rw11", world, frame)
    # a pixel of the big sphere in front (index 3, centre (4, 1, 0)): well off the look-at distance
    on3 = np.argwhere(surf[..., 3] == 3)
    assert len(on3), "inputs: sphere 3 is not visible"
    y, x = (int(v) for v in on3[len(on3) // 2])
    img = str(tmp_path / "focus.pfm")
    out = subprocess.run(CLI_BASE + ["--spp", "4", "--aperture", "0.3", "--focus-at", f"{x},{y}", "--pfm", img],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    fd = _json_lines(out)["focus_dist"]
    cam = np.array((13.0, 2.0, 3.0))
    axis = -cam / np.linalg.norm(cam)
    est = float(np.dot(rec[y, x, 2:5].astype(np.float64) - cam, axis))
    assert abs(fd - est) <= 1e-5 * est and abs(fd - np.linalg.norm(cam)) > 0.5, (fd, est)
    focused = rtx.set_aperture(rtx.camera_look_at(rc.W, rc.H, aspect=rc.W / rc.H, focus_dist=fd), 0.3)
    want, _ = oracle.render_rows(world, focused, np.arange(rc.H), nthreads=8)
    assert_bits_equal(read_pfm(img), want[..., :3], "--focus-at image")
    plain, _ = oracle.render_rows(world, rtx.set_aperture(frame, 0.3), np.arange(rc.H), nthreads=8)
    assert (plain[..., :3] != want[..., :3]).any(), "inputs: the focus distance changes nothing"
    my, mx = (int(v) for v in np.argwhere(surf[..., 3] < 0)[0])
    out = subprocess.run(CLI_BASE + ["--spp", "4", "--aperture", "0.3", "--focus-at", f"{mx},{my}"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "nothing under pixel" in out.stderr
    out = subprocess.run(CLI_BASE + ["--spp", "4", "--focus-at", f"{x},{y}"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode != 0 and "--aperture" in out.stderr
