"""Whole frames, bit for bit, through every small-scene scan regime and from
cameras that reach the layer-grid walk's long and give-up branches
(the worlds and cameras: regime_cases.py; that the cameras do
reach those branches: test_scan_regimes.py, on the CPU).

rtx_upload_world sends a scene with n_pad <= 1024 down one of four paths (R1:
sphere copy and position map in LDS; R2: sphere copy, no layout, the
scene-order grid; R3: no sphere copy, the position map in memory; R0: no
layout). Every world's test first asserts its row of that table against
rtx_debug_scene_info, so a constant that moves fails the test instead of
quietly sending the scene somewhere else; then every render kernel instance
draws it from every camera: the exact grid, the pre-pass and the persistent
render, k_trace with promotion and the group tiers, k_render_ps, the refine
instances, a row part, and the LINEAR upload. Each image must equal the
oracle's over every pixel, and the segment count the oracle's. No tolerance.
"""
import os

import numpy as np
import pytest

import regime_cases as rc
from test_gpu_grid_coop import _waves
from test_gpu_layout import assert_bits_equal
from test_gpu_parity import stress_ctx  # noqa: F401
from test_gpu_refine import TIER_SCHEDULES

pytestmark = pytest.mark.gpu

CTXS = ["gpu_ctx", "stress_ctx"]
NTHREADS = min(8, os.cpu_count() or 1)
ROWS = np.arange(rc.H)
SPP_GRID, SPP_SCHED, SPP_PS = 3, 10, 5  # the exact grid; the scheduled path (>= 8); per-sample RNG
PART = (4, 1, 3)  # tile_rows, part, nparts


def _rtx_world(rtx, case, spp):
    return rtx.World(case.spheres, case.mat_types, case.mat_values, case.depth, spp)


def _frame(rtx, camera, rng_mode=0):
    f = rtx.camera_look_at(**rc.camera_args(camera))
    f.rng_mode = rng_mode
    return f


def _oracle(oracle, world, frame, rows=ROWS):
    want, segs = oracle.render_rows(world, frame, rows, nthreads=NTHREADS)
    assert np.isfinite(want).all()  # NaN == NaN never decides a comparison here
    want.setflags(write=False)
    return want, segs


_WANT = {}


def wanted(oracle, rtx, name):
    """The oracle's frames of world `name`, computed once and read-only:
    [camera, "grid" | "sched" | "ps"] -> (image, segments), and
    ["default", "part"] for the rows of PART at SPP_SCHED."""
    if name not in _WANT:
        case = rc.world(name)
        out = {}
        for cam in rc.CAMERAS:
            out[cam, "grid"] = _oracle(oracle, _rtx_world(rtx, case, SPP_GRID), _frame(rtx, cam))
            out[cam, "sched"] = _oracle(oracle, _rtx_world(rtx, case, SPP_SCHED), _frame(rtx, cam))
            out[cam, "ps"] = _oracle(oracle, _rtx_world(rtx, case, SPP_PS), _frame(rtx, cam, 1))
        out["default", "part"] = _oracle(oracle, _rtx_world(rtx, case, SPP_SCHED), _frame(rtx, "default"),
                                         rtx.part_row_ids(rc.H, *PART))
        _WANT[name] = out
    return _WANT[name]


@pytest.fixture(scope="module")
def want_of(oracle, rtx):
    return lambda name: wanted(oracle, rtx, name)


def assert_info(ctx, name, linear=False):
    info = ctx.scene_info()
    want = rc.expected_info(name, linear)
    got = {k: info[k] for k in want}
    assert got == want, f"{name}: rtx_debug_scene_info says {info}, the regime table {want}"


def render_check(ctx, frame, want, what):
    img_want, segs = want
    ctx.set_frame(frame)
    ctx.stats_reset()
    img = ctx.render_image()
    st = ctx.stats()
    assert_bits_equal(img, img_want, what)
    assert st.segments == segs, what


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("name", list(rc.WORLDS))
def test_frames_bit_exact(request, rtx, want_of, ctx_name, name):
    ctx = request.getfixturevalue(ctx_name)
    case, want = rc.world(name), want_of(name)
    what = f"{ctx_name} {name}"
    ctx.set_scan_mode("auto")
    ctx.set_schedule()
    # a. chain RNG, spp 3: the exact-grid kernel
    ctx.upload_world(_rtx_world(rtx, case, SPP_GRID))
    assert_info(ctx, name)
    for cam in rc.CAMERAS:
        render_check(ctx, _frame(rtx, cam), want[cam, "grid"], f"{what} {cam} a (spp {SPP_GRID})")
    # d. per-sample RNG, spp 5: k_render_ps
    ctx.upload_world(_rtx_world(rtx, case, SPP_PS))
    assert_info(ctx, name)
    for cam in rc.CAMERAS:
        render_check(ctx, _frame(rtx, cam, 1), want[cam, "ps"], f"{what} {cam} d (per-sample, spp {SPP_PS})")
    # b. chain RNG, spp 10: the pre-pass, the cost queue and the persistent render
    ctx.upload_world(_rtx_world(rtx, case, SPP_SCHED))
    assert_info(ctx, name)
    for cam in rc.CAMERAS:
        render_check(ctx, _frame(rtx, cam), want[cam, "sched"], f"{what} {cam} b (spp {SPP_SCHED})")
    # c. the same under k_trace with promotion, and under the group tiers
    try:
        for i in (1, 2):
            ctx.set_schedule()
            ctx.set_schedule(**TIER_SCHEDULES[i])
            for cam in ("default", "grazing", "in_slab"):
                render_check(ctx, _frame(rtx, cam), want[cam, "sched"], f"{what} {cam} c (tier schedule {i})")
    finally:
        ctx.set_schedule()
    # e. refine(3) then refine(7): the kRefine instances; the plain render at spp 10
    for cam in ("default", "grazing"):
        img_want, segs = want[cam, "sched"]
        ctx.set_frame(_frame(rtx, cam))
        ctx.stats_reset()
        assert ctx.refine(3, reset=True) == 3
        assert ctx.refine(7) == 10
        st = ctx.stats()
        assert_bits_equal(ctx.download(), img_want, f"{what} {cam} e (refine 3 + 7)")
        assert st.segments == segs, f"{what} {cam} e"
    # f. part 1 of 3 in tiles of 4 rows
    ids = rtx.part_row_ids(rc.H, *PART)
    img_want, segs = want["default", "part"]
    ctx.set_frame(_frame(rtx, "default"))
    buf = ctx.alloc((len(ids), rc.W, 4))
    try:
        ctx.stats_reset()
        ctx.render_rows(*PART, buf.ptr)
        ctx.sync()
        st = ctx.stats()
        assert_bits_equal(buf.numpy(), img_want, f"{what} default f (part {PART[1]} of {PART[2]})")
        assert st.segments == segs, f"{what} default f"
    finally:
        buf.free()
    # g. the LINEAR upload: the same image and segments, no layout, no grid
    try:
        ctx.set_scan_mode("linear")
        ctx.upload_world(_rtx_world(rtx, case, SPP_SCHED))
        assert_info(ctx, name, linear=True)
        info = ctx.scene_info()
        assert info["layout"] == 0 and info["grid"] == 0 and info["map_in_lds"] == 0, info
        for cam in ("default", "far"):
            render_check(ctx, _frame(rtx, cam), want[cam, "sched"], f"{what} {cam} g (linear)")
    finally:
        ctx.set_scan_mode("auto")


@pytest.mark.parametrize("ctx_name", CTXS)
def test_twins_ties_in_render_kernels(request, rtx, oracle, ctx_name):
    """Every ray of rc.in_plane's frame lies in the plane z = 0 and meets a
    column's mirror twins at bit-equal roots; the later scene index, which is
    the earlier position, must win inside the render kernels as it does in
    rtx_debug_hit_world (test_gpu_layout.py): the twins' normals and
    materials differ, so the other choice changes the pixel. The exact grid,
    the scheduled render and k_render_ps, through the LDS position map.
    (That the frame does meet such ties: test_scan_regimes.py.)"""
    ctx = request.getfixturevalue(ctx_name)
    case = rc.world("twins")
    ctx.set_scan_mode("auto")
    ctx.set_schedule()
    for spp, rng_mode in ((SPP_GRID, 0), (SPP_SCHED, 0), (SPP_PS, 1)):
        world = _rtx_world(rtx, case, spp)
        frame = rc.in_plane(_frame(rtx, "default", rng_mode))
        ctx.upload_world(world)
        assert_info(ctx, "twins")
        render_check(ctx, frame, _oracle(oracle, world, frame), f"{ctx_name} twins in-plane spp {spp} rng {rng_mode}")


def _scaled_waves(name):
    """test_gpu_grid_coop's batches, made for x and z in +-11, over the
    extent of world `name`: x and z of origins and directions scaled by
    extent / 11 per axis (the `long` rays' start radius with them)."""
    sph = rc.world(name).spheres[1:]
    sx, sz = np.abs(sph[:, 0]).max() / 11.0, np.abs(sph[:, 2]).max() / 11.0
    scale = np.array([sx, 1.0, sz, sx, 1.0, sz], np.float32)
    return {k: np.ascontiguousarray(r * scale, np.float32) for k, r in _waves(np.random.default_rng(2024)).items()}


@pytest.mark.parametrize("ctx_name", CTXS)
def test_hand_built_waves_other_regimes(request, rtx, oracle, ctx_name):
    """The wave shapes of the shared layer-grid walk (no items, one lane with
    every item, a single live lane, many rounds, give-up lanes among long
    ones) through rtx_debug_hit_world where the grid is over the scene-order
    run (r2_run), where the map is in memory (r3_small) and on the 64 x 8 grid
    (strip, strip_r3): the oracle's answer and the LINEAR upload's."""
    ctx = request.getfixturevalue(ctx_name)
    hits = 0
    try:
        for name in ("r2_run", "r3_small", "strip", "strip_r3"):
            world = _rtx_world(rtx, rc.world(name), 1)
            waves = _scaled_waves(name)
            got = {}
            for mode in ("linear", "auto"):
                ctx.set_scan_mode(mode)
                ctx.upload_world(world)
                assert_info(ctx, name, linear=(mode == "linear"))
                got[mode] = {k: ctx.debug_hit_world(r) for k, r in waves.items()}
            for k, r in waves.items():
                want = oracle.hit_world_f32(world, r)
                assert_bits_equal(got["auto"][k], want, f"{ctx_name} {name} {k}: auto vs oracle")
                assert_bits_equal(got["linear"][k], got["auto"][k], f"{ctx_name} {name} {k}: linear vs auto")
                hits += int((want[:, 0] == 1).sum())
    finally:
        ctx.set_scan_mode("auto")
    assert hits > 200  # the batches do hit


def test_upload_sequence_across_regimes(gpu_ctx, rtx, oracle, want_of):
    """One context, one world after another across every regime, the culled
    kernels, LINEAR and the empty world: after each upload rtx_debug_scene_info
    is that world's row and the frame the oracle's. What an upload leaves
    behind (cpre, cperm, the grid, cflat_lo, a changed count) must not reach
    the next world's frame."""
    ctx = gpu_ctx
    frame = _frame(rtx, "default")
    big = rtx.random_world(20, depth=50, spp=SPP_SCHED)
    assert big.count > 1024
    empty = rtx.World(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros((0, 4), np.float32), 50,
                      SPP_SCHED)
    big_info = dict(count=big.count, n_pad=(big.count + 7) // 8 * 8, kernels=1, sphere_copy_lds=0, layout=0,
                    layout_positions=0, map_in_lds=0, grid=0, grid_nx=0, grid_nz=0)
    empty_info = dict(count=0, n_pad=0, kernels=0, layout=0, layout_positions=0, map_in_lds=0, flat_lo=0, flat_hi=0,
                      grid=0, grid_nx=0, grid_nz=0)
    steps = [("rtiow11", "auto"), ("r2_run", "auto"), ("r3_small", "auto"), (big, "auto"), ("no_layer", "auto"),
             ("lds_full", "auto"), ("rtiow11", "linear"), ("strip_r3", "auto"), (empty, "auto"), ("r3_full", "auto")]
    ctx.set_schedule()
    try:
        for i, (w, mode) in enumerate(steps):
            ctx.set_scan_mode(mode)
            if isinstance(w, str):
                ctx.upload_world(_rtx_world(rtx, rc.world(w), SPP_SCHED))
                assert_info(ctx, w, linear=(mode == "linear"))
                want = want_of(w)["default", "sched"]
            else:
                ctx.upload_world(w)
                info = ctx.scene_info()
                exp = big_info if w is big else empty_info
                assert {k: info[k] for k in exp} == exp, (i, info)
                want = _oracle(oracle, w, frame)
            render_check(ctx, frame, want, f"upload {i}: {w if isinstance(w, str) else w.count} ({mode})")
    finally:
        ctx.set_scan_mode("auto")
