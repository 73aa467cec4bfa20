"""Whole frames, bit for bit, through every shape of the large-scene culled
layout and from cameras inside, above, along and far outside it (DESIGN.md
§3e; the worlds and cameras: cull_cases.py; that the layouts are those shapes,
that their bounds are conservative and that the cameras reach every section
and both outcomes of every level's test: test_cull_cases.py, on the CPU).

Every scene with n_pad > 1024 runs through the layout rtx_cull.h builds at
upload: up to three sections, the flat one aligned to 512 blocks behind
never-passing padding, three levels of bounds whose partial last rows are cut
by masks, all hanging on cflat_lo. Every world's test first asserts its row
(the padded position count and the flat section's first block among it)
against rtx_debug_scene_info, so a rule that moves fails the test instead of
quietly giving the scene another layout; then every render kernel instance
draws it. Each image must equal the oracle's over every pixel, and the segment
count the oracle's. No tolerance.
"""
import os

import numpy as np
import pytest

import cull_cases as cc
import film_cases as fc
import paths_cases as pc
import regime_cases as rc
import test_gpu_cast as tcast
import test_gpu_features as tfeat
import test_gpu_film as tfilm
import test_gpu_paths as tpaths
from cases import grazing_rays
from test_gpu_layout import assert_bits_equal
from test_gpu_parity import stress_ctx, surface_rays  # noqa: F401
from test_gpu_refine import TIER_SCHEDULES

pytestmark = pytest.mark.gpu

CTXS = ["gpu_ctx", "stress_ctx"]
NTHREADS = min(8, os.cpu_count() or 1)
ROWS = np.arange(cc.H)
SPP_GRID, SPP_SCHED, SPP_PS = 3, 10, 5  # the exact grid; the scheduled path (>= 8); per-sample RNG
PART = (4, 1, 3)  # tile_rows, part, nparts
SHARES_DOWN = dict(medium_share=0.01, low_share=0.005, small_share=0.001)
f32 = np.float32


def _rtx_world(rtx, case, spp):
    return rtx.World(case.spheres, case.mat_types, case.mat_values, case.depth, spp)


def _frame(rtx, camera, rng_mode=0):
    f = rtx.camera_look_at(**cc.camera_args(camera))
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
    ["default", "part"] for the rows of PART at SPP_SCHED. "rtiow11" and
    "empty": the `default` camera's "sched" frame only."""
    if name not in _WANT:
        out = {}
        if name == "empty":
            out["default", "sched"] = _oracle(oracle, _empty(rtx), _frame(rtx, "default"))
        elif name == "rtiow11":
            out["default", "sched"] = _oracle(oracle, _rtx_world(rtx, rc.world(name), SPP_SCHED), _frame(rtx, "default"))
        else:
            case = cc.world(name)
            for cam in cc.CAMERAS:
                out[cam, "grid"] = _oracle(oracle, _rtx_world(rtx, case, SPP_GRID), _frame(rtx, cam))
                out[cam, "sched"] = _oracle(oracle, _rtx_world(rtx, case, SPP_SCHED), _frame(rtx, cam))
                out[cam, "ps"] = _oracle(oracle, _rtx_world(rtx, case, SPP_PS), _frame(rtx, cam, 1))
            out["default", "part"] = _oracle(oracle, _rtx_world(rtx, case, SPP_SCHED), _frame(rtx, "default"),
                                             rtx.part_row_ids(cc.H, *PART))
        _WANT[name] = out
    return _WANT[name]


def _empty(rtx):
    return rtx.World(np.zeros((0, 4), f32), np.zeros(0, f32), np.zeros((0, 4), f32), 50, SPP_SCHED)


@pytest.fixture(scope="module")
def want_of(oracle, rtx):
    return lambda name: wanted(oracle, rtx, name)


def assert_info(ctx, name, linear=False):
    info = ctx.scene_info()
    want = cc.expected_info(name, linear)
    got = {k: info[k] for k in want}
    assert got == want, f"{name}: rtx_debug_scene_info says {info}, the layout table {want}"


def render_check(ctx, frame, want, what):
    img_want, segs = want
    ctx.set_frame(frame)
    ctx.stats_reset()
    img = ctx.render_image()
    st = ctx.stats()
    assert_bits_equal(img, img_want, what)
    assert st.segments == segs, what


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("name", list(cc.WORLDS))
def test_frames_bit_exact(request, rtx, want_of, ctx_name, name):
    ctx = request.getfixturevalue(ctx_name)
    case, want = cc.world(name), want_of(name)
    what = f"{ctx_name} {name}"
    ctx.set_scan_mode("auto")
    ctx.set_schedule()
    # a. chain RNG, spp 3: the exact-grid kernel
    ctx.upload_world(_rtx_world(rtx, case, SPP_GRID))
    assert_info(ctx, name)
    for cam in cc.CAMERAS:
        render_check(ctx, _frame(rtx, cam), want[cam, "grid"], f"{what} {cam} a (spp {SPP_GRID})")
    # b. per-sample RNG, spp 5: k_render_ps
    ctx.upload_world(_rtx_world(rtx, case, SPP_PS))
    assert_info(ctx, name)
    for cam in cc.CAMERAS:
        render_check(ctx, _frame(rtx, cam, 1), want[cam, "ps"], f"{what} {cam} b (per-sample, spp {SPP_PS})")
    # c. chain RNG, spp 10: the pre-pass, the cost queue and the persistent render
    ctx.upload_world(_rtx_world(rtx, case, SPP_SCHED))
    assert_info(ctx, name)
    for cam in cc.CAMERAS:
        render_check(ctx, _frame(rtx, cam), want[cam, "sched"], f"{what} {cam} c (spp {SPP_SCHED})")
    # d. the same under k_trace with promotion and under the group tiers, both with
    # the large scenes' promotion; and with the share classes moved down
    try:
        scheds = [dict(TIER_SCHEDULES[1], promote_big_scene=1), dict(TIER_SCHEDULES[2], promote_big_scene=1),
                  SHARES_DOWN]
        for i, sched in enumerate(scheds):
            ctx.set_schedule()
            ctx.set_schedule(**sched)
            for cam in ("default", "grazing", "in_slab"):
                render_check(ctx, _frame(rtx, cam), want[cam, "sched"], f"{what} {cam} d (schedule {i}: {sched})")
    finally:
        ctx.set_schedule()
    # e. refine(3) then refine(7): the kRefine instances; the plain render at spp 10
    for cam in ("default", "in_slab"):
        img_want, segs = want[cam, "sched"]
        ctx.set_frame(_frame(rtx, cam))
        ctx.stats_reset()
        assert ctx.refine(3, reset=True) == 3
        assert ctx.refine(7) == 10
        st = ctx.stats()
        assert_bits_equal(ctx.download(), img_want, f"{what} {cam} e (refine 3 + 7)")
        assert st.segments == segs, f"{what} {cam} e"
    # f. part 1 of 3 in tiles of 4 rows
    ids = rtx.part_row_ids(cc.H, *PART)
    img_want, segs = want["default", "part"]
    ctx.set_frame(_frame(rtx, "default"))
    buf = ctx.alloc((len(ids), cc.W, 4))
    try:
        ctx.stats_reset()
        ctx.render_rows(*PART, buf.ptr)
        ctx.sync()
        st = ctx.stats()
        assert_bits_equal(buf.numpy(), img_want, f"{what} default f (part {PART[1]} of {PART[2]})")
        assert st.segments == segs, f"{what} default f"
    finally:
        buf.free()
    # g. the LINEAR upload: the same image and segments, no culled layout
    try:
        ctx.set_scan_mode("linear")
        ctx.upload_world(_rtx_world(rtx, case, SPP_SCHED))
        assert_info(ctx, name, linear=True)
        info = ctx.scene_info()
        assert info["kernels"] == 2 and info["cull_positions"] == 0 and info["cull_flat_lo"] == 0, info
        for cam in ("default", "far"):
            render_check(ctx, _frame(rtx, cam), want[cam, "sched"], f"{what} {cam} g (linear)")
    finally:
        ctx.set_scan_mode("auto")


_RAYS = {}


def hit_world_rays(oracle, rtx, name):
    """The primary rays of every camera, 4,000 grazing rays and 2,000 surface
    rays over world `name`, and the oracle's records at t_min 1e-6 and 1e-3:
    built once, read-only."""
    if name not in _RAYS:
        case = cc.world(name)
        rng = np.random.default_rng(300 + len(name))
        rays = np.concatenate([cc.primary_rays(_frame(rtx, cam)) for cam in cc.CAMERAS] +
                              [grazing_rays(case.spheres, 4000, rng, xaxis_frac=0.05),
                               surface_rays(case.spheres, 2000, rng)]).astype(f32)
        want = {t_min: oracle.hit_world_f32(case, rays, t_min) for t_min in (1e-6, 1e-3)}
        for a in (rays, *want.values()):
            a.setflags(write=False)
        _RAYS[name] = (rays, want)
    return _RAYS[name]


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("name", ["all_flat", "ground_flat", "bimodal"])
def test_hit_world_flat_first(request, oracle, rtx, ctx_name, name):
    """rtx_debug_hit_world through the per-lane culled scan and the
    wave-cooperative one in both walks (1, 8 and 32 rays per wave; the
    per-lane walk at 1 and 8) where the flat section is the first one
    (all_flat: cflat_lo == 0, b0 >= cflat_lo at every level from entry 0),
    where it follows 511 padding blocks (ground_flat), and where section 0
    has many blocks and layer-height members (bimodal): bit for bit against
    the oracle at t_min 1e-6 and 1e-3, and more than 30 % hits."""
    ctx = request.getfixturevalue(ctx_name)
    rays, want = hit_world_rays(oracle, rtx, name)
    ctx.set_scan_mode("auto")
    ctx.upload_world(_rtx_world(rtx, cc.world(name), 1))
    assert_info(ctx, name)
    forms = [("lane", rtx.DEBUG_CULLED), ("coop 1", rtx.DEBUG_CULLED_COOP(1)), ("coop 8", rtx.DEBUG_CULLED_COOP(8)),
             ("coop 32", rtx.DEBUG_CULLED_COOP(32)), ("coop 1, per-lane walk", rtx.DEBUG_CULLED_COOP_LANE(1)),
             ("coop 8, per-lane walk", rtx.DEBUG_CULLED_COOP_LANE(8))]
    for t_min, rec in want.items():
        assert (rec[:, 0] == 1).mean() > 0.3, (name, t_min)
        for what, start in forms:
            got = ctx.debug_hit_world(rays, t_min=t_min, start_block=start)
            assert_bits_equal(got, rec, f"{ctx_name} {name}, {what}, t_min {t_min}")


@pytest.mark.parametrize("name", ["all_flat", "no_flat", "bimodal", "wide"])
def test_other_entry_points(gpu_ctx, oracle, rtx, name):
    """The calls that trace without rendering a frame, one each per layout
    shape, each against the oracle with its own test file's helpers: the
    first-hit planes, rtx_cast_rays in both orders, rtx_trace_paths and
    rtx_trace_film."""
    ctx, case = gpu_ctx, cc.world(name)
    ctx.set_scan_mode("auto")
    # the first-hit feature planes of two frames
    world = tfeat.rtx_world(rtx, case)
    ctx.upload_world(world)
    assert_info(ctx, name)
    for cam in ("in_slab", "default"):
        frame = _frame(rtx, cam)
        ctx.set_frame(frame)
        tfeat.check_planes(ctx, tfeat.expected(oracle, ("cull", name, cam), world, frame), f"{name}/{cam}")
    # closest hits of the primary rays of every camera, as given and coherent
    r6 = np.concatenate([cc.primary_rays(_frame(rtx, cam)) for cam in cc.CAMERAS])
    want = tcast.want_records(rtx, oracle.hit_world_f32(case, r6, tcast.T_MIN))
    assert 0.2 < (want["index"] >= 0).mean(), "inputs: too few hits"
    tcast.upload(ctx, rtx, case)
    assert_info(ctx, name)
    for order in ("given", "coherent"):
        tcast.check(ctx, rtx, tcast.rays8(r6), want, order, name)
    # path queries: 8 rays over the world's extent, 8 x 4 seeds each, 4 samples
    # (recipe seed 4402: chosen on the CPU oracle so that expect's cap on all-sky rays holds in all four
    # worlds, all_flat, which has no ground, among them: 1, 0, 0 and 2 of 8)
    o, L = pc.ray_recipe(8, 4402, float(cc._extent(case.count)) / 11.0)
    e = pc.expect(case, o, L, samples=4)
    tpaths.upload(ctx, rtx, case)
    assert_info(ctx, name)
    tpaths.check(ctx, e, name, samples=4)
    # film records of every third pixel of the default frame, 4 samples
    frame = _frame(rtx, "default")
    lin = type("World", (), dict(spheres=case.spheres, mat_types=case.mat_types, mat_values=case.mat_values,
                                 depth=fc.DEPTH, spp=4))
    sums, _ = oracle.render_rows_linear(lin, frame, ROWS, nthreads=NTHREADS)
    pick = np.arange(0, cc.W * cc.H, 3)
    ys, xs = np.divmod(pick, cc.W)
    q, img_w, img_h = rtx.film_from_frame(frame, xs, ys)
    tfilm.upload(ctx, rtx, case, spp=4)
    assert_info(ctx, name)
    res, _ = tfilm.trace(ctx, np.ascontiguousarray(q).view(f32).reshape(-1, 16), 4, img=(img_w, img_h))
    assert_bits_equal(res[:, :3], sums.reshape(-1, 4)[pick, :3], f"{name}: film records of every third pixel")


def test_upload_sequence_across_layouts(gpu_ctx, rtx, oracle, want_of):
    """One context, one world after another across the layout shapes, a small
    scene, LINEAR and the empty world: after each upload rtx_debug_scene_info
    is that world's row and the frame the oracle's. What a larger layout
    leaves behind (cbnd3 rows, cperm, cflat_lo, n_cpad) must not reach the next
    world's frame."""
    ctx = gpu_ctx
    frame = _frame(rtx, "default")
    empty_info = dict(count=0, n_pad=0, kernels=0, layout=0, layout_positions=0, map_in_lds=0, flat_lo=0, flat_hi=0,
                      grid=0, grid_nx=0, grid_nz=0, cull_positions=0, cull_flat_lo=0)
    steps = [("wide", "auto"), ("no_flat", "auto"), ("all_flat", "auto"), ("rtiow11", "auto"), ("ground_flat", "auto"),
             ("mixed", "linear"), ("mixed", "auto"), ("empty", "auto"), ("bimodal", "auto")]
    ctx.set_schedule()
    try:
        for i, (w, mode) in enumerate(steps):
            ctx.set_scan_mode(mode)
            if w == "empty":
                ctx.upload_world(_empty(rtx))
                info = ctx.scene_info()
                assert {k: info[k] for k in empty_info} == empty_info, (i, info)
            elif w == "rtiow11":
                ctx.upload_world(_rtx_world(rtx, rc.world(w), SPP_SCHED))
                info = ctx.scene_info()
                want = dict(rc.expected_info(w), cull_positions=0, cull_flat_lo=0)
                assert {k: info[k] for k in want} == want, (i, info)
            else:
                ctx.upload_world(_rtx_world(rtx, cc.world(w), SPP_SCHED))
                assert_info(ctx, w, linear=(mode == "linear"))
            render_check(ctx, frame, want_of(w)["default", "sched"], f"upload {i}: {w} ({mode})")
    finally:
        ctx.set_scan_mode("auto")
