"""The cost map a refine launch records and the queue keys carried from it
(include/rtx.h rtx_refine_set_keys, rtx_refine_last_keys, rtx_refine_cost).

In either key mode the image after every step is the oracle's at the total
spp bit for bit, a step's segments are the oracle's difference, and the cost
map is exact: at every pixel it equals debug_pixel_cost(N) -
debug_pixel_cost(N_prev), the independent exact-grid pass whose row sums
test_gpu_parity.py pins to the oracle — through the exact grid, lane mode, the
tiers, k_trace and its regrouping, promotion, the pre-pass cap's restart and
the large-scene (kPF) kernels, on the product and the stress build.

What a launch is keyed by follows the header's rules: a step below kLptMinSpp
(8) is unscheduled; in carried mode a scheduled step takes the previous
launch's map when that map is valid and covers at least the samples a
pre-pass would trace (kCostSpp = 2; kCostSppLarge = 1 above 1,024 spheres),
an exact-grid step's map included. So the steps (3, 9, 12, 8) are keyed
unscheduled, carried, carried, carried (3 >= 2), and the sequence unscheduled,
pre-pass, carried, carried comes from the steps (1, 9, 12, 8) (1 < 2), which
one more run takes under the schedule whose pre-pass stops pixels.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_refine import ROOT, TIER_SCHEDULES, assert_bits_equal, oracle_at, read_pfm, stress_ctx  # noqa: F401

pytestmark = pytest.mark.gpu

RTX_ERR_INVALID, RTX_ERR_STATE = -1, -3
K_LPT_MIN_SPP, K_COST_SPP, K_COST_SPP_LARGE = 8, 2, 1


def expected_keys(mode, steps, large=False):
    """The header's rule, restated."""
    out, s_prev = [], 0
    for s in steps:
        if s < K_LPT_MIN_SPP:
            out.append("unscheduled")
        elif mode == "carried" and s_prev >= (K_COST_SPP_LARGE if large else K_COST_SPP):
            out.append("carried")
        else:
            out.append("prepass")
        s_prev = s
    return out


_COST = {}


def pixel_cost_at(ctx, key, n):
    """debug_pixel_cost of the context's current world and frame at spp = n
    (zeros at 0): computed once per (input, n), shared, never modified."""
    k = (key, n)
    if k not in _COST:
        f = ctx.frame
        c = ctx.debug_pixel_cost(n).astype(np.int64) if n else np.zeros((f.height, f.width), np.int64)
        c.setflags(write=False)
        _COST[k] = c
    return _COST[k]


def run_steps(ctx, oracle, rtx, key, world, frame, steps, what, mode, schedules=None, large=False, want_keys=None):
    """refine(s) for s in steps from a fresh state in key mode `mode`; after
    every step the image, the step's segments, one launch, what it was keyed by
    and the cost map. Returns the maps."""
    ctx.set_refine_keys(mode)
    want_keys = want_keys or expected_keys(mode, steps, large)
    n, prev_segs, maps = 0, 0, []
    for i, s in enumerate(steps):
        if schedules is not None:
            ctx.set_schedule()
            ctx.set_schedule(**schedules[i])
        ctx.stats_reset()
        got_n = ctx.refine(s, reset=(i == 0))
        st = ctx.stats()
        keyed = ctx.refine_last_keys
        where = f"{what} [{mode}]: step {i} ({s} samples, N = {n + s}, keyed {keyed})"
        assert got_n == n + s == ctx.refined_samples
        want, segs = oracle_at(oracle, rtx, key, world, frame, n + s)
        assert_bits_equal(ctx.download(), want, where)
        assert st.segments == segs - prev_segs, f"{where}: segments"
        assert st.samples == frame.width * frame.height * s and st.launches == 1, where
        assert keyed == want_keys[i], f"{where}: expected {want_keys[i]}"
        cost, covered = ctx.refine_cost()
        assert covered == s and cost.dtype == np.uint32 and cost.shape == (frame.height, frame.width), where
        want_cost = pixel_cost_at(ctx, key, n + s) - pixel_cost_at(ctx, key, n)
        bad = np.argwhere(cost.astype(np.int64) != want_cost)
        assert bad.size == 0, (f"{where}: the cost map differs at {len(bad)} pixels; first {bad[:5].tolist()}: "
                               f"got {cost[tuple(bad[0])]} want {want_cost[tuple(bad[0])]}")
        assert int(cost.sum(dtype=np.int64)) == st.segments, f"{where}: map sum"
        maps.append(cost)
        n += s
        prev_segs = segs
    return maps


@pytest.mark.parametrize("mode", ["carried", "prepass"])
@pytest.mark.parametrize("ctx_name", ["gpu_ctx", "stress_ctx"])
def test_steps_equal_one_shot_and_map_exact(request, oracle, rtx, ctx_name, mode):
    """486 spheres at 320 x 180, steps (3, 9, 12, 8) under every tier's
    schedule and once with the schedule changed between steps, then
    (1, 9, 12, 8) with the pre-pass cap: image, segments, one launch, the keys
    and the exact cost map after every step, in both key modes."""
    ctx = request.getfixturevalue(ctx_name)
    world = rtx.random_world(11, depth=50, spp=60)
    assert world.count == 486
    W, H = 320, 180
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    ctx.upload_world(world)
    ctx.set_frame(frame)
    steps = (3, 9, 12, 8)
    if mode == "carried":
        assert expected_keys(mode, steps) == ["unscheduled", "carried", "carried", "carried"]
    try:
        for sched in TIER_SCHEDULES:
            maps = run_steps(ctx, oracle, rtx, "c320", world, frame, steps, f"{ctx_name} {sched}", mode, [sched] * 4)
            if sched.get("promote_large") == 1:
                # this run is there for the promotion hand-over: promotion was
                # on at a threshold of 1 projected segment, and pixels far above
                # it were traced in the scheduled steps
                got = ctx.get_schedule()
                assert min(got.promote_small, got.promote_low, got.promote_medium, got.promote_large) == 1
                assert all(int(m.max()) > 1 for m in maps[1:])
        run_steps(ctx, oracle, rtx, "c320", world, frame, steps, f"{ctx_name} schedule changed between steps", mode,
                  [TIER_SCHEDULES[0], TIER_SCHEDULES[3], TIER_SCHEDULES[2], TIER_SCHEDULES[1]])
        # a 1-sample map is less than a pre-pass traces: the second step takes
        # the pre-pass (which stops pixels past 6 segments: restarts), the rest carry
        want = ["unscheduled", "prepass", "carried", "carried"] if mode == "carried" else None
        run_steps(ctx, oracle, rtx, "c320", world, frame, (1, 9, 12, 8), f"{ctx_name} short first step", mode,
                  [TIER_SCHEDULES[3]] * 4, want_keys=want)
    finally:
        ctx.set_schedule()
        ctx.set_refine_keys("prepass")


@pytest.mark.parametrize("mode", ["carried", "prepass"])
@pytest.mark.parametrize("ctx_name", ["gpu_ctx", "stress_ctx"])
def test_large_scene(request, oracle, rtx, ctx_name, mode):
    """The kPF kernels (culled scan): steps (2, 10, 10), default schedule and
    promotion with the share classes moved down. The first step is below
    kLptMinSpp (unscheduled); its 2-sample map covers kCostSppLarge = 1."""
    ctx = request.getfixturevalue(ctx_name)
    world = rtx.random_world(20, depth=50, spp=60)
    assert world.count > 1024
    W, H = 192, 108
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    ctx.upload_world(world)
    ctx.set_frame(frame)
    want = ["unscheduled", "carried", "carried"] if mode == "carried" else ["unscheduled", "prepass", "prepass"]
    try:
        for sched in (dict(), dict(promote_big_scene=1.0, medium_share=0.01, low_share=0.005, small_share=0.001)):
            run_steps(ctx, oracle, rtx, "big192", world, frame, (2, 10, 10), f"{ctx_name} {sched}", mode, [sched] * 3,
                      large=True, want_keys=want)
    finally:
        ctx.set_schedule()
        ctx.set_refine_keys("prepass")


def no_map(ctx):
    lib, h = ctx._lib, ctx._h
    f = ctx.frame
    buf = np.zeros((f.height, f.width), np.uint32)
    n = C.c_uint32(77)
    rc = lib.rtx_refine_cost(h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), buf.nbytes, C.byref(n))
    return rc == RTX_ERR_STATE


def test_validity_rules(gpu_ctx, oracle, rtx):
    """What drops the map (the next step is then not carried, and
    rtx_refine_cost right after the event is RTX_ERR_STATE) and what keeps it."""
    ctx = gpu_ctx
    W, H = 64, 36
    world = rtx.random_world(11, depth=20, spp=7)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    other = rtx.camera_look_at(W, H, look_from=(10.0, 3.0, 5.0), aspect=W / H)
    big = rtx.camera_look_at(96, 54, aspect=96 / 54)
    ctx.upload_world(world)
    ctx.set_frame(frame)
    ctx.set_refine_keys("carried")

    def img(key, fr, n):
        return oracle_at(oracle, rtx, key, world, fr, n)[0]

    try:
        with rtx.Context(0) as fresh:  # no launch yet
            assert fresh.refine_last_keys == "unscheduled"
        ctx.refine(9, reset=True)
        assert ctx.refine_last_keys == "prepass" and ctx.refine_cost()[1] == 9
        ctx.refine(8)
        assert ctx.refine_last_keys == "carried"
        # reset: the launch itself starts fresh, so it cannot carry
        ctx.refine(9, reset=True)
        assert ctx.refine_last_keys == "prepass"
        assert_bits_equal(ctx.download(), img("vr", frame, 9), "reset")
        # upload_world
        ctx.upload_world(world)
        assert no_map(ctx)
        ctx.refine(9)
        assert ctx.refine_last_keys == "prepass" and ctx.refined_samples == 9
        # equal frame bytes keep the map
        ctx.set_frame(rtx.camera_look_at(W, H, aspect=W / H))
        assert ctx.refine_cost()[1] == 9
        ctx.refine(8)
        assert ctx.refine_last_keys == "carried"
        assert_bits_equal(ctx.download(), img("vr", frame, 17), "equal bytes: 9 + 8")
        # a different camera
        ctx.set_frame(other)
        assert no_map(ctx)
        ctx.refine(9)
        assert ctx.refine_last_keys == "prepass"
        assert_bits_equal(ctx.download(), img("vr-other", other, 9), "other camera")
        # another size
        ctx.set_frame(big)
        assert no_map(ctx)
        ctx.refine(9)
        assert ctx.refine_last_keys == "prepass"
        assert_bits_equal(ctx.download(), img("vr-big", big, 9), "another size")
        ctx.set_frame(frame)
        # refine_import: the state file holds no map
        ctx.refine(9, reset=True)
        state = ctx.refine_export()
        ctx.refine_import(state, 9)
        assert no_map(ctx)
        ctx.refine(8)
        assert ctx.refine_last_keys == "prepass"
        assert_bits_equal(ctx.download(), img("vr", frame, 17), "imported 9 + 8")
        ctx.refine(9)
        assert ctx.refine_last_keys == "carried"
        # a depth == 0 step traces nothing: unscheduled, and no map after it
        flat = rtx.World(world.spheres, world.mat_types, world.mat_values, 0, 7)
        ctx.upload_world(flat)
        ctx.refine(9)
        assert ctx.refine_last_keys == "unscheduled" and no_map(ctx)
        ctx.refine(9)
        assert ctx.refine_last_keys == "unscheduled" and no_map(ctx)
        ctx.upload_world(world)
        # plain renders, accumulate and set_schedule between two steps keep the map
        ctx.refine(9, reset=True)
        assert_bits_equal(ctx.render_image(), img("vr", frame, 7), "plain render")  # world.spp = 7
        ctx.accumulate(reset=True)
        ctx.set_schedule(trace_small=0.3, promote_small=1)
        assert ctx.refine_cost()[1] == 9
        ctx.refine(8)
        assert ctx.refine_last_keys == "carried"
        assert_bits_equal(ctx.download(), img("vr", frame, 17), "9 + 8 after render, accumulate, set_schedule")
        # back to prepass mid-chain: the map and the state stay, the launch takes the pre-pass
        ctx.set_refine_keys("prepass")
        assert ctx.refine_cost()[1] == 8
        ctx.refine(9)
        assert ctx.refine_last_keys == "prepass" and ctx.refined_samples == 26
        assert_bits_equal(ctx.download(), img("vr", frame, 26), "9 + 8 + 9, the last in prepass mode")
        ctx.set_refine_keys("carried")
        ctx.refine(8)
        assert ctx.refine_last_keys == "carried"
        assert_bits_equal(ctx.download(), img("vr", frame, 34), "and carried again")
    finally:
        ctx.set_schedule()
        ctx.set_refine_keys("prepass")


@pytest.mark.parametrize("opts", ["frame_index", "lens", "guard", "all"])
def test_frame_options_carried(gpu_ctx, oracle, rtx, opts):
    """frame_index, the thin lens and the Lambert guard under carried keys:
    steps (1, 8, 5, 9) — unscheduled, pre-pass (a 1-sample map), unscheduled,
    carried."""
    world = rtx.random_world(11, depth=20, spp=60)
    W, H = 64, 36
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    if opts in ("frame_index", "all"):
        frame.frame_index = 3
    if opts in ("lens", "all"):
        rtx.set_aperture(frame, 0.1)
    if opts in ("guard", "all"):
        frame.flags = rtx.FRAME_LAMBERT_GUARD
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    try:
        run_steps(gpu_ctx, oracle, rtx, f"opt-{opts}", world, frame, (1, 8, 5, 9), opts, "carried",
                  want_keys=["unscheduled", "prepass", "unscheduled", "carried"])
    finally:
        gpu_ctx.set_refine_keys("prepass")


def test_refusals(gpu_ctx, rtx):
    """Refused before any launch; the mode, the state and the map stay."""
    lib, h = gpu_ctx._lib, gpu_ctx._h
    W, H = 64, 36
    world = rtx.random_world(11, depth=20, spp=4)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    try:
        gpu_ctx.set_refine_keys("carried")
        gpu_ctx.refine(9, reset=True)
        gpu_ctx.stats_reset()
        for bad in (2, 3, -1, 1 << 20):
            assert lib.rtx_refine_set_keys(h, bad) == RTX_ERR_INVALID
            assert b"rtx_refine_set_keys" in lib.rtx_last_error()
        assert lib.rtx_refine_set_keys(None, 1) == RTX_ERR_INVALID
        assert lib.rtx_refine_last_keys(None) < 0
        with pytest.raises(ValueError):
            gpu_ctx.set_refine_keys("unscheduled")
        buf = np.zeros((H, W), np.uint32)
        p = buf.ctypes.data_as(C.POINTER(C.c_uint32))
        n = C.c_uint32(77)
        assert lib.rtx_refine_cost(None, p, buf.nbytes, C.byref(n)) == RTX_ERR_INVALID
        assert lib.rtx_refine_cost(h, None, buf.nbytes, C.byref(n)) == RTX_ERR_INVALID
        assert lib.rtx_refine_cost(h, p, buf.nbytes, None) == RTX_ERR_INVALID
        assert lib.rtx_refine_cost(h, p, buf.nbytes - 4, C.byref(n)) == RTX_ERR_INVALID
        assert lib.rtx_refine_cost(h, p, buf.nbytes + 4, C.byref(n)) == RTX_ERR_INVALID
        assert b"rtx_refine_cost" in lib.rtx_last_error()
        assert n.value == 77 and not buf.any()
        assert lib.rtx_refine_cost(h, p, buf.nbytes, C.byref(n)) == 0 and n.value == 9 and buf.any()
        with rtx.Context(0) as fresh:
            assert lib.rtx_refine_cost(fresh._h, p, buf.nbytes, C.byref(n)) == RTX_ERR_STATE
        assert gpu_ctx.stats().launches == 0
        gpu_ctx.refine(8)  # the refused calls changed nothing: still carried mode, the map still there
        assert gpu_ctx.refine_last_keys == "carried"
    finally:
        gpu_ctx.set_refine_keys("prepass")


def test_cli_refine_keys(tmp_path, oracle, rtx):
    """rtx_cli --refine 3,9,12 --refine-keys carried writes the oracle's image
    at 24 samples; an unknown --refine-keys value exits nonzero."""
    cli = os.path.join(ROOT, "raytrace-we-gpu_amd", "bin", "rtx_cli")
    a = str(tmp_path / "a.pfm")
    base = [cli, "--width", "64", "--height", "36", "--depth", "50", "--scene", "rtiow11", "--refine", "3,9,12"]
    out = subprocess.run(base + ["--refine-keys", "carried", "--pfm", a], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert '"refine_keys": "carried"' in out.stdout
    world = rtx.random_world(11, depth=50, spp=60)
    frame = rtx.camera_look_at(64, 36, aspect=64 / 36)
    assert_bits_equal(read_pfm(a), oracle_at(oracle, rtx, "cli", world, frame, 24)[0][..., :3], "--refine-keys carried")
    out = subprocess.run(base + ["--refine-keys", "measured"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0
