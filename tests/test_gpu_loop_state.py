"""The lane-mode render keeps no loop-invariant value in scratch (RESULTS.md
S15): lane ranks come from v_mbcnt instead of per-lane 64-bit masks (refill,
take_from), the walk's nearest-mark search shifts the ballot instead of
masking it (grid_wave_mask), the dynamic priority's unit is an SGPR and its
three bars one load (dyn_level), and the wave's heartbeat time and private
queue run live in lanes of one VGPR (WaveWords). What those idioms could break
sits at wave edges, so the shapes are the smallest that reach them, on the
product and the stress library, bit for bit against the fp32 oracle with equal
segment counts.

A launch of fewer than 8 samples per pixel takes the exact grid and has no
persistent loop (rtx_refine_keys.h kLptMinSpp), so the 65 x 3 and 33 x 2 frames
run at spp 3 and at spp 9: only the latter reach refill and the priority site.
Their 195 and 66 pixels are fewer than the launch's lanes, so each wave refills
once, from an all-idle wave, the last one taking a partial run; a 96 x 64 frame
on ~1 % of the resident waves (more pixels than lanes, unequal costs) adds the
refills of waves whose idle lanes are any subset, lane 63 and both sides of
lane 32 included.
"""
import os

import numpy as np
import pytest

import hostile_cases as hc
import regime_cases as rc
from conftest import ROOT
from test_gpu_grid_coop import _rays

pytestmark = pytest.mark.gpu

STRESS_LIB = os.path.join(ROOT, "raytrace-we-gpu_amd", "lib", "variants", "librtx_stress.so")
CTXS = ["gpu_ctx", "stress_ctx"]
DEPTH = 8


@pytest.fixture(scope="module")
def stress_ctx(rtx):
    """The stress build (make all). A missing library is a failed build, not a reason to skip."""
    if not os.path.exists(STRESS_LIB):
        pytest.fail("stress build missing: make all")
    ctx = rtx.Context(0, lib=rtx.load_library(STRESS_LIB))
    yield ctx
    ctx.close()


def assert_bits_equal(a, b, what=""):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, what
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} values differ; first at {np.argwhere(~same)[:5].tolist()}"


# ---- frames ------------------------------------------------------------------

# (width, height, spp): 65 x 3 = three full waves and one of 3 lanes; 33 x 2 = one wave of 64 and one of 2
FRAMES = [(65, 3, 3), (65, 3, 9), (33, 2, 3), (33, 2, 9), (96, 64, 9)]
FEW_WAVES = dict(occupancy_small=0.01, occupancy_low=0.01, occupancy_normal=0.01)
# every pixel traced in lane mode to its end (tools/variant_bench.py --schedule lane-only)
LANE_ONLY = dict(tier1_bar=1e30, tier1_bar_small=1e30, tier1_bar_low=1e30, tier2_bar_small=1e30,
                 tier2_bar_medium=1e30, tier2_bar=1e30, trace_small=0.0, trace_low=0.0, trace_medium=0.0,
                 trace_large=0.0, promote_small=0.0, promote_low=0.0, promote_medium=0.0, promote_large=0.0,
                 promote_big_scene=0.0, tail_coop_max=1)
SCHEDULES = {
    "chunk1": dict(refill_chunk=1),    # one queue atomic per refill (refill's second path)
    "chunk16": dict(refill_chunk=16),  # the wave's private run of 16 slots (its first path)
    "lane_only": dict(LANE_ONLY),
}


def make_world(rtx, which, spp):
    if which == "rtiow11":
        w = rtx.random_world(11, depth=DEPTH, spp=spp)
        assert w.count == 486
        return w
    # nine spheres: the ground and eight of the three materials at different distances
    rng = np.random.default_rng(9)
    sph = np.c_[rng.uniform(-4, 4, 9), np.full(9, 0.5), rng.uniform(-4, 4, 9), np.full(9, 0.5)]
    sph[0] = (0, -1000, 0, 1000)
    mt = np.array([0, 0, 1, 2, 0, 1, 2, 0, 1], np.float32)
    mv = np.c_[rng.uniform(0.3, 1.0, (9, 3)), np.where(mt == 1, 0.1, 1.5)]
    return rtx.World(sph.astype(np.float32), mt, mv.astype(np.float32), DEPTH, spp)


_WANT = {}


def oracle_frame(oracle, rtx, which, w, h, spp):
    """(world, frame, oracle image, oracle segments): the oracle's part computed once, read-only."""
    world = make_world(rtx, which, spp)
    frame = rtx.camera_look_at(w, h, aspect=w / h)
    key = (which, w, h, spp)
    if key not in _WANT:
        img, segs = oracle.render_rows(world, frame, np.arange(h), nthreads=min(8, os.cpu_count() or 1))
        img.setflags(write=False)
        _WANT[key] = (img, segs)
    return world, frame, _WANT[key][0], _WANT[key][1]


def render_and_compare(ctx, oracle, rtx, which, shape, fields, what):
    w, h, spp = shape
    world, frame, want, segs = oracle_frame(oracle, rtx, which, w, h, spp)
    ctx.set_schedule()
    try:
        if (w, h) == (96, 64):
            fields = dict(FEW_WAVES, **fields)
        ctx.set_schedule(**fields)
        ctx.upload_world(world)
        ctx.set_frame(frame)
        ctx.stats_reset()
        img = ctx.render_image()
        assert ctx.stats().segments == segs, what
        assert_bits_equal(img, want, what)
    finally:
        ctx.set_schedule()


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("which", ["rtiow11", "nine"])
@pytest.mark.parametrize("shape", FRAMES, ids=lambda s: "%dx%d_spp%d" % s)
def test_refill_ranks(request, oracle, rtx, ctx_name, sched, which, shape):
    """Both refill paths and the lane-only schedule: every pixel is traced
    exactly once (a wrong rank gives two lanes one slot and leaves another
    untraced: the frame and the segment count both show it)."""
    ctx = request.getfixturevalue(ctx_name)
    render_and_compare(ctx, oracle, rtx, which, shape, SCHEDULES[sched], f"{ctx_name} {sched} {which} {shape}")


# prio_bar1 = 0 turns the dynamic priority off (cost_in NULL: the hot-slot
# priority); 1e-30 makes every wave with a pixel level 3 (the bar that
# rtx_set_schedule accepts nearest 0), 1e30 none
BARS = {"off": (0.0, 0.0, 0.0), "tiny": (1e-30, 1e-30, 1e-30), "huge": (1e30, 1e30, 1e30), "spread": (1e-30, 1.0, 1e30)}


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("bars", list(BARS))
@pytest.mark.parametrize("shape", [(65, 3, 9), (96, 64, 9)], ids=lambda s: "%dx%d_spp%d" % s)
def test_priority_site(request, oracle, rtx, ctx_name, bars, shape):
    """Priorities change timing only: the same frame and segment count with the
    dynamic priority off, and with bars no wave, every wave or some waves pass."""
    ctx = request.getfixturevalue(ctx_name)
    b1, b2, b3 = BARS[bars]
    render_and_compare(ctx, oracle, rtx, "rtiow11", shape, dict(prio_bar1=b1, prio_bar2=b2, prio_bar3=b3),
                       f"{ctx_name} bars {bars} {shape}")


# ---- the walk ------------------------------------------------------------------

BATCHES = (1, 31, 32, 33, 63, 64, 65)


def walk_batches():
    """{name: rays}: for each batch size, rays that all own items (long: many
    rounds; short: one or two items), and batches where only chosen lanes do:
    lanes 31 and 32 (owners on both sides of lane 32), lane 63 alone, and the
    single lane of a second wave."""
    rng = np.random.default_rng(15)
    out = {}
    for n in BATCHES:
        out[f"{n} long"] = _rays("long", n, rng)
        out[f"{n} short"] = _rays("short", n, rng)
        owners = [k for k in (0, 31, 32, 63, 64) if k < n]
        w = _rays("none", n, rng)
        w[owners] = _rays("long", len(owners), rng)
        out[f"{n}: owners at lanes {owners} only"] = w
        w = _rays("none", n, rng)
        w[n - 1] = _rays("long", 1, rng)[0]
        out[f"{n}: the last lane the only owner"] = w
    return out


_WALK = {}


def walk_case(oracle, name):
    """(case, {batch: rays}, {batch: oracle records}) of a regime_cases world, built once."""
    if name not in _WALK:
        case = rc.world(name)
        batches = walk_batches()
        want = {k: oracle.hit_world_f32(case, r) for k, r in batches.items()}
        for v in want.values():
            v.setflags(write=False)
        _WALK[name] = (case, batches, want)
    return _WALK[name]


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("name", ["rtiow11", "r3_small"])
def test_walk_sharing_at_wave_edges(request, oracle, rtx, ctx_name, name):
    """Batches of 1..65 rays through rtx_debug_hit_world on an R1 and an R3
    world (position map in LDS and in memory): every record is the oracle's."""
    ctx = request.getfixturevalue(ctx_name)
    assert rc.REGIME[name] == {"rtiow11": "R1", "r3_small": "R3"}[name]
    case, batches, want = walk_case(oracle, name)
    ctx.set_scan_mode("auto")
    ctx.upload_world(rtx.World(case.spheres, case.mat_types, case.mat_values, 1, 1))
    assert ctx.scene_info()["grid"] == 1
    hits = 0
    for k, rays in batches.items():
        assert_bits_equal(ctx.debug_hit_world(rays), want[k], f"{ctx_name} {name}: {k}")
        hits += int((want[k][:, 0] == 1).sum())
    assert hits > 100  # the batches do meet the layer


@pytest.mark.parametrize("ctx_name", CTXS)
def test_walk_with_a_lane_that_gives_up(request, oracle, rtx, ctx_name):
    """Rays with a NaN direction component (hostile_cases' class dx_nan) in
    partial-wave batches, alone and among grazing rays: the lane gives up the
    walk, the wave scans every block, and the shifted-ballot search is not
    reached with that lane's values."""
    ctx = request.getfixturevalue(ctx_name)
    case, _, classes = hc.degenerate_world(11)
    bad = classes["dx_nan"]
    rng = np.random.default_rng(16)
    batches = {"33 hostile": bad[:33], "1 hostile": bad[:1]}
    for n, at in ((33, (32,)), (65, (3, 64)), (64, (63,))):
        w = _rays("long", n, rng)
        w[list(at)] = bad[:len(at)]
        batches[f"{n} long, hostile at {at}"] = w
    ctx.set_scan_mode("auto")
    ctx.upload_world(rtx.World(case.spheres, case.mat_types, case.mat_values, 1, 1))
    for k, rays in batches.items():
        assert_bits_equal(ctx.debug_hit_world(rays), oracle.hit_world_f32(case, rays), f"{ctx_name}: {k}")
