"""The render kernel's small-scene instances read the launch's fields from
the kernel arguments where they are used (rtx_kernels.hip params_at) instead
of holding them across the lane-mode loop. What that could break, on the
product and the stress library:

* a workgroup whose four waves are in different cold states at once (one
  refilling, one in lane mode, one in the tail, one serving promotions): a
  launch of a few dozen waves at ~2 pixels per lane, with the heavy tiers, the
  promotion and a tail of up to 64 lanes all on;
* two launches of one context queued back to back, the second enqueued while
  the first may still run: each reads its own arguments, late;
* the stress library's kernel-argument check, extended to every field read
  that way, on the refine, adaptive and row-part instances.

Everything bit for bit the fp32 oracle's, with equal segment counts.
"""
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

STRESS_LIB = os.path.join(ROOT, "raytrace-we-gpu_amd", "lib", "variants", "librtx_stress.so")


@pytest.fixture(scope="module")
def stress_ctx(rtx):
    """The stress build (make all): every list overflow and fallback path, a
    20 ms promotion valve and the kernel-argument check (RTX_CHECK_KERNARG).
    A missing library is a failed build, not a reason to skip."""
    if not os.path.exists(STRESS_LIB):
        pytest.fail("stress build missing: make all")
    ctx = rtx.Context(0, lib=rtx.load_library(STRESS_LIB))
    yield ctx
    ctx.close()


CTXS = ["gpu_ctx", "stress_ctx"]
W, H, SPP, DEPTH = 96, 64, 12, 50
W2, H2, SPP2 = 64, 48, 9
# ~1 % of the resident waves: a few dozen waves, ~2 pixels per lane of 96 x 64
FEW_WAVES = dict(occupancy_small=0.01, occupancy_low=0.01, occupancy_normal=0.01)
COLD = dict(FEW_WAVES, tier2_bar_small=1.0, tier2_bar_medium=1.0, tier2_bar=1.0, promote_small=8, promote_low=8,
            promote_medium=8, promote_large=8, tail_coop_max=64)
SCHEDULES = {
    # tier 1 in the render kernel itself
    "tiers_in_render": dict(COLD, trace_small=0.0, trace_low=0.0, trace_medium=0.0, trace_large=0.0),
    # tier 1 in k_trace beside the render, which also serves promotions
    "k_trace": dict(COLD, trace_small=0.3, trace_low=0.3, trace_medium=0.3, trace_large=0.3),
}


def assert_bits_equal(a, b, what=""):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, what
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} values differ; first at {np.argwhere(~same)[:5].tolist()}"


def make_world(rtx, which, spp):
    if which == "rtiow11":
        w = rtx.random_world(11, depth=DEPTH, spp=spp)
        assert w.count == 486
        return w
    # three spheres: the ground, a glass ball and a metal one
    sph = np.array([[0, -1000, 0, 1000], [0, 1, 0, 1], [4, 1, 0, 1]], np.float32)
    mt = np.array([0, 2, 1], np.float32)
    mv = np.array([[0.5, 0.5, 0.5, 0], [1, 1, 1, 1.5], [0.7, 0.6, 0.5, 0.0]], np.float32)
    return rtx.World(sph, mt, mv, DEPTH, spp)


_WANT = {}


def oracle_frame(oracle, rtx, which, w, h, spp):
    """(world, frame, oracle image, oracle segments), the oracle's part computed once and never modified."""
    world = make_world(rtx, which, spp)
    frame = rtx.camera_look_at(w, h, aspect=w / h)
    key = (which, w, h, spp)
    if key not in _WANT:
        img, segs = oracle.render_rows(world, frame, np.arange(h), nthreads=min(8, os.cpu_count() or 1))
        img.setflags(write=False)
        _WANT[key] = (img, segs)
    return world, frame, _WANT[key][0], _WANT[key][1]


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("which", ["rtiow11", "three"])
def test_waves_in_different_cold_states(request, oracle, rtx, ctx_name, sched, which):
    """96 x 64, spp 12, depth 50 on a few dozen waves: refill, lane mode, the
    heavy tiers, promotion and a 64-lane tail in one launch.

    What the schedule guarantees by construction: 6,144 pixels on ~1 % of the
    resident waves is more than one pixel per lane, so every wave refills; a
    tail of up to 64 lanes means every wave runs its last pixels through the
    tail branch once the queue is exhausted. How many heavy slots and
    promotions a launch had is not observable through the C-ABI (no counter
    is exported), so this test cannot assert that they occurred: on the
    486-sphere world the cost spread makes them certain in practice, on the
    3-sphere world they may not occur, and that case then covers refill, lane
    mode and the tail only."""
    ctx = request.getfixturevalue(ctx_name)
    world, frame, want, segs = oracle_frame(oracle, rtx, which, W, H, SPP)
    ctx.set_schedule()
    try:
        ctx.set_schedule(**SCHEDULES[sched])
        ctx.upload_world(world)
        ctx.set_frame(frame)
        ctx.stats_reset()
        img = ctx.render_image()
        assert ctx.stats().segments == segs, f"{ctx_name} {sched} {which}"
        assert_bits_equal(img, want, f"{ctx_name} {sched} {which}")
    finally:
        ctx.set_schedule()


@pytest.mark.parametrize("ctx_name", CTXS)
def test_two_launches_back_to_back(request, oracle, rtx, ctx_name):
    """One world, uploaded once; 96 x 64 under one schedule, then 64 x 48 under
    the other, with only rtx_set_schedule and rtx_set_frame between the two
    rtx_render_rows calls: neither synchronises, so the second launch is
    enqueued while the first may still be running, and each must read its own
    frame size, queue length and schedule from its own kernel arguments."""
    ctx = request.getfixturevalue(ctx_name)
    world, fa, want_a, segs_a = oracle_frame(oracle, rtx, "rtiow11", W, H, SPP)
    _, fb, want_b, segs_b = oracle_frame(oracle, rtx, "rtiow11", W2, H2, SPP)
    a, b = ctx.alloc((H, W, 4)), ctx.alloc((H2, W2, 4))
    ctx.set_schedule()
    try:
        ctx.upload_world(world)
        ctx.stats_reset()
        ctx.set_schedule(**SCHEDULES["tiers_in_render"])
        ctx.set_frame(fa)
        ctx.render_rows(1, 0, 1, a.ptr)
        ctx.set_schedule(**SCHEDULES["k_trace"])
        ctx.set_frame(fb)
        ctx.render_rows(1, 0, 1, b.ptr)
        ctx.sync()
        assert ctx.stats().segments == segs_a + segs_b, ctx_name
        assert_bits_equal(a.numpy(), want_a, f"{ctx_name}: first launch")
        assert_bits_equal(b.numpy(), want_b, f"{ctx_name}: second launch")
    finally:
        ctx.set_schedule()
        a.free()
        b.free()


@pytest.mark.parametrize("ctx_name", CTXS)
def test_two_launches_another_spp(request, oracle, rtx, ctx_name):
    """96 x 64 spp 12, then 64 x 48 spp 9 under another schedule, the caller
    never synchronising in between. The samples per pixel belong to the world,
    and rtx_upload_world synchronises the stream before it replaces one, so
    here the first launch has ended before the second is enqueued: this case
    checks the change of every launch field between two launches of one
    context; test_two_launches_back_to_back is the overlapping pair."""
    ctx = request.getfixturevalue(ctx_name)
    wa, fa, want_a, segs_a = oracle_frame(oracle, rtx, "rtiow11", W, H, SPP)
    wb, fb, want_b, segs_b = oracle_frame(oracle, rtx, "rtiow11", W2, H2, SPP2)
    a, b = ctx.alloc((H, W, 4)), ctx.alloc((H2, W2, 4))
    ctx.set_schedule()
    try:
        ctx.upload_world(wa)
        ctx.set_frame(fa)
        ctx.stats_reset()
        ctx.set_schedule(**SCHEDULES["tiers_in_render"])
        ctx.render_rows(1, 0, 1, a.ptr)
        ctx.set_schedule(**SCHEDULES["k_trace"])
        ctx.upload_world(wb)
        ctx.set_frame(fb)
        ctx.render_rows(1, 0, 1, b.ptr)
        ctx.sync()
        assert ctx.stats().segments == segs_a + segs_b, ctx_name
        assert_bits_equal(a.numpy(), want_a, f"{ctx_name}: first launch")
        assert_bits_equal(b.numpy(), want_b, f"{ctx_name}: second launch")
    finally:
        ctx.set_schedule()
        a.free()
        b.free()


def test_stress_kernarg_check_on_every_family(stress_ctx, oracle, rtx):
    """One refine step, one adaptive step and one row part (R = 4) on the
    stress library, whose every launch compares the fields it reads late with
    its own argument: rtx_get_stats reports no error (it raises on one)."""
    world, frame, want, segs = oracle_frame(oracle, rtx, "rtiow11", W, H, SPP)
    stress_ctx.set_schedule()
    stress_ctx.upload_world(world)
    stress_ctx.set_frame(frame)
    stress_ctx.stats_reset()
    assert stress_ctx.refine(SPP, reset=True) == SPP
    assert stress_ctx.stats().segments == segs
    assert_bits_equal(stress_ctx.download(), want, "one refine step of 12 samples")
    traced = stress_ctx.refine_adaptive(4, 0.0)  # threshold 0: every pixel is still active
    assert traced == W * H
    stress_ctx.stats()
    tile, parts, part = 4, 4, 2
    ids = rtx.part_row_ids(H, tile, part, parts)
    buf = stress_ctx.alloc((len(ids), W, 4))
    try:
        stress_ctx.render_rows(tile, part, parts, buf.ptr)
        stress_ctx.stats()
        assert_bits_equal(buf.numpy(), want[ids], "part 2 of 4")
    finally:
        buf.free()
