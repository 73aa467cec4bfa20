"""rtx_refine_adaptive: refine only the pixels that are still noisy.

The expectation is built on the CPU alone. For every per-pixel count n that
occurs, the oracle renders the frame at spp n (render_rows: the image;
render_rows_linear: the linear sums). A step's error estimate E is
rtx.adaptive_error (the host's copy of the rule, pinned op by op by
tests/adaptive_check.cpp) on the oracle's sums; the mask and the counts come
from a numpy restatement of the rule; the expected image takes each pixel
from the oracle frame at its own count. After every call the framebuffer, the
counts, the errors, the active count and the chain sums are compared bit for
bit (NaN == NaN), the cost map and stats.segments against
debug_pixel_cost(n_new) - debug_pixel_cost(n_old) (the exact-grid pass that
test_gpu_parity.py pins to the oracle), and everything of an inactive pixel
against what it was.

The threshold of the selective steps is the 90th percentile of the expected
finite E after step 2; every selective step's expected active share must lie
between 5 % and 95 % (asserted: a condition on the inputs, so that no step is
trivially all or nothing).
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_refine import TIER_SCHEDULES, assert_bits_equal, oracle_at, stress_ctx  # noqa: F401

pytestmark = pytest.mark.gpu

RTX_ERR_INVALID, RTX_ERR_STATE = -1, -3
QUANTILE = 0.90
INF = float("inf")

_LIN = {}
_COST = {}
_PLAN = {}


def lin_at(oracle, rtx, key, world, frame, n):
    """The oracle's linear sums at spp = n, (H, W, 3); zeros at 0. Computed
    once per (input, n), shared and never modified."""
    k = (key, n)
    if k not in _LIN:
        if n == 0:
            lin = np.zeros((frame.height, frame.width, 3), np.float32)
        else:
            w = rtx.World(world.spheres, world.mat_types, world.mat_values, world.depth, n)
            lin = np.ascontiguousarray(oracle.render_rows_linear(w, frame, np.arange(frame.height), nthreads=8)[0][..., :3])
        lin.setflags(write=False)
        _LIN[k] = lin
    return _LIN[k]


def cost_at(ctx, key, n):
    """debug_pixel_cost at spp = n (zeros at 0), once per (input, n)."""
    k = (key, n)
    if k not in _COST:
        f = ctx.frame
        c = ctx.debug_pixel_cost(n).astype(np.int64) if n else np.zeros((f.height, f.width), np.int64)
        c.setflags(write=False)
        _COST[k] = c
    return _COST[k]


def dilate(m):
    """Some pixel of the 3 x 3 neighbourhood inside the image is set."""
    H, W = m.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = m
    out = np.zeros_like(m)
    for dy in range(3):
        for dx in range(3):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def expected_mask(err, counts, samples, thr, cap):
    """The rule of include/rtx.h, restated (err >= thr is False for a NaN)."""
    with np.errstate(invalid="ignore"):
        noisy = dilate(err >= np.float32(thr))
    room = np.ones_like(noisy) if cap == 0 else (counts.astype(np.int64) + samples <= cap)
    return noisy & room


def gather(frames, counts):
    """Per pixel the entry of frames[count of the pixel]."""
    out = np.empty_like(frames[int(counts.flat[0])])
    for n in np.unique(counts):
        sel = counts == n
        out[sel] = frames[int(n)][sel]
    return out


def plan(oracle, rtx, key, world, frame, calls, start=0):
    """The expected state after every call of `calls` = [(samples, threshold,
    max_samples)], from a uniform state of `start` samples; a threshold "q" is
    the QUANTILE of the finite expected E at that moment (fixed from then on),
    "max" the largest finite expected E. Computed once per (key, calls, start)."""
    pk = (key, tuple(calls), start)
    if pk in _PLAN:
        return _PLAN[pk]
    H, W = frame.height, frame.width
    counts = np.full((H, W), start, np.uint32)
    err = np.full((H, W), np.inf, np.float32)
    q = None
    steps = []
    for samples, thr, cap in calls:
        if thr == "q":
            if q is None:
                q = float(np.quantile(err[np.isfinite(err)], QUANTILE).astype(np.float32))
            thr = q
        elif thr == "max":
            thr = float(err[np.isfinite(err)].max())
        mask = expected_mask(err, counts, samples, thr, cap)
        old = counts.copy()
        counts = np.where(mask, counts + np.uint32(samples), counts).astype(np.uint32)
        err = err.copy()
        for y, x in np.argwhere(mask):
            n0, n1 = int(old[y, x]), int(counts[y, x])
            err[y, x] = rtx.adaptive_error(lin_at(oracle, rtx, key, world, frame, n0)[y, x], n0,
                                           lin_at(oracle, rtx, key, world, frame, n1)[y, x], n1)
        ns = [int(n) for n in np.unique(counts)]
        image = gather({n: oracle_at(oracle, rtx, key, world, frame, n)[0] for n in ns}, counts)
        sums = gather({n: lin_at(oracle, rtx, key, world, frame, n) for n in ns}, counts)
        steps.append(dict(samples=samples, thr=thr, cap=cap, mask=mask, old=old, counts=counts, err=err, image=image,
                          sums=sums))
    _PLAN[pk] = steps
    return steps


def check_shares(steps, selective):
    px = steps[0]["mask"].size
    for i in selective:
        share = steps[i]["mask"].sum() / px
        assert 0.05 <= share <= 0.95, f"inputs: step {i} would trace {share:.1%} of the pixels"


def precompute_costs(ctx, key, steps):
    for st in steps:
        for n in set(np.unique(st["old"]).tolist()) | set(np.unique(st["counts"]).tolist()):
            cost_at(ctx, key, int(n))


def run_plan(ctx, key, steps, what, schedules=None, reset_first=True, cost=None):
    """The calls of a plan on the GPU, everything compared after each.
    cost: the expected cost map before the first call (None: no valid map)."""
    precompute_costs(ctx, key, steps)
    px = steps[0]["mask"].size
    prev_image = None
    for i, st in enumerate(steps):
        if schedules is not None:
            ctx.set_schedule()
            ctx.set_schedule(**schedules[i])
        want_active = int(st["mask"].sum())
        where = f"{what}: call {i} ({st['samples']} samples, threshold {st['thr']!r}, cap {st['cap']}, {want_active} active)"
        if not (i == 0 and reset_first):
            assert ctx.refine_pending(st["samples"], st["thr"], st["cap"]) == want_active, f"{where}: pending"
        total = ctx.refined_samples if not (i == 0 and reset_first) else 0
        ctx.stats_reset()
        got = ctx.refine_adaptive(st["samples"], st["thr"], st["cap"], reset=(i == 0 and reset_first))
        stats = ctx.stats()
        assert got == want_active, f"{where}: active count {got}"
        assert stats.launches == (1 if want_active else 0), f"{where}: launches"
        assert stats.samples == want_active * st["samples"], f"{where}: stats.samples"
        assert ctx.refine_last_keys == ("carried" if want_active else "unscheduled"), where
        assert ctx.refined_samples == total + (st["samples"] if want_active else 0), where
        assert_bits_equal(ctx.download()[..., :3], st["image"][..., :3], f"{where}: framebuffer")
        assert (ctx.refine_counts() == st["counts"]).all(), f"{where}: counts"
        assert_bits_equal(ctx.refine_error(), st["err"], f"{where}: errors")
        assert_bits_equal(ctx.refine_export()[..., :3], st["sums"], f"{where}: chain sums")
        m = st["mask"]
        step_cost = np.zeros(m.shape, np.int64)
        for n0 in np.unique(st["old"][m]) if want_active else ():
            sel = m & (st["old"] == n0)
            n1 = int(n0) + st["samples"]
            step_cost[sel] = (cost_at(ctx, key, n1) - cost_at(ctx, key, int(n0)))[sel]
        assert stats.segments == int(step_cost.sum()), f"{where}: stats.segments"
        if want_active or cost is not None:
            cost = np.where(m, step_cost, cost if cost is not None else 0)
            got_cost, covered = ctx.refine_cost()
            if want_active:
                assert covered == st["samples"], where
            bad = np.argwhere(got_cost.astype(np.int64) != cost)
            assert bad.size == 0, f"{where}: the cost map differs at {len(bad)} pixels; first {bad[:5].tolist()}"
        if want_active == 0 and prev_image is not None:
            assert_bits_equal(ctx.download(), prev_image, f"{where}: nothing traced, nothing changed")
        prev_image = ctx.download()
        assert want_active <= px
    return cost


def c1_inputs(rtx):
    world = rtx.random_world(11, depth=50, spp=60)
    assert world.count == 486
    W, H = 162, 91  # neither a multiple of 16 or 64
    return world, rtx.camera_look_at(W, H, aspect=W / H)


FIVE_OF_8 = [(8, INF, 0), (8, INF, 0), (8, "q", 0), (8, "q", 0), (8, "q", 0)]


@pytest.mark.parametrize("sched", range(len(TIER_SCHEDULES)), ids=["default", "k_trace-promote1", "groups", "cap6",
                                                                    "private-runs"])
@pytest.mark.parametrize("ctx_name", ["gpu_ctx", "stress_ctx"])
def test_five_steps_every_tier(request, oracle, rtx, ctx_name, sched):
    """486 spheres at 162 x 91, depth 50, five steps of 8: two over the whole
    frame (E is +inf until a pixel has a second step), three selective, under
    the default schedule and every tier's, on the product and the stress build."""
    ctx = request.getfixturevalue(ctx_name)
    world, frame = c1_inputs(rtx)
    steps = plan(oracle, rtx, "a162", world, frame, FIVE_OF_8)
    assert steps[0]["mask"].all() and steps[1]["mask"].all()
    check_shares(steps, (2, 3, 4))
    ctx.upload_world(world)
    ctx.set_frame(frame)
    try:
        run_plan(ctx, "a162", steps, f"{ctx_name} {TIER_SCHEDULES[sched]}", [TIER_SCHEDULES[sched]] * 5)
    finally:
        ctx.set_schedule()


def test_mixed_steps(gpu_ctx, oracle, rtx):
    """Steps (3, 9, 12, 5, 8): mixed per-pixel counts, a step below kLptMinSpp
    (still a scheduled launch) and pixels that are re-activated."""
    world, frame = c1_inputs(rtx)
    calls = [(3, 0.0, 0), (9, 0.0, 0), (12, "q", 0), (5, "q", 0), (8, "q", 0)]
    steps = plan(oracle, rtx, "a162", world, frame, calls)
    check_shares(steps, (2, 3, 4))
    assert len(np.unique(steps[-1]["counts"])) >= 3
    back = steps[4]["mask"] & ~steps[3]["mask"] & steps[2]["mask"]
    assert back.any(), "inputs: no pixel is re-activated"
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    run_plan(gpu_ctx, "a162", steps, "mixed steps")


@pytest.mark.parametrize("ctx_name", ["gpu_ctx", "stress_ctx"])
def test_large_scene(request, oracle, rtx, ctx_name):
    """Above 1,024 spheres (the kPF instances) at 96 x 54, steps (8, 8, 8)."""
    ctx = request.getfixturevalue(ctx_name)
    world = rtx.random_world(20, depth=50, spp=60)
    assert world.count > 1024
    W, H = 96, 54
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    steps = plan(oracle, rtx, "abig96", world, frame, [(8, INF, 0), (8, INF, 0), (8, "q", 0)])
    check_shares(steps, (2,))
    ctx.upload_world(world)
    ctx.set_frame(frame)
    run_plan(ctx, "abig96", steps, f"{ctx_name} large scene")


def test_edges(gpu_ctx, oracle, rtx):
    """A +inf threshold (nothing active, no launch, nothing changes), the
    largest finite E as the threshold (at most 9 pixels: a queue shorter than
    a wave), and a max_samples that retires pixels still above the threshold."""
    world, frame = c1_inputs(rtx)
    calls = [(8, INF, 0), (8, INF, 0), (8, INF, 0), (8, "max", 0), (8, "q", 24), (8, "q", 24), (8, "q", 32)]
    steps = plan(oracle, rtx, "a162", world, frame, calls)
    assert steps[2]["mask"].sum() == 0
    assert 1 <= steps[3]["mask"].sum() <= 9
    # (call 5 is the cap's edge: its few pixels are those a neighbour's noise newly reaches)
    check_shares(steps, (4, 6))
    with np.errstate(invalid="ignore"):
        noisy = dilate(steps[4]["err"] >= np.float32(steps[5]["thr"]))
    retired = noisy & ~steps[5]["mask"]
    assert retired.any() and (steps[4]["counts"][retired] == 24).all(), "inputs: the cap retires nobody"
    assert steps[5]["mask"].any() and steps[6]["mask"].any()
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    run_plan(gpu_ctx, "a162", steps, "edges")


def test_frame_options(gpu_ctx, oracle, rtx):
    """The thin lens, frame_index and the Lambert guard together."""
    world = rtx.random_world(11, depth=20, spp=60)
    W, H = 64, 36
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    frame.frame_index = 3
    rtx.set_aperture(frame, 0.1)
    frame.flags = rtx.FRAME_LAMBERT_GUARD
    steps = plan(oracle, rtx, "aopt", world, frame, [(8, INF, 0), (8, INF, 0), (8, "q", 0), (8, "q", 0)])
    check_shares(steps, (2, 3))
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    run_plan(gpu_ctx, "aopt", steps, "lens + frame_index + guard")


def test_transitions(gpu_ctx, oracle, rtx):
    """rtx_refine 8 + 8 then adaptive; rtx_refine on a non-uniform state is
    refused; reset works; export, import, then adaptive."""
    lib, h = gpu_ctx._lib, gpu_ctx._h
    world = rtx.random_world(11, depth=20, spp=60)
    W, H = 64, 36
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    ref = plan(oracle, rtx, "atr", world, frame, [(8, INF, 0), (8, INF, 0), (8, "q", 0)])
    check_shares(ref, (2,))
    # refine 8 + 8: a uniform state of 16 samples, no estimate yet (E = +inf): the call traces everything
    gpu_ctx.refine(8, reset=True)
    gpu_ctx.refine(8)
    assert (gpu_ctx.refine_counts() == 16).all() and np.isposinf(gpu_ctx.refine_error()).all()
    cost16 = cost_at(gpu_ctx, "atr", 16) - cost_at(gpu_ctx, "atr", 8)
    after = plan(oracle, rtx, "atr", world, frame, [(8, INF, 0), (8, "q", 0), (8, "q", 0)], start=16)
    assert after[0]["mask"].all()
    thr = after[1]["thr"]
    check_shares(after, (1, 2))
    run_plan(gpu_ctx, "atr", after, "after refine 8 + 8", reset_first=False, cost=cost16)
    # a non-uniform state: rtx_refine is refused and names the way on, nothing changes
    gpu_ctx.stats_reset()
    assert lib.rtx_refine(h, 8, 0) == RTX_ERR_STATE
    assert b"rtx_refine_adaptive" in lib.rtx_last_error()
    assert gpu_ctx.stats().launches == 0 and gpu_ctx.refined_samples == 40
    assert (gpu_ctx.refine_counts() == after[2]["counts"]).all()
    assert_bits_equal(gpu_ctx.download()[..., :3], after[2]["image"][..., :3], "after the refused rtx_refine")
    # export still copies the state; import yields a uniform one
    state = gpu_ctx.refine_export()
    assert_bits_equal(state[..., :3], after[2]["sums"], "export of a non-uniform state")
    # rtx_refine with reset starts over
    assert gpu_ctx.refine(8, reset=True) == 8
    assert_bits_equal(gpu_ctx.download(), oracle_at(oracle, rtx, "atr", world, frame, 8)[0], "refine with reset")
    # adaptive with reset starts over too
    run_plan(gpu_ctx, "atr", ref, "reset")
    # export, import, then adaptive: a uniform state of 16
    gpu_ctx.refine(8, reset=True)
    gpu_ctx.refine(8)
    state = gpu_ctx.refine_export()
    with rtx.Context(0) as b:
        b.upload_world(world)
        b.set_frame(frame)
        b.refine_import(state, 16)
        assert b.refine_pending(8, thr) == W * H and b.refine_pending(8, thr, 23) == 0
        assert (b.refine_counts() == 16).all() and np.isposinf(b.refine_error()).all()
        run_plan(b, "atr", after, "after import", reset_first=False, cost=None)
        b.refine_import(state, 16)  # uniform again: rtx_refine continues
        assert b.refine(8) == 24
        assert_bits_equal(b.download(), oracle_at(oracle, rtx, "atr", world, frame, 24)[0], "import, refine")


def test_refusals(gpu_ctx, rtx):
    """Refused before any launch; the state stays."""
    lib, h = gpu_ctx._lib, gpu_ctx._h
    W, H = 64, 36
    world = rtx.random_world(11, depth=20, spp=4)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    assert gpu_ctx.refine_adaptive(8, 0.0, reset=True) == W * H
    n = C.c_uint32(77)
    gpu_ctx.stats_reset()
    for samples, thr, cap in ((0, 0.1, 0), (8, float("nan"), 0), (8, 0.1, 7), (0xFFFFFFF8, 0.1, 0)):
        assert lib.rtx_refine_adaptive(h, samples, thr, cap, 0, C.byref(n)) == RTX_ERR_INVALID, (samples, thr, cap)
        assert b"rtx_refine_adaptive" in lib.rtx_last_error()
        assert lib.rtx_refine_pending(h, samples, thr, cap, C.byref(n)) == RTX_ERR_INVALID
        assert b"rtx_refine_pending" in lib.rtx_last_error()
    assert lib.rtx_refine_adaptive(h, 1 << 28, 0.1, 0, 1, C.byref(n)) == RTX_ERR_INVALID  # samples * depth >= 2^32
    assert lib.rtx_refine_pending(h, 8, 0.1, 0, None) == RTX_ERR_INVALID
    buf = np.zeros((H, W), np.uint32)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.rtx_refine_counts(h, p, buf.nbytes - 4) == RTX_ERR_INVALID
    assert lib.rtx_refine_counts(h, None, buf.nbytes) == RTX_ERR_INVALID
    assert lib.rtx_refine_error(h, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.nbytes + 4) == RTX_ERR_INVALID
    assert n.value == 77 and not buf.any() and gpu_ctx.stats().launches == 0
    with rtx.Context(0) as fresh:
        assert lib.rtx_refine_adaptive(fresh._h, 8, 0.1, 0, 0, C.byref(n)) == RTX_ERR_STATE  # no world
        assert lib.rtx_refine_counts(fresh._h, p, buf.nbytes) == RTX_ERR_STATE
        assert lib.rtx_refine_error(fresh._h, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.nbytes) == RTX_ERR_STATE
        fresh.upload_world(world)
        assert lib.rtx_refine_pending(fresh._h, 8, 0.1, 0, C.byref(n)) == RTX_ERR_STATE  # no frame
        flat = rtx.World(world.spheres, world.mat_types, world.mat_values, 0, 4)
        fresh.upload_world(flat)
        fresh.set_frame(frame)
        assert lib.rtx_refine_adaptive(fresh._h, 8, 0.1, 0, 0, C.byref(n)) == RTX_ERR_INVALID  # depth 0
        fresh.upload_world(world)
        ps = rtx.camera_look_at(W, H, aspect=W / H)
        ps.rng_mode = rtx.RNG_PER_SAMPLE
        fresh.set_frame(ps)
        assert lib.rtx_refine_adaptive(fresh._h, 8, 0.1, 0, 0, C.byref(n)) == RTX_ERR_INVALID
        assert b"per-sample" in lib.rtx_last_error()
    assert n.value == 77
    # the refused calls changed nothing: the state of 8 samples goes on
    assert gpu_ctx.refined_samples == 8 and (gpu_ctx.refine_counts() == 8).all()
    assert gpu_ctx.refine_adaptive(8, 0.0) == W * H
    # plain renders and accumulate overwrite the framebuffer only
    gpu_ctx.render_image()
    gpu_ctx.accumulate(reset=True)
    assert (gpu_ctx.refine_counts() == 16).all() and gpu_ctx.refine_pending(8, INF) == 0


def test_cli_refine_adaptive(tmp_path, oracle, rtx):
    """rtx_cli --refine-adaptive 8,0.15 --steps 4: each step's active count,
    the image and the --dump-counts map are the plan's; --save-state refuses
    the non-uniform state and says why."""
    import json
    import os
    import subprocess

    from test_gpu_refine import ROOT, read_pfm

    cli = os.path.join(ROOT, "raytrace-we-gpu_amd", "bin", "rtx_cli")
    world = rtx.random_world(11, depth=50, spp=60)
    frame = rtx.camera_look_at(64, 36, aspect=64 / 36)
    steps = plan(oracle, rtx, "acli", world, frame, [(8, 0.15, 0)] * 4)
    check_shares(steps, (2, 3))
    img, cnt, s = str(tmp_path / "a.pfm"), str(tmp_path / "n.pfm"), str(tmp_path / "s.bin")
    base = [cli, "--width", "64", "--height", "36", "--depth", "50", "--scene", "rtiow11", "--refine-adaptive", "8,0.15",
            "--steps", "4"]
    out = subprocess.run(base + ["--pfm", img, "--dump-counts", cnt], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rep = json.loads(out.stdout.strip().splitlines()[0])["refine_adaptive"]
    assert rep["active"] == [int(st["mask"].sum()) for st in steps] and rep["steps_run"] == 4
    for k, st in enumerate(steps):
        assert f"adaptive step {k + 1}: {int(st['mask'].sum())} active" in out.stderr
    assert_bits_equal(read_pfm(img), steps[-1]["image"][..., :3], "--refine-adaptive image")
    assert (read_pfm(cnt)[..., 0] == steps[-1]["counts"]).all()
    out = subprocess.run(base + ["--save-state", s], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "counts differ" in out.stderr and not os.path.exists(s)
    out = subprocess.run(base[:-4] + ["--refine-adaptive", "8,nan"], capture_output=True, text=True, timeout=120)
    assert out.returncode != 0
