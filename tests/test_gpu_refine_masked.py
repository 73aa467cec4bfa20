"""rtx_refine_masked: refine the pixels that show chosen objects.

The expectation is built on the CPU alone, as test_gpu_refine_adaptive.py
builds its own: the mask from the oracle's first hits (test_gpu_features.py's
expectation and its numpy restatement of the id-mask rule), the counts from the
masked rule, each pixel's image value and linear sum from the oracle's frame at
the pixel's own count, each step's error estimate from rtx.adaptive_error on
the oracle's sums. After every call the framebuffer, the counts, the errors, the
chain sums and the active count are compared bit for bit, the cost map and
stats.segments against debug_pixel_cost differences, and everything of an
untouched pixel against what it was.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_features import expected, expected_id_mask
from test_gpu_refine import ROOT, TIER_SCHEDULES, assert_bits_equal, oracle_at, read_pfm
from test_gpu_refine_adaptive import cost_at, expected_mask, gather, lin_at, run_plan

pytestmark = pytest.mark.gpu

RTX_ERR_INVALID, RTX_ERR_STATE = -1, -3
W, H = 64, 36
KEY = "mr11"
IDS, GROW = (1, 2, 3), 1
# (samples, max_samples): three steps over the mask, then a cap that the masked pixels (at 32) are past
CALLS = [(8, 0), (8, 0), (8, 0), (8, 24)]

_PLAN = {}


def inputs(rtx):
    world = rtx.random_world(11, depth=20, spp=60)
    return world, rtx.camera_look_at(W, H, aspect=W / H)


def masked_plan(oracle, rtx, world, frame, start=8, calls=CALLS):
    """The id mask and the expected state after every call, from the oracle."""
    pk = (start, tuple(calls))
    if pk in _PLAN:
        return _PLAN[pk]
    mask = expected_id_mask(expected(oracle, "rw11", world, frame)[1], IDS, GROW)
    share = mask.mean()
    assert 0.05 <= share <= 0.60, f"inputs: the mask covers {share:.1%} of the frame"
    counts = np.full((H, W), start, np.uint32)
    err = np.full((H, W), np.inf, np.float32)
    steps = []
    for samples, cap in calls:
        active = mask & (np.ones_like(mask) if cap == 0 else (counts.astype(np.int64) + samples <= cap))
        old = counts.copy()
        counts = np.where(active, counts + np.uint32(samples), counts).astype(np.uint32)
        err = err.copy()
        for y, x in np.argwhere(active):
            n0, n1 = int(old[y, x]), int(counts[y, x])
            err[y, x] = rtx.adaptive_error(lin_at(oracle, rtx, KEY, world, frame, n0)[y, x], n0,
                                           lin_at(oracle, rtx, KEY, world, frame, n1)[y, x], n1)
        ns = [int(n) for n in np.unique(counts)]
        image = gather({n: oracle_at(oracle, rtx, KEY, world, frame, n)[0] for n in ns}, counts)
        sums = gather({n: lin_at(oracle, rtx, KEY, world, frame, n) for n in ns}, counts)
        steps.append(dict(samples=samples, cap=cap, mask=active, old=old, counts=counts, err=err, image=image,
                          sums=sums))
    # the capped call traces nothing, and only because of the cap
    assert steps[-1]["mask"].sum() == 0 and (steps[-2]["counts"][mask] == 32).all() and mask.sum() > 0
    _PLAN[pk] = (mask, steps)
    return _PLAN[pk]


def device_mask(ctx, want_mask):
    """The mask through rtx_features_rows and rtx_mask_from_ids, on the device."""
    f = ctx.frame
    surf = ctx.alloc((f.height, f.width, 4))
    ctx.features_rows(1, 0, 1, 0, surf.ptr)
    mask, n = ctx.mask_from_ids(surf, IDS, GROW)
    surf.free()
    assert n == int(want_mask.sum()) and (mask.numpy() == want_mask.astype(np.uint8)).all()
    return mask


def snapshot(ctx):
    return dict(image=ctx.download(), state=ctx.refine_export(), counts=ctx.refine_counts(), err=ctx.refine_error(),
                cost=ctx.refine_cost()[0])


@pytest.mark.parametrize("sched", [0, 2], ids=["default", "groups"])
def test_masked_steps(gpu_ctx, oracle, rtx, sched):
    """refine 8, three masked steps of 8 over the three big spheres' pixels
    (grown by 1), a step whose cap of 24 the masked pixels (at 32) are past,
    rtx_refine refused on the non-uniform counts, then an adaptive step from
    the maps; under the default schedule and the pixel-group tiers'."""
    ctx = gpu_ctx
    lib, h = ctx._lib, ctx._h
    world, frame = inputs(rtx)
    mask, steps = masked_plan(oracle, rtx, world, frame)
    ctx.set_scan_mode("auto")
    ctx.upload_world(world)
    ctx.set_frame(frame)
    for st in steps:
        for n in set(np.unique(st["old"]).tolist()) | set(np.unique(st["counts"]).tolist()):
            cost_at(ctx, KEY, int(n))
    try:
        ctx.set_schedule()
        ctx.set_schedule(**TIER_SCHEDULES[sched])
        assert ctx.refine(8, reset=True) == 8
        assert_bits_equal(ctx.download(), oracle_at(oracle, rtx, KEY, world, frame, 8)[0], "refine 8")
        d_mask = device_mask(ctx, mask)
        cost = np.array(cost_at(ctx, KEY, 8))
        total = 8
        for i, st in enumerate(steps):
            want_active = int(st["mask"].sum())
            where = f"call {i} ({st['samples']} samples, cap {st['cap']}, {want_active} active)"
            before = snapshot(ctx)
            ctx.stats_reset()
            got = ctx.refine_masked(st["samples"], d_mask, st["cap"])
            stats = ctx.stats()
            assert got == want_active, f"{where}: active count {got}"
            assert stats.launches == (1 if want_active else 0), f"{where}: launches"
            assert stats.samples == want_active * st["samples"], f"{where}: stats.samples"
            assert ctx.refine_last_keys == ("carried" if want_active else "unscheduled"), where
            total += st["samples"] if want_active else 0
            assert ctx.refined_samples == total, where
            now = snapshot(ctx)
            assert_bits_equal(now["image"][..., :3], st["image"][..., :3], f"{where}: framebuffer")
            assert (now["counts"] == st["counts"]).all(), f"{where}: counts"
            assert_bits_equal(now["err"], st["err"], f"{where}: errors")
            assert_bits_equal(now["state"][..., :3], st["sums"], f"{where}: chain sums")
            m = st["mask"]
            step_cost = np.zeros(m.shape, np.int64)
            for n0 in np.unique(st["old"][m]) if want_active else ():
                sel = m & (st["old"] == n0)
                step_cost[sel] = (cost_at(ctx, KEY, int(n0) + st["samples"]) - cost_at(ctx, KEY, int(n0)))[sel]
            assert stats.segments == int(step_cost.sum()), f"{where}: stats.segments"
            cost = np.where(m, step_cost, cost)
            assert (now["cost"].astype(np.int64) == cost).all(), f"{where}: cost map"
            # every untouched pixel is bitwise what it was
            for k in ("image", "state", "err"):
                assert_bits_equal(now[k][~m], before[k][~m], f"{where}: untouched {k}")
            assert (now["counts"][~m] == before["counts"][~m]).all() and (now["cost"][~m] == before["cost"][~m]).all()
        # the counts differ now: rtx_refine without reset refuses and names the way on
        ctx.stats_reset()
        assert lib.rtx_refine(h, 8, 0) == RTX_ERR_STATE
        assert b"rtx_refine_adaptive" in lib.rtx_last_error()
        assert ctx.stats().launches == 0 and ctx.refined_samples == total
        # rtx_refine_adaptive continues from the maps, by the numpy rule on the expected ones
        last = steps[-1]
        finite = last["err"][np.isfinite(last["err"])]
        thr = float(np.quantile(finite, 0.9).astype(np.float32))
        am = expected_mask(last["err"], last["counts"], 8, thr, 0)
        assert (~mask).sum() <= am.sum() < W * H, "inputs: the adaptive step is all or nothing"
        counts = np.where(am, last["counts"] + np.uint32(8), last["counts"]).astype(np.uint32)
        err = last["err"].copy()
        for y, x in np.argwhere(am):
            n0, n1 = int(last["counts"][y, x]), int(counts[y, x])
            err[y, x] = rtx.adaptive_error(lin_at(oracle, rtx, KEY, world, frame, n0)[y, x], n0,
                                           lin_at(oracle, rtx, KEY, world, frame, n1)[y, x], n1)
        ns = [int(n) for n in np.unique(counts)]
        step = dict(samples=8, thr=thr, cap=0, mask=am, old=last["counts"], counts=counts, err=err,
                    image=gather({n: oracle_at(oracle, rtx, KEY, world, frame, n)[0] for n in ns}, counts),
                    sums=gather({n: lin_at(oracle, rtx, KEY, world, frame, n) for n in ns}, counts))
        run_plan(ctx, KEY, [step], "adaptive after masked", reset_first=False, cost=cost)
        d_mask.free()
    finally:
        ctx.set_schedule()


def test_refusals(gpu_ctx, oracle, rtx):
    """Each refused before any launch; the state stays."""
    ctx = gpu_ctx
    lib, h = ctx._lib, ctx._h
    world, frame = inputs(rtx)
    ctx.set_scan_mode("auto")
    ctx.upload_world(world)
    ctx.set_frame(frame)
    ones = ctx.alloc((H, W), np.uint8)
    ones.upload(np.ones((H, W), np.uint8))
    dm = C.c_void_p(ones.ptr)
    n = C.c_uint32(77)
    ctx.stats_reset()
    # no state (upload_world dropped it)
    assert lib.rtx_refine_masked(h, 8, dm, 0, C.byref(n)) == RTX_ERR_STATE
    assert b"rtx_refine_masked" in lib.rtx_last_error()
    # a part state
    rows = rtx.part_rows(H, 4, 1, 3)
    out = ctx.alloc((rows, W, 4))
    ctx.refine_rows(4, 1, 3, 8, reset=True, d_out=out.ptr)
    ctx.stats_reset()
    assert lib.rtx_refine_masked(h, 8, dm, 0, C.byref(n)) == RTX_ERR_STATE
    assert ctx.refine_shape() == (4, 1, 3) and ctx.refined_samples == 8
    out.free()
    # a whole-frame state: the argument rules
    ctx.refine(8, reset=True)
    ctx.stats_reset()
    assert lib.rtx_refine_masked(h, 8, None, 0, C.byref(n)) == RTX_ERR_INVALID
    assert lib.rtx_refine_masked(h, 0, dm, 0, C.byref(n)) == RTX_ERR_INVALID
    assert lib.rtx_refine_masked(h, 8, dm, 7, C.byref(n)) == RTX_ERR_INVALID
    assert lib.rtx_refine_masked(h, 0xFFFFFFF8, dm, 0, C.byref(n)) == RTX_ERR_INVALID
    assert n.value == 77 and ctx.stats().launches == 0
    # the refused calls changed nothing: the state of 8 samples goes on, over every pixel of an all-ones mask
    assert ctx.refined_samples == 8 and ctx.refine_masked(8, ones) == W * H
    assert_bits_equal(ctx.download(), oracle_at(oracle, rtx, KEY, world, frame, 16)[0], "all-ones mask")
    assert (ctx.refine_counts() == 16).all() and ctx.refine(8) == 24  # uniform counts: rtx_refine continues
    # a per-sample-RNG frame (a frame of other bytes ends the chain state: last)
    ps = rtx.camera_look_at(W, H, aspect=W / H)
    ps.rng_mode = rtx.RNG_PER_SAMPLE
    ctx.set_frame(ps)
    ctx.stats_reset()
    assert lib.rtx_refine_masked(h, 8, dm, 0, C.byref(n)) == RTX_ERR_INVALID
    assert b"per-sample" in lib.rtx_last_error()
    assert n.value == 77 and ctx.stats().launches == 0
    ones.free()


def test_cli_refine_ids(tmp_path, oracle, rtx):
    """rtx_cli --refine 8 --refine-ids 8,1,2,3 --grow 1 --steps 2: each step's
    active count, the image and the --dump-counts map are the plan's; without
    --refine or --load-state it is refused and says so."""
    cli = os.path.join(ROOT, "raytrace-we-gpu_amd", "bin", "rtx_cli")
    world, frame = inputs(rtx)
    mask, steps = masked_plan(oracle, rtx, world, frame)
    img, cnt = str(tmp_path / "m.pfm"), str(tmp_path / "n.pfm")
    base = [cli, "--width", str(W), "--height", str(H), "--depth", "20", "--scene", "rtiow11"]
    ids = ["--refine-ids", "8," + ",".join(str(i) for i in IDS), "--grow", str(GROW), "--steps", "2"]
    out = subprocess.run(base + ["--refine", "8"] + ids + ["--pfm", img, "--dump-counts", cnt], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(line) for line in out.stdout.strip().splitlines()]
    rep = lines[0]["refine_masked"]
    assert rep["active"] == [int(st["mask"].sum()) for st in steps[:2]] and rep["steps_run"] == 2
    assert rep["mask_pixels"] == int(mask.sum()) and rep["ids"] == list(IDS) and rep["grow"] == GROW
    assert lines[-1]["refine"] == [8, 8, 8] and lines[-1]["refined_samples"] == 24
    assert_bits_equal(read_pfm(img), steps[1]["image"][..., :3], "--refine-ids image")
    assert (read_pfm(cnt)[..., 0] == steps[1]["counts"]).all()
    # after --load-state instead: a state of 8 samples saved by one run, masked steps in the next
    state, img2 = str(tmp_path / "s.bin"), str(tmp_path / "m2.pfm")
    out = subprocess.run(base + ["--refine", "8", "--save-state", state], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    out = subprocess.run(base + ["--load-state", state] + ids + ["--pfm", img2], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(line) for line in out.stdout.strip().splitlines()]
    assert lines[0]["refine_masked"]["active"] == rep["active"]
    assert lines[-1]["refine"] == [8, 8] and lines[-1]["loaded_samples"] == 8 and lines[-1]["refined_samples"] == 24
    assert_bits_equal(read_pfm(img2), steps[1]["image"][..., :3], "--load-state --refine-ids image")
    out = subprocess.run(base + ids, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--refine or --load-state" in out.stderr
