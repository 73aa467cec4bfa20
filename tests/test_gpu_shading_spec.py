"""The GPU's shading against the independent restatement of the compute
shader (shading_spec.py), under the rule of shading_cases.py.

The expectation is the restatement's, computed here on the host and cached
per module; the CPU oracle is not consulted, so a failure here cannot be
explained away by it. Path cases go through rtx_trace_paths (order "given",
pre-filled buffers with slack: test_gpu_paths.trace), whose record has what the
rule asks of a path: the sum, the end seed and the segment count. Frames go
through the render proper.
"""
import numpy as np
import pytest

import regime_cases as rc
import shading_cases as sc
from test_gpu_paths import CONTINUE, gpu_frame, stress_ctx, trace, upload  # noqa: F401
from test_shading_spec import check_device_math

pytestmark = pytest.mark.gpu


def check_paths(ctx, rtx, name, what, mode="auto"):
    tol = sc.checked_tolerance(name)
    case, (_, s64) = sc.case(name), sc.specs(name)
    try:
        upload(ctx, rtx, case.world, depth=case.depth, mode=mode)
        res, seg = trace(ctx, case.queries, case.samples, order="given")
    finally:
        ctx.set_scan_mode("auto")
    if name in sc.BLACK:
        sc.assert_black(what, s64, res[:, :3], seeds=res[:, 3], segments=seg)
        return
    v = sc.accept(what, tol, s64, res[:, :3], seeds=res[:, 3], segments=seg)
    assert not v.ratio > 2, f"{v}: further from fp64 than twice the fp32 restatement is"


@pytest.mark.parametrize("name", sc.NAMES)
def test_paths_against_spec(gpu_ctx, rtx, name):
    check_paths(gpu_ctx, rtx, name, f"gpu, {name}")


def test_rtiow11_linear_scan(gpu_ctx, rtx):
    """The shading does not depend on the scan regime: every block of every
    segment in scene order."""
    case = sc.case("rtiow11")
    try:
        upload(gpu_ctx, rtx, case.world, depth=case.depth, mode="linear")
        info = gpu_ctx.scene_info()
        assert {k: info[k] for k in rc.expected_info("rtiow11", True)} == rc.expected_info("rtiow11", True), info
    finally:
        gpu_ctx.set_scan_mode("auto")
    check_paths(gpu_ctx, rtx, "rtiow11", "gpu, rtiow11, linear scan", mode="linear")


@pytest.mark.parametrize("name", sc.SMALL)
def test_small_worlds_on_the_stress_build(stress_ctx, rtx, name):  # noqa: F811
    check_paths(stress_ctx, rtx, name, f"stress build, {name}")


def test_continue_on_glass_ball(gpu_ctx, rtx):
    """RTX_PATHS_CONTINUE: 1 sample and 1 more give the restatement's 2."""
    name = "glass_ball"
    tol = sc.checked_tolerance(name)
    case, (_, s64) = sc.case(name), sc.specs(name)
    upload(gpu_ctx, rtx, case.world, depth=case.depth)
    first, seg1 = trace(gpu_ctx, case.queries, 1)
    scrubbed = np.array(case.queries)
    scrubbed[:, 3] = np.nan  # a continuing call reads the record's seed, not the query's
    both, seg2 = trace(gpu_ctx, scrubbed, 1, flags=CONTINUE, start=first)
    v = sc.accept("gpu, glass_ball, 1 + 1 samples", tol, s64, both[:, :3], seeds=both[:, 3],
                  segments=seg1.astype(np.int64) + seg2)
    assert not v.ratio > 2, str(v)


@pytest.mark.parametrize("name,spp", [("mix", sc.FSPP), ("test_world", sc.FSPP), ("test_world", 8)])
def test_frames_against_spec(gpu_ctx, rtx, name, spp):
    """The two 16 x 9 frames through the render at spp 4, the exact-grid
    kernel, and test_world once at spp 8, the scheduled render (pre-pass, cost
    queue, persistent loop). Gamma colours per pixel under the rule,
    stats().segments against the restatement's total. (mix at spp 8 is not
    asked: there the fp32 and fp64 restatements part on 1 of the 144 pixels,
    over half the cap, so the frame fails the set-up condition on the
    reference alone.)"""
    tol = sc.frame_tolerance(name, spp)
    tol.assert_reference_within_half_cap(f"frame {name}")
    w = sc.frame_world(name, spp)
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.set_schedule()
    gpu_ctx.upload_world(rtx.World(w.spheres, w.mat_types, w.mat_values, w.depth, w.spp))
    gpu_ctx.set_frame(gpu_frame(rtx, sc.frame_of(name)))
    gpu_ctx.stats_reset()
    img = gpu_ctx.render_image()
    assert img.shape == (sc.FH, sc.FW, 4) and (img[..., 3] == 1).all()
    v = sc.judge_frame(f"gpu, frame {name}, spp {spp}", tol, sc.frame_specs(name, spp)[1], img,
                       gpu_ctx.stats().segments)
    assert v.ok, str(v)


def test_device_math_against_spec(gpu_ctx):
    """hash1, hash3 (bits) and random_in_unit_sphere on the device."""
    check_device_math(gpu_ctx.debug_math)
