"""The small-scene resolve round (rtx_kernels.hip resolve_pre_t, kLean) and
the persistent render around it, through whole frames and
rtx_debug_hit_world: 96 x 54 at spp 8, so the pre-pass, the cost queue and the
persistent render draw them, each frame the oracle's bit for bit with the
oracle's segment count. Both builds: the product's 12-entry candidate lists,
and the stress build's lists of one entry, where scan and resolve alternate at
every flagged block (every resolve call then starts from the running key of
the one before). Worlds and cameras from regime_cases.py where they fit.

What each case is for:
  rtiow11          the benchmark's world from its camera and from layer height
                   (grazing rays: the longest candidate lists)
  r3_full          1,012 spheres seen edge-on: the most candidates per lane a
                   small scene gives, no LDS copy (cen and cperm from memory)
  r3_small         641 spheres: the smallest scene without the LDS copy
  coincident       equal roots: the later scene index wins, also for a copy of
                   the ground at index 1 and one at the last index
  no_layer         no layout and no grid: positions are scene indices
  lds_full         block 0 of the layout holds 8 off-layer spheres
"""
import os

import numpy as np
import pytest

import hostile_cases as hc
import regime_cases as rc
from test_gpu_layout import _twins, assert_bits_equal
from test_gpu_parity import stress_ctx  # noqa: F401

pytestmark = pytest.mark.gpu

W, H, SPP = 96, 54, 8
CTXS = ["gpu_ctx", "stress_ctx"]
NTHREADS = min(8, os.cpu_count() or 1)
BENCH_CAMERA = {}  # camera_look_at's defaults: the benchmark's camera


def _coincident():
    """_twins(True) with two more copies of the ground, at index 1 and at the
    last index, and a material of its own for every sphere: any winner but the
    last copy changes the pixel."""
    sph = _twins(True)
    sph = np.concatenate([sph[:1], sph[:1], sph[1:], sph[:1]])
    mt, mv = rc._materials(np.random.default_rng(61), len(sph))
    mv[-1] = (0.9, 0.1, 0.1, 0.0)
    mt[-1] = 0.0
    return rc.Case(sph, mt, mv, len(sph) - 3)


CASES = {
    "rtiow11": (lambda: rc.world("rtiow11"), (BENCH_CAMERA, rc.CAMERAS["grazing"])),
    "r3_full": (lambda: rc.world("r3_full"), (rc.CAMERAS["grazing"], rc.CAMERAS["in_slab"])),
    "r3_small": (lambda: rc.world("r3_small"), (BENCH_CAMERA, rc.CAMERAS["grazing"])),
    "coincident": (_coincident, (rc.CAMERAS["default"], rc.CAMERAS["grazing"])),
    "no_layer": (lambda: rc.world("no_layer"), (BENCH_CAMERA,)),
    "lds_full": (lambda: rc.world("lds_full"), (BENCH_CAMERA, rc.CAMERAS["grazing"])),
}
# scene_info fields each case must show (the constants as DESIGN.md §3f states them)
INFO = {
    "rtiow11": dict(kernels=0, sphere_copy_lds=1, layout=1, map_in_lds=1, grid=1),
    "r3_full": dict(kernels=0, sphere_copy_lds=0, layout=1, map_in_lds=0, grid=1, count=1012),
    "r3_small": dict(kernels=0, sphere_copy_lds=0, layout=1, map_in_lds=0, grid=1, count=641),
    "coincident": dict(kernels=0, sphere_copy_lds=1, layout=1, map_in_lds=1),
    "no_layer": dict(kernels=0, sphere_copy_lds=1, layout=0, grid=0),
    "lds_full": dict(kernels=0, sphere_copy_lds=1, layout=1, map_in_lds=1, flat_lo=2),
}
_WANT = {}


def _world(rtx, case):
    return rtx.World(case.spheres, case.mat_types, case.mat_values, case.depth, SPP)


def _frame(rtx, cam):
    return rtx.camera_look_at(W, H, aspect=W / H, **cam)


def _wanted(oracle, rtx, name):
    """The oracle's frames of case `name`, one per camera: computed once, read-only."""
    if name not in _WANT:
        make, cams = CASES[name]
        case = make()
        out = []
        for cam in cams:
            img, segs = oracle.render_rows(_world(rtx, case), _frame(rtx, cam), np.arange(H), nthreads=NTHREADS)
            assert np.isfinite(img).all()
            img.setflags(write=False)
            out.append((img, segs))
        _WANT[name] = (case, out)
    return _WANT[name]


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("name", list(CASES))
def test_frames_bit_exact(request, rtx, oracle, ctx_name, name):
    ctx = request.getfixturevalue(ctx_name)
    case, want = _wanted(oracle, rtx, name)
    ctx.set_scan_mode("auto")
    ctx.set_schedule()
    ctx.upload_world(_world(rtx, case))
    info = ctx.scene_info()
    assert {k: info[k] for k in INFO[name]} == INFO[name], info
    for cam, (img_want, segs) in zip(CASES[name][1], want):
        ctx.set_frame(_frame(rtx, cam))
        ctx.stats_reset()
        img = ctx.render_image()
        st = ctx.stats()
        assert_bits_equal(img, img_want, f"{ctx_name} {name} {cam}")
        assert st.segments == segs, (ctx_name, name, cam)


@pytest.mark.parametrize("ctx_name", CTXS)
def test_row_part_through_the_persistent_render_bit_exact(request, rtx, oracle, ctx_name):
    """A row part (nparts 3) of the benchmark's world through the persistent
    small-scene render (the launch whose priority site is not thinned): the
    oracle's rows and segment count. How often the site looks is timing and
    cannot be seen from here."""
    ctx = request.getfixturevalue(ctx_name)
    case = rc.world("rtiow11")
    world, frame = _world(rtx, case), _frame(rtx, BENCH_CAMERA)
    part = (4, 1, 3)
    ids = rtx.part_row_ids(H, *part)
    img_want, segs = oracle.render_rows(world, frame, ids, nthreads=NTHREADS)
    ctx.set_scan_mode("auto")
    ctx.set_schedule()
    ctx.upload_world(world)
    ctx.set_frame(frame)
    buf = ctx.alloc((len(ids), W, 4))
    try:
        ctx.stats_reset()
        ctx.render_rows(*part, buf.ptr)
        ctx.sync()
        st = ctx.stats()
        assert_bits_equal(buf.numpy(), img_want, f"{ctx_name} part {part}")
        assert st.segments == segs
    finally:
        buf.free()


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("key", [11, "r3_small"], ids=["lds_copy", "from_memory"])
def test_hostile_rays_take_the_fallback(request, rtx, oracle, ctx_name, key):
    """NaN, infinite and zero-length rays, directions down to 3e-39 (their
    discriminants lie far below 2^-96: sqrt_rn's slow branch) and huge ones
    (non-finite roots: the `ok` fallback), whole waves of one class each, on
    the degenerate world (zero, negative and tiny radii, concentric spheres):
    the layout's answer equals the LINEAR upload's and the oracle's."""
    ctx = request.getfixturevalue(ctx_name)
    case, _, classes = hc.degenerate_world(key)
    rays, where = hc.grouped(classes)
    world = rtx.World(case.spheres, case.mat_types, case.mat_values, 1, 1)
    want = oracle.hit_world_f32(world, rays)
    got = {}
    try:
        for mode in ("linear", "auto"):
            ctx.set_scan_mode(mode)
            ctx.upload_world(world)
            assert ctx.scene_info()["kernels"] == 0
            got[mode] = ctx.debug_hit_world(rays)
    finally:
        ctx.set_scan_mode("auto")
    for name, sl in where.items():
        assert_bits_equal(got["auto"][sl], got["linear"][sl], f"{ctx_name} {key} {name}: auto vs linear")
        assert_bits_equal(got["auto"][sl], want[sl], f"{ctx_name} {key} {name}: auto vs oracle")
    # the classes do what they are for: non-finite roots and tiny discriminants both occur
    hit = want[:, 0] == 1
    assert (hit & ~np.isfinite(want[:, 1])).sum() > 64
    assert (hit & np.isfinite(want[:, 1])).sum() > 64
