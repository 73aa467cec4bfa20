"""GPU side of the lane-mode segment's straight-line set-up (grid_stretch
computes every output and decides once, rtx_grid.h; shade takes 1 / a once for
the scattered and the restarted lanes; CPU side: test_setup_equiv.py), on the
product and the stress library.

hit_world on hand-built rays of the families the set-up decides on, and small
frames from the cameras that make its outcomes: everything bit for bit the
fp32 oracle's, with equal segment counts. The stress library also checks the
kernel-argument layout at every launch (RTX_CHECK_KERNARG): a launch that
failed it raises from the next synchronisation.
"""
import os

import numpy as np
import pytest

import hostile_cases
import regime_cases
from test_gpu_parity import stress_ctx  # noqa: F401

pytestmark = pytest.mark.gpu

CTXS = ["gpu_ctx", "stress_ctx"]
W, H, SPP = 96, 54, 8  # 5,184 pixels = 81 wave runs of 64: queue tiles, the tail and the promotion all occur
CAMERAS = {
    "default": dict(),
    # inside the layer, looking along it: long stretches, walks that give up
    "in_layer": dict(look_from=(-10.5, 0.2, 0.3), look_at=(10.0, 0.2, 0.0), vfov=50.0),
    "straight_down": dict(look_from=(0.0, 20.0, 0.0), look_at=(0.0, 0.0, 0.0), vup=(0.0, 0.0, 1.0), vfov=40.0),
    "default_lens": dict(lens=0.1),
}


def assert_bits_equal(a, b, what=""):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, what
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} values differ; first at {np.argwhere(~same)[:5].tolist()}"


@pytest.fixture(scope="module")
def world(rtx):
    w = rtx.random_world(11, depth=50, spp=SPP)
    assert w.count == 486
    return w


@pytest.fixture(scope="module")
def small_world(rtx):
    """100 spheres, no two at one height: no layer, so no layer grid."""
    c = regime_cases.world("no_layer")
    return rtx.World(c.spheres, c.mat_types, c.mat_values, 50, SPP)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def ray_families(spheres, rng, per=256):
    """{family: (per, 6) float32 rays} over a scene whose layer lies at y = 0.2
    (the 486-sphere world: x and z in -11..11, a slab of about 0..0.4)."""
    sph = np.asarray(spheres, np.float64)
    small = sph[sph[:, 3] < 1.0]
    out = {}
    # near-tangent: past a sphere at r (1 + delta) from its centre, at every slope down to grazing the layer
    c = small[rng.integers(0, len(small), per)]
    d = _unit(rng.normal(size=(per, 3)))
    graze = rng.random(per) < 0.5
    d[graze, 1] = 10.0 ** rng.uniform(-7, -1, graze.sum()) * rng.choice([-1.0, 1.0], graze.sum())
    d = _unit(d)
    e = np.cross(d, _unit(rng.normal(size=(per, 3))))
    e = _unit(e)
    delta = 10.0 ** rng.uniform(-9, -1, per) * rng.choice([-1.0, 1.0], per)
    o = c[:, :3] + (c[:, 3] * (1.0 + delta))[:, None] * e - rng.uniform(0.1, 30.0, per)[:, None] * d
    out["near_tangent"] = np.c_[o, d * 10.0 ** rng.uniform(-2, 2, (per, 1))]
    # through cell corners: aimed at lattice points of the layer's plane (cells of the grid are 1/8 .. 1 wide)
    tgt = np.c_[rng.integers(-88, 89, per) / 8.0, rng.uniform(0.0, 0.4, per), rng.integers(-88, 89, per) / 8.0]
    d = _unit(rng.normal(size=(per, 3)))
    out["cell_corners"] = np.c_[tgt - rng.uniform(0.5, 20.0, per)[:, None] * d, d]
    # along the axes: one or two components exactly +0 or -0
    o = np.c_[rng.uniform(-11, 11, per), rng.uniform(-0.2, 0.8, per), rng.uniform(-11, 11, per)]
    d = rng.normal(size=(per, 3))
    k = rng.integers(0, 6, per)
    for i in range(3):
        z = (k == i) | ((k >= 3) & (k - 3 != i))
        d[z, i] = rng.choice([0.0, -0.0], z.sum())
    out["signed_zeros"] = np.c_[o, d]
    # level inside the slab (dy = 0), and origins on its faces
    o = np.c_[rng.uniform(-12, 12, per), rng.uniform(0.0, 0.4, per), rng.uniform(-12, 12, per)]
    d = rng.normal(size=(per, 3))
    d[:, 1] = rng.choice([0.0, -0.0], per)
    out["level_in_slab"] = np.c_[o, d]
    o = np.c_[rng.uniform(-12, 12, per), rng.choice([0.0, 0.4, 0.2, -0.01, 0.41], per), rng.uniform(-12, 12, per)]
    d = rng.normal(size=(per, 3))
    d[:, 1] *= 10.0 ** rng.uniform(-6, 0, per)
    out["on_slab_faces"] = np.c_[o, d]
    # |o| just below and above 64 (the grid's origin range), aimed at the layer
    o = _unit(rng.normal(size=(per, 3))) * (64.0 * (1.0 + rng.integers(-4, 5, per) * 6e-8))[:, None]
    tgt = np.c_[rng.uniform(-11, 11, per), np.full(per, 0.2), rng.uniform(-11, 11, per)]
    out["origin_at_64"] = np.c_[o, tgt - o]
    # leaving a sphere's surface, radially or at random
    c = small[rng.integers(0, len(small), per)]
    nrm = _unit(rng.normal(size=(per, 3)))
    o = c[:, :3] + (c[:, 3] * (1.0 + rng.choice([0.0, 1e-6, -1e-6], per)))[:, None] * nrm
    d = np.where((rng.random(per) < 0.5)[:, None], nrm, _unit(rng.normal(size=(per, 3))))
    out["off_a_surface"] = np.c_[o, d]
    out = {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}
    # NaN / inf / zero / tiny / huge components: every hostile class, 8 rays each
    hz = hostile_cases.hostile_rays(spheres, np.arange(4, 12), rng, per=8)
    out["hostile"] = np.concatenate(list(hz.values()))
    return out


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("which", ["world", "small_world"])
def test_hit_world_on_set_up_ray_families(request, oracle, rtx, ctx_name, which):
    """A few thousand rays, whole waves of one family and all of them shuffled
    together, on the 486-sphere scene (layer grid) and on one without a grid:
    hit, t and index bits as the oracle's."""
    ctx = request.getfixturevalue(ctx_name)
    w = request.getfixturevalue(which)
    fam = ray_families(w.spheres, np.random.default_rng(7))
    rays = np.concatenate(list(fam.values()))
    assert 2000 <= len(rays) <= 4000
    mixed = rays[np.random.default_rng(8).permutation(len(rays))]
    ctx.upload_world(w)
    with np.errstate(all="ignore"):
        want, want_mixed = oracle.hit_world_f32(w, rays), oracle.hit_world_f32(w, mixed)
    assert_bits_equal(ctx.debug_hit_world(rays), want, f"{ctx_name} {which}: families in whole waves")
    assert_bits_equal(ctx.debug_hit_world(mixed), want_mixed, f"{ctx_name} {which}: families mixed")
    if which == "world":
        assert (want[:, 0] == 1).sum() > 500  # the rays do hit the scene


_ORACLE = {}


def frame_and_oracle(oracle, rtx, world, camera):
    """The camera's frame and the oracle's image and segment count, computed
    once per camera and shared by both libraries' tests."""
    args = dict(CAMERAS[camera])
    lens = args.pop("lens", 0.0)
    frame = rtx.camera_look_at(W, H, aspect=W / H, **args)
    if lens > 0.0:
        rtx.set_aperture(frame, lens)
    if camera not in _ORACLE:
        img, segs = oracle.render_rows(world, frame, np.arange(H), nthreads=min(8, os.cpu_count() or 1))
        img.setflags(write=False)
        _ORACLE[camera] = (img, segs)
    return frame, _ORACLE[camera]


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("camera", list(CAMERAS))
def test_frames_bit_exact_with_equal_segments(request, oracle, rtx, world, ctx_name, camera):
    """96 x 54, spp 8, depth 50, 486 spheres."""
    ctx = request.getfixturevalue(ctx_name)
    frame, (want, segs) = frame_and_oracle(oracle, rtx, world, camera)
    ctx.upload_world(world)
    ctx.set_frame(frame)
    ctx.stats_reset()
    img = ctx.render_image()  # (a launch that failed the stress library's kernarg check raises here)
    assert ctx.stats().segments == segs, f"{ctx_name} {camera}"
    assert_bits_equal(img, want, f"{ctx_name} {camera}")


def test_stress_library_reports_no_kernarg_error(stress_ctx, oracle, rtx, world):  # noqa: F811
    """The kernel-argument layout check of the stress library over a 3-way row
    part and one refine step at the frames' size: no launch reports an error
    (a report raises from the synchronisation), and both are the oracle's."""
    frame, (want, segs) = frame_and_oracle(oracle, rtx, world, "default")
    stress_ctx.upload_world(world)
    stress_ctx.set_frame(frame)
    tile, parts, part = 6, 3, 1
    ids = rtx.part_row_ids(H, tile, part, parts)
    buf = stress_ctx.alloc((len(ids), W, 4))
    try:
        stress_ctx.render_rows(tile, part, parts, buf.ptr)
        stress_ctx.sync()
        assert_bits_equal(buf.numpy(), want[ids], "part 1 of 3")
    finally:
        buf.free()
    stress_ctx.stats_reset()
    assert stress_ctx.refine(SPP, reset=True) == SPP
    stress_ctx.sync()
    assert stress_ctx.stats().segments == segs
    assert_bits_equal(stress_ctx.download(), want, "one refine step of 8 samples")
