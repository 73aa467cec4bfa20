"""GPU parity on the inputs the library accepts but no well-behaved scene
makes (hostile_cases.py): rays with NaN, infinite, zero, tiny and huge
components, spheres of zero or negative radius, concentric and exactly
representable ones, materials with NaN, infinite or negative parameters,
frames with a NaN origin or every direction zero.

The bar is the suite's: every record and every pixel bit-identical to the
oracle, NaN equal to NaN. What a non-finite ray hits depends on scene order
(a NaN root is accepted, and after it every later sphere whose discriminant
is not negative), so the answer has to survive the spatial layouts, the
culled order, wrapped scan starts and the split of one ray over 2..64 lanes.
That the inputs do have such roots, and that NaN rays are traced mid-path, is
asserted on the CPU in test_hostile_inputs.py.
"""
import os

import numpy as np
import pytest

import hostile_cases as hc
import regime_cases as rc
from conftest import GOLDEN
from test_gpu_features import expected
from test_gpu_parity import assert_bits_equal, render_gpu

pytestmark = pytest.mark.gpu

STRESS_LIB = os.path.join(os.path.dirname(GOLDEN), "..", "raytrace-we-gpu_amd", "lib", "variants",
                          "librtx_stress.so")
W, H = 64, 36
NT = min(8, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def stress_ctx(rtx):
    """The stress build (make all): candidate lists of 1 entry and 2
    sphere-major pairs, so resolve rounds, list overflows and the exact
    sequential fallbacks run all the time."""
    if not os.path.exists(STRESS_LIB):
        pytest.fail("stress build missing: make all")
    ctx = rtx.Context(0, lib=rtx.load_library(STRESS_LIB))
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------
# hit_world
# ---------------------------------------------------------------------------
_RAYS, _WANT = {}, {}


def ray_sets(key):
    """[(name, rays, t_min)] of a degenerate world: every class grouped in
    whole waves and shuffled 1:1 among grazing rays, at t_min 0.001, and the
    tiny-|d| classes at t_min 1e-30. Built once."""
    if key not in _RAYS:
        case, _, classes = hc.degenerate_world(key)
        seed = 500 + (key if isinstance(key, int) else sum(map(ord, key)))
        grouped, _ = hc.grouped(classes)
        mixed, hostile = hc.mixed(classes, case.spheres, np.random.default_rng(seed))
        assert len(grouped) == 36 * 64 and len(mixed) == 2 * len(grouped) and hostile.sum() == len(grouped)
        tiny, _ = hc.grouped({k: classes[k] for k in hc.TINY_CLASSES})
        _RAYS[key] = [("grouped", grouped, 0.001), ("mixed", mixed, 0.001), ("tiny |d|", tiny, 1e-30)]
    return _RAYS[key]


def want_of(oracle, wkey, world, name, rays, t_min):
    k = (wkey, name, t_min)
    if k not in _WANT:
        _WANT[k] = oracle.hit_world_f32(world, rays, t_min)
        _WANT[k].setflags(write=False)
    return _WANT[k]


def check_hit_world(ctx, oracle, rtx, wkey, case, sets, starts, what):
    ctx.upload_world(rtx.World(case.spheres, case.mat_types, case.mat_values, 1, 1))
    for name, rays, t_min in sets:
        want = want_of(oracle, wkey, case, name, rays, t_min)
        for start in starts:
            got = ctx.debug_hit_world(rays, t_min=t_min, start_block=start)
            assert_bits_equal(got, want, f"{what}: {name} rays, t_min {t_min:g}, start {start}")


def test_hit_world_plain_scan_66_spheres(gpu_ctx, oracle, rtx):
    """Degenerate random_world(4): 66 spheres, n % 8 = 2, so the last block is
    padded with copies of sphere n - 1, the sphere every NaN ray hits."""
    case, _, _ = hc.degenerate_world(4)
    nblk = (case.count + 7) // 8
    check_hit_world(gpu_ctx, oracle, rtx, 4, case, ray_sets(4), (None, 0, nblk // 2, nblk - 1), "66 spheres")


@pytest.mark.parametrize("mode", ["auto", "linear"])
@pytest.mark.parametrize("ctx_name", ["gpu_ctx", "stress_ctx"])
def test_hit_world_layout_and_grid_486_spheres(request, oracle, rtx, ctx_name, mode):
    """Degenerate random_world(11): the spatial layout and the layer grid
    (auto), scene-order blocks (RTX_SCAN_LINEAR)."""
    ctx = request.getfixturevalue(ctx_name)
    case, _, _ = hc.degenerate_world(11)
    nblk = (case.count + 7) // 8
    try:
        ctx.set_scan_mode(mode)
        check_hit_world(ctx, oracle, rtx, 11, case, ray_sets(11), (None, 0, nblk // 2, nblk + 3),
                        f"486 spheres, {ctx_name}, {mode}")
        info = ctx.scene_info()
        assert info["kernels"] == 0 and info["layout"] == info["grid"] == int(mode == "auto"), info
    finally:
        ctx.set_scan_mode("auto")


def test_hit_world_reordered_layout_r3_full(gpu_ctx, oracle, rtx):
    """regime_cases' r3_full (1,012 spheres, the layer interleaved with 500
    off-layer spheres: the position map in memory), degenerated."""
    case, _, _ = hc.degenerate_world("r3_full")
    check_hit_world(gpu_ctx, oracle, rtx, "r3_full", case, ray_sets("r3_full"), (None,), "r3_full")
    info = gpu_ctx.scene_info()
    assert info["layout"] == 1 and info["map_in_lds"] == 0 and info["grid"] == 1, info


def culled_forms(rtx, nblk):
    forms = [None, rtx.DEBUG_CULLED, 0, nblk // 2]
    for q in (1, 8, 32, 64):
        forms += [rtx.DEBUG_CULLED_COOP(q), rtx.DEBUG_CULLED_COOP_LANE(q)]
    return forms


@pytest.mark.parametrize("variant", ["degenerate", "radius_1e15", "centre_x_1e15"])
@pytest.mark.parametrize("ctx_name", ["gpu_ctx", "stress_ctx"])
def test_hit_world_culled_2500_spheres(request, oracle, rtx, ctx_name, variant):
    """Degenerate random_world(25) and its two 1e15 variants: the culled scan
    in lane mode, split over 64..1 lanes per ray in both walks, and the
    wrapped scan from blocks 0 and nblk / 2."""
    ctx = request.getfixturevalue(ctx_name)
    case, _, _ = hc.degenerate_world(25)
    if variant != "degenerate":
        case = hc.Case(hc.large_variants(case.spheres)[variant])
    nblk = (case.count + 7) // 8
    check_hit_world(ctx, oracle, rtx, (25, variant), case, ray_sets(25), culled_forms(rtx, nblk),
                    f"2,500 spheres, {variant}, {ctx_name}")
    assert ctx.scene_info()["kernels"] == 1


def test_hit_world_culled_ties_go_to_the_later_duplicate(gpu_ctx, oracle, rtx):
    """The degenerate 2,500-sphere world with 16 of its spheres repeated at
    the end: whatever root a sphere is accepted with, finite, infinite or NaN,
    its later copy is accepted with too, so no winner is an earlier copy."""
    base, _, _ = hc.degenerate_world(25)
    dup_src = 1 + np.random.default_rng(77).choice(base.count - 1, 16, replace=False)
    case = hc.Case(np.concatenate([base.spheres, base.spheres[dup_src]]))
    sets = ray_sets(25)
    check_hit_world(gpu_ctx, oracle, rtx, (25, "dup"), case, sets,
                    (rtx.DEBUG_CULLED, rtx.DEBUG_CULLED_COOP(8), rtx.DEBUG_CULLED_COOP_LANE(1)), "duplicates")
    for name, rays, t_min in sets:
        want = want_of(oracle, (25, "dup"), case, name, rays, t_min)
        hit = want[:, 0] == 1
        assert hit.mean() > 0.5
        assert not np.isin(want[hit, 9], dup_src).any(), "a tie must go to the later duplicate"


@pytest.mark.parametrize("ctx_name", ["gpu_ctx", "stress_ctx"])
def test_nan_discriminant_among_negative_ones(request, oracle, rtx, ctx_name):
    """hostile_cases.divergence_case: in sphere 10's batch of 8 its
    discriminant is NaN (inf * 0) and the other seven are -inf. The reference
    takes sphere 10 with t = NaN; an all-miss early out by a max over the batch
    would drop it (fmax drops a NaN operand). 64 identical rays: a wave-wide
    ballot finds no neighbour to be saved by."""
    ctx = request.getfixturevalue(ctx_name)
    sph, rays, k = hc.divergence_case()
    case = hc.Case(sph)
    want = oracle.hit_world_f32(case, rays)
    assert (want[:, 0] == 1).all() and np.isnan(want[:, 1]).all() and (want[:, 9] == k).all()
    ctx.upload_world(rtx.World(case.spheres, case.mat_types, case.mat_values, 1, 1))
    for start in (None, 0, 1, 2):
        got = ctx.debug_hit_world(rays, start_block=start)
        assert (got[:, 0] == 1).all() and np.isnan(got[:, 1]).all() and (got[:, 9] == k).all(), (start, got[0])
        assert_bits_equal(got, want, f"NaN among -inf, start {start}")


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------
_FRAMES = {}


def oracle_frame(oracle, key, world, frame):
    if key not in _FRAMES:
        img, segs = oracle.render_rows(world, frame, np.arange(frame.height), nthreads=NT)
        img.setflags(write=False)
        _FRAMES[key] = (img, segs)
    return _FRAMES[key]


def look_at(rtx, rng_mode=0):
    f = rtx.camera_look_at(W, H, aspect=W / H)
    f.rng_mode = rng_mode
    return f


MATERIAL_WORLDS = [(4, "lambert"), (4, "unknown"), (11, "lambert"), (11, "metal"), (11, "glass"), (11, "unknown"),
                   (25, "lambert"), (25, "unknown")]


@pytest.mark.parametrize("ext,last", MATERIAL_WORLDS)
def test_hostile_material_frames(gpu_ctx, oracle, rtx, ext, last):
    """The hostile-material worlds at spp 4 (the exact grid) and spp 9 (the
    cost pre-pass and the ordered persistent render), in both RNG modes, and
    for the 486-sphere world under both scan modes: image and segment count."""
    base = hc.hostile_materials(ext, last, hc.MATERIAL_SEED[ext])
    try:
        for mode in (("auto", "linear") if ext == 11 else ("auto",)):
            gpu_ctx.set_scan_mode(mode)
            for spp in (4, 9):
                for rng_mode in (0, 1):
                    case, frame = base.at_spp(spp), look_at(rtx, rng_mode)
                    world = rtx.World(case.spheres, case.mat_types, case.mat_values, case.depth, spp)
                    want, segs = oracle_frame(oracle, (ext, last, spp, rng_mode), case, frame)
                    img, st = render_gpu(gpu_ctx, world, frame)
                    what = f"random_world({ext}), last = {last}, spp {spp}, rng_mode {rng_mode}, {mode}"
                    assert_bits_equal(img, want, what)
                    assert st.segments == segs, what
    finally:
        gpu_ctx.set_scan_mode("auto")


@pytest.mark.parametrize("ext", [11, 25])
def test_hostile_material_share_on_the_stress_build(stress_ctx, oracle, rtx, ext):
    """An 8-way share (part 3, 5-row tiles) at spp 12 on the stress build: so
    small a share takes the heavy-pixel coop tiers, which then carry NaN rays,
    with every list overflow and fallback forced."""
    case = hc.hostile_materials(ext, "lambert", hc.MATERIAL_SEED[ext], spp=12)
    frame = look_at(rtx)
    stress_ctx.upload_world(rtx.World(case.spheres, case.mat_types, case.mat_values, case.depth, case.spp))
    stress_ctx.set_frame(frame)
    rows = rtx.part_row_ids(H, 5, 3, 8)
    buf = stress_ctx.alloc((H, W, 4))
    stress_ctx.stats_reset()
    stress_ctx.render_rows(5, 3, 8, buf.ptr)
    stress_ctx.sync()
    st = stress_ctx.stats()
    got = buf.numpy().reshape(-1)[: len(rows) * W * 4].reshape(len(rows), W, 4)
    buf.free()
    want, segs = oracle.render_rows(case, frame, rows, nthreads=NT)
    assert_bits_equal(got, want, f"random_world({ext}) part 3 of 8, stress build")
    assert st.segments == segs


@pytest.mark.parametrize("kind", hc.HOSTILE_FRAMES)
def test_hostile_frames(gpu_ctx, oracle, rtx, kind):
    """A NaN origin, |d| about 3e19 and every direction zero over the
    hostile-material 486-sphere world at spp 4."""
    case = hc.hostile_materials(11, "lambert", hc.MATERIAL_SEED[11])
    frame = hc.hostile_frame(look_at(rtx), kind)
    want, segs = oracle_frame(oracle, (11, "lambert", kind), case, frame)
    img, st = render_gpu(gpu_ctx, rtx.World(case.spheres, case.mat_types, case.mat_values, case.depth, case.spp), frame)
    assert_bits_equal(img, want, f"frame {kind}")
    assert st.segments == segs


def test_refine_chain_carries_nan_sums(gpu_ctx, oracle, rtx):
    """refine(5) then refine(4) is the plain spp-9 image: the chain state
    between the two steps holds the NaN sums of the pixels that have them."""
    case = hc.hostile_materials(11, "lambert", hc.MATERIAL_SEED[11], spp=9)
    frame = look_at(rtx)
    want, segs = oracle_frame(oracle, (11, "lambert", 9, 0), case, frame)
    assert np.isnan(want).any(), "inputs: no NaN pixel"
    gpu_ctx.upload_world(rtx.World(case.spheres, case.mat_types, case.mat_values, case.depth, case.spp))
    gpu_ctx.set_frame(frame)
    gpu_ctx.stats_reset()
    assert gpu_ctx.refine(5, reset=True) == 5
    assert gpu_ctx.refine(4) == 9
    assert_bits_equal(gpu_ctx.download(), want, "refine(5) + refine(4)")
    assert gpu_ctx.stats().segments == segs


@pytest.mark.parametrize("kind", ["look_at", "nan_origin"])
def test_features_and_pick_on_the_degenerate_world(gpu_ctx, oracle, rtx, kind):
    """rtx_features and rtx_pick on the degenerate 486-sphere world (with
    random_world(11)'s materials) against the oracle's first hit on the
    pixel-centre rays, as test_gpu_features.py computes it; under the NaN-origin
    frame every pixel shows sphere n - 1 with a NaN depth."""
    geo, _, _ = hc.degenerate_world(11)
    _, mt, mv = oracle.random_world(11)
    case = hc.Case(geo.spheres, mt, mv)
    world = rtx.World(case.spheres, case.mat_types, case.mat_values, 12, 1)
    frame = look_at(rtx) if kind == "look_at" else hc.hostile_frame(look_at(rtx), kind)
    geom, surf, rec = expected(oracle, ("hostile", kind), world, frame)
    if kind == "nan_origin":
        assert (surf[..., 3] == case.count - 1).all() and np.isnan(geom[..., 3]).all()
    else:
        radius = case.spheres[surf[..., 3][surf[..., 3] >= 0].astype(int), 3]
        assert len(np.unique(surf[..., 3])) >= 30 and (radius <= 0).any(), "inputs: no degenerate sphere in view"
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    got_geom, got_surf = gpu_ctx.features()
    assert_bits_equal(got_geom, geom, f"{kind}: geom plane")
    assert_bits_equal(got_surf, surf, f"{kind}: surf plane")
    rng = np.random.default_rng(9)
    for x, y in [(int(rng.integers(W)), int(rng.integers(H))) for _ in range(10)] + [(0, 0), (W - 1, H - 1)]:
        got = gpu_ctx.pick(x, y)
        r, i = rec[y, x], int(surf[y, x, 3])
        assert got["index"] == i and got["hit"] == (i >= 0), (x, y)
        assert_bits_equal(got["depth"], geom[y, x, 3], f"pick {x},{y}: depth")
        if i < 0:
            continue
        assert_bits_equal(got["normal"], geom[y, x, :3], f"pick {x},{y}: normal")
        assert_bits_equal(got["albedo"], surf[y, x, :3], f"pick {x},{y}: albedo")
        assert_bits_equal(got["p"], r[2:5], f"pick {x},{y}: p")
        assert_bits_equal(got["t"], r[1], f"pick {x},{y}: t")
        assert got["front_face"] == bool(r[8]) and got["material"] == int(mt[i])
        assert_bits_equal(got["mat_param"], mv[i, 3], f"pick {x},{y}: mat_param")
