"""rtx_trace_film on the GPU: path queries whose every sample is jittered over
a film footprint of the query's own, one result record per query on device
buffers.

The expectation is the CPU oracle's render of the frame a record states
(film_cases.expect, cached per module): query (o, L, H, V, fx = x, fy = y,
rtx_path_seed(x, y, f)) is pixel (x, y) of oracle.render_rows_linear in that
frame. 8 x 4 pixels per ray, img_w, img_h = 8, 4, 6 samples, depth 8 unless a
test says otherwise. Every float is compared with assert_bits_equal (equal
bits, NaN equal to NaN); segment counts exactly, per frame. Result and segment
buffers hold a byte pattern before each call and are 16 records longer than the
batch, so a record that was not written, or one written past the end, shows.
`order` is a schedule: "given" and "cost" must give the same records.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import film_cases as fc
import hostile_cases as hc
import paths_cases as pc
import regime_cases as rc
from conftest import GOLDEN, ROOT
from test_film_host import RECIPES, case_of as _case_of
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu

f32 = np.float32
STRESS_LIB = os.path.join(os.path.dirname(GOLDEN), "..", "raytrace-we-gpu_amd", "lib", "variants",
                          "librtx_stress.so")
CLI = os.path.join(ROOT, "raytrace-we-gpu_amd", "bin", "rtx_cli")
ORDERS = ("given", "cost")
FILL = 0xA5   # the byte every output buffer holds before a call
SLACK = 16    # records an output buffer has beyond the batch
RTX_ERR_INVALID, RTX_ERR_STATE = -1, -3
GUARD, CONTINUE, LENS = 1, 2, 4
PER = fc.W * fc.H
IMG = (float(fc.W), float(fc.H))


@pytest.fixture(scope="module")
def stress_ctx(rtx):
    """The stress build (make all): candidate lists of 1 entry, so resolve
    rounds, list overflows and the exact sequential fallbacks run all the time."""
    if not os.path.exists(STRESS_LIB):
        pytest.fail("stress build missing: make all")
    ctx = rtx.Context(0, lib=rtx.load_library(STRESS_LIB))
    yield ctx
    ctx.close()


# ---------------------------------------------------------------------------
# cases, expectations, the call
# ---------------------------------------------------------------------------
_CASES, _EXPECT = {}, {}


def case_of(oracle, name):
    if name not in _CASES:
        _CASES[name] = _case_of(oracle, name)
    return _CASES[name]


def expectation(oracle, name, rays=None, lens=None, **kw):
    """film_cases.expect of world `name` with its recipe (its first `rays`
    rays), built once per (name, rays, options). lens: None; "all": lens_r =
    0.05 in every frame; "third": 0.05, and 0 in every third frame; "zero": 96-
    byte records whose radii are all 0."""
    key = (name, rays, lens, tuple(sorted(kw.items())))
    if key not in _EXPECT:
        n, seed, scale = RECIPES[name]
        o, L, hor, ver, lu, lv = (a[:rays] for a in fc.recipe(n, seed, scale))
        ln = None
        if lens is not None:
            r = np.full(len(o), fc.LENS_R if lens != "zero" else f32(0))
            if lens == "third":
                r[::3] = 0
            ln = (lu, lv, r)
        _EXPECT[key] = fc.expect(case_of(oracle, name), o, L, hor, ver, lens=ln, **kw)
    return _EXPECT[key]


def upload(ctx, rtx, case, depth=fc.DEPTH, mode="auto", spp=1):
    ctx.set_scan_mode(mode)
    ctx.upload_world(rtx.World(case.spheres, case.mat_types, case.mat_values, depth, spp))


def filled(ctx, n, dtype):
    d = ctx.alloc((n,), dtype)
    d.upload(np.frombuffer(bytes([FILL]) * d.nbytes, dtype))
    return d


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == FILL).all()


def trace(ctx, recs, samples=fc.SAMPLES, n=None, order="given", flags=0, start=None, segments=True, img=IMG):
    """rtx_trace_film on device buffers: the first n rows of `recs` ((m, 16)
    float32, or (m, 24): RTX_FILM_LENS) into pre-filled buffers of n + SLACK
    records (start: the (n, 4) records a continuing call begins from). Returns
    ((n, 4) float32 results, (n,) uint32 segments or None) after checking that
    nothing beyond record n - 1 was written and every record before it was."""
    recs = np.ascontiguousarray(recs, f32)
    width = recs.shape[1]
    assert width in (16, 24)
    n = len(recs) if n is None else n
    d_q = ctx.alloc((max(len(recs), 1), width))
    d_r = filled(ctx, n + SLACK, np.dtype([("v", "<f4", (4,))]))
    d_s = filled(ctx, n + SLACK, np.uint32) if segments else None
    try:
        if len(recs):
            d_q.upload(recs)
        if start is not None:
            keep = d_r.numpy()
            keep["v"][:n] = start
            d_r.upload(keep)
        got = ctx.trace_film(d_q, samples, img[0], img[1], flags=flags, order=order, results=d_r,
                             segments=d_s if segments else False, n=n, lens=width == 24)
        assert got[0] is d_r and got[1] is d_s
        ctx.sync()
        res = d_r.numpy()["v"]
        seg = d_s.numpy() if segments else None
        what = f"n = {n}, {order}"
        assert untouched(res[n:]) and (seg is None or untouched(seg[n:])), f"{what}: a record past the batch was written"
        if start is None:  # (a continuing call's buffer held records already)
            assert not (res[:n].view(np.uint8).reshape(n, 16) == FILL).all(1).any(), f"{what}: a result was not written"
        assert seg is None or not (seg[:n] == np.uint32(0xA5A5A5A5)).any(), f"{what}: a segment count was not written"
        return np.array(res[:n]), (None if seg is None else np.array(seg[:n]))
    finally:
        for d in (d_q, d_r, d_s):
            if d is not None:
                d.free()


def check(ctx, e, what, order="given", flags=0, samples=fc.SAMPLES, img=IMG, ran=None):
    res, seg = trace(ctx, e.recs, samples, order=order, flags=flags, img=img)
    assert_bits_equal(res[:, :3], e.sums, f"{what}, {order}: sums")
    assert (seg.reshape(-1, e.per).sum(1) == e.frame_segs).all(), f"{what}, {order}: segments per frame"
    assert ctx.film_last_order() == (order if ran is None else ran), what
    return res, seg


# ---------------------------------------------------------------------------
# 1. scan classes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["test_world", "rtiow11", "r2_mixed", "r3_small", "no_layer"])
def test_small_scenes(gpu_ctx, oracle, rtx, name):
    """4 spheres; the LDS-copy class with layout and grid; the scene-order run;
    the map in memory; no layer at all."""
    e = expectation(oracle, name)
    upload(gpu_ctx, rtx, case_of(oracle, name))
    info = gpu_ctx.scene_info()
    if name != "test_world":
        for k, v in rc.expected_info(name).items():
            assert info[k] == v, (name, k, info)
    assert info["kernels"] == 0
    check(gpu_ctx, e, name)


@pytest.mark.parametrize("mode", ["auto", "linear"])
def test_large_world(gpu_ctx, oracle, rtx, mode):
    """random_world(25), above 1,024 spheres: the culled scan (auto, kernels 1)
    and the large linear scan (kernels 2)."""
    e = expectation(oracle, "rw25")
    try:
        upload(gpu_ctx, rtx, case_of(oracle, "rw25"), mode=mode)
        assert gpu_ctx.scene_info()["kernels"] == (1 if mode == "auto" else 2)
        check(gpu_ctx, e, f"random_world(25), {mode}")
    finally:
        gpu_ctx.set_scan_mode("auto")


@pytest.mark.parametrize("name", ["rtiow11", "rw25"])
def test_stress_build(stress_ctx, oracle, rtx, name):
    e = expectation(oracle, name)
    upload(stress_ctx, rtx, case_of(oracle, name))
    check(stress_ctx, e, f"stress build, {name}")


# ---------------------------------------------------------------------------
# 2. the lens
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rtiow11", "rw25"])
@pytest.mark.parametrize("lens", ["all", "third"])
def test_lens(gpu_ctx, oracle, rtx, name, lens):
    """96-byte records with lens_r = 0.05; and the same batch with lens_r = 0
    in every third frame, so that lanes with and without a lens share a wave
    (a frame is 32 records: half a wave)."""
    e = expectation(oracle, name, lens=lens)
    assert e.recs.shape[1] == 24 and (e.recs[:, 19] > 0).any()
    assert ((e.recs[:, 19] == 0).any()) == (lens == "third")
    upload(gpu_ctx, rtx, case_of(oracle, name))
    for order in ORDERS:
        check(gpu_ctx, e, f"{name}, lens {lens}", order)


def test_lens_records_without_a_lens_equal_the_short_records(gpu_ctx, oracle, rtx):
    e, z = expectation(oracle, "rtiow11"), expectation(oracle, "rtiow11", lens="zero")
    assert z.recs.shape[1] == 24 and not z.recs[:, 19].any() and (z.recs[:, :16].view(np.uint32)
                                                                  == e.recs.view(np.uint32)).all()
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    short, short_seg = check(gpu_ctx, e, "64-byte records")
    long_, long_seg = check(gpu_ctx, z, "96-byte records, radii 0")
    assert_bits_equal(long_, short, "96-byte records with all radii 0 against the 64-byte call")
    assert (long_seg == short_seg).all()


# ---------------------------------------------------------------------------
# 3. a camera's frame
# ---------------------------------------------------------------------------
CW, CH = 64, 36


@pytest.fixture(scope="module")
def camera(oracle, rtx):
    """camera_look_at 64 x 36 on rtiow11 at 6 spp, depth 8: the frame, its
    records for every pixel, and the oracle's linear sums."""
    case = case_of(oracle, "rtiow11")
    frame = rtx.camera_look_at(CW, CH, aspect=CW / CH)
    world = hc.Case(case.spheres, case.mat_types, case.mat_values, fc.DEPTH, fc.SAMPLES)
    want, segs = oracle.render_rows_linear(world, frame, np.arange(CH), nthreads=min(8, os.cpu_count() or 1))
    ys, xs = np.divmod(np.arange(CW * CH), CW)
    q, img_w, img_h = rtx.film_from_frame(frame, xs, ys)
    recs = np.ascontiguousarray(q).view(f32).reshape(-1, 16)
    for a in (want, recs):
        a.setflags(write=False)
    return type("Camera", (), dict(frame=frame, want=want.reshape(CW * CH, 4), segs=segs, recs=recs,
                                   img=(img_w, img_h), xs=xs, ys=ys))


def test_camera_frame_equals_oracle_and_render_sum(gpu_ctx, oracle, rtx, camera):
    """film_from_frame of every pixel equals oracle.render_rows_linear and the
    GPU's rtx_render_sum of that frame; a fixed shuffle gives the permuted
    records; a rectangle and every third pixel give their own pixels."""
    case = case_of(oracle, "rtiow11")
    upload(gpu_ctx, rtx, case, spp=fc.SAMPLES)
    res, seg = trace(gpu_ctx, camera.recs, img=camera.img)
    assert_bits_equal(res[:, :3], camera.want[:, :3], "every pixel against the oracle")
    assert int(seg.sum()) == camera.segs
    gpu_ctx.set_frame(camera.frame)
    d_sum = gpu_ctx.alloc((CW * CH, 4))
    try:
        gpu_ctx.render_sum(0, d_sum.ptr)
        gpu_ctx.sync()
        assert_bits_equal(res[:, :3], d_sum.numpy()[:, :3], "every pixel against rtx_render_sum")
    finally:
        d_sum.free()
    perm = np.random.default_rng(78).permutation(CW * CH)
    for order in ORDERS:
        res_p, seg_p = trace(gpu_ctx, camera.recs[perm], img=camera.img, order=order)
        assert_bits_equal(res_p, res[perm], f"a fixed shuffle, {order}")
        assert (seg_p == seg[perm]).all()
    rect = np.array([y * CW + x for y in range(7, 19) for x in range(21, 50)])
    for name, pick in (("a rectangle", rect), ("every third pixel", np.arange(0, CW * CH, 3))):
        q, w, h = rtx.film_from_frame(camera.frame, camera.xs[pick], camera.ys[pick])
        assert (w, h) == camera.img
        sub, sub_seg = trace(gpu_ctx, np.ascontiguousarray(q).view(f32).reshape(-1, 16), img=camera.img)
        assert_bits_equal(sub, res[pick], name)
        assert_bits_equal(sub[:, :3], camera.want[pick, :3], f"{name} against the oracle")
        assert (sub_seg == seg[pick]).all()


def test_camera_frame_is_the_refine_chain_state(gpu_ctx, oracle, rtx, camera):
    """All four result floats equal rtx_refine_export after refine(6), and a
    continuing call of 3 more samples equals refine(3)."""
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    res, _ = trace(gpu_ctx, camera.recs, img=camera.img)
    more, _ = trace(gpu_ctx, camera.recs, 3, flags=CONTINUE, start=res, img=camera.img)
    gpu_ctx.set_frame(camera.frame)
    assert gpu_ctx.refine(fc.SAMPLES, reset=True) == fc.SAMPLES
    assert_bits_equal(res, gpu_ctx.refine_export().reshape(CW * CH, 4), "results against the chain state")
    assert gpu_ctx.refine(3) == fc.SAMPLES + 3
    assert_bits_equal(more, gpu_ctx.refine_export().reshape(CW * CH, 4), "3 more samples either way")


# ---------------------------------------------------------------------------
# 4., 5. zero footprint, unit form
# ---------------------------------------------------------------------------
def test_zero_footprint_is_trace_paths(gpu_ctx, oracle, rtx):
    """H = V = 0 records give rtx_trace_paths' sums, seeds and segments for the
    twin queries (o, fl(L - o), seed)."""
    n, seed, scale = RECIPES["rtiow11"]
    o, L = pc.ray_recipe(n, seed, scale)
    recs = np.concatenate([fc.records(o[i], L[i], np.zeros(3), np.zeros(3)) for i in range(n)])
    twins = np.concatenate([pc.probes(o[i], L[i]) for i in range(n)])
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    res, seg = trace(gpu_ctx, recs)
    d_q = gpu_ctx.alloc((len(twins), 8))
    try:
        d_q.upload(twins)
        r, s = gpu_ctx.trace_paths(d_q, fc.SAMPLES, order="given", segments=True, n=len(twins))
        gpu_ctx.sync()
        assert_bits_equal(res, r.numpy().view(f32).reshape(-1, 4), "zero footprint against rtx_trace_paths")
        assert (seg == s.numpy()).all()
        r.free()
        s.free()
    finally:
        d_q.free()


def test_unit_form(gpu_ctx, oracle, rtx):
    """film_camera("equirect", 16 x 8) records, seeds replaced by
    path_seed(0, 0, 1 + k), traced with img_w = img_h = 2, against the oracle's
    one-pixel frames with frame_index = 1 + k."""
    case = case_of(oracle, "rtiow11")
    q = rtx.film_camera("equirect", 16, 8, look_from=(3.0, 1.5, 2.0), look_at=(0.0, 0.5, 0.0))
    for k in range(len(q)):
        q["seed"][k] = rtx.path_seed(0, 0, 1 + k)
    world = hc.Case(case.spheres, case.mat_types, case.mat_values, fc.DEPTH, fc.SAMPLES)
    want, segs = [], []
    for k, r in enumerate(q):
        frame = fc.film_frame(r["o"], r["lower_left"], r["horizontal"], r["vertical"], 1, 1, 2, 2, frame_index=1 + k)
        img, s = oracle.render_rows_linear(world, frame, np.arange(1))
        want.append(img.reshape(4)[:3])
        segs.append(s)
    assert sum(s > fc.SAMPLES for s in segs) > len(q) // 4  # (the camera sees the scene)
    upload(gpu_ctx, rtx, case)
    res, seg = trace(gpu_ctx, np.ascontiguousarray(q).view(f32).reshape(-1, 16), img=(2.0, 2.0))
    assert_bits_equal(res[:, :3], np.array(want, f32), "unit-form records against one-pixel frames")
    assert (seg == np.array(segs)).all()


# ---------------------------------------------------------------------------
# 6., 7. batch edges, orders
# ---------------------------------------------------------------------------
def test_batch_edges(gpu_ctx, oracle, rtx):
    """n = 1, 63, 64, 65 and 257 as prefixes of one record buffer: part of a
    wave, a whole wave, a wave and a lane, a workgroup and a lane. Nothing past
    n - 1 is written and every record below it is (trace checks both)."""
    e = expectation(oracle, "rtiow11")
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    full, full_seg = trace(gpu_ctx, e.recs[:320])
    for n in (1, 63, 64, 65, 257):
        for order in ORDERS:
            res, seg = trace(gpu_ctx, e.recs[:320], n=n, order=order)
            assert_bits_equal(res[:, :3], e.sums[:n], f"n = {n}, {order}")
            assert_bits_equal(res[:, 3], full[:n, 3], f"n = {n}, {order}: seeds")
            assert (seg == full_seg[:n]).all(), f"n = {n}, {order}: segments"


@pytest.mark.parametrize("name", ["rtiow11", "rw25"])
def test_orders(gpu_ctx, oracle, rtx, name):
    """given and cost give equal records and summed segments, film_last_order
    names the one that ran, auto is given, samples <= the probe runs given,
    coherent is refused, and a sorted film call leaves rtx_debug_paths_order
    nothing to report (RTX_ERR_STATE)."""
    e = expectation(oracle, name)
    upload(gpu_ctx, rtx, case_of(oracle, name))
    probe = 1 if name == "rw25" else 2
    assert (gpu_ctx.scene_info()["n_pad"] > 1024) == (probe == 1)
    got = {order: check(gpu_ctx, e, name, order) for order in ORDERS}
    assert_bits_equal(got["given"][0], got["cost"][0], f"{name}: records under the two orders")
    assert (got["given"][1] == got["cost"][1]).all()
    perm = np.empty(len(e.recs), np.uint32)
    rc_ = gpu_ctx._lib.rtx_debug_paths_order(gpu_ctx._h, perm.ctypes.data_as(C.POINTER(C.c_uint32)), perm.nbytes)
    assert rc_ == RTX_ERR_STATE
    res, seg = trace(gpu_ctx, e.recs, order="auto")
    assert gpu_ctx.film_last_order() == "given"
    assert_bits_equal(res, got["given"][0], f"{name}: auto")
    few = expectation(oracle, name, samples=probe, all_sky_max=None)
    check(gpu_ctx, few, f"{name}: {probe} samples under cost", "cost", samples=probe, ran="given")
    with pytest.raises(rtx.RtxError, match="coherent"):
        trace(gpu_ctx, e.recs, order="coherent")


# ---------------------------------------------------------------------------
# 8. chains
# ---------------------------------------------------------------------------
def test_continue_equals_one_call(gpu_ctx, oracle, rtx):
    """6 samples in one call equal 2 samples followed by a continuing call of
    4, sums and seeds; the continuing call reports its own segments only, and
    the query's own seed is not read by it."""
    e = expectation(oracle, "rtiow11")
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    whole, seg6 = check(gpu_ctx, e, "6 samples")
    first, seg2 = trace(gpu_ctx, e.recs, 2)
    assert (seg2 >= 2).all() and (seg2 < seg6).all()
    scrubbed = np.array(e.recs)
    scrubbed[:, 3] = np.nan  # the seed a continuing call must not read
    for order in ORDERS:
        rest, seg4 = trace(gpu_ctx, scrubbed, 4, order=order, flags=CONTINUE, start=first)
        assert_bits_equal(rest, whole, f"2 + 4 samples, {order}: sums and seeds")
        assert (seg2 + seg4 == seg6).all(), "a continuing call reports its own segments"
    e2 = expectation(oracle, "rtiow11", samples=2)
    assert_bits_equal(first[:, :3], e2.sums, "2 samples")
    assert (seg2.reshape(-1, PER).sum(1) == e2.frame_segs).all()


# ---------------------------------------------------------------------------
# 9. other dimensions, frame index, guard, depth
# ---------------------------------------------------------------------------
def test_other_dimensions(gpu_ctx, oracle, rtx):
    e = expectation(oracle, "rtiow11", rays=16, img_w=11.5, img_h=3.25)
    plain = expectation(oracle, "rtiow11", rays=16)
    assert (e.sums.view(np.uint32) != plain.sums.view(np.uint32)).any(1).mean() > 0.9
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    for order in ORDERS:
        check(gpu_ctx, e, "img_w, img_h = 11.5, 3.25", order, img=(11.5, 3.25))


@pytest.mark.parametrize("frame_index", [1, 0x7FFFFFFF])
def test_frame_index_seeds(gpu_ctx, oracle, rtx, frame_index):
    e = expectation(oracle, "rtiow11", rays=16, frame_index=frame_index)
    assert e.recs[3, 3] == rtx.path_seed(3, 0, frame_index) != rtx.path_seed(3, 0)
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    check(gpu_ctx, e, f"frame_index {frame_index}")


def test_lambert_guard(gpu_ctx, oracle, rtx):
    e = expectation(oracle, "rtiow11", rays=16, flags=1)
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    for order in ORDERS:
        check(gpu_ctx, e, "RTX_PATHS_LAMBERT_GUARD", order, flags=GUARD)


@pytest.mark.parametrize("depth", [1, 50])
def test_depth(gpu_ctx, oracle, rtx, depth):
    """The depth is the uploaded world's. At depth 1 every sample is one
    segment, so expect's all-sky count cannot tell a bounce from the sky: the
    rays are rtiow11's first 16, which meet its cap at depth 8 and 50."""
    expectation(oracle, "rtiow11", rays=16)  # (the cap holds for these rays)
    e = expectation(oracle, "rtiow11", rays=16, depth=depth, all_sky_max=None if depth == 1 else fc.ALL_SKY_MAX)
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"), depth=depth)
    res, seg = check(gpu_ctx, e, f"depth {depth}")
    assert (seg == fc.SAMPLES).all() if depth == 1 else seg.max() > 8


# ---------------------------------------------------------------------------
# 10. hostile records
# ---------------------------------------------------------------------------
def test_hostile_records(gpu_ctx, oracle, rtx):
    """A NaN in H and a zero direction (L = o, H = V = 0) among ordinary
    records, and one call with img_w = 1 (u = x / 0): sums and segment counts
    equal the oracle's, and the ordinary rays' records are what they are without
    them."""
    n, seed, scale = RECIPES["rtiow11"]
    o, L, hor, ver, _, _ = (a[:4].copy() for a in fc.recipe(n, seed, scale))
    hor[1, 1] = np.nan
    L[2], hor[2], ver[2] = o[2], 0, 0
    case = case_of(oracle, "rtiow11")
    for key, kw in ((("rtiow11", "hostile"), {}), (("rtiow11", "hostile, img_w 1"), dict(img_w=1.0))):
        if key not in _EXPECT:
            _EXPECT[key] = fc.expect(case, o, L, hor, ver, all_sky_max=None, **kw)
    e, e1 = _EXPECT[("rtiow11", "hostile")], _EXPECT[("rtiow11", "hostile, img_w 1")]
    assert np.isnan(e.recs[PER:2 * PER, 9]).all() and (e.recs[2 * PER:3 * PER, 4:7] == e.recs[2 * PER:3 * PER, 0:3]).all()
    upload(gpu_ctx, rtx, case)
    for order in ORDERS:
        res, _ = check(gpu_ctx, e, "hostile records", order)
        check(gpu_ctx, e1, "img_w = 1", order, img=(1.0, float(fc.H)))
    clean = expectation(oracle, "rtiow11")
    assert_bits_equal(res[:PER, :3], clean.sums[:PER], "ray 0 beside the hostile ones")
    assert_bits_equal(res[3 * PER:, :3], clean.sums[3 * PER:4 * PER], "ray 3 beside the hostile ones")


# ---------------------------------------------------------------------------
# 11. no side effects, no frame, refusals, an empty batch
# ---------------------------------------------------------------------------
def test_no_frame_needed(oracle, rtx):
    """A context with a world and no frame."""
    e = expectation(oracle, "rtiow11", rays=16)
    with rtx.Context(0) as fresh:
        assert fresh.film_last_order() == "given"
        upload(fresh, rtx, case_of(oracle, "rtiow11"))
        for order in ORDERS:
            check(fresh, e, "no frame", order)


def test_trace_touches_nothing_else(gpu_ctx, oracle, rtx):
    """After a frame and two refine steps: the stats, the framebuffer, the
    chain state, its sample count and the cost map are the same after film
    queries in both orders, and the next refine step continues the chain as if
    nothing had happened."""
    world = rtx.random_world(11, depth=fc.DEPTH, spp=4)
    frame = rtx.camera_look_at(rc.W, rc.H, aspect=rc.W / rc.H)
    e = expectation(oracle, "rtiow11")
    gpu_ctx.set_scan_mode("auto")
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    gpu_ctx.stats_reset()
    gpu_ctx.render()
    assert gpu_ctx.refine(5, reset=True) == 5 and gpu_ctx.refine(4) == 9

    def snapshot():
        st = gpu_ctx.stats()
        cost, covered = gpu_ctx.refine_cost()
        return (bytes(st)[8:], gpu_ctx.download().tobytes(), gpu_ctx.refine_export().tobytes(),
                gpu_ctx.refined_samples, np.asarray(cost).tobytes(), covered, gpu_ctx.refine_last_keys,
                gpu_ctx.cast_last_order(), gpu_ctx.paths_last_order())

    before = snapshot()
    for order in ORDERS:
        check(gpu_ctx, e, "between refine steps", order)
    after = snapshot()
    for k, (a, b) in enumerate(zip(before, after)):
        assert a == b, f"snapshot item {k} changed"
    assert gpu_ctx.refine(3) == 12
    case = hc.Case(world.spheres, world.mat_types, world.mat_values, fc.DEPTH, 12)
    img, _ = oracle.render_rows(case, frame, np.arange(rc.H), nthreads=min(8, os.cpu_count() or 1))
    assert_bits_equal(gpu_ctx.download(), img, "refine(5) + refine(4) + film queries + refine(3)")


def test_refusals(gpu_ctx, oracle, rtx):
    lib, h = gpu_ctx._lib, gpu_ctx._h
    e = expectation(oracle, "rtiow11", rays=16)
    case = case_of(oracle, "rtiow11")
    d_q = gpu_ctx.alloc((64, 16))
    d_q.upload(np.ascontiguousarray(e.recs[:64]))
    d_r, d_s = filled(gpu_ctx, 64, rtx.PATH_RESULT_DTYPE), filled(gpu_ctx, 64, np.uint32)
    q, r, s = C.c_void_p(d_q.ptr), C.c_void_p(d_r.ptr), C.c_void_p(d_s.ptr)
    with rtx.Context(0) as fresh:  # no world
        assert fresh._lib.rtx_trace_film(fresh._h, q, 64, 6, 8, 4, 0, 1, r, s) == RTX_ERR_STATE
        assert b"no world" in fresh._lib.rtx_last_error()
    upload(gpu_ctx, rtx, case, depth=0)
    assert lib.rtx_trace_film(h, q, 64, 6, 8, 4, 0, 1, r, s) == RTX_ERR_INVALID and b"depth is 0" in lib.rtx_last_error()
    upload(gpu_ctx, rtx, case, depth=65536)
    assert lib.rtx_trace_film(h, q, 64, 65536, 8, 4, 0, 1, r, s) == RTX_ERR_INVALID and b"32 bits" in lib.rtx_last_error()
    upload(gpu_ctx, rtx, case)
    for args, word in [((None, 64, 6, 8, 4, 0, 1, r, s), b"d_queries"), ((q, 64, 6, 8, 4, 0, 1, None, s), b"d_results"),
                       ((q, 64, 0, 8, 4, 0, 1, r, s), b"samples"), ((q, 64, 6, 8, 4, 8, 1, r, s), b"flags"),
                       ((q, 64, 6, 8, 4, 0, 2, r, s), b"coherent"), ((q, 64, 6, 8, 4, 0, 4, r, s), b"order")]:
        assert lib.rtx_trace_film(h, *args) == RTX_ERR_INVALID, args
        assert lib.rtx_last_error().startswith(b"rtx_trace_film:") and word in lib.rtx_last_error()
    for order in (0, 1, 3):
        assert lib.rtx_trace_film(h, None, 0, 6, 8, 4, 0, order, None, None) == 0  # an empty batch: no buffer, no launch
    with pytest.raises(rtx.RtxError):
        gpu_ctx.trace_film(d_q, 6, 8, 4, cont=True, n=64)  # nothing to continue from
    gpu_ctx.sync()
    assert untouched(d_r.numpy()) and untouched(d_s.numpy())
    assert lib.rtx_trace_film(h, q, 64, 6, 8, 4, 0, 3, r, None) == 0  # segments are optional, in the cost order too
    gpu_ctx.sync()
    assert_bits_equal(d_r.numpy().view(f32).reshape(64, 4)[:, :3], e.sums[:64], "no segment buffer")
    assert untouched(d_s.numpy())
    for d in (d_q, d_r, d_s):
        d.free()


# ---------------------------------------------------------------------------
# 12. numpy in and out, torch tensors, the command line
# ---------------------------------------------------------------------------
def test_numpy_in_and_out(gpu_ctx, oracle, rtx):
    e, el = expectation(oracle, "rtiow11", rays=16), expectation(oracle, "rtiow11", rays=16, lens="all")
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    for host in (np.array(e.recs), np.array(e.recs).view(rtx.FILM_QUERY_DTYPE).reshape(-1)):
        res, seg = gpu_ctx.trace_film(host, fc.SAMPLES, *IMG, segments=True)
        assert res.dtype == rtx.PATH_RESULT_DTYPE and seg.dtype == np.uint32 and len(res) == len(seg) == len(e.recs)
        assert_bits_equal(res["sum"], e.sums, "numpy in and out")
        assert (seg.reshape(-1, PER).sum(1) == e.frame_segs).all()
    for host in (np.array(el.recs), np.array(el.recs).view(rtx.FILM_LENS_QUERY_DTYPE).reshape(-1)):
        got, seg = gpu_ctx.trace_film(host, fc.SAMPLES, *IMG, order="cost")
        assert seg is None and gpu_ctx.film_last_order() == "cost"
        assert_bits_equal(got["sum"], el.sums, "numpy lens records")
    first, seg = gpu_ctx.trace_film(np.array(e.recs), 2, *IMG)
    assert seg is None
    rest, _ = gpu_ctx.trace_film(np.array(e.recs), 4, *IMG, results=first, cont=True)
    assert_bits_equal(rest["sum"], res["sum"], "numpy, continued")
    assert_bits_equal(rest["seed"], res["seed"], "numpy, continued: seeds")
    assert gpu_ctx.trace_film(np.zeros((0, 16), f32), 3, *IMG)[0].shape == (0,)
    with pytest.raises(rtx.RtxError):
        gpu_ctx.trace_film(np.array(e.recs), 2, *IMG, lens=True)
    # the image of the first frame's 8 x 4 records: toGamma(sum / samples), alpha 1
    img = gpu_ctx.film_image(res[:PER], fc.SAMPLES, fc.W, fc.H)
    mean = (res["sum"][:PER] / f32(fc.SAMPLES)).astype(f32)
    assert img.shape == (fc.H, fc.W, 4) and (img[..., 3] == 1).all()
    want = oracle.math("pow", mean.ravel(), np.full(mean.size, 0.454545454545, f32)).reshape(PER, 3)
    assert_bits_equal(img[..., :3].reshape(PER, 3), want, "film_image against toGamma(sum / samples)")


def test_torch_tensors_on_the_current_stream(tmp_path, oracle, rtx):
    """Torch tensors in place with the context on torch's current stream
    (child process: torch must load before librtx)."""
    e = expectation(oracle, "rtiow11", rays=16)
    case = case_of(oracle, "rtiow11")
    for name, a in (("queries", e.recs), ("sums", e.sums), ("spheres", case.spheres), ("mat_types", case.mat_types),
                    ("mat_values", case.mat_values)):
        np.save(tmp_path / f"{name}.npy", np.asarray(a))
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_film_check.py")
    out = subprocess.run([sys.executable, script, str(tmp_path), str(fc.SAMPLES), str(fc.DEPTH), str(fc.W), str(fc.H)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_cli_round_trip(tmp_path, oracle, rtx):
    """rtx_cli --scene rtiow11 --film Q.bin --film-dim 8,4 --samples 2, then
    --samples 4 --continue --film-order cost on the same result file: raw
    records in and out, 6 samples' expectation; --segments holds the last
    call's own counts. With --film-lens the 96-byte records."""
    for lens in (False, True):
        e = expectation(oracle, "rtiow11", lens="third" if lens else None)
        src, dst, sg = str(tmp_path / "q.bin"), str(tmp_path / "r.bin"), str(tmp_path / "s.bin")
        np.asarray(e.recs).tofile(src)
        base = [CLI, "--scene", "rtiow11", "--width", "64", "--height", "36", "--depth", str(fc.DEPTH), "--film", src,
                "--film-dim", f"{fc.W},{fc.H}", "--results", dst, "--segments", sg] + (["--film-lens"] if lens else [])
        total = 0
        for samples, more in ((2, []), (4, ["--continue", "--film-order", "cost"])):
            out = subprocess.run(base + ["--samples", str(samples)] + more, capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
            rep = json.loads(out.stdout.strip().splitlines()[-1])["film"]
            seg = np.fromfile(sg, np.uint32)
            assert rep["queries"] == len(e.recs) and rep["samples"] == samples and rep["segments"] == int(seg.sum())
            assert rep["continued"] == bool(more) and rep["order"] == ("cost" if more else "given") and rep["lens"] == lens
            total = total + seg
        got = np.fromfile(dst, rtx.PATH_RESULT_DTYPE)
        assert_bits_equal(got["sum"], e.sums, "rtx_cli --film, 2 + 4 samples")
        assert (total.reshape(-1, PER).sum(1) == e.frame_segs).all()
    bad = subprocess.run([CLI, "--scene", "rtiow11", "--film", src, "--samples", "2", "--results", dst],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--film-dim" in bad.stderr


@pytest.mark.parametrize("model,ext", [("equirect", "pfm"), ("fisheye", "ppm")])
def test_cli_film_camera_writes_an_image(tmp_path, model, ext):
    out_path = str(tmp_path / f"pano.{ext}")
    out = subprocess.run([CLI, "--scene", "rtiow11", "--width", "32", "--height", "16", "--depth", str(fc.DEPTH),
                          "--film-camera", model, "--film-fov", "170", "--samples", "3", "--out", out_path],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])["film"]
    assert rep["queries"] == 32 * 16 and rep["samples"] == 3 and rep["segments"] >= 3 * 32 * 16
    data = open(out_path, "rb").read()
    if ext == "pfm":
        head = data.split(b"\n", 3)
        assert head[0] == b"PF" and head[1].split() == [b"32", b"16"] and len(head[3]) == 32 * 16 * 12
        px = np.frombuffer(head[3], "<f4" if float(head[2]) < 0 else ">f4")
        assert np.isfinite(px).all() and px.min() >= 0 and px.max() > 0.2
    else:
        head = data.split(b"\n", 3)
        assert head[0] == b"P6" and head[1].split() == [b"32", b"16"] and len(head[3]) == 32 * 16 * 3
