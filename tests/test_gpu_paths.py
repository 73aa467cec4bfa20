"""rtx_trace_paths on the GPU: what rays of the caller's choosing see, one
result record per query on device buffers.

The expectation is the zero-film twin on the CPU oracle (paths_cases.expect,
cached per module): query (o, d, rtx_path_seed(x, y, f)) is pixel (x, y) of
oracle.render_rows_linear in the frame whose every pixel starts on the ray
(o, d). 8 x 4 seeds per ray, 6 samples, depth 8 unless a test says otherwise.
Every float is compared with assert_bits_equal (equal bits, NaN equal to NaN);
segment counts exactly. Result and segment buffers hold a byte pattern before
each call and are 16 records longer than the batch, so a record that was not
written, or one written past the end, shows. `order` is a schedule: "given" and
"coherent" must give the same records.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hostile_cases as hc
import paths_cases as pc
import regime_cases as rc
from conftest import GOLDEN, ROOT
from test_gpu_parity import assert_bits_equal

pytestmark = pytest.mark.gpu

f32 = np.float32
STRESS_LIB = os.path.join(os.path.dirname(GOLDEN), "..", "raytrace-we-gpu_amd", "lib", "variants",
                          "librtx_stress.so")
CLI = os.path.join(ROOT, "raytrace-we-gpu_amd", "bin", "rtx_cli")
ORDERS = ("given", "coherent")
FILL = 0xA5   # the byte every output buffer holds before a call
SLACK = 16    # records an output buffer has beyond the batch
RTX_ERR_INVALID, RTX_ERR_STATE = -1, -3
GUARD, CONTINUE = 1, 2
PER = pc.W * pc.H


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
        if name == "test_world":
            _CASES[name] = hc.Case(*oracle.test_world())
        elif name == "rw25":
            sph, mt, mv = oracle.random_world(25)
            assert len(sph) > 1024
            _CASES[name] = hc.Case(sph, mt, mv)
        else:
            _CASES[name] = rc.world(name)
    return _CASES[name]


# (rays, recipe seed, recipe scale): chosen on the CPU oracle so that expect's cap on all-sky rays holds
# (1 of 16, 4 of 48, 4 of 48, 4 of 48, 3 of 48, 2 of 16; RESULTS.md)
RECIPES = {"test_world": (16, 4110, 0.25), "rtiow11": (48, 4100 + len("rtiow11"), 1.0),
           "r2_mixed": (48, 4100 + len("r2_mixed"), 1.0), "r3_small": (48, 4100 + len("r3_small"), 1.0),
           "no_layer": (48, 4100 + len("no_layer"), 1.0), "rw25": (16, 4125, 25 / 11)}


def expectation(oracle, name, rays=None, **kw):
    """paths_cases.expect of world `name` with its recipe (its first `rays`
    rays), built once per (name, rays, options)."""
    key = (name, rays, tuple(sorted(kw.items())))
    if key not in _EXPECT:
        n, seed, scale = RECIPES[name]
        o, L = pc.ray_recipe(n, seed, scale)
        _EXPECT[key] = pc.expect(case_of(oracle, name), o[:rays], L[:rays], **kw)
    return _EXPECT[key]


def upload(ctx, rtx, case, depth=pc.DEPTH, mode="auto"):
    ctx.set_scan_mode(mode)
    ctx.upload_world(rtx.World(case.spheres, case.mat_types, case.mat_values, depth, 1))


def filled(ctx, n, dtype):
    d = ctx.alloc((n,), dtype)
    d.upload(np.frombuffer(bytes([FILL]) * d.nbytes, dtype))
    return d


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == FILL).all()


def trace(ctx, queries, samples=pc.SAMPLES, n=None, order="given", flags=0, start=None, segments=True):
    """rtx_trace_paths on device buffers: the first n rows of `queries`
    ((m, 8) float32) into pre-filled buffers of n + SLACK records (start: the
    (n, 4) records a continuing call begins from). Returns ((n, 4) float32
    results, (n,) uint32 segments or None) after checking that nothing beyond
    record n - 1 was written and every record before it was."""
    queries = np.ascontiguousarray(queries, f32).reshape(-1, 8)
    n = len(queries) if n is None else n
    d_q = ctx.alloc((max(len(queries), 1), 8))
    d_r = filled(ctx, n + SLACK, np.dtype([("v", "<f4", (4,))]))
    d_s = filled(ctx, n + SLACK, np.uint32) if segments else None
    try:
        if len(queries):
            d_q.upload(queries)
        if start is not None:
            keep = d_r.numpy()
            keep["v"][:n] = start
            d_r.upload(keep)
        got = ctx.trace_paths(d_q, samples, flags=flags, order=order, results=d_r, segments=d_s if segments else False,
                              n=n)
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


def check(ctx, e, what, order="given", flags=0, samples=pc.SAMPLES):
    res, seg = trace(ctx, e.rays, samples, order=order, flags=flags)
    assert_bits_equal(res[:, :3], e.sums, f"{what}, {order}: sums")
    assert (seg.reshape(-1, e.per).sum(1) == e.twin_segs).all(), f"{what}, {order}: segments per twin"
    assert ctx.paths_last_order() == order, what
    return res, seg


# ---------------------------------------------------------------------------
# scan classes
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
# batch edges, neighbours, orders
# ---------------------------------------------------------------------------
def test_batch_edges(gpu_ctx, oracle, rtx):
    """n = 1, 63, 64, 65 and 257 as prefixes of one query buffer: part of a
    wave, a whole wave, a wave and a lane, a workgroup and a lane. Nothing past
    n - 1 is written and every record below it is (trace checks both)."""
    e = expectation(oracle, "rtiow11")
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    full, full_seg = trace(gpu_ctx, e.rays[:320])
    for n in (1, 63, 64, 65, 257):
        for order in ORDERS:
            res, seg = trace(gpu_ctx, e.rays[:320], n=n, order=order)
            assert_bits_equal(res[:, :3], e.sums[:n], f"n = {n}, {order}")
            assert_bits_equal(res[:, 3], full[:n, 3], f"n = {n}, {order}: seeds")
            assert (seg == full_seg[:n]).all(), f"n = {n}, {order}: segments"


def test_neighbours_do_not_matter(gpu_ctx, oracle, rtx):
    """The same queries in twin order and in a fixed shuffle: a query's record
    (sum, seed, segments) does not depend on which lanes share its wave."""
    e = expectation(oracle, "rtiow11")
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    res, seg = trace(gpu_ctx, e.rays)
    perm = np.random.default_rng(77).permutation(len(e.rays))
    res_p, seg_p = trace(gpu_ctx, e.rays[perm])
    assert_bits_equal(res_p, res[perm], "a fixed shuffle")
    assert (seg_p == seg[perm]).all()
    assert_bits_equal(res_p[:, :3], e.sums[perm], "a fixed shuffle against the oracle")


@pytest.mark.parametrize("name", ["rtiow11", "rw25"])
def test_orders(gpu_ctx, oracle, rtx, name):
    """given and coherent give equal records, paths_last_order names the one
    that ran, and auto resolves to given."""
    e = expectation(oracle, name)
    upload(gpu_ctx, rtx, case_of(oracle, name))
    got = {order: check(gpu_ctx, e, name, order) for order in ORDERS}
    assert_bits_equal(got["given"][0], got["coherent"][0], f"{name}: records under the two orders")
    assert (got["given"][1] == got["coherent"][1]).all()
    res, seg = trace(gpu_ctx, e.rays, order="auto")
    assert gpu_ctx.paths_last_order() == "given"
    assert_bits_equal(res, got["given"][0], f"{name}: auto")


# ---------------------------------------------------------------------------
# chains, segments
# ---------------------------------------------------------------------------
def test_continue_equals_one_call(gpu_ctx, oracle, rtx):
    """6 samples in one call equal 2 samples followed by a continuing call of
    4, sums and seeds; the continuing call reports its own segments only, and
    the query's own seed is not read by it."""
    e = expectation(oracle, "rtiow11")
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    whole, seg6 = check(gpu_ctx, e, "6 samples")
    first, seg2 = trace(gpu_ctx, e.rays, 2)
    assert (seg2 >= 2).all() and (seg2 < seg6).all()
    scrubbed = np.array(e.rays)
    scrubbed[:, 3] = np.nan  # the seed a continuing call must not read
    for order in ORDERS:
        rest, seg4 = trace(gpu_ctx, scrubbed, 4, order=order, flags=CONTINUE, start=first)
        assert_bits_equal(rest, whole, f"2 + 4 samples, {order}: sums and seeds")
        assert (seg2 + seg4 == seg6).all(), "a continuing call reports its own segments"
    e2 = expectation(oracle, "rtiow11", samples=2)
    assert_bits_equal(first[:, :3], e2.sums, "2 samples")
    assert (seg2.reshape(-1, PER).sum(1) == e2.twin_segs).all()


def gpu_frame(rtx, f):
    g = rtx.rtx_frame()
    C.memmove(C.byref(g), C.byref(f), C.sizeof(g))
    return g


@pytest.mark.parametrize("ray", [0, 5])
def test_results_are_the_refine_chain_state(gpu_ctx, oracle, rtx, ray):
    """One ray's 8 x 4 queries equal, in all four floats, rtx_refine_export
    after rtx_refine(6) on that ray's twin frame: the sum and the seed after
    the last sample. A second refine step continues as a continuing call does."""
    e = expectation(oracle, "rtiow11")
    assert e.twin_segs[ray] > PER * pc.SAMPLES  # the ray bounces
    case = case_of(oracle, "rtiow11")
    upload(gpu_ctx, rtx, case)
    q = e.rays[ray * PER:(ray + 1) * PER]
    res, _ = trace(gpu_ctx, q)
    more, _ = trace(gpu_ctx, q, 3, flags=CONTINUE, start=res)
    gpu_ctx.set_frame(gpu_frame(rtx, pc.twin_frame(e.o[ray], e.L[ray])))
    assert gpu_ctx.refine(pc.SAMPLES, reset=True) == pc.SAMPLES
    state = gpu_ctx.refine_export().reshape(PER, 4)
    assert_bits_equal(res, state, "results against the chain state")
    assert_bits_equal(res[:, :3], e.sums[ray * PER:(ray + 1) * PER], "and against the oracle")
    assert gpu_ctx.refine(3) == pc.SAMPLES + 3
    assert_bits_equal(more, gpu_ctx.refine_export().reshape(PER, 4), "3 more samples either way")


# ---------------------------------------------------------------------------
# frame index, guard, depth, hostile rays
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("frame_index", [1, 0x7FFFFFFF])
def test_frame_index_seeds(gpu_ctx, oracle, rtx, frame_index):
    e = expectation(oracle, "rtiow11", rays=16, frame_index=frame_index)
    assert e.rays[3, 3] == rtx.path_seed(3, 0, frame_index) != rtx.path_seed(3, 0)
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
    e = expectation(oracle, "rtiow11", rays=16, depth=depth, all_sky_max=None if depth == 1 else pc.ALL_SKY_MAX)
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"), depth=depth)
    res, seg = check(gpu_ctx, e, f"depth {depth}")
    assert (seg == pc.SAMPLES).all() if depth == 1 else seg.max() > 8


def test_hostile_rays(gpu_ctx, oracle, rtx):
    """A zero direction and a NaN target among ordinary rays: their sums and
    segment counts equal the oracle's, and the ordinary rays' records are what
    they are without them."""
    n, seed, scale = RECIPES["rtiow11"]
    o, L = pc.ray_recipe(n, seed, scale)
    o, L = o[:4].copy(), L[:4].copy()
    L[1] = o[1]
    L[2, 1] = np.nan
    key = ("rtiow11", "hostile")
    if key not in _EXPECT:
        _EXPECT[key] = pc.expect(case_of(oracle, "rtiow11"), o, L, all_sky_max=None)
    e = _EXPECT[key]
    assert (e.rays[PER:2 * PER, 4:7] == 0).all() and np.isnan(e.rays[2 * PER:3 * PER, 5]).all()
    # what the oracle makes of them: every root is NaN, such a ray "hits" the last sphere at t = NaN again and
    # again, and each of its samples ends black at the depth
    assert (e.twin_segs[1:3] == PER * pc.SAMPLES * pc.DEPTH).all() and not e.sums[PER:3 * PER].any()
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    for order in ORDERS:
        res, _ = check(gpu_ctx, e, "hostile rays", order)
    clean = expectation(oracle, "rtiow11")
    assert_bits_equal(res[:PER, :3], clean.sums[:PER], "ray 0 beside the hostile ones")
    assert_bits_equal(res[3 * PER:, :3], clean.sums[3 * PER:4 * PER], "ray 3 beside the hostile ones")


# ---------------------------------------------------------------------------
# no side effects
# ---------------------------------------------------------------------------
def test_no_frame_needed(oracle, rtx):
    """A context with a world and no frame."""
    e = expectation(oracle, "rtiow11", rays=16)
    with rtx.Context(0) as fresh:
        assert fresh.paths_last_order() == "given"
        upload(fresh, rtx, case_of(oracle, "rtiow11"))
        check(fresh, e, "no frame")


def test_trace_touches_nothing_else(gpu_ctx, oracle, rtx):
    """After a frame and two refine steps: the stats, the framebuffer, the
    chain state, its sample count and the cost map are the same after path
    queries in both orders, and the next refine step continues the chain as if
    nothing had happened."""
    world = rtx.random_world(11, depth=pc.DEPTH, spp=4)
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
                gpu_ctx.cast_last_order())

    before = snapshot()
    for order in ORDERS:
        check(gpu_ctx, e, "between refine steps", order)
    after = snapshot()
    for k, (a, b) in enumerate(zip(before, after)):
        assert a == b, f"snapshot item {k} changed"
    assert gpu_ctx.refine(3) == 12
    case = hc.Case(world.spheres, world.mat_types, world.mat_values, pc.DEPTH, 12)
    img, _ = oracle.render_rows(case, frame, np.arange(rc.H), nthreads=min(8, os.cpu_count() or 1))
    assert_bits_equal(gpu_ctx.download(), img, "refine(5) + refine(4) + path queries + refine(3)")


# ---------------------------------------------------------------------------
# errors once the world is known
# ---------------------------------------------------------------------------
def test_refusals(gpu_ctx, oracle, rtx):
    lib, h = gpu_ctx._lib, gpu_ctx._h
    e = expectation(oracle, "rtiow11", rays=16)
    case = case_of(oracle, "rtiow11")
    d_q = gpu_ctx.alloc((64, 8))
    d_q.upload(np.ascontiguousarray(e.rays[:64]))
    d_r, d_s = filled(gpu_ctx, 64, rtx.PATH_RESULT_DTYPE), filled(gpu_ctx, 64, np.uint32)
    q, r, s = C.c_void_p(d_q.ptr), C.c_void_p(d_r.ptr), C.c_void_p(d_s.ptr)
    with rtx.Context(0) as fresh:  # no world
        assert fresh._lib.rtx_trace_paths(fresh._h, q, 64, 6, 0, 1, r, s) == RTX_ERR_STATE
        assert b"no world" in fresh._lib.rtx_last_error()
    upload(gpu_ctx, rtx, case, depth=0)
    assert lib.rtx_trace_paths(h, q, 64, 6, 0, 1, r, s) == RTX_ERR_INVALID and b"depth is 0" in lib.rtx_last_error()
    upload(gpu_ctx, rtx, case, depth=65536)
    assert lib.rtx_trace_paths(h, q, 64, 65536, 0, 1, r, s) == RTX_ERR_INVALID and b"32 bits" in lib.rtx_last_error()
    upload(gpu_ctx, rtx, case)
    for args in [(None, 64, 6, 0, 1, r, s), (q, 64, 6, 0, 1, None, s), (q, 64, 0, 0, 1, r, s), (q, 64, 6, 4, 1, r, s),
                 (q, 64, 6, 0, 3, r, s)]:
        assert lib.rtx_trace_paths(h, *args) == RTX_ERR_INVALID, args
        assert lib.rtx_last_error().startswith(b"rtx_trace_paths:")
    assert lib.rtx_trace_paths(h, None, 0, 6, 0, 1, None, None) == 0  # an empty batch: no buffer, no launch
    with pytest.raises(rtx.RtxError):
        gpu_ctx.trace_paths(d_q, 6, cont=True, n=64)  # nothing to continue from
    gpu_ctx.sync()
    assert untouched(d_r.numpy()) and untouched(d_s.numpy())
    assert lib.rtx_trace_paths(h, q, 64, 6, 0, 1, r, None) == 0  # segments are optional
    gpu_ctx.sync()
    assert_bits_equal(d_r.numpy().view(f32).reshape(64, 4)[:, :3], e.sums[:64], "no segment buffer")
    assert untouched(d_s.numpy())
    for d in (d_q, d_r, d_s):
        d.free()


# ---------------------------------------------------------------------------
# numpy in and out, torch tensors, the command line
# ---------------------------------------------------------------------------
def test_numpy_in_and_out(gpu_ctx, oracle, rtx):
    e = expectation(oracle, "rtiow11", rays=16)
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    for host in (np.array(e.rays), np.array(e.rays).view(rtx.PATH_QUERY_DTYPE).reshape(-1)):
        res, seg = gpu_ctx.trace_paths(host, pc.SAMPLES, segments=True)
        assert res.dtype == rtx.PATH_RESULT_DTYPE and seg.dtype == np.uint32 and len(res) == len(seg) == len(e.rays)
        assert_bits_equal(res["sum"], e.sums, "numpy in and out")
        assert (seg.reshape(-1, PER).sum(1) == e.twin_segs).all()
    first, seg = gpu_ctx.trace_paths(np.array(e.rays), 2)
    assert seg is None
    rest, _ = gpu_ctx.trace_paths(np.array(e.rays), 4, results=first, cont=True)
    assert_bits_equal(rest["sum"], res["sum"], "numpy, continued")
    assert_bits_equal(rest["seed"], res["seed"], "numpy, continued: seeds")
    built = rtx.path_queries(e.rays[:, 0:3], e.rays[:, 4:7], e.rays[:, 3])
    assert_bits_equal(gpu_ctx.trace_paths(built, pc.SAMPLES)[0]["sum"], e.sums, "path_queries")
    assert gpu_ctx.trace_paths(np.zeros((0, 8), f32), 3)[0].shape == (0,)


def test_torch_tensors_on_the_current_stream(tmp_path, oracle, rtx):
    """Torch tensors in place with the context on torch's current stream
    (child process: torch must load before librtx)."""
    e = expectation(oracle, "rtiow11", rays=16)
    case = case_of(oracle, "rtiow11")
    for name, a in (("queries", e.rays), ("sums", e.sums), ("spheres", case.spheres), ("mat_types", case.mat_types),
                    ("mat_values", case.mat_values)):
        np.save(tmp_path / f"{name}.npy", np.asarray(a))
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_paths_check.py")
    out = subprocess.run([sys.executable, script, str(tmp_path), str(pc.SAMPLES), str(pc.DEPTH)], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_cli_round_trip(tmp_path, oracle, rtx):
    """rtx_cli --scene rtiow11 --paths Q.bin --samples 2, then --samples 4
    --continue on the same result file: raw records in and out, 6 samples'
    expectation; --segments holds the last call's own counts."""
    e = expectation(oracle, "rtiow11")
    src, dst, sg = str(tmp_path / "q.bin"), str(tmp_path / "r.bin"), str(tmp_path / "s.bin")
    np.asarray(e.rays).tofile(src)
    base = [CLI, "--scene", "rtiow11", "--width", "64", "--height", "36", "--depth", str(pc.DEPTH), "--paths", src,
            "--results", dst, "--segments", sg]
    total = 0
    for samples, more in ((2, []), (4, ["--continue", "--cast-order", "coherent"])):
        out = subprocess.run(base + ["--samples", str(samples)] + more, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        rep = json.loads(out.stdout.strip().splitlines()[-1])["paths"]
        seg = np.fromfile(sg, np.uint32)
        assert rep["queries"] == len(e.rays) and rep["samples"] == samples and rep["segments"] == int(seg.sum())
        assert rep["continued"] == bool(more) and rep["order"] == ("coherent" if more else "given")
        total = total + seg
    got = np.fromfile(dst, rtx.PATH_RESULT_DTYPE)
    assert_bits_equal(got["sum"], e.sums, "rtx_cli --paths, 2 + 4 samples")
    assert (total.reshape(-1, PER).sum(1) == e.twin_segs).all()
    bad = subprocess.run([CLI, "--scene", "rtiow11", "--paths", src, "--samples", "2"], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode == 2 and "--results" in bad.stderr
