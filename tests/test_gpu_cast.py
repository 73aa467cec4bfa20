"""rtx_cast_rays on the GPU: batched closest-hit queries on device buffers,
each ray over (t_min, its own t_max), under both orders.

The expectation is built from oracle.hit_world_f32 alone and mapped into the
32-byte record (want_records): a hit keeps t, the index, the flipped normal and
front_face, a miss is (+inf, -1, 0 ...), and a ray whose range is empty,
!(t_max >= t_min), misses without the oracle being asked. Every float is
compared with assert_bits_equal (equal bits, NaN equal to NaN, as in the rest
of the suite); the integer fields (index, front_face, reserved) and the bytes
exactly. Output buffers hold a byte pattern before each call and are longer
than the batch, so a record that was not written, or one written past the end,
shows. `order` is a schedule: "given" and "coherent" must give the same
records, and rtx_cast_last_order names the one that ran.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hostile_cases as hc
import regime_cases as rc
from cases import grazing_rays
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
T_MIN = 0.001
RTX_ERR_INVALID, RTX_ERR_STATE = -1, -3
# rtx_ray_hit, as rtx.RAY_HIT_DTYPE states it (test_cast_host.py checks that one against the header)
HIT_DTYPE = np.dtype([("t", "<f4"), ("index", "<i4"), ("normal", "<f4", (3,)), ("front_face", "<u4"),
                      ("reserved", "<u4", (2,))])


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
# rays, expectations, the call
# ---------------------------------------------------------------------------
def rays8(rays6, t_max=np.inf):
    """(n, 6) (origin, direction) -> (n, 8) float32 rows (o, t_max, d, tag);
    the tag, which the library ignores, is a pattern of its own per ray."""
    rays6 = np.ascontiguousarray(rays6, f32).reshape(-1, 6)
    out = np.empty((len(rays6), 8), f32)
    out[:, 0:3], out[:, 4:7] = rays6[:, 0:3], rays6[:, 3:6]
    out[:, 3] = t_max
    out.view(np.uint32)[:, 7] = 0xC0FFEE00 + np.arange(len(rays6), dtype=np.uint32)
    return out


def want_records(rtx, rec, live=None):
    """The oracle's (n, 10) records (hit, t, p, normal, front_face, index) as
    rtx_ray_hit records; live: False where the ray's range is empty (a miss,
    whatever rec holds there)."""
    rec = np.asarray(rec, f32)
    hit = rec[:, 0] != 0
    if live is not None:
        hit &= live
    out = np.zeros(len(rec), rtx.RAY_HIT_DTYPE)
    out["t"] = np.where(hit, rec[:, 1], f32(np.inf))
    out["index"] = np.where(hit, rec[:, 9], -1).astype(np.int32)
    out["normal"] = np.where(hit[:, None], rec[:, 5:8], f32(0))
    out["front_face"] = np.where(hit, rec[:, 8] != 0, False).astype(np.uint32)
    out.setflags(write=False)
    return out


def assert_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.flatnonzero(got["index"] != want["index"])
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(got)} indices differ; first {bad[:5].tolist()}: " \
                          f"gpu {got['index'][bad[:5]].tolist()} vs oracle {want['index'][bad[:5]].tolist()}"
    assert_bits_equal(got["t"], want["t"], f"{what}: t")
    assert_bits_equal(got["normal"], want["normal"], f"{what}: normal")
    assert (got["front_face"] == want["front_face"]).all(), f"{what}: front_face"
    assert not got["reserved"].any(), f"{what}: reserved"


def filled(ctx, n, dtype):
    """A device buffer of n records whose every byte is FILL."""
    d = ctx.alloc((n,), dtype)
    d.upload(np.frombuffer(bytes([FILL]) * d.nbytes, dtype))
    return d


def untouched(a):
    return (np.ascontiguousarray(a).view(np.uint8) == FILL).all()


def cast(ctx, rays, order, n=None, t_min=T_MIN, hits=True, occluded=True):
    """rtx_cast_rays on device buffers: the first n rows of `rays` ((m, 8)
    float32) into pre-filled buffers of n + SLACK records. Returns the whole
    buffers as numpy arrays (None for an output not asked for), after checking
    that nothing beyond record n - 1 was written."""
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
    n = len(rays) if n is None else n
    d_rays = ctx.alloc((max(len(rays), 1), 8))
    d_hits = filled(ctx, n + SLACK, HIT_DTYPE) if hits else None
    d_occ = filled(ctx, n + SLACK, np.uint8) if occluded else None
    try:
        if len(rays):
            d_rays.upload(rays)
        got = ctx.cast(d_rays, t_min=t_min, order=order, hits=d_hits if hits else False,
                       occluded=d_occ if occluded else False, n=n)
        assert got[0] is d_hits and got[1] is d_occ
        ctx.sync()
        out = tuple(None if d is None else d.numpy() for d in (d_hits, d_occ))
        for a in out:
            assert a is None or untouched(a[n:]), f"n = {n}, {order}: a record past the batch was written"
        return out
    finally:
        for d in (d_rays, d_hits, d_occ):
            if d is not None:
                d.free()


def check(ctx, rtx, rays, want, order, what, t_min=T_MIN):
    hits, occ = cast(ctx, rays, order, t_min=t_min)
    n = len(want)
    assert_records(hits[:n], want, f"{what}, {order}")
    assert (occ[:n] == (want["index"] >= 0)).all(), f"{what}, {order}: the occluded bytes"
    assert ctx.cast_last_order() == order, what


_SETS = {}


def frame_and_grazing(oracle, rtx, key, case, seed):
    """(rays (n, 8), expectation) of a world: a seeded shuffle of the 67 x 35
    look-at frame's pixel-centre rays plus 300 grazing rays. Built once."""
    if key not in _SETS:
        frame = rtx.camera_look_at(67, 35, aspect=67 / 35)
        rng = np.random.default_rng(seed)
        r6 = np.concatenate([rc.primary_rays(frame), grazing_rays(case.spheres, 300, rng, xaxis_frac=0.05)])
        r6 = np.ascontiguousarray(r6[rng.permutation(len(r6))], f32)
        rec = oracle.hit_world_f32(case, r6, T_MIN)
        hit = rec[:, 0] != 0
        assert len(r6) == 67 * 35 + 300 and 0.2 < hit.mean() < 0.98, "inputs: hits and misses both"
        rays = rays8(r6)
        rays.setflags(write=False)
        _SETS[key] = (rays, want_records(rtx, rec))
    return _SETS[key]


def upload(ctx, rtx, case, mode="auto"):
    ctx.set_scan_mode(mode)
    ctx.upload_world(rtx.World(case.spheres, case.mat_types, case.mat_values, 1, 1))


def large_case(oracle):
    sph, mt, mv = oracle.random_world(25)
    assert len(sph) > 2400
    return hc.Case(sph, mt, mv)


# ---------------------------------------------------------------------------
# 1, 2, 8: scenes and scan forms
# ---------------------------------------------------------------------------
SMALL = ("rtiow11", "r2_run", "strip", "r3_full", "no_layer")


def small_scene(ctx, oracle, rtx, name):
    case = rc.world(name)
    rays, want = frame_and_grazing(oracle, rtx, name, case, 700 + SMALL.index(name))
    try:
        upload(ctx, rtx, case)
        info = ctx.scene_info()
        for k, v in rc.expected_info(name).items():
            assert info[k] == v, (name, k, info)
        for order in ORDERS:
            check(ctx, rtx, rays, want, order, name)
    finally:
        ctx.set_scan_mode("auto")


@pytest.mark.parametrize("name", SMALL)
def test_small_scenes(gpu_ctx, oracle, rtx, name):
    """The small-scene regimes (layout and grid in LDS, the scene-order run,
    the strip's 64 x 8 grid, the map in memory, no layer at all): 2,645 rays
    in a seeded shuffle, both orders."""
    small_scene(gpu_ctx, oracle, rtx, name)


def large_scene(ctx, oracle, rtx, mode):
    case = large_case(oracle)
    rays, want = frame_and_grazing(oracle, rtx, "rw25", case, 725)
    try:
        upload(ctx, rtx, case, mode)
        assert ctx.scene_info()["kernels"] == (1 if mode == "auto" else 2)
        for order in ORDERS:
            check(ctx, rtx, rays, want, order, f"random_world(25), {mode}")
    finally:
        ctx.set_scan_mode("auto")


@pytest.mark.parametrize("mode", ["auto", "linear"])
def test_large_scene(gpu_ctx, oracle, rtx, mode):
    """random_world(25), 2,504 spheres: the culled scan (auto, kernels 1) and
    the linear scan of the large-scene kernels (kernels 2)."""
    large_scene(gpu_ctx, oracle, rtx, mode)


def test_small_scene_linear(gpu_ctx, oracle, rtx):
    """rtiow11 under RTX_SCAN_LINEAR: scene-order blocks, no layout, no grid."""
    case = rc.world("rtiow11")
    rays, want = frame_and_grazing(oracle, rtx, "rtiow11", case, 700)
    try:
        upload(gpu_ctx, rtx, case, "linear")
        info = gpu_ctx.scene_info()
        assert info["kernels"] == 0 and info["layout"] == 0 and info["grid"] == 0, info
        for order in ORDERS:
            check(gpu_ctx, rtx, rays, want, order, "rtiow11, linear")
    finally:
        gpu_ctx.set_scan_mode("auto")


def test_stress_build_small(stress_ctx, oracle, rtx):
    small_scene(stress_ctx, oracle, rtx, "rtiow11")


def test_stress_build_culled(stress_ctx, oracle, rtx):
    large_scene(stress_ctx, oracle, rtx, "auto")


# ---------------------------------------------------------------------------
# 3: sizes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_sizes(gpu_ctx, oracle, rtx, order):
    """n = 0, 1, 63, 64, 65, 255, 256, 257 as prefixes of one set: part of a
    wave, a whole wave, a wave and a lane, and the same around the workgroup.
    Records past n keep the fill pattern (cast checks it); n = 0 writes
    nothing and is no launch."""
    case = rc.world("rtiow11")
    rays, want = frame_and_grazing(oracle, rtx, "rtiow11", case, 700)
    upload(gpu_ctx, rtx, case)
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        hits, occ = cast(gpu_ctx, rays[:300], order, n=n)
        assert_records(hits[:n], want[:n], f"n = {n}, {order}")
        assert (occ[:n] == (want["index"][:n] >= 0)).all()
        if n == 0:
            assert untouched(hits) and untouched(occ)


# ---------------------------------------------------------------------------
# 4: one bucket, hostile keys
# ---------------------------------------------------------------------------
def test_one_bucket(gpu_ctx, oracle, rtx):
    """300 copies of one ray: every key equal, one bucket holds the batch."""
    case = rc.world("rtiow11")
    rays, want = frame_and_grazing(oracle, rtx, "rtiow11", case, 700)
    k = int(np.flatnonzero(want["index"] > 0)[0])
    upload(gpu_ctx, rtx, case)
    for order in ORDERS:
        check(gpu_ctx, rtx, np.repeat(rays[k:k + 1], 300, 0), np.repeat(want[k:k + 1], 300), order, "one ray, 300 times")


_HOSTILE = {}


def hostile_set(oracle, rtx, ext):
    """Every hostile class of the degenerate world, grouped in whole waves,
    then the same rays shuffled among grazing rays. Built once."""
    if ext not in _HOSTILE:
        case, _, classes = hc.degenerate_world(ext)
        assert set(hc.ALWAYS_NONFINITE) | set(hc.ORDER_DEPENDENT) <= set(classes) and len(classes) == 36
        grouped, _ = hc.grouped(classes)
        mixed, _ = hc.mixed(classes, case.spheres, np.random.default_rng(900 + ext))
        r6 = np.concatenate([grouped, mixed[:2048]])
        rec = oracle.hit_world_f32(case, r6, T_MIN)
        assert np.isnan(rec[:, 1]).any() and (rec[:, 0] == 0).any()
        _HOSTILE[ext] = (case, rays8(r6), want_records(rtx, rec))
    return _HOSTILE[ext]


@pytest.mark.parametrize("ext", [11, 25])
def test_hostile_rays(gpu_ctx, oracle, rtx, ext):
    """NaN, infinite, zero, tiny and huge rays on the degenerate 486- and
    2,500-sphere worlds, the order-dependent classes included: what the key
    makes of them changes the schedule and no record."""
    case, rays, want = hostile_set(oracle, rtx, ext)
    upload(gpu_ctx, rtx, case)
    assert gpu_ctx.scene_info()["kernels"] == (0 if ext == 11 else 1)
    for order in ORDERS:
        check(gpu_ctx, rtx, rays, want, order, f"hostile rays, degenerate random_world({ext})")


# ---------------------------------------------------------------------------
# 5: per-ray t_max
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["rtiow11", "rw25"])
def test_per_ray_t_max(gpu_ctx, oracle, rtx, which):
    """200 rays that hit something, each with a t_max of its own from {+inf,
    half its hit t, exactly its hit t, the float just below it, t_min, the
    float below t_min, 0, -1, -inf, NaN}. The oracle is asked one ray at a
    time with (t_min, t_max); an empty range is a miss by the rule."""
    case = rc.world("rtiow11") if which == "rtiow11" else large_case(oracle)
    frame = rtx.camera_look_at(67, 35, aspect=67 / 35)
    r6 = rc.primary_rays(frame)
    t_hit = oracle.hit_world_f32(case, r6, T_MIN)
    r6 = r6[np.flatnonzero(t_hit[:, 0] != 0)[::7][:200]]
    assert len(r6) == 200
    t = oracle.hit_world_f32(case, r6, T_MIN)[:, 1].astype(f32)
    tm = f32(T_MIN)
    pick = np.arange(200) % 10
    t_max = np.select([pick == k for k in range(10)],
                      [np.full(200, np.inf, f32), (t * f32(0.5)).astype(f32), t, np.nextafter(t, f32(0)),
                       np.full(200, tm), np.full(200, np.nextafter(tm, f32(0))), np.zeros(200, f32),
                       np.full(200, -1, f32), np.full(200, -np.inf, f32), np.full(200, np.nan, f32)]).astype(f32)
    live = t_max >= tm
    rec = np.zeros((200, 10), f32)
    for i in np.flatnonzero(live):
        rec[i] = oracle.hit_world_f32(case, r6[i:i + 1], T_MIN, float(t_max[i]))[0]
    want = want_records(rtx, rec, live)
    # what the classes are there for: exactly t still hits, just below it does not hit the same sphere at t
    assert (want["index"][pick == 2] >= 0).all() and (want["t"][pick == 2] == t[pick == 2]).all()
    assert not (want["t"][pick == 3] == t[pick == 3]).any() and (want["index"][pick >= 5] == -1).all()
    upload(gpu_ctx, rtx, case)
    for order in ORDERS:
        check(gpu_ctx, rtx, rays8(r6, t_max), want, order, f"per-ray t_max, {which}")


# ---------------------------------------------------------------------------
# 6: outputs, and the numpy path of Context.cast
# ---------------------------------------------------------------------------
def test_outputs(gpu_ctx, oracle, rtx):
    """Hits only, bytes only and both; then host arrays in and out, as rows of
    8 floats and as RAY_DTYPE records."""
    case = rc.world("rtiow11")
    rays, want = frame_and_grazing(oracle, rtx, "rtiow11", case, 700)
    rays, want = rays[:500], want[:500]
    occ_want = want["index"] >= 0
    upload(gpu_ctx, rtx, case)
    for order in ORDERS:
        hits, occ = cast(gpu_ctx, rays, order, occluded=False)
        assert occ is None
        assert_records(hits[:500], want, f"hits only, {order}")
        hits, occ = cast(gpu_ctx, rays, order, hits=False)
        assert hits is None and (occ[:500] == occ_want).all(), f"bytes only, {order}"
        hits, occ = cast(gpu_ctx, rays, order)
        assert_records(hits[:500], want, f"both, {order}")
        assert (occ[:500] == occ_want).all()
        for host in (np.array(rays), np.array(rays).view(rtx.RAY_DTYPE).reshape(-1)):
            h, o = gpu_ctx.cast(host, order=order, hits=True, occluded=True)
            assert isinstance(h, np.ndarray) and h.dtype == rtx.RAY_HIT_DTYPE and o.dtype == np.uint8
            assert_records(h, want, f"numpy in and out, {order}")
            assert (o == occ_want).all()
        h, o = gpu_ctx.cast(np.array(rays), order=order)
        assert o is None
        assert_records(h, want, f"numpy, hits by default, {order}")
    assert gpu_ctx.cast(np.zeros((0, 8), f32))[0].shape == (0,)


# ---------------------------------------------------------------------------
# 7: side effects
# ---------------------------------------------------------------------------
def test_cast_touches_nothing_else(gpu_ctx, oracle, rtx):
    """After a frame and two refine steps (a chain state with its cost map):
    the stats, the framebuffer, the chain state, its sample count and the cost
    map are the same after casts in both orders, and the next refine step
    continues the chain as if nothing had happened."""
    world = rtx.random_world(11, depth=12, spp=4)
    frame = rtx.camera_look_at(rc.W, rc.H, aspect=rc.W / rc.H)
    rays, want = frame_and_grazing(oracle, rtx, "rtiow11", rc.world("rtiow11"), 700)
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
                gpu_ctx.refined_samples, np.asarray(cost).tobytes(), covered, gpu_ctx.refine_last_keys)

    before = snapshot()
    for order in ORDERS:
        check(gpu_ctx, rtx, rays, want, order, "between refine steps")
    after = snapshot()
    for k, (a, b) in enumerate(zip(before, after)):
        assert a == b, f"snapshot item {k} changed"
    # (bytes(st)[8:]: launches, samples, segments, sphere_tests, without kernel_ms's event times)
    assert gpu_ctx.refine(3) == 12
    case = hc.Case(world.spheres, world.mat_types, world.mat_values, 12, 12)
    img, _ = oracle.render_rows(case, frame, np.arange(rc.H), nthreads=min(8, os.cpu_count() or 1))
    assert_bits_equal(gpu_ctx.download(), img, "refine(5) + refine(4) + casts + refine(3)")


# ---------------------------------------------------------------------------
# 9, 10: torch tensors, the command line
# ---------------------------------------------------------------------------
def test_torch_tensors_on_the_current_stream(tmp_path, oracle, rtx):
    """Torch tensors in and out with the context on torch's current stream
    (child process: torch must load before librtx); the context's own stream
    is restored afterwards and still works."""
    case = rc.world("rtiow11")
    rays, want = frame_and_grazing(oracle, rtx, "rtiow11", case, 700)
    np.save(tmp_path / "rays.npy", np.asarray(rays))
    np.save(tmp_path / "want.npy", np.asarray(want))
    np.save(tmp_path / "spheres.npy", case.spheres)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_cast_check.py")
    out = subprocess.run([sys.executable, script, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.parametrize("order", ["auto", "coherent"])
def test_cli_round_trip(tmp_path, oracle, rtx, order):
    """rtx_cli --scene rtiow11 --cast RAYS.bin --hits OUT.bin: raw records in,
    raw records out, the same expectation."""
    rays, want = frame_and_grazing(oracle, rtx, "rtiow11", rc.world("rtiow11"), 700)
    src, dst = str(tmp_path / "rays.bin"), str(tmp_path / "hits.bin")
    np.asarray(rays).tofile(src)
    out = subprocess.run([CLI, "--scene", "rtiow11", "--width", "64", "--height", "36", "--cast", src, "--hits", dst,
                          "--cast-order", order, "--t-min", "0.001"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])["cast"]
    got = np.fromfile(dst, rtx.RAY_HIT_DTYPE)
    assert_records(got, want, f"rtx_cli --cast, {order}")
    assert rep["rays"] == len(want) and rep["hits"] == int((want["index"] >= 0).sum())
    assert rep["order"] == ("coherent" if order == "coherent" else rep["order"]) and rep["order"] in ORDERS
    bad = subprocess.run([CLI, "--scene", "rtiow11", "--cast", src], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--hits" in bad.stderr


# ---------------------------------------------------------------------------
# 11: refusals
# ---------------------------------------------------------------------------
def test_refusals(gpu_ctx, oracle, rtx):
    """On a live context every argument rule answers RTX_ERR_INVALID and
    writes nothing; a context without a world answers RTX_ERR_STATE; "auto"
    resolves to one of the two orders."""
    lib, h = gpu_ctx._lib, gpu_ctx._h
    case = rc.world("rtiow11")
    rays, want = frame_and_grazing(oracle, rtx, "rtiow11", case, 700)
    upload(gpu_ctx, rtx, case)
    d_rays = gpu_ctx.alloc((64, 8))
    d_rays.upload(rays[:64])
    d_hits, d_occ = filled(gpu_ctx, 64, rtx.RAY_HIT_DTYPE), filled(gpu_ctx, 64, np.uint8)
    r, ht, oc = C.c_void_p(d_rays.ptr), C.c_void_p(d_hits.ptr), C.c_void_p(d_occ.ptr)
    for args in [(None, 64, 0.001, 1, ht, oc), (r, 64, 0.001, 1, None, None), (r, 64, 0.0, 1, ht, oc),
                 (r, 64, -0.001, 2, ht, oc), (r, 64, float("nan"), 1, ht, oc), (r, 64, float("inf"), 2, ht, oc),
                 (r, 64, 0.001, 3, ht, oc), (r, 64, 0.001, 99, ht, oc)]:
        assert lib.rtx_cast_rays(h, *args) == RTX_ERR_INVALID, args
        assert lib.rtx_last_error().startswith(b"rtx_cast_rays:")
    assert lib.rtx_cast_rays(None, r, 64, 0.001, 1, ht, oc) == RTX_ERR_INVALID
    gpu_ctx.sync()
    assert untouched(d_hits.numpy()) and untouched(d_occ.numpy())
    assert lib.rtx_cast_rays(h, None, 0, 0.001, 1, None, None) == 0  # an empty batch needs no buffer
    with pytest.raises(rtx.RtxError):
        gpu_ctx.cast(d_rays, hits=False, occluded=False, n=64)
    got = gpu_ctx.cast(d_rays, order="auto", hits=d_hits, occluded=d_occ, n=64)
    gpu_ctx.sync()
    assert gpu_ctx.cast_last_order() in ORDERS
    assert_records(got[0].numpy(), want[:64], "auto")
    with rtx.Context(0) as fresh:
        assert fresh.cast_last_order() == "given"
        assert fresh._lib.rtx_cast_rays(fresh._h, r, 64, 0.001, 1, ht, oc) == RTX_ERR_STATE
        assert b"no world" in fresh._lib.rtx_last_error()
    for d in (d_rays, d_hits, d_occ):
        d.free()
