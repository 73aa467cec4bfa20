"""rtx_trace_paths_keyed on the GPU: path queries in cost order, by the
library's probe or by the caller's keys.

The order is a schedule and nothing else, so every test ends in "the records
— sums, end seeds, per-query segment counts — are, bit for bit, what
trace_paths(order="given") writes", and the sums are the CPU oracle's. Worlds,
recipes and expectations are test_gpu_paths.py's (its cache is shared): rtiow11
is 48 rays x 32 seeds = 1,536 queries, rw25 16 x 32 = 512, 6 samples, depth 8.
Output buffers hold a byte pattern before each call and are 16 records longer
than the batch, so a record that was not written, or one written past the end,
shows. That the schedule is applied at all is seen through paths_order()
(rtx_debug_paths_order): the permutation the last keyed call ran.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import hostile_cases as hc
import paths_cases as pc
import regime_cases as rc
from test_gpu_parity import assert_bits_equal
from test_gpu_paths import (CLI, CONTINUE, FILL, PER, RECIPES, RTX_ERR_INVALID, RTX_ERR_STATE, SLACK, _EXPECT,
                            case_of, expectation, filled, stress_ctx, trace, untouched, upload)  # noqa: F401

pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
COST = 3   # RTX_PATHS_ORDER_COST
KEY_MAX = 65535


def keyed(ctx, queries, samples=pc.SAMPLES, n=None, keys=None, probe=0, flags=0, start=None, segments=True):
    """rtx_trace_paths_keyed on device buffers, as test_gpu_paths.trace calls
    rtx_trace_paths: the first n rows of `queries` into pre-filled buffers of
    n + SLACK records (keys: None, or (n,) uint32 uploaded to a buffer of its
    own; start: the records a continuing call begins from). Returns (results,
    segments) after checking that nothing beyond record n - 1 was written and
    every record before it was."""
    queries = np.ascontiguousarray(queries, f32).reshape(-1, 8)
    n = len(queries) if n is None else n
    d_q = ctx.alloc((max(len(queries), 1), 8))
    d_r = filled(ctx, n + SLACK, np.dtype([("v", "<f4", (4,))]))
    d_s = filled(ctx, n + SLACK, np.uint32) if segments else None
    d_k = None
    try:
        if len(queries):
            d_q.upload(queries)
        if keys is not None:
            d_k = filled(ctx, n + SLACK, np.uint32)
            pad = d_k.numpy()
            pad[:n] = keys
            d_k.upload(pad)
        if start is not None:
            keep = d_r.numpy()
            keep["v"][:n] = start
            d_r.upload(keep)
        got = ctx.trace_paths_keyed(d_q, samples, keys=d_k, probe=probe, flags=flags, results=d_r,
                                    segments=d_s if segments else False, n=n)
        assert got[0] is d_r and got[1] is d_s
        ctx.sync()
        res = d_r.numpy()["v"]
        seg = d_s.numpy() if segments else None
        what = f"n = {n}, keyed"
        assert untouched(res[n:]) and (seg is None or untouched(seg[n:])), f"{what}: a record past the batch was written"
        if start is None:
            assert not (res[:n].view(np.uint8).reshape(n, 16) == FILL).all(1).any(), f"{what}: a result was not written"
        assert seg is None or not (seg[:n] == u32(0xA5A5A5A5)).any(), f"{what}: a segment count was not written"
        if d_k is not None:  # the keys are read, never written
            assert (d_k.numpy()[:n] == np.asarray(keys, u32)).all() and untouched(d_k.numpy()[n:])
        return np.array(res[:n]), (None if seg is None else np.array(seg[:n]))
    finally:
        for d in (d_q, d_r, d_s, d_k):
            if d is not None:
                d.free()


def same_records(got, want, what):
    assert_bits_equal(got[0], want[0], f"{what}: sums and seeds")
    assert (got[1] == want[1]).all(), f"{what}: segments per query"


def check_order(ctx, keys, n, what):
    """paths_order() is a permutation of 0 .. n-1 along which min(key, 65535)
    does not increase."""
    perm = ctx.paths_order()
    assert perm.dtype == u32 and perm.shape == (n,)
    assert (np.sort(perm) == np.arange(n)).all(), f"{what}: not a permutation"
    ck = np.minimum(np.asarray(keys, np.uint64), KEY_MAX)[perm]
    assert (ck[:-1] >= ck[1:]).all(), f"{what}: keys increase along the order"
    return perm


def order_state(ctx, n):
    buf = np.zeros(max(n, 1), u32)
    return ctx._lib.rtx_debug_paths_order(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), 4 * n)


# ---------------------------------------------------------------------------
# the probed order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("test_world", "auto"), ("rtiow11", "auto"), ("rw25", "auto"), ("rw25", "linear")])
def test_probed_order_equals_given(gpu_ctx, oracle, rtx, name, mode):
    """The default probe (2 samples; 1 above 1,024 padded spheres): the small
    classes, the culled scan and the large linear scan."""
    e = expectation(oracle, name)
    try:
        upload(gpu_ctx, rtx, case_of(oracle, name), mode=mode)
        if name == "rw25":
            assert gpu_ctx.scene_info()["kernels"] == (1 if mode == "auto" else 2)
        # the keys the library will use: its probe's segment counts
        probe_segs = trace(gpu_ctx, e.rays, 1 if name == "rw25" else 2)[1]
        want = trace(gpu_ctx, e.rays)
        assert gpu_ctx.paths_last_order() == "given"
        got = keyed(gpu_ctx, e.rays)
        assert gpu_ctx.paths_last_order() == "cost"
        assert_bits_equal(got[0][:, :3], e.sums, f"{name}, {mode}: sums against the oracle")
        assert (got[1].reshape(-1, e.per).sum(1) == e.twin_segs).all(), f"{name}, {mode}: segments per twin"
        same_records(got, want, f"{name}, {mode}, probed")
        check_order(gpu_ctx, probe_segs, len(e.rays), f"{name}, {mode}")
    finally:
        gpu_ctx.set_scan_mode("auto")


def test_probed_order_on_the_stress_build(stress_ctx, oracle, rtx):
    e = expectation(oracle, "rtiow11")
    upload(stress_ctx, rtx, case_of(oracle, "rtiow11"))
    want = trace(stress_ctx, e.rays)
    got = keyed(stress_ctx, e.rays)
    assert stress_ctx.paths_last_order() == "cost"
    assert_bits_equal(got[0][:, :3], e.sums, "stress build: sums against the oracle")
    same_records(got, want, "stress build, probed")


@pytest.mark.parametrize("probe,ran", [(1, "cost"), (5, "cost"), (6, "given"), (7, "given")])
def test_probe_sizes(gpu_ctx, oracle, rtx, probe, ran):
    """probe = 1 and samples - 1 sort; with samples <= probe the call is one
    plain launch in the given order and says so."""
    e = expectation(oracle, "rtiow11")
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    want = trace(gpu_ctx, e.rays, order="coherent")  # (and paths_last_order is not "given" or "cost" before the call)
    got = keyed(gpu_ctx, e.rays, probe=probe)
    assert gpu_ctx.paths_last_order() == ran
    assert_bits_equal(got[0][:, :3], e.sums, f"probe = {probe}: sums against the oracle")
    same_records(got, want, f"probe = {probe}")
    assert order_state(gpu_ctx, len(e.rays)) == (0 if ran == "cost" else RTX_ERR_STATE)


# ---------------------------------------------------------------------------
# the caller's keys
# ---------------------------------------------------------------------------
def key_sets(n, seg6):
    return {"segments": seg6, "zeros": np.zeros(n, u32), "ones": np.full(n, 0xFFFFFFFF, u32),
            "random": np.random.default_rng(4242).integers(0, 1 << 32, n, dtype=np.uint64).astype(u32),
            "arange": np.arange(n, dtype=u32), "reversed": np.arange(n, dtype=u32)[::-1].copy()}


@pytest.mark.parametrize("which", ["segments", "zeros", "ones", "random", "arange", "reversed"])
def test_callers_keys(gpu_ctx, oracle, rtx, which):
    """Any keys give the given order's records: a 6-sample call's segments, all
    0, all 0xFFFFFFFF, seeded random words, arange(n) and its reverse."""
    e = expectation(oracle, "rtiow11")
    n = len(e.rays)
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    want = trace(gpu_ctx, e.rays)
    keys = key_sets(n, want[1])[which]
    got = keyed(gpu_ctx, e.rays, keys=keys)
    assert gpu_ctx.paths_last_order() == "cost"
    assert_bits_equal(got[0][:, :3], e.sums, f"keys {which}: sums against the oracle")
    same_records(got, want, f"keys {which}")
    perm = check_order(gpu_ctx, keys, n, f"keys {which}")
    if which == "reversed":  # distinct keys below 65,536 fix the order: already longest first
        assert (perm == np.arange(n)).all()
    if which == "arange":
        assert (perm == np.arange(n)[::-1]).all()


def test_the_schedule_is_applied(gpu_ctx, oracle, rtx):
    """paths_order() after the probed call and after the segments-keyed call:
    a permutation with the keys non-increasing, the keys taking at least 3
    values; RTX_ERR_STATE once a coherent cast or a plain trace_paths has come
    between."""
    e = expectation(oracle, "rtiow11")
    n = len(e.rays)
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    _, seg2 = trace(gpu_ctx, e.rays, 2)
    _, seg6 = trace(gpu_ctx, e.rays)
    assert len(np.unique(np.minimum(seg2, KEY_MAX))) >= 3 and len(np.unique(np.minimum(seg6, KEY_MAX))) >= 3
    assert order_state(gpu_ctx, n) == RTX_ERR_STATE  # the last path call did not sort by cost

    keyed(gpu_ctx, e.rays)
    perm = check_order(gpu_ctx, seg2, n, "probed")
    assert (perm != np.arange(n)).any()  # (the batch is not in cost order as given)
    assert (check_order(gpu_ctx, seg2, n, "probed, read again") == perm).all()
    assert order_state(gpu_ctx, n + 1) == RTX_ERR_INVALID and b"bytes" in gpu_ctx._lib.rtx_last_error()
    rays = np.ascontiguousarray(e.rays[:64]).copy()
    rays[:, 3] = 1e30  # t_max
    gpu_ctx.cast(rays, order="coherent")
    assert gpu_ctx.cast_last_order() == "coherent"
    assert order_state(gpu_ctx, n) == RTX_ERR_STATE and b"rtx_debug_paths_order" in gpu_ctx._lib.rtx_last_error()
    with pytest.raises(rtx.RtxError):
        gpu_ctx.paths_order()

    keyed(gpu_ctx, e.rays, keys=seg6)
    check_order(gpu_ctx, seg6, n, "keyed by segments")
    gpu_ctx.cast(rays, order="given")  # sorts nothing, reuses nothing
    check_order(gpu_ctx, seg6, n, "after a cast in the given order")
    trace(gpu_ctx, e.rays[:64], 2)
    assert order_state(gpu_ctx, n) == RTX_ERR_STATE
    keyed(gpu_ctx, e.rays, keys=seg6)
    trace(gpu_ctx, e.rays[:64], 2, order="coherent")
    assert order_state(gpu_ctx, n) == RTX_ERR_STATE


# ---------------------------------------------------------------------------
# batch edges, keys in place, continuing
# ---------------------------------------------------------------------------
def test_batch_edges(gpu_ctx, oracle, rtx):
    """n = 1, 63, 64, 65, 257 as prefixes; 2,049 and 3,072 from the queries
    tiled twice, across the sort's 2,048 records per workgroup. Probed and
    keyed."""
    e = expectation(oracle, "rtiow11")
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    rays, sums = np.tile(e.rays, (2, 1)), np.tile(e.sums, (2, 1))
    full = trace(gpu_ctx, rays)
    for n in (1, 63, 64, 65, 257, 2049, 3072):
        for how, kw in (("probed", {}), ("keyed", {"keys": full[1][:n]})):
            got = keyed(gpu_ctx, rays, n=n, **kw)
            assert gpu_ctx.paths_last_order() == "cost"
            assert_bits_equal(got[0][:, :3], sums[:n], f"n = {n}, {how}")
            same_records(got, (full[0][:n], full[1][:n]), f"n = {n}, {how}")
            if how == "keyed":
                check_order(gpu_ctx, full[1][:n], n, f"n = {n}")


def test_keys_in_place(gpu_ctx, oracle, rtx):
    """keys is segments: after a 2-sample call a keyed continuing call of 4
    with d_keys == d_segments gives the 6-sample records; segments then holds
    the continuing call's own counts, seg2 + seg4 == seg6, and the order was
    seg2's."""
    e = expectation(oracle, "rtiow11")
    n = len(e.rays)
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    whole, seg6 = trace(gpu_ctx, e.rays)
    d_q = gpu_ctx.alloc((n, 8))
    d_q.upload(np.ascontiguousarray(e.rays))
    d_r = filled(gpu_ctx, n + SLACK, np.dtype([("v", "<f4", (4,))]))
    d_s = filled(gpu_ctx, n + SLACK, np.uint32)
    try:
        gpu_ctx.trace_paths(d_q, 2, order="given", results=d_r, segments=d_s, n=n)
        gpu_ctx.sync()
        seg2 = np.array(d_s.numpy()[:n])
        gpu_ctx.trace_paths_keyed(d_q, 4, keys=d_s, results=d_r, segments=d_s, cont=True, n=n)
        gpu_ctx.sync()
        assert gpu_ctx.paths_last_order() == "cost"
        res, seg4 = d_r.numpy()["v"], d_s.numpy()
        assert untouched(res[n:]) and untouched(seg4[n:])
        assert_bits_equal(res[:n], whole, "2 + 4 samples, keys in place: sums and seeds")
        assert (seg2 + seg4[:n] == seg6).all(), "segments hold the continuing call's own counts"
        check_order(gpu_ctx, seg2, n, "keys in place")
    finally:
        for d in (d_q, d_r, d_s):
            d.free()


def test_continue(gpu_ctx, oracle, rtx):
    """2 samples, then a probed-order continuing call of 4 with the query
    seeds scrubbed to NaN, equals one call of 6; the call reports its own
    segments, the probe's included."""
    e = expectation(oracle, "rtiow11")
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    whole, seg6 = trace(gpu_ctx, e.rays)
    first, seg2 = trace(gpu_ctx, e.rays, 2)
    scrubbed = np.array(e.rays)
    scrubbed[:, 3] = np.nan
    for probe in (0, 1, 3):
        rest, seg4 = keyed(gpu_ctx, scrubbed, 4, probe=probe, flags=CONTINUE, start=first)
        assert gpu_ctx.paths_last_order() == "cost"
        assert_bits_equal(rest, whole, f"2 + 4 samples, probe {probe}: sums and seeds")
        assert (seg2 + seg4 == seg6).all(), "a continuing call reports its own segments"
    rest, _ = keyed(gpu_ctx, scrubbed, 4, flags=CONTINUE, start=first, segments=False)
    assert_bits_equal(rest, whole, "2 + 4 samples, no segment buffer")


def test_hostile_rays(gpu_ctx, oracle, rtx):
    """The zero-direction and NaN-target queries of test_gpu_paths'
    test_hostile_rays, probed: the given order's records."""
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
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    want = trace(gpu_ctx, e.rays)
    for kw in ({}, {"probe": 1}, {"keys": want[1]}):
        got = keyed(gpu_ctx, e.rays, **kw)
        assert gpu_ctx.paths_last_order() == "cost"
        assert_bits_equal(got[0][:, :3], e.sums, f"hostile rays, {kw and list(kw)}: sums against the oracle")
        same_records(got, want, f"hostile rays, {kw and list(kw)}")
    # the hostile queries are as long as a query can be (every sample runs to the depth): such queries lead the order
    assert (want[1][PER:3 * PER] == pc.SAMPLES * pc.DEPTH).all()
    perm = check_order(gpu_ctx, want[1], len(e.rays), "hostile rays")
    assert (want[1][perm[:2 * PER]] == pc.SAMPLES * pc.DEPTH).all()


# ---------------------------------------------------------------------------
# no side effects, refusals
# ---------------------------------------------------------------------------
def test_touches_nothing_else(gpu_ctx, oracle, rtx):
    """After a frame and two refine steps: the stats, the framebuffer, the
    chain state, its sample count, the cost map and the cast order are the same
    after probed and keyed path queries, and the next refine step continues the
    chain as if nothing had happened."""
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
    got = keyed(gpu_ctx, e.rays)
    assert_bits_equal(got[0][:, :3], e.sums, "between refine steps, probed")
    got = keyed(gpu_ctx, e.rays, keys=got[1])
    assert_bits_equal(got[0][:, :3], e.sums, "between refine steps, keyed")
    after = snapshot()
    for k, (a, b) in enumerate(zip(before, after)):
        assert a == b, f"snapshot item {k} changed"
    assert gpu_ctx.refine(3) == 12
    case = hc.Case(world.spheres, world.mat_types, world.mat_values, pc.DEPTH, 12)
    img, _ = oracle.render_rows(case, frame, np.arange(rc.H), nthreads=min(8, os.cpu_count() or 1))
    assert_bits_equal(gpu_ctx.download(), img, "refine(5) + refine(4) + keyed path queries + refine(3)")


def test_refusals(gpu_ctx, oracle, rtx):
    lib, h = gpu_ctx._lib, gpu_ctx._h
    e = expectation(oracle, "rtiow11", rays=16)
    case = case_of(oracle, "rtiow11")
    d_q = gpu_ctx.alloc((64, 8))
    d_q.upload(np.ascontiguousarray(e.rays[:64]))
    d_r, d_s, d_k = (filled(gpu_ctx, 64, rtx.PATH_RESULT_DTYPE), filled(gpu_ctx, 64, np.uint32),
                     filled(gpu_ctx, 64, np.uint32))
    q, r, s, k = (C.c_void_p(d.ptr) for d in (d_q, d_r, d_s, d_k))
    with rtx.Context(0) as fresh:  # no world
        assert fresh._lib.rtx_trace_paths_keyed(fresh._h, q, 64, 6, 0, None, 0, r, s) == RTX_ERR_STATE
        assert b"no world" in fresh._lib.rtx_last_error()
        assert order_state(fresh, 64) == RTX_ERR_STATE
    upload(gpu_ctx, rtx, case, depth=0)
    assert lib.rtx_trace_paths_keyed(h, q, 64, 6, 0, None, 0, r, s) == RTX_ERR_INVALID
    assert b"depth is 0" in lib.rtx_last_error()
    upload(gpu_ctx, rtx, case, depth=65536)
    assert lib.rtx_trace_paths_keyed(h, q, 64, 65536, 0, k, 0, r, s) == RTX_ERR_INVALID
    assert b"32 bits" in lib.rtx_last_error()
    upload(gpu_ctx, rtx, case)
    for args in [(None, 64, 6, 0, None, 0, r, s), (q, 64, 6, 0, None, 0, None, s), (q, 64, 0, 0, None, 0, r, s),
                 (q, 64, 6, 4, None, 0, r, s), (q, 64, 6, 0, k, 2, r, s)]:
        assert lib.rtx_trace_paths_keyed(h, *args) == RTX_ERR_INVALID, args
        assert lib.rtx_last_error().startswith(b"rtx_trace_paths_keyed:")
    assert lib.rtx_trace_paths(h, q, 64, 6, 0, COST, r, s) == RTX_ERR_INVALID  # no order of the plain entry point
    assert lib.rtx_trace_paths_keyed(h, None, 0, 6, 0, None, 0, None, None) == 0  # an empty batch: no buffer, no launch
    assert lib.rtx_trace_paths_keyed(h, None, 0, 6, 0, k, 0, None, None) == 0
    with pytest.raises(rtx.RtxError):
        gpu_ctx.trace_paths_keyed(d_q, 6, cont=True, n=64)  # nothing to continue from
    gpu_ctx.sync()
    assert untouched(d_r.numpy()) and untouched(d_s.numpy()) and untouched(d_k.numpy())
    assert lib.rtx_trace_paths_keyed(h, q, 64, 6, 0, None, 0, r, None) == 0  # segments are optional
    gpu_ctx.sync()
    assert gpu_ctx.paths_last_order() == "cost"
    assert_bits_equal(d_r.numpy().view(f32).reshape(64, 4)[:, :3], e.sums[:64], "no segment buffer")
    assert untouched(d_s.numpy())
    for d in (d_q, d_r, d_s, d_k):
        d.free()


# ---------------------------------------------------------------------------
# numpy in and out, the command line
# ---------------------------------------------------------------------------
def test_numpy_in_and_out(gpu_ctx, oracle, rtx):
    e = expectation(oracle, "rtiow11", rays=16)
    upload(gpu_ctx, rtx, case_of(oracle, "rtiow11"))
    want, want_seg = gpu_ctx.trace_paths(np.array(e.rays), pc.SAMPLES, order="given", segments=True)
    for host in (np.array(e.rays), np.array(e.rays).view(rtx.PATH_QUERY_DTYPE).reshape(-1)):
        res, seg = gpu_ctx.trace_paths_keyed(host, pc.SAMPLES, segments=True)
        assert res.dtype == rtx.PATH_RESULT_DTYPE and seg.dtype == np.uint32 and len(res) == len(seg) == len(e.rays)
        assert_bits_equal(res["sum"], e.sums, "numpy in and out")
        assert_bits_equal(res["seed"], want["seed"], "numpy in and out: seeds")
        assert (seg == want_seg).all()
    assert gpu_ctx.paths_last_order() == "cost" and len(gpu_ctx.paths_order()) == len(e.rays)
    res, seg = gpu_ctx.trace_paths_keyed(np.array(e.rays), pc.SAMPLES, keys=want_seg)
    assert seg is None
    assert_bits_equal(res["sum"], e.sums, "numpy keys")
    first, _ = gpu_ctx.trace_paths(np.array(e.rays), 2)
    rest, _ = gpu_ctx.trace_paths_keyed(np.array(e.rays), 4, results=first, cont=True)
    assert_bits_equal(rest["sum"], want["sum"], "numpy, continued")
    assert_bits_equal(rest["seed"], want["seed"], "numpy, continued: seeds")
    with pytest.raises(rtx.RtxError):
        gpu_ctx.trace_paths_keyed(np.array(e.rays), 4, keys=want_seg[:5])
    assert gpu_ctx.trace_paths_keyed(np.zeros((0, 8), f32), 3)[0].shape == (0,)


def test_cli_round_trip(tmp_path, oracle, rtx):
    """rtx_cli --paths Q.bin --samples 6 with and without --paths-order cost,
    and with --paths-keys: the same result and segment files, byte for byte."""
    e = expectation(oracle, "rtiow11")
    n = 256
    src = str(tmp_path / "q.bin")
    np.asarray(e.rays[:n]).tofile(src)
    runs = {"given": [], "cost": ["--paths-order", "cost"], "probe1": ["--paths-order", "cost", "--paths-probe", "1"],
            "keys": ["--paths-keys", str(tmp_path / "s_given.bin")]}
    for name, more in runs.items():
        dst, sg = str(tmp_path / f"r_{name}.bin"), str(tmp_path / f"s_{name}.bin")
        out = subprocess.run([CLI, "--scene", "rtiow11", "--width", "64", "--height", "36", "--depth", str(pc.DEPTH),
                              "--paths", src, "--results", dst, "--segments", sg, "--samples", str(pc.SAMPLES)] + more,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        rep = json.loads(out.stdout.strip().splitlines()[-1])["paths"]
        assert rep["queries"] == n and rep["samples"] == pc.SAMPLES
        assert rep["order"] == ("given" if name == "given" else "cost") and rep["continued"] is False
        assert rep["segments"] == int(np.fromfile(sg, np.uint32).sum())
    given = np.fromfile(str(tmp_path / "r_given.bin"), rtx.PATH_RESULT_DTYPE)
    assert_bits_equal(given["sum"], e.sums[:n], "rtx_cli --paths")
    for name in ("cost", "probe1", "keys"):
        for kind in "rs":
            assert open(tmp_path / f"{kind}_{name}.bin", "rb").read() == open(tmp_path / f"{kind}_given.bin", "rb").read(), \
                f"--paths {name}: file {kind}"
    bad = subprocess.run([CLI, "--scene", "rtiow11", "--paths", src, "--samples", "2", "--results", str(tmp_path / "x.bin"),
                          "--paths-keys", str(tmp_path / "s_given.bin"), "--paths-probe", "2"], capture_output=True,
                         text=True, timeout=120)
    assert bad.returncode == 2 and "--paths-probe" in bad.stderr
