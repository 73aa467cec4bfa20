"""rtx_refine_rows: progressive refinement of a row part on one context.

A part's chain state covers its own rows only, and the refine kernel instances
(k_render<..., kRefine>, k_trace, promotion, the pre-pass cap's restart) run
over a part's rows, which fall into the small / low share classes. After steps
adding s1..sk every part's d_out must be, bit for bit (NaN == NaN), the
oracle's full frame at spp = s1 + ... + sk on the part's rows (part_row_ids),
and the parts' step segments must add up to the oracle's at N minus its count
at the previous N — on the product and the stress build, under the default
schedule and the tier-forcing ones, with pre-pass and with carried keys."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from refine_parts import assert_bits_equal, frame_of, oracle_at, world_of
from test_gpu_refine import TIER_SCHEDULES

pytestmark = pytest.mark.gpu

STRESS_LIB = os.path.join(os.path.dirname(GOLDEN), "..", "raytrace-we-gpu_amd", "lib", "variants",
                          "librtx_stress.so")
RTX_ERR_INVALID, RTX_ERR_STATE = -1, -3
W, H, T, PARTS = 160, 90, 4, 3
STEPS = (3, 9, 12)  # the exact grid (below 8 samples), then two scheduled launches
# k_trace with promotion at 1; k_trace in groups of 4; the pre-pass cap's restart (prepass_cap_split=6)
PART_SCHEDULES = TIER_SCHEDULES[1:4]


@pytest.fixture(scope="module")
def stress_ctx(rtx):
    """The stress build (make all): every list overflow and fallback path, a
    20 ms promotion valve and the kernarg layout check."""
    if not os.path.exists(STRESS_LIB):
        pytest.fail("stress build missing: make all")
    ctx = rtx.Context(0, lib=rtx.load_library(STRESS_LIB))
    yield ctx
    ctx.close()


def setup(ctx, rtx):
    frame = frame_of(rtx, W, H)
    ctx.upload_world(world_of(rtx))
    ctx.set_frame(frame)
    return frame


def run_parts(ctx, oracle, rtx, frame, what, schedule=None):
    """Every part through STEPS from a reset, on its own state: images against
    the oracle after every step; returns (segments[part][step],
    cost maps[part][step], last keys[part][step], exported states[part])."""
    assert sum(rtx.part_rows(H, T, p, PARTS) for p in range(PARTS)) == H
    segs, costs, keys, states = [], [], [], []
    for part in range(PARTS):
        ids = rtx.part_row_ids(H, T, part, PARTS)
        out = ctx.alloc((len(ids), W, 4))
        try:
            n, s_part, c_part, k_part = 0, [], [], []
            for i, s in enumerate(STEPS):
                if schedule is not None:
                    ctx.set_schedule()
                    ctx.set_schedule(**schedule)
                ctx.stats_reset()
                got_n = ctx.refine_rows(T, part, PARTS, s, reset=(i == 0), d_out=out.ptr)
                st = ctx.stats()
                n += s
                assert got_n == n == ctx.refined_samples
                assert ctx.refine_shape() == (T, part, PARTS)
                want, _ = oracle_at(oracle, rtx, frame, n)
                assert_bits_equal(out.numpy(), want[ids], f"{what}: part {part} after step {i} (N = {n})")
                assert st.samples == len(ids) * W * s and st.launches == 1
                s_part.append(st.segments)
                cost, covers = ctx.refine_cost()
                assert cost.shape == (len(ids), W) and covers == s
                assert int(cost.sum(dtype=np.uint64)) == st.segments  # the map's sum is the launch's segments
                c_part.append(cost)
                k_part.append(ctx.refine_last_keys)
            states.append(ctx.refine_export())
            assert states[-1].shape == (len(ids), W, 4)
        finally:
            out.free()
        segs.append(s_part)
        costs.append(c_part)
        keys.append(k_part)
    # the parts' step segments add up to the oracle's difference
    n, prev = 0, 0
    for i, s in enumerate(STEPS):
        n += s
        total = oracle_at(oracle, rtx, frame, n)[1]
        assert sum(segs[p][i] for p in range(PARTS)) == total - prev, f"{what}: step {i} segments"
        prev = total
    return segs, costs, keys, states


@pytest.mark.parametrize("ctx_name", ["gpu_ctx", "stress_ctx"])
def test_part_steps_equal_the_oracle_with_either_keys(request, oracle, rtx, ctx_name):
    ctx = request.getfixturevalue(ctx_name)
    frame = setup(ctx, rtx)
    try:
        ctx.set_refine_keys("prepass")
        _, cost_p, keys_p, _ = run_parts(ctx, oracle, rtx, frame, f"{ctx_name} prepass")
        ctx.set_refine_keys("carried")
        _, cost_c, keys_c, _ = run_parts(ctx, oracle, rtx, frame, f"{ctx_name} carried")
    finally:
        ctx.set_refine_keys("prepass")
    for part in range(PARTS):
        assert keys_p[part] == ["unscheduled", "prepass", "prepass"]
        assert keys_c[part][0] == "unscheduled" and keys_c[part][2] == "carried"
        for i in range(len(STEPS)):
            np.testing.assert_array_equal(cost_p[part][i], cost_c[part][i])


@pytest.mark.parametrize("ctx_name", ["gpu_ctx", "stress_ctx"])
def test_part_steps_under_the_tier_schedules(request, oracle, rtx, ctx_name):
    ctx = request.getfixturevalue(ctx_name)
    frame = setup(ctx, rtx)
    try:
        for sched in PART_SCHEDULES:
            run_parts(ctx, oracle, rtx, frame, f"{ctx_name} {sched}", sched)
    finally:
        ctx.set_schedule()


def test_part_states_gather_to_the_one_context_state(gpu_ctx, oracle, rtx):
    frame = setup(gpu_ctx, rtx)
    _, _, _, states = run_parts(gpu_ctx, oracle, rtx, frame, "states")
    whole = np.empty((H, W, 4), np.float32)
    for part in range(PARTS):
        whole[rtx.part_row_ids(H, T, part, PARTS)] = states[part]
    n = 0
    for i, s in enumerate(STEPS):
        n = gpu_ctx.refine(s, reset=(i == 0))
    assert n == sum(STEPS) and gpu_ctx.refine_shape() == (1, 0, 1)
    assert_bits_equal(whole, gpu_ctx.refine_export(), "gathered part states (sums and seeds)")


def test_shape_rules(gpu_ctx, rtx):
    """Another tile_rows or part restarts the state; every nparts == 1 shape is
    the whole frame's; a part without rows launches nothing and changes nothing."""
    setup(gpu_ctx, rtx)
    lib, h = gpu_ctx._lib, gpu_ctx._h
    out = gpu_ctx.alloc((H, W, 4))
    try:
        assert gpu_ctx.refine_rows(T, 0, PARTS, 3, reset=True, d_out=out.ptr) == 3
        assert gpu_ctx.refine_rows(T, 0, PARTS, 2, d_out=out.ptr) == 5
        assert gpu_ctx.refine_shape() == (T, 0, PARTS)
        assert gpu_ctx.refine_rows(T + 1, 0, PARTS, 2, d_out=out.ptr) == 2  # another tile_rows
        assert gpu_ctx.refine_shape() == (T + 1, 0, PARTS)
        assert gpu_ctx.refine_rows(T + 1, 1, PARTS, 2, d_out=out.ptr) == 2  # another part
        assert gpu_ctx.refine_rows(T + 1, 1, PARTS + 1, 2, d_out=out.ptr) == 2  # another nparts
        assert gpu_ctx.refine_shape() == (T + 1, 1, PARTS + 1)
        # a part that owns no rows: 90 rows in tiles of 64 are two tiles for three parts
        assert rtx.part_rows(H, 64, 2, 3) == 0
        gpu_ctx.stats_reset()
        assert gpu_ctx.refine_rows(64, 2, 3, 4, reset=True, d_out=out.ptr) == 2
        assert gpu_ctx.refine_shape() == (T + 1, 1, PARTS + 1) and gpu_ctx.stats().launches == 0
        # the whole frame, whatever tile_rows: one shape, continued by rtx_refine
        assert gpu_ctx.refine_rows(7, 0, 1, 3) == 3
        assert gpu_ctx.refine_shape() == (1, 0, 1)
        assert gpu_ctx.refine_rows(2, 0, 1, 2, d_out=out.ptr) == 5
        assert gpu_ctx.refine(1) == 6
        # refused before any launch
        gpu_ctx.stats_reset()
        assert lib.rtx_refine_rows(h, T, 0, PARTS, 2, 0, None) == RTX_ERR_INVALID  # d_out NULL, three parts
        assert lib.rtx_refine_rows(h, T, PARTS, PARTS, 2, 0, C.c_void_p(out.ptr)) == RTX_ERR_INVALID
        assert lib.rtx_refine_rows(h, T, 0, PARTS, 0, 0, C.c_void_p(out.ptr)) == RTX_ERR_INVALID
        assert gpu_ctx.refined_samples == 6 and gpu_ctx.stats().launches == 0
        with rtx.Context(0) as fresh:
            t = C.c_uint32(0)
            assert lib.rtx_refine_shape(fresh._h, C.byref(t), None, None) == RTX_ERR_STATE
            assert lib.rtx_refine_rows(fresh._h, T, 0, PARTS, 2, 0, C.c_void_p(out.ptr)) == RTX_ERR_STATE  # no world
    finally:
        out.free()


def test_import_rows_continues_the_part(gpu_ctx, oracle, rtx):
    """refine_import_rows of an exported part, continued by 8 samples, equals
    the uninterrupted run (and the oracle at N + 8)."""
    frame = setup(gpu_ctx, rtx)
    part = 1
    ids = rtx.part_row_ids(H, T, part, PARTS)
    out = gpu_ctx.alloc((len(ids), W, 4))
    try:
        gpu_ctx.refine_rows(T, part, PARTS, 3, reset=True, d_out=out.ptr)
        assert gpu_ctx.refine_rows(T, part, PARTS, 9, d_out=out.ptr) == 12
        img12, state = out.numpy(), gpu_ctx.refine_export()
        assert gpu_ctx.refine_rows(T, part, PARTS, 8, d_out=out.ptr) == 20
        img20 = out.numpy()
    finally:
        out.free()
    assert_bits_equal(img20, oracle_at(oracle, rtx, frame, 20)[0][ids], "uninterrupted 3 + 9 + 8")
    with rtx.Context(0) as b:
        b.upload_world(world_of(rtx))
        b.set_frame(frame)
        outb = b.alloc((len(ids), W, 4))
        try:
            b.stats_reset()
            b.refine_import_rows(T, part, PARTS, state, 12, d_out=outb.ptr)
            assert b.refined_samples == 12 and b.refine_shape() == (T, part, PARTS)
            assert_bits_equal(outb.numpy(), img12, "imported part's image")
            assert b.stats().launches == 0
            lib, fp = b._lib, state.ctypes.data_as(C.POINTER(C.c_float))
            assert lib.rtx_refine_import_rows(b._h, T, part, PARTS, fp, state.nbytes - 16, 12,
                                              C.c_void_p(outb.ptr)) == RTX_ERR_INVALID
            assert b.refined_samples == 12
            assert b.refine_rows(T, part, PARTS, 8, d_out=outb.ptr) == 20
            assert_bits_equal(outb.numpy(), img20, "12 imported + 8")
            # no image without d_out; the state is installed all the same
            b.refine_import_rows(T, part, PARTS, state, 12)
            assert b.refined_samples == 12
            assert_bits_equal(b.refine_export(), state, "re-exported part state")
        finally:
            outb.free()


def test_adaptive_entry_points_refuse_a_part_state(gpu_ctx, rtx):
    setup(gpu_ctx, rtx)
    lib, h = gpu_ctx._lib, gpu_ctx._h
    out = gpu_ctx.alloc((H, W, 4))
    try:
        assert gpu_ctx.refine_rows(T, 0, PARTS, 8, reset=True, d_out=out.ptr) == 8
    finally:
        out.free()
    gpu_ctx.stats_reset()
    n = C.c_uint32(0)
    buf = np.empty((H, W), np.uint32)
    for rc in (lib.rtx_refine_adaptive(h, 8, 0.1, 0, 0, C.byref(n)),
               lib.rtx_refine_pending(h, 8, 0.1, 0, C.byref(n)),
               lib.rtx_refine_counts(h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), buf.nbytes),
               lib.rtx_refine_error(h, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.nbytes)):
        assert rc == RTX_ERR_STATE
        assert b"row part" in lib.rtx_last_error()
    assert gpu_ctx.stats().launches == 0 and gpu_ctx.refined_samples == 8
    # with reset it starts its whole-frame state, as before
    assert gpu_ctx.refine_adaptive(8, 0.1, reset=True) == W * H
    assert gpu_ctx.refine_shape() == (1, 0, 1) and gpu_ctx.refined_samples == 8
    assert gpu_ctx.refine_counts().shape == (H, W)
