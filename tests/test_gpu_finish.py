"""Where a pixel is finished ("the coalesced image").

A cost-ordered launch stages every pixel by queue slot as its linear sample
sum with the launch's tag in w; k_unpermute (k_unpermute_adaptive) divides by
the launch's divisor, applies the gamma and writes the framebuffer in pixel
order. A pixel without a slot (a promoted one) is finished by whoever ends it,
straight into the framebuffer. These tests pin every divisor and every writer
of the staging image at the smallest shapes that take each path; every
comparison is against the fp32 oracle, bit for bit (NaN == NaN), zero
differing values.

The launch does not report how many pixels it promoted (rtx_stats has no such
count), so the promotion tests rely on the threshold of 1 projected segment
that tests/test_gpu_parity.py uses for the same purpose: every lane that
reaches a sample boundary after its queue ran dry hands its pixel over.
"""
import numpy as np
import pytest

from test_gpu_parity import assert_bits_equal
from test_gpu_refine import oracle_at, run_steps
from test_gpu_refine_adaptive import INF, check_shares, plan, run_plan

pytestmark = pytest.mark.gpu

DEPTH = 16
SENTINEL = np.float32(-7.0)  # no pixel of a frame is negative: an unwritten pixel shows
PROMOTE_ALL = dict(promote_small=1, promote_low=1, promote_medium=1, promote_large=1)
TRACE = dict(trace_small=0.3, trace_low=0.3, trace_medium=0.3, trace_large=0.3)

_WANT = {}


def oracle_frame(oracle, world, frame, key):
    """The oracle's frame and segment count, once per input, never modified."""
    if key not in _WANT:
        img, segs = oracle.render_rows(world, frame, np.arange(frame.height), nthreads=8)
        img.setflags(write=False)
        _WANT[key] = (img, segs)
    return _WANT[key]


def render_into_sentinel(ctx, rows, width, tile_rows, part, nparts):
    """render_rows of one part into a buffer that held SENTINEL everywhere."""
    buf = ctx.alloc((rows, width, 4))
    buf.upload(np.full((rows, width, 4), SENTINEL, np.float32))
    ctx.stats_reset()
    ctx.render_rows(tile_rows, part, nparts, buf.ptr)
    st = ctx.stats()
    got = buf.numpy()
    buf.free()
    return got, st


@pytest.mark.parametrize("spp", [8, 10])
@pytest.mark.parametrize("w,h", [(160, 90), (150, 70)])
def test_whole_frame_scheduled(gpu_ctx, oracle, rtx, w, h, spp):
    """The scheduled path's whole frame: spp 8 is the smallest that takes it,
    spp 10 a divisor that is no power of two; 150x70 has partial 16x16 queue
    tiles and unused slots. Every row, and the segment count."""
    world = rtx.random_world(11, depth=DEPTH, spp=spp)
    assert world.count == 486
    frame = rtx.camera_look_at(w, h, aspect=w / h)
    gpu_ctx.set_schedule()
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    want, segs = oracle_frame(oracle, world, frame, ("frame", w, h, spp))
    got, st = render_into_sentinel(gpu_ctx, h, w, 1, 0, 1)
    assert_bits_equal(got, want, f"{w}x{h} spp {spp}")
    assert st.segments == segs


@pytest.mark.parametrize("sched", [dict(), TRACE], ids=["default", "k_trace"])
def test_row_parts(gpu_ctx, oracle, rtx, sched):
    """160x90 in 5-row tiles over 3 parts, every part: k_trace finishes tier-1
    pixels beside k_render through the same staging image (default schedule,
    and k_trace given 30 % of the waves in every share class)."""
    W, H, T, R, spp = 160, 90, 5, 3, 10
    world = rtx.random_world(11, depth=DEPTH, spp=spp)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    want, segs = oracle_frame(oracle, world, frame, ("frame", W, H, spp))
    gpu_ctx.set_schedule()
    try:
        gpu_ctx.set_schedule(**sched)
        total = 0
        for part in range(R):
            ids = rtx.part_row_ids(H, T, part, R)
            got, st = render_into_sentinel(gpu_ctx, len(ids), W, T, part, R)
            assert_bits_equal(got, want[ids], f"part {part} of {R}")
            total += st.segments
        assert total == segs
    finally:
        gpu_ctx.set_schedule()


@pytest.mark.parametrize("sched", [PROMOTE_ALL, dict(PROMOTE_ALL, **TRACE)], ids=["render-serves", "k_trace-serves"])
def test_promoted_pixels(gpu_ctx, oracle, rtx, sched):
    """Promotion threshold 1: a promoted pixel's slot is zeroed and its server
    finishes it straight into the framebuffer. The frame (whole, and one of
    two parts) over a buffer of sentinels must be the oracle's: no pixel left
    unwritten, none replaced by its zeroed slot; the segment count says that
    none was traced twice. Then the same launch accumulating: a pixel finished
    twice would add its sum to the accumulator twice."""
    W, H, T, spp = 160, 90, 5, 10
    world = rtx.random_world(11, depth=DEPTH, spp=spp)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    want, segs = oracle_frame(oracle, world, frame, ("frame", W, H, spp))
    gpu_ctx.set_schedule()
    try:
        gpu_ctx.set_schedule(**sched)
        got, st = render_into_sentinel(gpu_ctx, H, W, 1, 0, 1)
        assert_bits_equal(got, want, "whole frame")
        assert st.segments == segs
        ids = rtx.part_row_ids(H, T, 1, 2)
        got, _ = render_into_sentinel(gpu_ctx, len(ids), W, T, 1, 2)
        assert_bits_equal(got, want[ids], "part 1 of 2")
        assert gpu_ctx.accumulate(reset=True) == 1
        assert_bits_equal(gpu_ctx.download(), want, "first accumulated frame")
    finally:
        gpu_ctx.set_schedule()


@pytest.mark.parametrize("sched", [dict(), PROMOTE_ALL], ids=["default", "promote"])
def test_progressive_accumulation(gpu_ctx, oracle, rtx, sched):
    """Three frames into one accumulator at 96x54, spp 8 (the scheduled path):
    frame k's image is toGamma(sum over frames / ((k + 1) * spp)) of the
    oracle's linear sums, added in fp32 frame by frame."""
    W, H, spp = 96, 54, 8
    world = rtx.random_world(11, depth=DEPTH, spp=spp)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    gpu_ctx.set_schedule()
    try:
        gpu_ctx.set_schedule(**sched)
        total = np.zeros((H, W, 3), np.float32)
        for k in range(3):
            assert gpu_ctx.accumulate(reset=(k == 0)) == k + 1
            key = ("linear", W, H, spp, k)
            if key not in _WANT:
                f = rtx.camera_look_at(W, H, aspect=W / H)
                f.frame_index = k
                _WANT[key] = oracle.render_rows_linear(world, f, np.arange(H), nthreads=8)[0][..., :3].copy()
            total = total + _WANT[key]
            mean = (total / np.float32((k + 1) * spp)).astype(np.float32)
            want = np.ones((H, W, 4), np.float32)
            want[..., :3] = oracle.math("pow", mean.ravel(), np.full(mean.size, 0.454545454545, np.float32)).reshape(mean.shape)
            assert_bits_equal(gpu_ctx.download(), want, f"accumulated frame {k + 1}")
    finally:
        gpu_ctx.set_schedule()


def test_tags_second_launch_replaces_first(gpu_ctx, oracle, rtx):
    """Two launches into the same image buffer with different cameras: the
    second image is the oracle's second frame everywhere (no pixel of the
    first survives, no slot moves under another launch's tag), and rendering
    the first again gives the first again."""
    W, H, spp = 96, 54, 8
    world = rtx.random_world(11, depth=DEPTH, spp=spp)
    cams = [rtx.camera_look_at(W, H, aspect=W / H),
            rtx.camera_look_at(W, H, look_from=(-9.0, 3.0, 8.0), aspect=W / H)]
    wants = [oracle_frame(oracle, world, f, ("cam", W, H, spp, i))[0] for i, f in enumerate(cams)]
    assert not (wants[0].view(np.uint32) == wants[1].view(np.uint32))[..., :3].all(axis=-1).all()
    gpu_ctx.set_schedule()
    gpu_ctx.upload_world(world)
    buf = gpu_ctx.alloc((H, W, 4))
    buf.upload(np.full((H, W, 4), SENTINEL, np.float32))
    try:
        for i in (0, 1, 0):
            gpu_ctx.set_frame(cams[i])
            gpu_ctx.render_rows(1, 0, 1, buf.ptr)
            assert_bits_equal(buf.numpy(), wants[i], f"camera {i}")
    finally:
        buf.free()


@pytest.mark.parametrize("ext,scan", [(13, "auto"), (17, "auto"), (17, "linear")])
def test_larger_scene_instances(gpu_ctx, oracle, rtx, ext, scan):
    """The other render instances stage too: a scene above the coop's LDS
    copy (extent 13: 678 spheres), and one above 1,024 spheres in the culled
    and the linear scan mode. 96x54, spp 8, a handful of rows."""
    W, H, spp = 96, 54, 8
    world = rtx.random_world(ext, depth=DEPTH, spp=spp)
    assert world.count > (640 if ext == 13 else 1024)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    rows = np.array([0, 13, 26, 27, 40, 53], np.uint32)
    key = ("rows", ext, W, H, spp)
    if key not in _WANT:
        _WANT[key] = oracle.render_rows(world, frame, rows, nthreads=8)[0]
    gpu_ctx.set_schedule()
    gpu_ctx.set_scan_mode(scan)
    try:
        gpu_ctx.upload_world(world)
        info = gpu_ctx.scene_info()
        assert info["kernels"] == (0 if ext == 13 else 2 if scan == "linear" else 1)
        gpu_ctx.set_frame(frame)
        got, st = render_into_sentinel(gpu_ctx, H, W, 1, 0, 1)
        assert_bits_equal(got[rows], _WANT[key], f"extent {ext}, {scan} scan")
        assert (got != SENTINEL).all()
        assert st.samples == W * H * spp
    finally:
        gpu_ctx.set_scan_mode("auto")


@pytest.mark.parametrize("keys", ["prepass", "carried"])
def test_refine_two_steps_of_8(gpu_ctx, oracle, rtx, keys):
    """rtx_refine 8 + 8 samples is the 16-spp frame: the second launch divides
    by the chain's 16 samples (out_n), not by its own 8."""
    W, H = 96, 54
    world = rtx.random_world(11, depth=DEPTH, spp=16)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    gpu_ctx.set_schedule()
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    gpu_ctx.set_refine_keys(keys)
    try:
        run_steps(gpu_ctx, oracle, rtx, "finish96", world, frame, (8, 8), f"refine 8 + 8, {keys} keys")
        assert gpu_ctx.refine_last_keys == keys
    finally:
        gpu_ctx.set_refine_keys("prepass")


def test_adaptive_step_divides_by_each_pixels_count(gpu_ctx, oracle, rtx):
    """Two uniform steps of 8, then one selective step: a refined pixel is
    toGamma(sum / 24) with its own count, an unrefined one keeps its
    framebuffer value (16 samples). run_plan compares the framebuffer, the
    counts, the errors and the sums after every call."""
    W, H = 96, 54
    world = rtx.random_world(11, depth=DEPTH, spp=8)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    gpu_ctx.set_schedule()
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    steps = plan(oracle, rtx, "finish96", world, frame, [(8, INF, 0), (8, INF, 0), (8, "q", 0)])
    check_shares(steps, [2])
    assert set(np.unique(steps[2]["counts"]).tolist()) == {16, 24}
    run_plan(gpu_ctx, "finish96", steps, "adaptive 8, 8, then selective 8")
    assert_bits_equal(gpu_ctx.download()[~steps[2]["mask"]], oracle_at(oracle, rtx, "finish96", world, frame, 16)[0][~steps[2]["mask"]],
                      "unrefined pixels keep the 16-sample frame")
