"""Progressive frames dealt across a group's members (include/rtx.h
rtx_render_sum, rtx_fold_frames, rtx_group_accumulate), on the box's one
MI355X: the fold kernel against sequential fp32 adds in numpy, a frame's linear
sums against the oracle, and the rehearsal (every member on device 0, one
after another) against both the oracle's frame-by-frame fold and the same
number of rtx_accumulate calls on one context, bit for bit. RCCL runs with the
one rank the box allows, in a child process (rtx_cli). More than one device,
peer copies and RCCL with several ranks have never run; nothing here claims
they have."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytrace-we-gpu_amd", "bin", "rtx_cli")
W, H, SPP, DEPTH = 64, 36, 2, 20
GAMMA = 0.454545454545


def _same(a, b):
    """Bit-identical, NaN equal to NaN (as test_gpu_group._same)."""
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _assert_same(got, want, what):
    same = _same(np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32))
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} values differ"


def _world(rtx):
    return rtx.random_world(11, depth=DEPTH, spp=SPP)


def _frame(rtx, w=W, h=H, rng=None):
    f = rtx.camera_look_at(w, h, aspect=w / h)
    if rng is not None:
        f.rng_mode = rng
    return f


# ---------------------------------------------------------------------------
# references, computed once and shared (never modified)
# ---------------------------------------------------------------------------
_LINEAR = {}   # (rng_mode, frame_index) -> oracle linear sums (H, W, 4) at 64x36
_ORACLE = {}   # (rng_mode, frames) -> oracle image of the frame-by-frame fold
_ONECTX = {}   # (rng_mode, w, h) -> [image after k + 1 rtx_accumulate calls]


def _linear(oracle, rtx, rng, k):
    if (rng, k) not in _LINEAR:
        f = _frame(rtx, rng=rng)
        f.frame_index = k
        lin, _ = oracle.render_rows_linear(_world(rtx), f, np.arange(H), nthreads=min(8, os.cpu_count() or 1))
        lin.setflags(write=False)
        _LINEAR[(rng, k)] = lin
    return _LINEAR[(rng, k)]


def _gamma(oracle, total, divisor):
    mean = (total[..., :3] / np.float32(divisor)).astype(np.float32)
    want = np.ones(total.shape, np.float32)
    want[..., :3] = oracle.math("pow", mean.ravel(), np.full(mean.size, GAMMA, np.float32)).reshape(mean.shape)
    return want


def _oracle_fold(oracle, rtx, rng, frames):
    """The oracle's frame-by-frame fold, as test_progressive_accumulation_bit_exact builds it."""
    if (rng, frames) not in _ORACLE:
        total = np.zeros((H, W, 4), np.float32)
        for k in range(frames):
            total[..., :3] = total[..., :3] + _linear(oracle, rtx, rng, k)[..., :3]
        _ORACLE[(rng, frames)] = _gamma(oracle, total, frames * SPP)
    return _ORACLE[(rng, frames)]


def _one_context(gpu_ctx, rtx, frames, rng=0, w=W, h=H):
    """Image after `frames` calls of rtx_accumulate on one context."""
    key = (rng, w, h)
    have = _ONECTX.setdefault(key, [])
    if len(have) < frames:
        gpu_ctx.upload_world(_world(rtx))
        gpu_ctx.set_frame(_frame(rtx, w, h, rng))
        del have[:]
        for k in range(max(frames, 9 if (w, h, rng) == (W, H, 0) else frames)):
            assert gpu_ctx.accumulate(reset=(k == 0)) == k + 1
            have.append(gpu_ctx.download())
    return have[frames - 1]


# ---------------------------------------------------------------------------
# 1. the fold kernel against numpy
# ---------------------------------------------------------------------------
ROT = np.array([1e8, 1.0, -1e8, 1.0, 3e-39], np.float32)  # the order of the adds matters


def _fold_inputs(pixels, m):
    slot = pixels + 3
    p = np.arange(pixels)
    k = np.arange(m)[:, None]
    sums = np.full((m, slot, 4), 1e30, np.float32)  # the slots' padding: never to be read
    sums[:, :pixels, 0] = ROT[(k + p) % 5]
    sums[:, :pixels, 1] = ROT[(k + 2 * p + 1) % 5]
    sums[:, :pixels, 2] = ROT[(2 * k + p + 3) % 5]
    sums[:, :pixels, 3] = 123.0                      # a sum's w is not part of the fold
    accum = np.empty((slot, 4), np.float32)
    accum[:, 0] = 3.0 + (np.arange(slot) % 7)
    accum[:, 1] = 1.0 + 0.25 * (np.arange(slot) % 5)
    accum[:, 2] = 5.0e7
    accum[:, 3] = 77.0 + np.arange(slot)             # the sentinel
    if pixels >= 63:
        sums[0, 3, :3] = np.nan
        sums[m - 1, 5, 0] = np.inf
        sums[:, 7, :3] = 0.0
        accum[7, :3] = 0.0                           # the all-zero pixel
    return sums, accum


def _fold_sequential(sums, accum, pixels):
    a = accum[:pixels, :3].copy()
    with np.errstate(all="ignore"):
        for k in range(sums.shape[0]):
            a = (a + sums[k, :pixels, :3]).astype(np.float32)
    return a


def _fold_tree(sums, accum, pixels):
    parts = [sums[k, :pixels, :3] for k in range(sums.shape[0])]
    with np.errstate(all="ignore"):
        while len(parts) > 1:
            parts = [(parts[i] + parts[i + 1]).astype(np.float32) if i + 1 < len(parts) else parts[i]
                     for i in range(0, len(parts), 2)]
        return (accum[:pixels, :3] + parts[0]).astype(np.float32)


@pytest.mark.parametrize("m", [1, 2, 5, 64])
@pytest.mark.parametrize("pixels", [1, 63, 64 * 4 * 3 + 5])
def test_fold_frames_equals_sequential_fp32_adds(gpu_ctx, oracle, pixels, m):
    slot = pixels + 3
    divisor = 2 * m + 1
    sums, accum = _fold_inputs(pixels, m)
    want_a = _fold_sequential(sums, accum, pixels)
    # the test can see a reordered fold: a pairwise (tree) sum of the same inputs differs somewhere. (m = 1
    # has one add and no other order; m = 2 at a single pixel: that pixel's a + (s0 + s1) rounds as (a + s0) + s1.)
    if m >= 3 or (m == 2 and pixels > 1):
        assert not _same(_fold_tree(sums, accum, pixels), want_a).all()
    d_sums, d_accum, d_image = gpu_ctx.alloc(sums.shape), gpu_ctx.alloc(accum.shape), gpu_ctx.alloc(accum.shape)
    try:
        image0 = np.full(accum.shape, -5.0, np.float32)
        d_sums.upload(sums)
        d_accum.upload(accum)
        d_image.upload(image0)
        gpu_ctx.fold_frames(d_accum.ptr, d_sums.ptr, m, slot, pixels, divisor, d_image.ptr)
        gpu_ctx.sync()
        got_a, got_i = d_accum.numpy(), d_image.numpy()
    finally:
        for d in (d_sums, d_accum, d_image):
            d.free()
    _assert_same(got_a[:pixels, :3], want_a, "accumulator xyz")
    np.testing.assert_array_equal(got_a[:, 3], accum[:, 3])            # w unchanged
    np.testing.assert_array_equal(got_a[pixels:], accum[pixels:])      # nothing past `pixels`
    np.testing.assert_array_equal(got_i[pixels:], image0[pixels:])
    with np.errstate(all="ignore"):
        mean = (want_a / np.float32(divisor)).astype(np.float32)
    want_i = oracle.math("pow", mean.ravel(), np.full(mean.size, GAMMA, np.float32)).reshape(mean.shape)
    _assert_same(got_i[:pixels, :3], want_i, "image xyz")
    np.testing.assert_array_equal(got_i[:pixels, 3], np.ones(pixels, np.float32))


def test_fold_frames_refusals(gpu_ctx, rtx):
    lib = rtx.load_library()
    bufs = [gpu_ctx.alloc((8, 4)) for _ in range(3)]
    a, s, i = (b.ptr for b in bufs)
    try:
        for args, word in [((a, s, 0, 4, 4, 1, i), "m outside"), ((a, s, 65, 4, 4, 1, i), "m outside"),
                           ((a, s, 1, 3, 4, 1, i), "slot_pixels"), ((a, s, 1, 4, 0, 1, i), "pixels"),
                           ((a, s, 1, 4, 4, 0, i), "divisor"), ((None, s, 1, 4, 4, 1, i), "null"),
                           ((a, None, 1, 4, 4, 1, i), "null"), ((a, s, 1, 4, 4, 1, None), "null")]:
            assert lib.rtx_fold_frames(gpu_ctx._h, *args) == -1, args
            msg = lib.rtx_last_error().decode()
            assert msg.startswith("rtx_fold_frames:") and word in msg, msg
        with pytest.raises(rtx.RtxError, match="divisor"):
            gpu_ctx.fold_frames(a, s, 1, 4, 4, 0, i)
    finally:
        for b in bufs:
            b.free()


# ---------------------------------------------------------------------------
# 2. one frame's linear sums against the oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rng,frame_index", [(0, 0), (0, 3), (1, 2)])
def test_render_sum_equals_the_oracle_linear_sums(gpu_ctx, oracle, rtx, rng, frame_index):
    lib = rtx.load_library()
    gpu_ctx.upload_world(_world(rtx))
    gpu_ctx.set_frame(_frame(rtx, rng=rng))
    assert gpu_ctx.accumulate(reset=True) == 1 and gpu_ctx.accumulate() == 2
    d_sum = gpu_ctx.alloc((H, W, 4))
    try:
        d_sum.upload(np.full((H, W, 4), 7.0, np.float32))  # rtx_render_sum clears it itself
        gpu_ctx.render_sum(frame_index, d_sum.ptr)
        gpu_ctx.sync()
        got = d_sum.numpy()
    finally:
        d_sum.free()
    assert lib.rtx_accumulated_frames(gpu_ctx._h) == 2  # the context's accumulation is untouched
    _assert_same(got[..., :3], _linear(oracle, rtx, rng, frame_index)[..., :3], "linear sums")
    assert (got[..., 3].view(np.uint32) == 0).all()
    assert gpu_ctx.accumulate() == 3
    with pytest.raises(rtx.RtxError, match="d_sum"):
        gpu_ctx.render_sum(0, 0)
    assert lib.rtx_render_sum(gpu_ctx._h, 0x80000000, 1) == -1


# ---------------------------------------------------------------------------
# 3.-6. the rehearsal
# ---------------------------------------------------------------------------
def _group(rtx, devices, rng=None, gather="copy"):
    g = rtx.Group(devices, gather)
    g.upload_world(_world(rtx))
    g.set_frame(_frame(rtx, rng=rng))
    for m in range(len(devices)):
        g.ctx(m).stats_reset()
    return g


def test_rehearsal_rounds_equal_oracle_and_one_context(gpu_ctx, oracle, rtx):
    """[0,0,0]: 7 frames in rounds of 3, 3, 1, then 2 more."""
    with _group(rtx, [0, 0, 0]) as g:
        assert g.gather == "copy" and g.accumulated_frames == 0
        assert g.accumulate(7, reset=True) == 7
        img7 = g.download()
        t7 = g.accumulate_times()
        assert g.accumulate(2) == 9 and g.accumulated_frames == 9
        img9 = g.download()
        t9 = g.accumulate_times()
        stats = [g.ctx(m).stats() for m in range(3)]
        assert g.image_ptr() != 0
    for frames, img in ((7, img7), (9, img9)):
        _assert_same(img, _oracle_fold(oracle, rtx, 0, frames), f"{frames} frames against the oracle's fold")
        _assert_same(img, _one_context(gpu_ctx, rtx, frames), f"{frames} frames against rtx_accumulate")
    assert [s.launches for s in stats] == [4, 3, 2]
    assert [s.samples for s in stats] == [k * W * H * SPP for k in (4, 3, 2)]
    # the last round: frame 6 alone on the root; then frames 7, 8 on members 0 and 1
    for t, took in ((t7, [True, False, False]), (t9, [True, True, False])):
        assert len(t["render_ms"]) == 3 and t["gather_ms"] >= 0 and t["fold_ms"] >= 0
        assert [ms > 0 for ms in t["render_ms"]] == took and all(ms >= 0 for ms in t["render_ms"])


def test_more_members_than_frames(gpu_ctx, rtx):
    with _group(rtx, [0, 0, 0, 0]) as g:
        assert g.accumulate(2, True) == 2
        img = g.download()
        stats = [g.ctx(m).stats() for m in range(4)]
        times = g.accumulate_times()
    assert [s.launches for s in stats] == [1, 1, 0, 0]
    assert [ms > 0 for ms in times["render_ms"]] == [True, True, False, False]
    _assert_same(img, _one_context(gpu_ctx, rtx, 2), "2 frames on 4 members")


def test_per_sample_rng(gpu_ctx, rtx):
    with _group(rtx, [0, 0], rng=rtx.RNG_PER_SAMPLE) as g:
        assert g.accumulate(3) == 3  # a first call restarts by itself
        img = g.download()
    _assert_same(img, _one_context(gpu_ctx, rtx, 3, rng=rtx.RNG_PER_SAMPLE), "3 per-sample frames")


def test_restart_and_mixing_with_render(gpu_ctx, rtx):
    with _group(rtx, [0, 0, 0]) as g:
        assert g.accumulate(2) == 2
        g.set_frame(_frame(rtx, 32, 18))
        assert g.accumulate(1) == 1  # another size: restarted without reset
        small = g.download()
        assert small.shape == (18, 32, 4)
        g.set_frame(_frame(rtx))
        assert g.accumulate(2, True) == 2
        plain = g.render_image(4)    # overwrites the image, not the accumulator
        assert g.accumulate(1) == 3
        img3 = g.download()
        # a row-split frame of another size in between replaces the image, not the accumulator
        g.set_frame(_frame(rtx, 32, 18))
        assert g.render_image(4).shape == (18, 32, 4)
        g.set_frame(_frame(rtx))
        assert g.accumulate(1) == 4
        img4 = g.download()
    _assert_same(img4, _one_context(gpu_ctx, rtx, 4), "4 frames around a render of another size")
    gpu_ctx.upload_world(_world(rtx))
    gpu_ctx.set_frame(_frame(rtx, 32, 18))
    _assert_same(small, gpu_ctx.render_image(), "1 frame at 32x18 against the plain frame")
    gpu_ctx.set_frame(_frame(rtx))
    _assert_same(plain, gpu_ctx.render_image(), "the row-split frame between two accumulate calls")
    _assert_same(img3, _one_context(gpu_ctx, rtx, 3), "3 frames around a render")


def test_accumulate_refusals(rtx):
    lib = rtx.load_library()
    with rtx.Group([0, 0], "copy") as g:
        assert lib.rtx_group_accumulate(g._h, 1, 0) == -3 and b"no frame" in lib.rtx_last_error()  # RTX_ERR_STATE
        g.upload_world(rtx.random_world(11, depth=DEPTH, spp=4))
        g.set_frame(_frame(rtx))
        # (spp 4: 0x7fffffff frames fit the seed's 31 bits, their divisor 0x7fffffff * 4 does not fit uint32)
        for frames, word in ((0, "frames is 0"), (0x80000000, "0x7fffffff"), (0x7fffffff, "2^32")):
            assert lib.rtx_group_accumulate(g._h, frames, 1) == -1, frames
            assert word in lib.rtx_last_error().decode(), lib.rtx_last_error()
        assert g.accumulated_frames == 0
        with pytest.raises(rtx.RtxError, match="rtx_group_sync first|no round"):
            g.accumulate_times()


# ---------------------------------------------------------------------------
# 7. rtx_cli --split frames
# ---------------------------------------------------------------------------
def _cli(args, timeout=120):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


SIZE = ["--width", "160", "--height", "90", "--spp", "4"]


def test_cli_split_frames_writes_the_accumulated_image(tmp_path):
    a, b = str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm")
    line = _cli(SIZE + ["--devices", "0,0", "--split", "frames", "--frames", "5", "--pfm", a])
    one = _cli(SIZE + ["--accumulate", "--frames", "5", "--pfm", b])
    assert "split" not in one and "fold_ms" not in one
    assert line["split"] == "frames" and line["accumulated_frames"] == 5 and line["fold_ms"] >= 0
    assert line["n_gpus"] == 2 and line["gather"] == "copy" and line["gather_ms"] >= 0
    assert [m["frames"] for m in line["per_member"]] == [3, 2]
    assert line["segments"] == one["segments"]
    assert open(a, "rb").read() == open(b, "rb").read()
    # the default split is rows: today's line
    rows = _cli(SIZE + ["--devices", "0,0", "--split", "rows"])
    assert "split" not in rows and "deinterleave_ms" in rows and "tile_rows" in rows
    # --split frames needs a group
    r = subprocess.run([CLI] + SIZE + ["--split", "frames"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--split frames" in r.stderr


def test_cli_split_frames_rccl_one_rank(tmp_path):
    a, b = str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm")
    line = _cli(SIZE + ["--gpus", "1", "--gather", "rccl", "--split", "frames", "--frames", "3", "--pfm", a])
    assert line["gather"] == "rccl" and line["rccl_version"] and line["accumulated_frames"] == 3
    assert [m["frames"] for m in line["per_member"]] == [3]
    _cli(SIZE + ["--accumulate", "--frames", "3", "--pfm", b])
    assert open(a, "rb").read() == open(b, "rb").read()
