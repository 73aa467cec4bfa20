"""One frame across several members through the C-ABI (include/rtx.h
rtx_group), on the box's one MI355X: the rehearsal (every member on device 0,
rendering one after another) runs the partition, the buffers, the copies and
the de-interleave of the multi-GPU path, and the assembled image must equal
the one-context frame and the oracle bit for bit. RCCL runs with the one rank
the box allows, in a child process (rtx_cli): it starts with no torch runtime
loaded, and a transport failure cannot take the test session with it. More
than one RCCL rank has never run anywhere; nothing here claims it has."""
import json
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytrace-we-gpu_amd", "bin", "rtx_cli")


def _same(a, b):
    """Bit-identical, NaN equal to NaN (as __graft_entry__.smoke)."""
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _one_context(gpu_ctx, world, frame):
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    gpu_ctx.stats_reset()
    img = gpu_ctx.render_image()
    return img, gpu_ctx.stats().segments


def _oracle_rows(oracle, world, frame, H):
    rows = np.unique(np.linspace(0, H - 1, 8).astype(np.uint32))
    want, _ = oracle.render_rows(world, frame, rows, nthreads=min(16, os.cpu_count() or 1))
    return rows, want


@pytest.mark.parametrize("devices,gather,W,H,spp,T,parts", [
    ([0, 0, 0], "copy", 320, 180, 8, 4, [60, 60, 60]),
    # three tiles (8, 8 and a ragged 4 rows) for four members: one renders nothing
    ([0, 0, 0, 0], "auto", 160, 20, 4, 8, [8, 8, 4, 0]),
])
def test_rehearsal_group_equals_one_context_and_oracle(gpu_ctx, oracle, rtx, devices, gather, W, H, spp, T, parts):
    world = rtx.random_world(11, depth=50, spp=spp)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    n = len(devices)
    assert [rtx.part_rows(H, T, m, n) for m in range(n)] == parts
    with rtx.Group(devices, gather) as g:
        assert len(g) == n and g.gather == "copy" and g.rccl_version is None
        g.upload_world(world)
        g.set_frame(frame)
        for m in range(n):
            g.ctx(m).stats_reset()
        got = g.render_image(T)
        assert g.image_ptr() != 0
        stats = [g.ctx(m).stats() for m in range(n)]
        times = g.times()
    whole, segments = _one_context(gpu_ctx, world, frame)
    same = _same(got, whole)
    assert same.all(), f"{int((~same).sum())} values differ from the one-context frame"
    rows, want = _oracle_rows(oracle, world, frame, H)
    assert len(rows) == 8
    np.testing.assert_array_equal(got[rows].view(np.uint32), want.view(np.uint32))
    assert sum(s.segments for s in stats) == segments
    assert [s.launches for s in stats] == [1 if r else 0 for r in parts]
    assert [s.samples for s in stats] == [r * W * spp for r in parts]
    assert len(times["render_ms"]) == n and times["gather_ms"] >= 0 and times["deinterleave_ms"] >= 0
    for r, ms in zip(parts, times["render_ms"]):
        assert (ms > 0) if r else (ms == 0)


def test_rehearsal_group_per_sample_rng(gpu_ctx, rtx):
    W, H, spp, T = 320, 180, 8, 4
    world = rtx.random_world(11, depth=50, spp=spp)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    frame.rng_mode = rtx.RNG_PER_SAMPLE
    with rtx.Group([0, 0, 0], "copy") as g:
        g.upload_world(world)
        g.set_frame(frame)
        got = g.render_image(T)
    whole, _ = _one_context(gpu_ctx, world, frame)
    same = _same(got, whole)
    assert same.all(), f"{int((~same).sum())} values differ from the one-context frame"


def test_group_buffers_follow_the_frame_size(gpu_ctx, rtx):
    """A second render after set_frame to another size (and another tile_rows):
    the gathered buffer, the send buffers and the image are replaced."""
    spp = 8
    world = rtx.random_world(11, depth=50, spp=spp)
    with rtx.Group([0, 0, 0], "copy") as g:
        g.upload_world(world)
        for (W, H, T) in [(320, 180, 4), (128, 72, 4), (128, 72, 7)]:
            frame = rtx.camera_look_at(W, H, aspect=W / H)
            g.set_frame(frame)
            got = g.render_image(T)
            assert got.shape == (H, W, 4)
            whole, _ = _one_context(gpu_ctx, world, frame)
            same = _same(got, whole)
            assert same.all(), f"{W}x{H} T {T}: {int((~same).sum())} values differ from the one-context frame"


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0  # little endian
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)


def _cli(args, timeout=120):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


def test_cli_rccl_one_rank(tmp_path, oracle, rtx):
    W, H, spp = 320, 180, 8
    pfm = str(tmp_path / "rccl.pfm")
    line = _cli(["--gpus", "1", "--gather", "rccl", "--width", str(W), "--height", str(H), "--spp", str(spp),
                 "--pfm", pfm])
    assert line["n_gpus"] == 1 and line["devices"] == [0]
    assert line["gather"] == "rccl" and line["rccl_version"]
    (pm,) = line["per_member"]
    assert pm["rows"] == H and pm["render_ms"] >= 0
    assert line["gather_ms"] >= 0 and line["deinterleave_ms"] >= 0
    got = _read_pfm(pfm)
    world = rtx.random_world(11, depth=50, spp=spp)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    rows, want = _oracle_rows(oracle, world, frame, H)
    assert len(rows) == 8
    np.testing.assert_array_equal(got[rows].view(np.uint32), want[..., :3].view(np.uint32))


def test_cli_rehearsal_writes_the_single_context_image(tmp_path):
    W, H, spp = 320, 180, 8
    size = ["--width", str(W), "--height", str(H), "--spp", str(spp)]
    one, two = str(tmp_path / "one.pfm"), str(tmp_path / "two.pfm")
    plain = _cli(size + ["--pfm", one])
    assert "n_gpus" not in plain and "gather" not in plain  # the line without a group is the earlier one
    line = _cli(size + ["--devices", "0,0", "--gather", "copy", "--pfm", two])
    assert line["n_gpus"] == 2 and line["devices"] == [0, 0] and line["gather"] == "copy"
    assert line["rccl_version"] is None and [m["rows"] for m in line["per_member"]] == [90, 90]
    assert line["segments"] == plain["segments"] and line["sphere_tests"] == plain["sphere_tests"]
    assert open(one, "rb").read() == open(two, "rb").read()
    # --accumulate with a group is refused with a message
    r = subprocess.run([CLI] + size + ["--devices", "0,0", "--accumulate"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--accumulate" in r.stderr
