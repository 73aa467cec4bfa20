"""rtx_group_refine: progressive refinement across a group's members, on the
box's one MI355X through one-device rehearsal groups (every member on device
0, one after another): the partition, the members' part states, the buffers,
the copies and the de-interleave of the multi-GPU path. After steps adding
s1..sk the group's image must be, bit for bit (NaN == NaN), the oracle's full
frame at spp = s1 + ... + sk; its exported state must be the one-context
state; and one state moves between a context and groups of other shapes. RCCL
runs with the one rank the box allows, in a child process (rtx_cli). More than
one RCCL rank and peer copies have never run anywhere; nothing here claims
they have."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from refine_parts import assert_bits_equal, frame_of, oracle_at, world_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "raytrace-we-gpu_amd", "bin", "rtx_cli")
RTX_ERR_STATE = -3
STEPS = (3, 9, 12)


@pytest.mark.parametrize("devices,gather,W,H,T,parts", [
    ([0, 0, 0], "copy", 160, 90, 4, [32, 30, 28]),
    # three tiles (8, 8 and a ragged 4 rows) for four members: one refines nothing
    ([0, 0, 0, 0], "auto", 160, 20, 8, [8, 8, 4, 0]),
])
def test_group_steps_equal_the_oracle(oracle, rtx, devices, gather, W, H, T, parts):
    frame = frame_of(rtx, W, H)
    n_members = len(devices)
    assert [rtx.part_rows(H, T, m, n_members) for m in range(n_members)] == parts
    with rtx.Group(devices, gather) as g:
        assert g.gather == "copy"
        g.upload_world(world_of(rtx))
        g.set_frame(frame)
        assert g.refined_samples == 0
        n, prev = 0, 0
        for i, s in enumerate(STEPS):
            for m in range(n_members):
                g.ctx(m).stats_reset()
            got_n = g.refine(s, tile_rows=T, reset=(i == 0))
            img = g.download()
            stats = [g.ctx(m).stats() for m in range(n_members)]
            n += s
            assert got_n == n == g.refined_samples
            want, segs = oracle_at(oracle, rtx, frame, n)
            assert_bits_equal(img, want, f"{devices} T {T}: after step {i} (N = {n})")
            assert sum(st.segments for st in stats) == segs - prev, f"step {i} segments"
            assert [st.launches for st in stats] == [1 if r else 0 for r in parts]
            assert [st.samples for st in stats] == [r * W * s for r in parts]
            assert [g.ctx(m).refined_samples for m in range(n_members)] == [n if r else 0 for r in parts]
            prev = segs
        times = g.times()  # the last frame was a refined one
        for r, ms in zip(parts, times["render_ms"]):
            assert (ms > 0) if r else (ms == 0)
        assert times["gather_ms"] >= 0 and times["deinterleave_ms"] >= 0


def test_one_state_moves_between_a_context_and_groups(gpu_ctx, oracle, rtx):
    W, H = 160, 90
    frame = frame_of(rtx, W, H)
    world = world_of(rtx)
    gpu_ctx.upload_world(world)
    gpu_ctx.set_frame(frame)
    gpu_ctx.refine(3, reset=True)
    assert gpu_ctx.refine(9) == 12
    one = gpu_ctx.refine_export()
    with rtx.Group([0, 0, 0], "copy") as g:
        g.upload_world(world)
        g.set_frame(frame)
        g.refine(3, tile_rows=4, reset=True)
        assert g.refine(9, tile_rows=4) == 12
        state = g.refine_export()
    assert state.shape == (H, W, 4)
    assert_bits_equal(state, one, "group state against the one-context state (sums and seeds)")
    want12, want20 = oracle_at(oracle, rtx, frame, 12)[0], oracle_at(oracle, rtx, frame, 20)[0]
    # into a group of another shape: the image shows at once, then 8 more samples
    with rtx.Group([0, 0], "copy") as g2:
        g2.upload_world(world)
        g2.set_frame(frame)
        for m in range(2):
            g2.ctx(m).stats_reset()
        g2.refine_import(state, 12, tile_rows=5)
        assert g2.refined_samples == 12
        assert_bits_equal(g2.download(), want12, "imported into [0,0] T 5: the image before anything is traced")
        assert [g2.ctx(m).stats().launches for m in range(2)] == [0, 0]
        assert g2.refine(8, tile_rows=5) == 20
        assert_bits_equal(g2.download(), want20, "imported into [0,0] T 5, + 8")
        assert_bits_equal(g2.refine_export()[..., :3], oracle_linear(oracle, rtx, frame, 20), "its state at 20")
    # the reverse: the group's state into one context
    with rtx.Context(0) as b:
        b.upload_world(world)
        b.set_frame(frame)
        b.refine_import(state, 12)
        assert_bits_equal(b.download(), want12, "group state imported into a context")
        assert b.refine(8) == 20
        assert_bits_equal(b.download(), want20, "group state in a context, + 8")


def oracle_linear(oracle, rtx, frame, n):
    base = world_of(rtx)
    lin, _ = oracle.render_rows_linear(rtx.World(base.spheres, base.mat_types, base.mat_values, base.depth, n), frame,
                                       np.arange(frame.height), nthreads=8)
    return lin[..., :3]


def test_fresh_rules(oracle, rtx):
    W, H = 160, 90
    frame = frame_of(rtx, W, H)
    with rtx.Group([0, 0, 0], "copy") as g:
        g.upload_world(world_of(rtx))
        g.set_frame(frame)
        assert g.refine(3, tile_rows=4, reset=True) == 3
        # a plain frame between two steps overwrites the image, not the states (world.spp 4 is its own)
        plain = g.render_image(7)
        assert_bits_equal(plain, oracle_at(oracle, rtx, frame, 4)[0], "plain group frame between two steps")
        assert g.refined_samples == 3
        assert g.refine(9, tile_rows=4) == 12
        assert_bits_equal(g.download(), oracle_at(oracle, rtx, frame, 12)[0], "3 + 9 around a plain frame")
        # the same frame bytes again keep the state; another tile_rows restarts it
        g.set_frame(frame_of(rtx, W, H))
        assert g.refined_samples == 12
        assert g.refine(3, tile_rows=6) == 3
        assert_bits_equal(g.download(), oracle_at(oracle, rtx, frame, 3)[0], "another tile_rows restarts")
        assert g.refine(9, tile_rows=6) == 12
        assert_bits_equal(g.download(), oracle_at(oracle, rtx, frame, 12)[0], "T 6: 3 + 9")
        # set_frame with other bytes restarts
        other = frame_of(rtx, W, H, look_from=(10.0, 3.0, 5.0))
        g.set_frame(other)
        assert g.refined_samples == 0
        assert g.refine(3, tile_rows=6) == 3
        assert_bits_equal(g.download(), oracle_at(oracle, rtx, other, 3)[0], "another camera restarts")
        # upload_world restarts
        g.upload_world(world_of(rtx))
        assert g.refined_samples == 0
        assert g.refine(3, tile_rows=6) == 3
        assert_bits_equal(g.download(), oracle_at(oracle, rtx, other, 3)[0], "after upload_world")


def test_a_member_refined_behind_the_groups_back(oracle, rtx):
    W, H, T = 160, 90, 4
    frame = frame_of(rtx, W, H)
    with rtx.Group([0, 0, 0], "copy") as g:
        lib = g._lib
        g.upload_world(world_of(rtx))
        g.set_frame(frame)
        assert g.refine(3, tile_rows=T, reset=True) == 3
        member = g.ctx(1)
        out = member.alloc((rtx.part_rows(H, T, 1, 3), W, 4))
        try:
            assert member.refine_rows(T, 1, 3, 2, d_out=out.ptr) == 5
        finally:
            out.free()
        for m in range(3):
            g.ctx(m).stats_reset()
        assert lib.rtx_group_refine(g._h, 9, T, 0) == RTX_ERR_STATE
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_group_refine: member 1:"), msg
        buf = np.empty((H, W, 4), np.float32)
        assert lib.rtx_group_refine_export(g._h, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.nbytes) == RTX_ERR_STATE
        assert [g.ctx(m).stats().launches for m in range(3)] == [0, 0, 0]  # nothing was launched
        assert g.refined_samples == 3
        # a reset puts everyone back in step
        assert g.refine(3, tile_rows=T, reset=True) == 3
        assert g.refine(9, tile_rows=T) == 12
        assert_bits_equal(g.download(), oracle_at(oracle, rtx, frame, 12)[0], "after the reset")


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline() == b"PF\n"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0  # little endian
        return np.frombuffer(f.read(), "<f4").reshape(h, w, 3)


CLI_SIZE = ["--width", "64", "--height", "36", "--depth", "50", "--scene", "rtiow11"]


def _cli(args, timeout=120):
    r = subprocess.run([CLI] + CLI_SIZE + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


def test_cli_group_refine_writes_the_single_context_files(tmp_path):
    a, b = str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm")
    sa, sb = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    line = _cli(["--devices", "0,0", "--refine", "4,8", "--pfm", a, "--save-state", sa])
    assert line["n_gpus"] == 2 and line["devices"] == [0, 0] and line["gather"] == "copy"
    assert [m["rows"] for m in line["per_member"]] == [20, 16] and line["tile_rows"] == 5
    assert line["refine"] == [4, 8] and line["refined_samples"] == 12 and line["loaded_samples"] == 0
    assert line["refine_keys"] == "prepass" and line["gather_ms"] >= 0 and line["deinterleave_ms"] >= 0
    one = _cli(["--refine", "12", "--pfm", b, "--save-state", sb])
    assert "n_gpus" not in one and one["refined_samples"] == 12
    assert line["segments"] == one["segments"]
    assert open(a, "rb").read() == open(b, "rb").read()
    assert os.path.getsize(sa) == 40 + 64 * 36 * 16 and open(sa, "rb").read() == open(sb, "rb").read()
    # --refine-adaptive with a group keeps its refusal
    r = subprocess.run([CLI] + CLI_SIZE + ["--devices", "0,0", "--refine-adaptive", "8,0.1"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "--refine-adaptive" in r.stderr


def test_cli_state_files_move_between_a_group_and_a_context(tmp_path, oracle, rtx):
    sg, s1 = str(tmp_path / "group.bin"), str(tmp_path / "one.bin")
    c, d = str(tmp_path / "c.pfm"), str(tmp_path / "d.pfm")
    _cli(["--devices", "0,0,0", "--tile-rows", "4", "--refine", "4,8", "--refine-keys", "carried", "--save-state", sg])
    _cli(["--refine", "12", "--save-state", s1])
    one = _cli(["--load-state", sg, "--refine", "8", "--pfm", c])  # a group's file into one context
    assert one["loaded_samples"] == 12 and one["refined_samples"] == 20
    grp = _cli(["--devices", "0,0", "--tile-rows", "3", "--load-state", s1, "--refine", "8", "--pfm", d])  # and back
    assert grp["loaded_samples"] == 12 and grp["refined_samples"] == 20 and grp["n_gpus"] == 2
    want = oracle_at(oracle, rtx, frame_of(rtx, 64, 36), 20)[0][..., :3]
    assert_bits_equal(_read_pfm(c), want, "group state continued on one context")
    assert_bits_equal(_read_pfm(d), want, "one-context state continued on a group")


def test_cli_rccl_one_rank_refines(tmp_path, oracle, rtx):
    pfm = str(tmp_path / "rccl.pfm")
    line = _cli(["--gpus", "1", "--gather", "rccl", "--refine", "8", "--pfm", pfm])
    assert line["n_gpus"] == 1 and line["devices"] == [0]
    assert line["gather"] == "rccl" and line["rccl_version"]
    assert line["refine"] == [8] and line["refined_samples"] == 8
    (pm,) = line["per_member"]
    assert pm["rows"] == 36 and pm["render_ms"] >= 0
    assert_bits_equal(_read_pfm(pfm), oracle_at(oracle, rtx, frame_of(rtx, 64, 36), 8)[0][..., :3], "--gather rccl")
