"""Progressive frames dealt across a group's members (include/rtx.h
rtx_group_accumulate), CPU only.

The accumulation arithmetic — rounds of a call, which member takes which
frame_index, the transfers into the root's [n][pixels] buffer, the divisor
after each round — lives in the HIP-free plan header
(raytrace-we-gpu_amd/csrc/rtx_group_plan.h); tests/group_accum_check.cpp runs
it on host memory against a sequential one-accumulator emulation. The new
entry points decide their bad arguments before they touch HIP, so those checks
run without a GPU. The GPU side is test_gpu_group_accum.py."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "group_accum_check.cpp")

NAMES = ("rtx_render_sum", "rtx_fold_frames", "rtx_group_accumulate", "rtx_group_accumulated_frames",
         "rtx_group_get_accumulate_times")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_accum_plan_equals_the_sequential_accumulator(tmp_path, flags):
    """(n, frames per call) = (3,[7,2]) (4,[2]) (1,[3]) (8,[8,8]) (5,[1,1,1])
    (64,[65]) and (3,[4, reset 5]) at 37 pixels: the result equals the
    one-accumulator emulation exactly, no access outside a buffer, no render
    beyond a call's frames, every frame_index once, and the tags can see a
    reversed fold; once more as a stand-alone program under ASan and UBSan."""
    exe = str(tmp_path / "group_accum_check")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, SRC], check=True)
    # (no leak pass at exit: it needs ptrace, which a sandboxed runner may lack)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert rep["cases"] == 7 and rep["mismatches"] == 0 and rep["out_of_bounds"] == 0, rep
    assert rep["idle_renders"] == 0, rep
    # 7 + 2, 2, 3, 8 + 8, 1 + 1 + 1, 65 frames, and 4 + 5 of the reset case
    assert rep["frames_rendered"] == 7 + 2 + 2 + 3 + 16 + 3 + 65 + 9, rep
    # rounds: 3+1, 1, 3, 1+1, 3, 2, 2+2; one transfer per taking member but the root
    assert rep["rounds"] == 19 and rep["ops"] == 88, rep
    assert rep["order_sensitive"] is True and rep["order_rounds"] >= 5, rep


def test_null_handles(rtx):
    lib = rtx.load_library()
    assert lib.rtx_group_accumulate(None, 1, 0) == -1
    assert b"rtx_group_accumulate" in lib.rtx_last_error()
    assert lib.rtx_render_sum(None, 0, None) == -1
    assert b"rtx_render_sum" in lib.rtx_last_error()
    assert lib.rtx_fold_frames(None, None, None, 1, 1, 1, 1, None) == -1
    assert b"rtx_fold_frames" in lib.rtx_last_error()
    assert lib.rtx_group_get_accumulate_times(None, None, None, None) == -1
    assert b"rtx_group_get_accumulate_times" in lib.rtx_last_error()
    assert lib.rtx_group_accumulated_frames(None) == 0


def test_header_declares_the_accumulation(rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    lib = rtx.load_library()
    for name in NAMES:
        assert "RTX_API" in text and f" {name}(" in text.replace("*", " "), name
        assert hasattr(lib, name), name
    assert "#define RTX_FOLD_MAX 64" in text and "#define RTX_VERSION 145" in text
    assert lib.rtx_version() == 145
    exported = subprocess.run(["nm", "-D", "--defined-only", rtx.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in exported, name
    assert callable(getattr(rtx.Group, "accumulate", None))
    assert isinstance(rtx.Group.accumulated_frames, property) and callable(rtx.Group.accumulate_times)
    assert callable(rtx.Context.render_sum) and callable(rtx.Context.fold_frames)
