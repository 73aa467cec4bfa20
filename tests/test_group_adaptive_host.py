"""Adaptive refinement on row parts and across a group's members (include/rtx.h
rtx_refine_adaptive_rows, rtx_group_refine_adaptive), CPU only.

The activity rule on a part (rtx_adaptive.h adaptive_active_rows) and the halo
plan that feeds it (rtx_group_plan.h make_halo_plan) are headers with no HIP in
them; tests/group_adaptive_check.cpp runs both on host memory against the
whole-frame rule. The new entry points decide their bad arguments before they
look at the handle or touch HIP, so those rules run without a GPU. The GPU
side is test_gpu_group_refine_adaptive.py."""
import ctypes as C
import inspect
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "group_adaptive_check.cpp")

CTX_NAMES = ("rtx_refine_adaptive_rows", "rtx_refine_pending_rows", "rtx_refine_edges", "rtx_refine_counts_rows",
             "rtx_refine_error_rows")
GROUP_NAMES = ("rtx_group_refine_adaptive", "rtx_group_refine_pending", "rtx_group_refine_counts",
               "rtx_group_refine_error")
INVALID = -1
NAN = float("nan")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_the_rule_on_parts_is_the_rule_on_the_frame(tmp_path, flags):
    """Every (H, T, n) in 1..13 x 1..5 x 1..5 at widths 1, 2 and 7: scatter,
    edges, the halo plan between guard words, adaptive_active_rows on every
    local pixel == adaptive_active on the whole frame; once more as a
    stand-alone program under ASan and UBSan."""
    exe = str(tmp_path / "group_adaptive_check")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, SRC], check=True)
    # (no leak pass at exit: it needs ptrace, which a sandboxed runner may lack)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert rep["cases"] == 13 * 5 * 5 * 3 and rep["pixels"] == 91 * 5 * 5 * 10, rep
    assert rep["mismatches"] == 0 and rep["guard_hits"] == 0, rep
    assert rep["outside_written"] == 0 and rep["unfilled"] == 0, rep
    # the inputs exercise the halo: pixels active only through a neighbour's row, members
    # without rows, and transfers at all
    assert rep["halo_only"] > 100 and rep["idle_members"] > 0 and rep["transfers"] > 0, rep
    assert 0.05 < rep["active"] / rep["pixels"] < 0.95, rep


def test_null_handles(rtx):
    lib = rtx.load_library()
    buf = (C.c_float * 4)()
    ubuf = (C.c_uint32 * 4)()
    n = C.c_uint32(7)
    out = C.c_void_p(C.addressof(buf))
    assert lib.rtx_refine_adaptive_rows(None, 4, 0, 3, 8, 0.1, 0, 0, None, out, C.byref(n)) == INVALID
    assert b"rtx_refine_adaptive_rows" in lib.rtx_last_error()
    assert lib.rtx_refine_pending_rows(None, 4, 0, 3, 8, 0.1, 0, None, C.byref(n)) == INVALID
    assert b"rtx_refine_pending_rows" in lib.rtx_last_error()
    assert lib.rtx_refine_edges(None, out) == INVALID and b"rtx_refine_edges" in lib.rtx_last_error()
    assert lib.rtx_refine_counts_rows(None, ubuf, 16) == INVALID
    assert b"rtx_refine_counts_rows" in lib.rtx_last_error()
    assert lib.rtx_refine_error_rows(None, buf, 16) == INVALID and b"rtx_refine_error_rows" in lib.rtx_last_error()
    assert lib.rtx_group_refine_adaptive(None, 8, 0.1, 0, 5, 0, C.byref(n)) == INVALID
    assert b"rtx_group_refine_adaptive" in lib.rtx_last_error()
    assert lib.rtx_group_refine_pending(None, 8, 0.1, 0, 5, C.byref(n)) == INVALID
    assert b"rtx_group_refine_pending" in lib.rtx_last_error()
    assert lib.rtx_group_refine_counts(None, ubuf, 16) == INVALID
    assert b"rtx_group_refine_counts" in lib.rtx_last_error()
    assert lib.rtx_group_refine_error(None, buf, 16) == INVALID and b"rtx_group_refine_error" in lib.rtx_last_error()
    assert n.value == 7


def test_argument_rules_are_answered_before_the_handle_is_used(rtx):
    """The argument rules of rtx_refine_adaptive and of rtx_refine_rows'
    partition are RTX_ERR_INVALID before the context or the group is looked
    at, so before any HIP call: the handle here is an opaque block of zero
    bytes that is no context, and no GPU is needed."""
    lib = rtx.load_library()
    block = C.create_string_buffer(1 << 16)
    h = C.cast(block, C.c_void_p)
    out = C.c_void_p(C.addressof(block))  # (a non-null d_out / d_halo; never written or read)
    n = C.c_uint32(7)
    # (tile_rows, part, nparts, samples, threshold, max_samples, reset, d_halo, d_out)
    for args, word in [((4, 0, 3, 0, 0.1, 0, 0, out, out), "samples is 0"),
                       ((4, 0, 3, 8, NAN, 0, 0, out, out), "NaN"),
                       ((4, 0, 3, 8, 0.1, 7, 0, out, out), "max_samples"),
                       ((0, 0, 3, 8, 0.1, 0, 0, out, out), "partition"),
                       ((4, 0, 0, 8, 0.1, 0, 0, out, out), "partition"),
                       ((4, 3, 3, 8, 0.1, 0, 1, out, out), "partition"),
                       ((4, 0, 2, 8, 0.1, 0, 0, out, None), "d_out NULL")]:
        assert lib.rtx_refine_adaptive_rows(h, *args, C.byref(n)) == INVALID, args
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_refine_adaptive_rows:") and word in msg, msg
    for args, word in [((4, 0, 3, 0, 0.1, 0, out), "samples is 0"),
                       ((4, 0, 3, 8, NAN, 0, out), "NaN"),
                       ((4, 0, 3, 8, 0.1, 7, out), "max_samples"),
                       ((0, 0, 3, 8, 0.1, 0, out), "partition"),
                       ((4, 5, 3, 8, 0.1, 0, out), "partition")]:
        assert lib.rtx_refine_pending_rows(h, *args, C.byref(n)) == INVALID, args
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_refine_pending_rows:") and word in msg, msg
    assert lib.rtx_refine_edges(h, None) == INVALID
    assert lib.rtx_refine_counts_rows(h, None, 16) == INVALID and lib.rtx_refine_error_rows(h, None, 16) == INVALID
    for args, word in [((0, 0.1, 0, 5, 0), "samples is 0"), ((8, NAN, 0, 5, 0), "NaN"),
                       ((8, 0.1, 7, 5, 0), "max_samples"), ((8, 0.1, 0, 0, 0), "tile_rows is 0")]:
        assert lib.rtx_group_refine_adaptive(h, *args, C.byref(n)) == INVALID, args
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_group_refine_adaptive:") and word in msg, msg
        assert lib.rtx_group_refine_pending(h, *args[:4], C.byref(n)) == INVALID, args
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_group_refine_pending:") and word in msg, msg
    assert lib.rtx_group_refine_counts(h, None, 16) == INVALID and lib.rtx_group_refine_error(h, None, 16) == INVALID
    assert n.value == 7
    assert bytes(block.raw) == bytes(1 << 16)  # and nothing wrote to it


def test_symbols_and_signatures(rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    lib = rtx.load_library()
    flat = text.replace("*", " ")
    exported = subprocess.run(["nm", "-D", "--defined-only", rtx.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    for name in CTX_NAMES + GROUP_NAMES:
        assert f" {name}(" in flat, name
        assert hasattr(lib, name), name
        assert f" T {name}\n" in exported, name
    assert 'dlsym "rtx_refine_adaptive_rows"' in text and "#define RTX_VERSION 145" in text
    assert lib.rtx_version() == 145
    assert "Not covered" not in text

    def params(fn):
        return list(inspect.signature(fn).parameters)[1:]

    assert params(rtx.Context.refine_adaptive_rows) == ["tile_rows", "part", "nparts", "samples", "threshold",
                                                        "max_samples", "reset", "d_halo", "d_out"]
    assert params(rtx.Context.refine_pending_rows) == ["tile_rows", "part", "nparts", "samples", "threshold",
                                                       "max_samples", "d_halo"]
    assert params(rtx.Context.refine_edges) == ["d_edges"]
    assert params(rtx.Context.refine_counts_rows) == [] and params(rtx.Context.refine_error_rows) == []
    assert params(rtx.Group.refine_adaptive) == ["samples", "threshold", "max_samples", "tile_rows", "reset"]
    sig = inspect.signature(rtx.Group.refine_adaptive).parameters
    assert sig["max_samples"].default == 0 and sig["tile_rows"].default == 5 and sig["reset"].default is False
    assert params(rtx.Group.refine_pending) == ["samples", "threshold", "max_samples", "tile_rows"]
    assert params(rtx.Group.refine_counts) == [] and params(rtx.Group.refine_error) == []
    # the ctypes prototypes: argument counts of the C declarations
    assert len(lib.rtx_refine_adaptive_rows.argtypes) == 11 and len(lib.rtx_refine_pending_rows.argtypes) == 9
    assert len(lib.rtx_group_refine_adaptive.argtypes) == 7 and len(lib.rtx_group_refine_pending.argtypes) == 6
