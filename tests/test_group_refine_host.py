"""Progressive refinement across a group's members (include/rtx.h
rtx_refine_rows, rtx_group_refine), CPU only.

The checkpoint of a group is one whole-frame chain state; the row shuffling
between it and the members' parts is host code in a header with no HIP in it
(raytrace-we-gpu_amd/csrc/rtx_group_plan.h group_scatter_state /
group_gather_state). tests/group_refine_check.cpp runs those same functions on
tagged pixels between guard words. The new entry points decide their bad
arguments before they look at the handle or touch HIP, so those rules run
without a GPU. The GPU side is test_gpu_refine_rows.py and
test_gpu_group_refine.py."""
import ctypes as C
import inspect
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "group_refine_check.cpp")

CTX_NAMES = ("rtx_refine_rows", "rtx_refine_import_rows", "rtx_refine_shape")
GROUP_NAMES = ("rtx_group_refine", "rtx_group_refined_samples", "rtx_group_refine_export", "rtx_group_refine_import")
INVALID = -1


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_scatter_and_gather_of_a_state(tmp_path, flags):
    """(W, H, T, n) = (7,20,8,4) (5,9,2,3) (3,1,1,2) (4,6,3,1): every part holds
    the rows part_row_ids names, ascending; the gather of the scatter is the
    whole; no guard word changes; once more as a stand-alone program under ASan
    and UBSan."""
    exe = str(tmp_path / "group_refine_check")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, SRC], check=True)
    # (no leak pass at exit: it needs ptrace, which a sandboxed runner may lack)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert rep["cases"] == 4 and rep["mismatches"] == 0 and rep["guard_hits"] == 0, rep
    # 20 + 9 + 1 + 6 rows; members past the tile count: 1 of (7,20,8,4), 1 of (3,1,1,2)
    assert rep["rows_checked"] == 36 and rep["idle_members"] == 2, rep


def test_checker_cases_equal_the_library_partition(rtx):
    """The rows the checker expects per part (tile k belongs to member k % n)
    are part_row_ids', and their number rtx_part_rows'."""
    for W, H, T, n in [(7, 20, 8, 4), (5, 9, 2, 3), (3, 1, 1, 2), (4, 6, 3, 1)]:
        ids = [rtx.part_row_ids(H, T, m, n) for m in range(n)]
        assert [len(i) for i in ids] == [rtx.part_rows(H, T, m, n) for m in range(n)]
        assert sorted(int(y) for i in ids for y in i) == list(range(H))


def test_null_handles(rtx):
    lib = rtx.load_library()
    buf = (C.c_float * 4)()
    t = C.c_uint32(7)
    assert lib.rtx_refine_rows(None, 4, 0, 3, 8, 0, None) == INVALID
    assert b"rtx_refine_rows" in lib.rtx_last_error()
    assert lib.rtx_refine_import_rows(None, 4, 0, 3, buf, 16, 8, None) == INVALID
    assert b"rtx_refine_import_rows" in lib.rtx_last_error()
    assert lib.rtx_refine_shape(None, C.byref(t), C.byref(t), C.byref(t)) == INVALID and t.value == 7
    assert b"rtx_refine_shape" in lib.rtx_last_error()
    assert lib.rtx_group_refine(None, 8, 5, 0) == INVALID
    assert b"rtx_group_refine" in lib.rtx_last_error()
    assert lib.rtx_group_refined_samples(None) == 0
    assert lib.rtx_group_refine_export(None, buf, 16) == INVALID
    assert b"rtx_group_refine_export" in lib.rtx_last_error()
    assert lib.rtx_group_refine_import(None, 5, buf, 16, 8) == INVALID
    assert b"rtx_group_refine_import" in lib.rtx_last_error()


def test_argument_rules_are_answered_before_the_handle_is_used(rtx):
    """samples == 0, tile_rows == 0, part >= nparts, and d_out NULL with two
    parts are RTX_ERR_INVALID before the context or the group is looked at, so
    before any HIP call: the handle here is an opaque block of zero bytes that
    is no context, and no GPU is needed."""
    lib = rtx.load_library()
    block = C.create_string_buffer(1 << 16)
    h = C.cast(block, C.c_void_p)
    out = C.c_void_p(C.addressof(block))  # (a non-null d_out; never written)
    buf = (C.c_float * 4)()
    for args, word in [((4, 0, 3, 0, 0, out), "samples is 0"),
                       ((0, 0, 3, 8, 0, out), "partition"),
                       ((4, 0, 0, 8, 0, out), "partition"),
                       ((4, 3, 3, 8, 0, out), "partition"),
                       ((4, 5, 3, 8, 1, out), "partition"),
                       ((4, 0, 2, 8, 0, None), "d_out NULL")]:
        assert lib.rtx_refine_rows(h, *args) == INVALID, args
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_refine_rows:") and word in msg, msg
    for args, word in [((4, 0, 3, buf, 16, 0, out), "samples is 0"),
                       ((0, 0, 3, buf, 16, 8, out), "partition"),
                       ((4, 3, 3, buf, 16, 8, out), "partition")]:
        assert lib.rtx_refine_import_rows(h, *args) == INVALID, args
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_refine_import_rows:") and word in msg, msg
    assert lib.rtx_group_refine(h, 0, 5, 0) == INVALID and b"samples is 0" in lib.rtx_last_error()
    assert lib.rtx_group_refine(h, 8, 0, 0) == INVALID and b"tile_rows is 0" in lib.rtx_last_error()
    assert lib.rtx_group_refine_import(h, 5, buf, 16, 0) == INVALID and b"samples is 0" in lib.rtx_last_error()
    assert lib.rtx_group_refine_import(h, 0, buf, 16, 8) == INVALID and b"tile_rows is 0" in lib.rtx_last_error()
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
    assert 'dlsym "rtx_group_refine"' in text and "#define RTX_VERSION 145" in text
    assert lib.rtx_version() == 145
    assert "Not covered (later changes): row parts" not in text

    def params(fn):
        return list(inspect.signature(fn).parameters)[1:]

    assert params(rtx.Context.refine_rows) == ["tile_rows", "part", "nparts", "samples", "reset", "d_out"]
    assert params(rtx.Context.refine_import_rows) == ["tile_rows", "part", "nparts", "state", "samples", "d_out"]
    assert params(rtx.Context.refine_shape) == []
    assert params(rtx.Group.refine) == ["samples", "tile_rows", "reset"]
    sig = inspect.signature(rtx.Group.refine).parameters
    assert sig["tile_rows"].default == 5 and sig["reset"].default is False
    assert params(rtx.Group.refine_import) == ["state", "samples", "tile_rows"]
    assert inspect.signature(rtx.Group.refine_import).parameters["tile_rows"].default == 5
    assert params(rtx.Group.refine_export) == [] and isinstance(rtx.Group.refined_samples, property)
    # the ctypes prototypes: argument counts of the C declarations
    assert len(lib.rtx_refine_rows.argtypes) == 7 and len(lib.rtx_refine_import_rows.argtypes) == 8
    assert len(lib.rtx_group_refine.argtypes) == 4 and len(lib.rtx_group_refine_import.argtypes) == 5
