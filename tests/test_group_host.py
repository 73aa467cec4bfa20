"""The multi-GPU frame's host side (include/rtx.h rtx_group), CPU only.

The partition and buffer arithmetic lives in a header with no HIP in it
(raytrace-we-gpu_amd/csrc/rtx_group_plan.h); tests/group_plan_check.cpp runs
that plan on host memory — members fill their send buffers with (member, local
row) tags, the gather's transfers are memcpy, the de-interleave is the
kernel's index arithmetic — and every image row must carry its owner's tag.
rtx_group_create decides every bad argument before it touches HIP, so those
checks run without a GPU. The GPU side is test_gpu_group.py."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "group_plan_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_group_plan_assembles_every_row(tmp_path, flags):
    """(H, T, n) = (1080,5,8) (1081,5,8) (117,8,3) (117,64,5) (10,3,8) (1,1,2)
    (20,8,4): no mismatch, no access outside a buffer, no render for a member
    without rows; once more as a stand-alone program under ASan and UBSan."""
    exe = str(tmp_path / "group_plan_check")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, SRC], check=True)
    # (no leak pass at exit: it needs ptrace, which a sandboxed runner may lack)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert rep["cases"] == 7 and rep["mismatches"] == 0 and rep["out_of_bounds"] == 0, rep
    assert rep["idle_renders"] == 0, rep
    # 1080 + 1081 + 117 + 117 + 10 + 1 + 20 rows; n - 1 transfers per case;
    # members past the tile count: 3 of (117,64,5), 4 of (10,3,8), 1 of (1,1,2), 1 of (20,8,4)
    assert rep["rows_checked"] == 2426 and rep["ops"] == 31 and rep["idle_members"] == 9, rep


def test_plan_rows_equal_the_library_partition(rtx):
    """The plan header restates rtx_part_rows: the checker's cases, against the
    library's own arithmetic (the checker compares with the definition)."""
    for H, T, n in [(1080, 5, 8), (1081, 5, 8), (117, 8, 3), (117, 64, 5), (10, 3, 8), (1, 1, 2), (20, 8, 4)]:
        rows = [rtx.part_rows(H, T, m, n) for m in range(n)]
        assert sum(rows) == H and rows[0] == max(rows)
        assert rows == [len(rtx.part_row_ids(H, T, m, n)) for m in range(n)]


def _create(lib, devices, n, mode, out=True):
    arr = (C.c_int * max(1, len(devices)))(*devices) if devices is not None else None
    h = C.c_void_p()
    rc = lib.rtx_group_create(arr, n, mode, C.byref(h) if out else None)
    return rc, h.value, lib.rtx_last_error().decode()


@pytest.mark.parametrize("devices,n,mode,out,word", [
    (None, 2, 0, True, "devices"),            # null device list
    ([0, 1], 2, 0, False, "out"),             # null out
    ([0], 0, 0, True, "n is 0"),              # no members
    ([0] * 65, 65, 0, True, "RTX_GROUP_MAX"),  # too many
    ([0, -1], 2, 0, True, "devices[1]"),      # negative device
    ([-3], 1, 2, True, "devices[0]"),
    ([0, 1], 2, 3, True, "gather_mode"),      # unknown mode
    ([0, 1], 2, -1, True, "gather_mode"),
    ([0, 1, 0], 3, 0, True, "distinct or all equal"),  # neither distinct nor equal
    ([2, 2, 3], 3, 2, True, "distinct or all equal"),
    ([0, 0], 2, 1, True, "RTX_GATHER_RCCL"),  # RCCL needs distinct devices
])
def test_group_create_rejects_bad_arguments_without_a_gpu(rtx, devices, n, mode, out, word):
    lib = rtx.load_library()
    rc, handle, msg = _create(lib, devices, n, mode, out)
    assert rc == -1 and not handle
    assert msg.startswith("rtx_group_create:") and word in msg, msg


def test_group_null_handles(rtx):
    lib = rtx.load_library()
    assert lib.rtx_group_size(None) == 0
    assert lib.rtx_group_sync(None) == -1 and b"rtx_group_sync" in lib.rtx_last_error()
    assert lib.rtx_group_ctx(None, 0) is None and lib.rtx_group_image(None) is None
    assert lib.rtx_group_render(None, 5) == -1
    assert lib.rtx_group_upload_world(None, None) == -1
    assert lib.rtx_group_set_frame(None, None) == -1
    assert lib.rtx_group_download(None, None, 0) == -1
    assert lib.rtx_group_get_times(None, None, None, None) == -1
    lib.rtx_group_destroy(None)  # a no-op


def test_python_group_rejects_bad_arguments(rtx):
    with pytest.raises(rtx.RtxError, match="distinct or all equal"):
        rtx.Group([0, 1, 1])
    with pytest.raises(rtx.RtxError, match="n is 0"):
        rtx.Group([])
    with pytest.raises(ValueError):
        rtx.Group([0], gather="mpi")


def test_library_does_not_link_rccl(rtx):
    """RCCL is loaded at run time: librtx.so names no RCCL among its needed
    libraries, so a single-GPU user never loads it."""
    out = subprocess.run(["readelf", "-d", rtx.LIB_PATH], capture_output=True, text=True, check=True).stdout
    needed = [l for l in out.splitlines() if "NEEDED" in l]
    assert needed and not [l for l in needed if "rccl" in l.lower() or "nccl" in l.lower()], needed


def test_header_declares_the_group(rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    for name in ("rtx_group_create", "rtx_group_destroy", "rtx_group_size", "rtx_group_ctx",
                 "rtx_group_upload_world", "rtx_group_set_frame", "rtx_group_render", "rtx_group_sync",
                 "rtx_group_image", "rtx_group_download", "rtx_group_get_times"):
        assert "RTX_API" in text and f" {name}(" in text.replace("*", " "), name
        assert hasattr(rtx.load_library(), name), name
    assert "#define RTX_VERSION 145" in text and "#define RTX_GROUP_MAX 64" in text
