"""Queue keys carried from the previous refine launch's cost map (include/rtx.h
rtx_refine_set_keys), CPU only.

The carried key and the host's rule for when a launch takes it live in a
HIP-free header (raytrace-we-gpu_amd/csrc/rtx_refine_keys.h) that the kernels,
rtx_refine and tests/carried_key_check.cpp all compile; the checker runs it on
host memory, plain and as a stand-alone program under ASan and UBSan. The new
entry points decide their bad arguments before they touch HIP, so those checks
run without a GPU. The GPU side is test_gpu_refine_carried.py."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "carried_key_check.cpp")

NAMES = ("rtx_refine_set_keys", "rtx_refine_last_keys", "rtx_refine_cost")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_carried_key_and_fallback_rule(tmp_path, flags):
    """The key equals the pre-pass's formula for s_prev = kCostSpp and 1
    (1-pixel-wide and 1-row images included), never increases when a window
    entry grows, does not overflow at entries of 2^32 - 1 (s_prev 1: the top
    bucket; s_prev 2^32 - 1: one segment per sample, bucket 255 - 9), and the
    host's rule gives the expected answer on its table of cases."""
    exe = str(tmp_path / "carried_key_check")
    subprocess.run(["g++", "-std=c++17", *flags, "-o", exe, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0, (out.stdout, out.stderr)
    # 7 shapes x 2 s_prev x 8 maps, every pixel
    assert rep["equal_checks"] == 16 * (35 + 9 + 9 + 1 + 4 + 48 + 561) and rep["equal_bad"] == 0, rep
    assert rep["mono_checks"] >= 400 and rep["mono_bad"] == 0, rep
    assert rep["top_checks"] == 3 * 2 * (35 + 9 + 9 + 1 + 4 + 48 + 561) + 1 and rep["top_bad"] == 0, rep
    assert rep["rule_cases"] == 13 + 8 and rep["rule_bad"] == 0, rep


def test_null_handles(rtx):
    lib = rtx.load_library()
    assert lib.rtx_refine_set_keys(None, 1) == -1
    assert b"rtx_refine_set_keys" in lib.rtx_last_error()
    assert lib.rtx_refine_last_keys(None) < 0
    assert b"rtx_refine_last_keys" in lib.rtx_last_error()
    buf = (C.c_uint32 * 4)()
    n = C.c_uint32(0)
    assert lib.rtx_refine_cost(None, buf, 16, C.byref(n)) == -1
    assert b"rtx_refine_cost" in lib.rtx_last_error()


def test_header_declares_the_key_modes(rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    lib = rtx.load_library()
    for name in NAMES:
        assert f" {name}(" in text.replace("*", " "), name
        assert hasattr(lib, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", rtx.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in exported, name
    assert 'dlsym "rtx_refine_set_keys"' in text and "#define RTX_VERSION 145" in text
    for name, value in (("PREPASS", 0), ("CARRIED", 1), ("UNSCHEDULED", 2)):
        assert f"#define RTX_REFINE_KEYS_{name} {value}" in text
    assert lib.rtx_version() == 145
    assert rtx.REFINE_KEYS == {"prepass": 0, "carried": 1, "unscheduled": 2}
    assert callable(rtx.Context.set_refine_keys) and callable(rtx.Context.refine_cost)
    assert isinstance(rtx.Context.refine_last_keys, property)
