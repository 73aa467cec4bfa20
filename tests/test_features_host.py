"""First-hit feature buffers, picking, the id mask and masked refinement
(include/rtx.h rtx_features), CPU only.

The rules — the pixel-centre ray's operations, the depth, which pixels an id
list marks and the masked step's cap — live in a HIP-free header
(raytrace-we-gpu_amd/csrc/rtx_features.h) that the kernels, the host and
tests/features_check.cpp all compile; the checker runs it on host memory, plain
and as a stand-alone program under ASan and UBSan, with fp contraction off. The
entry points refuse a null handle before they touch HIP. The GPU side is
test_gpu_features.py and test_gpu_refine_masked.py."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "features_check.cpp")

NAMES = ("rtx_features", "rtx_features_rows", "rtx_pick", "rtx_mask_from_ids", "rtx_refine_masked")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_ray_depth_and_mask_rule(tmp_path, flags):
    """The ray and the depth equal their op-by-op restatements bit for bit; the
    id mask equals the brute force over all pixel pairs on 1x1, 1x5, 5x1 and
    17x9 images at grow 0, 1, 3 and 8 with lists of 1 and 256 ids (absent ids
    and the entry "-1" included); a miss is never listed; the cap rule."""
    exe = str(tmp_path / "features_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert rep["ray_checks"] == 100000 and rep["ray_bad"] == 0, rep
    assert rep["depth_checks"] == 100000 and rep["depth_bad"] == 0, rep
    # 4 shapes x 4 grows x 2 list sizes x 10 maps, every pixel; neither all on nor all off
    assert rep["mask_checks"] == 4 * 2 * 10 * (1 + 5 + 5 + 153) and rep["mask_bad"] == 0, rep
    assert 0.1 < rep["mask_on"] / rep["mask_checks"] < 0.9, rep
    assert rep["listed_on"] > 0 and rep["miss_listed"] == 0 and rep["odd_bad"] == 0, rep
    assert rep["cap_cases"] == 8 and rep["cap_bad"] == 0, rep


def test_null_handles(rtx):
    """Each entry point refuses a null handle with RTX_ERR_INVALID and names
    itself, before any HIP call (this test runs without a GPU)."""
    lib = rtx.load_library()
    n = C.c_uint32(7)
    one = C.c_void_p(16)  # never dereferenced: the handle is checked first
    assert lib.rtx_features(None, one, one) == -1
    assert b"rtx_features" in lib.rtx_last_error() and b"rtx_features_rows" not in lib.rtx_last_error()
    assert lib.rtx_features_rows(None, 1, 0, 1, one, one) == -1
    assert b"rtx_features_rows" in lib.rtx_last_error()
    hit = rtx.rtx_hit()
    assert lib.rtx_pick(None, 0, 0, C.byref(hit)) == -1
    assert b"rtx_pick" in lib.rtx_last_error()
    ids = (C.c_uint32 * 1)(3)
    assert lib.rtx_mask_from_ids(None, one, ids, 1, 0, one, C.byref(n)) == -1
    assert b"rtx_mask_from_ids" in lib.rtx_last_error()
    assert lib.rtx_refine_masked(None, 8, one, 0, C.byref(n)) == -1
    assert b"rtx_refine_masked" in lib.rtx_last_error()
    assert n.value == 7 and hit.hit == 0


def test_header_declares_the_entry_points(rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    lib = rtx.load_library()
    flat = text.replace("*", " ")
    for name in NAMES:
        assert f" {name}(" in flat, name
        assert hasattr(lib, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", rtx.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    for name in NAMES:
        assert f" T {name}\n" in exported, name
    assert 'dlsym "rtx_features"' in text and "#define RTX_VERSION 145" in text
    assert "typedef struct rtx_hit" in text and C.sizeof(rtx.rtx_hit) == 72
    assert lib.rtx_version() == 145
    for method in ("features", "features_rows", "pick", "mask_from_ids", "refine_masked"):
        assert callable(getattr(rtx.Context, method)), method
