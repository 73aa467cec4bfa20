"""Adaptive refinement (include/rtx.h rtx_refine_adaptive), CPU only.

The rule — a pixel's error estimate after a step and which pixels a call
traces — lives in a HIP-free header (raytrace-we-gpu_amd/csrc/rtx_adaptive.h)
that the kernels, rtx_api.hip and tests/adaptive_check.cpp all compile; the
checker runs it on host memory, plain and as a stand-alone program under ASan
and UBSan, with fp contraction off. rtx_adaptive_error is the same text behind
the C-ABI and needs no GPU; the entry points refuse a null handle before they
touch HIP. The GPU side is test_gpu_refine_adaptive.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "adaptive_check.cpp")

NAMES = ("rtx_adaptive_error", "rtx_refine_adaptive", "rtx_refine_pending", "rtx_refine_counts", "rtx_refine_error")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "asan-ubsan"])
def test_error_and_mask_rule(tmp_path, flags):
    """E is +inf at n_old == 0, NaN sums give NaN, E equals the op-by-op
    restatement bit for bit on random and extreme inputs, the mask equals the
    brute-force restatement on 1x1, 1x5, 5x1, 3x3 and 17x9 images (NaN and
    +inf errors, +inf thresholds and caps included), and the argument rules."""
    exe = str(tmp_path / "adaptive_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0, (out.stdout, out.stderr)
    assert rep["inf_checks"] == 64 and rep["inf_bad"] == 0, rep
    assert rep["nan_checks"] == 6 and rep["nan_bad"] == 0, rep
    assert rep["eq_checks"] > 200000 and rep["eq_bad"] == 0, rep
    # 5 shapes x 40 maps, every pixel, and two cap cases near 2^32; neither all on nor all off
    assert rep["mask_checks"] == 40 * (1 + 5 + 5 + 9 + 153) + 2 and rep["mask_bad"] == 0, rep
    assert 0.2 < rep["mask_on"] / rep["mask_checks"] < 0.8, rep
    assert rep["arg_cases"] == 8 and rep["arg_bad"] == 0, rep


def error_restated(so, n0, sn, n1):
    """The formula of include/rtx.h in numpy float32 scalars (each operation
    rounds to fp32; numpy's float32 division and sqrt are correctly rounded)."""
    f = np.float32
    if n0 == 0:
        return f(np.inf)
    a, b, sf = f(n0), f(n1), f(n1 - n0)
    m0 = [f(v) / a for v in so]
    m1 = [f(v) / b for v in sn]
    d = (abs(m1[0] - m0[0]) + abs(m1[1] - m0[1])) + abs(m1[2] - m0[2])
    lum = (m1[0] + m1[1]) + m1[2]
    return (d * np.sqrt(a / sf)) / np.sqrt(lum + f(0.01))


def test_adaptive_error_through_the_abi(rtx):
    """rtx_adaptive_error needs no context and no GPU."""
    rng = np.random.default_rng(5)
    assert rtx.adaptive_error((1, 2, 3), 0, (2, 3, 4), 8) == np.inf
    assert np.isnan(rtx.adaptive_error((1, np.nan, 3), 8, (2, 3, 4), 16))
    assert np.isnan(rtx.adaptive_error((1, 2, 3), 8, (2, 3, np.nan), 16))
    assert rtx.adaptive_error((1, 2, 3), 8, (2, 4, 6), 16) == 0.0  # equal means
    with np.errstate(all="ignore"):
        for _ in range(2000):
            n0 = int(rng.integers(1, 500))
            n1 = n0 + int(rng.integers(1, 40))
            so = (rng.random(3) * n0).astype(np.float32)
            sn = (so + rng.random(3) * (n1 - n0) * 5).astype(np.float32)
            got, want = np.float32(rtx.adaptive_error(so, n0, sn, n1)), error_restated(so, n0, sn, n1)
            assert got.view(np.uint32) == np.float32(want).view(np.uint32), (so, n0, sn, n1, got, want)


def test_null_handles(rtx):
    lib = rtx.load_library()
    n = C.c_uint32(7)
    assert lib.rtx_refine_adaptive(None, 8, 0.1, 0, 0, C.byref(n)) == -1
    assert b"rtx_refine_adaptive" in lib.rtx_last_error()
    assert lib.rtx_refine_adaptive(None, 8, 0.1, 0, 0, None) == -1
    assert lib.rtx_refine_pending(None, 8, 0.1, 0, C.byref(n)) == -1
    assert b"rtx_refine_pending" in lib.rtx_last_error()
    assert n.value == 7
    buf = (C.c_uint32 * 4)()
    assert lib.rtx_refine_counts(None, buf, 16) == -1
    assert b"rtx_refine_counts" in lib.rtx_last_error()
    fbuf = (C.c_float * 4)()
    assert lib.rtx_refine_error(None, fbuf, 16) == -1
    assert b"rtx_refine_error" in lib.rtx_last_error()


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
    assert 'dlsym "rtx_refine_adaptive"' in text and "#define RTX_VERSION 145" in text
    assert lib.rtx_version() == 145
    for method in ("refine_adaptive", "refine_pending", "refine_counts", "refine_error"):
        assert callable(getattr(rtx.Context, method)), method
    assert callable(rtx.adaptive_error)
