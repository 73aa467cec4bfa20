"""Progressive refinement along the reference's RNG chain (include/rtx.h
rtx_refine), CPU only.

The chain-state file of rtx_cli (include/rtx_app.hpp write_chain_state /
read_chain_state) is host code: tests/chain_state_check.cpp writes states with
NaN, denormal, -0 and infinite values, reads them back bit for bit, and damages
the file in every way the reader must refuse. The new entry points decide
their bad arguments before they touch HIP, so those checks run without a GPU.
The GPU side is test_gpu_refine.py."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "raytrace-we-gpu_amd", "lib")

NAMES = ("rtx_refine", "rtx_refined_samples", "rtx_refine_state", "rtx_refine_export", "rtx_refine_import")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    if not os.path.exists(os.path.join(LIBDIR, "librtx.so")):
        pytest.fail("librtx.so missing: build first")
    exe = str(tmp_path_factory.mktemp("cs") / "chain_state_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-o", exe, os.path.join(ROOT, "tests", "chain_state_check.cpp"),
                    os.path.join(ROOT, "raytrace-we-gpu_amd", "csrc", "rtx_app.cpp"),
                    "-L", LIBDIR, "-lrtx", "-Wl,-rpath," + LIBDIR], check=True)
    return exe


def test_chain_state_file_round_trips_and_refuses(checker, tmp_path):
    """7x5, 1x1 and 64x3 states round-trip with identical bits; per size the
    reader refuses a truncated payload, a truncated header, a flipped magic
    byte, another version, a header width that disagrees with the length, a
    byte after the payload, another size, another world hash and another
    frame hash; a missing file; the hashes see every input."""
    out = subprocess.run([checker, str(tmp_path)], capture_output=True, text=True, timeout=60)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0 and rep["failures"] == 0, rep
    assert rep["round_trips"] == 3 and rep["refusals"] == 27, rep
    assert rep["hash_changes"] == 8 and rep["fnv_ok"] is True, rep


def test_chain_state_file_layout(checker, tmp_path):
    """Little-endian: magic, version 1, width, height, N, two 64-bit hashes,
    then width*height float4."""
    subprocess.run([checker, str(tmp_path)], check=True, capture_output=True, timeout=60)
    raw = open(tmp_path / "s7x5.bin", "rb").read()
    assert len(raw) == 40 + 7 * 5 * 16
    assert raw[:8] == b"RTXCHAIN"
    version, w, h, n = (int.from_bytes(raw[8 + 4 * i:12 + 4 * i], "little") for i in range(4))
    assert (version, w, h, n) == (1, 7, 5, 1007)
    assert int.from_bytes(raw[24:32], "little") == 0x0123456789abcdef ^ 7
    assert int.from_bytes(raw[32:40], "little") == 0xfedcba9876543210 ^ 5
    assert raw[40:44] == (0x7fc00000).to_bytes(4, "little")  # the first special value, a NaN, bit for bit


def test_null_handles(rtx):
    lib = rtx.load_library()
    assert lib.rtx_refine(None, 1, 0) == -1
    assert b"rtx_refine" in lib.rtx_last_error()
    assert lib.rtx_refined_samples(None) == 0
    assert not lib.rtx_refine_state(None)
    buf = (C.c_float * 4)()
    assert lib.rtx_refine_export(None, buf, 16) == -1
    assert b"rtx_refine_export" in lib.rtx_last_error()
    assert lib.rtx_refine_import(None, buf, 16, 1) == -1
    assert b"rtx_refine_import" in lib.rtx_last_error()


def test_header_declares_the_refinement(rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    lib = rtx.load_library()
    for name in NAMES:
        assert f" {name}(" in text.replace("*", " "), name
        assert hasattr(lib, name), name
    assert 'dlsym "rtx_refine"' in text and "#define RTX_VERSION 145" in text
    assert lib.rtx_version() == 145
    assert callable(rtx.Context.refine) and isinstance(rtx.Context.refined_samples, property)
    assert callable(rtx.Context.refine_export) and callable(rtx.Context.refine_import)
