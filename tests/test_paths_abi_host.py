"""rtx_trace_paths (include/rtx.h), CPU only: the header text, the exported
symbols, the record layouts, the argument rules that are answered before the
context is looked at, and the HIP-free rules of
raytrace-we-gpu_amd/csrc/rtx_paths.h that the entry point and its kernel run —
checked by tests/paths_args_check.cpp, a stand-alone program, plain and under
ASan and UBSan. The GPU side is test_gpu_paths.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "paths_args_check.cpp")
NAMES = ("rtx_trace_paths", "rtx_paths_last_order")
INVALID = -1


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_argument_and_launch_rules(tmp_path, flags):
    """rtx_paths.h on the CPU: paths_args over 2,560 argument tuples equals the
    rule as include/rtx.h words it, first failure first; the world rules at
    the 2^32 boundary; the exact grid, the live-lane test and the record
    offsets at the ends of 32 bits; and 39 launches (the given order, a
    permutation, arbitrary perm words) played on host buffers of exactly n
    records, where every record is written once and none outside."""
    exe = str(tmp_path / "paths_args_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout, out.stderr)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["arg_checks"] == 2 * 2 * 4 * 4 * 8 * 5 and rep["arg_bad"] == 0, rep
    assert rep["world_bad"] == 0 and rep["grid_bad"] == 0, rep
    assert rep["launches"] == 39 and rep["play_bad"] == 0 and rep["lanes"] > 2 * 3 * 4099, rep
    assert rep["query_bytes"] == 32 and rep["result_bytes"] == 16 and rep["flag_mask"] == 3, rep


def test_argument_rules_are_answered_before_the_handle_is_used(rtx):
    """Every RTX_ERR_INVALID case of rtx_trace_paths that does not need the
    world, on a handle that is an opaque block of zero bytes and no context:
    no GPU is needed, and nothing writes to the block."""
    lib = rtx.load_library()
    block = C.create_string_buffer(1 << 16)
    h = C.cast(block, C.c_void_p)
    p = C.c_void_p(C.addressof(block))  # a non-null buffer; never read or written
    # (d_queries, n, samples, flags, order, d_results, d_segments)
    cases = [((None, 5, 6, 0, 1, p, p), "d_queries"), ((p, 5, 6, 0, 1, None, p), "d_results"),
             ((None, 5, 6, 0, 1, None, None), "d_queries"),         # the first rule that fails answers
             ((p, 5, 0, 0, 1, p, None), "samples"), ((p, 0, 0, 0, 1, p, None), "samples"),  # an empty batch too
             ((None, 0, 0, 0, 0, None, None), "samples"),
             ((p, 5, 6, 4, 1, p, p), "flags"), ((p, 5, 6, 0x80000001, 0, p, p), "flags"),
             ((p, 5, 6, 0xFFFFFFFF, 2, p, p), "flags"),
             ((p, 5, 6, 0, 3, p, p), "order"), ((p, 5, 6, 3, 0xFFFFFFFF, p, p), "order"),
             ((None, 0, 1, 2, 7, None, None), "order")]
    for args, word in cases:
        assert lib.rtx_trace_paths(h, *args) == INVALID, args
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_trace_paths:") and word in msg, msg
    assert lib.rtx_trace_paths(None, p, 5, 6, 0, 1, p, p) == INVALID and b"null ctx" in lib.rtx_last_error()
    assert lib.rtx_paths_last_order(None) == INVALID and b"rtx_paths_last_order" in lib.rtx_last_error()
    assert bytes(block.raw) == bytes(1 << 16)


def test_header_exports_and_record_sizes(rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    lib = rtx.load_library()
    flat = text.replace("*", " ")
    exported = subprocess.run(["nm", "-D", "--defined-only", rtx.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    for name in NAMES:
        assert f" {name}(" in flat, name
        assert hasattr(lib, name), name
        assert f" T {name}\n" in exported, name
    assert 'dlsym "rtx_trace_paths"' in text and "#define RTX_VERSION 145" in text and lib.rtx_version() == 145
    assert "typedef struct rtx_path_query " in text and "typedef struct rtx_path_result " in text
    assert "enum { RTX_PATHS_LAMBERT_GUARD = 1, RTX_PATHS_CONTINUE = 2 };" in text
    assert "not yet" not in open(os.path.join(ROOT, "README.md")).read().split("What a ray sees")[1][:400]


def test_dtypes_against_sizeof(tmp_path, rtx):
    """PATH_QUERY_DTYPE and PATH_RESULT_DTYPE against the compiler's sizeof and
    offsetof of the header's structs; a query's o and d sit where rtx_ray's do."""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtx.h"\n'
                   "int main(void) {\n"
                   '    printf("[%zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu]\\n", sizeof(rtx_path_query),\n'
                   "           offsetof(rtx_path_query, o), offsetof(rtx_path_query, seed), offsetof(rtx_path_query, d),\n"
                   "           offsetof(rtx_path_query, tag), sizeof(rtx_path_result), offsetof(rtx_path_result, sum),\n"
                   "           offsetof(rtx_path_result, seed), offsetof(rtx_ray, o), offsetof(rtx_ray, d));\n"
                   "    return 0;\n}\n")
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    got = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    q, r = rtx.PATH_QUERY_DTYPE, rtx.PATH_RESULT_DTYPE
    assert got == [q.itemsize, *(q.fields[k][1] for k in ("o", "seed", "d", "tag")), r.itemsize,
                   r.fields["sum"][1], r.fields["seed"][1], rtx.RAY_DTYPE.fields["o"][1], rtx.RAY_DTYPE.fields["d"][1]]
    assert got[:6] == [32, 0, 12, 16, 28, 16] and got[1] == got[8] and got[3] == got[9]
    assert (rtx.PATHS_LAMBERT_GUARD, rtx.PATHS_CONTINUE) == (1, 2)
    for method in ("trace_paths", "paths_last_order"):
        assert callable(getattr(rtx.Context, method)), method
    qs = rtx.path_queries([1, 2, 3], [[0, 0, 1], [0, 1, 0]], [0.25, 0.5], tags=[7, 8])
    assert qs.dtype == q and qs.shape == (2,) and qs.view(np.float32).reshape(2, 8)[1].tolist()[:7] == [1, 2, 3, 0.5, 0, 1, 0]
    assert qs["tag"].tolist() == [7, 8]
    app = open(os.path.join(ROOT, "include", "rtx_app.hpp")).read()
    assert "bool TracePaths(const std::vector<rtx_path_query> &queries, uint32_t samples" in app
