"""rtx_trace_paths_keyed and rtx_debug_paths_order (include/rtx.h), CPU only:
the header text, the exported symbols, the argument rules that are answered
before the context is looked at, and the HIP-free rules of
raytrace-we-gpu_amd/csrc/rtx_paths.h that the entry point and its key kernel
run — checked by tests/paths_order_check.cpp, a stand-alone program, plain and
under ASan and UBSan. The GPU side is test_gpu_paths_keyed.py."""
import ctypes as C
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "paths_order_check.cpp")
NAMES = ("rtx_trace_paths_keyed", "rtx_debug_paths_order")
INVALID = -1


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_rules_and_sort_passes(tmp_path, flags):
    """rtx_paths.h on the CPU: paths_keyed_args over 4,096 argument tuples
    equals the rule as include/rtx.h words it, first failure first; the default
    probe at 1,024 and 1,032 padded spheres; paths_two_phase at samples = p - 1,
    p, p + 1; paths_cost_bucket at 0, 1, 65534, 65535, 65536 and 0xFFFFFFFF;
    and 63 sorts (7 sizes around the workgroup's 2,048 records; equal,
    distinct, two-valued, probe-like and arbitrary keys) replayed pass by pass
    on arrays of exactly n words: every slot of perm written once and none
    outside, a permutation, min(key, 65535) non-increasing along it."""
    exe = str(tmp_path / "paths_order_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout, out.stderr)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["arg_checks"] == 2 * 2 * 4 * 4 * 8 * 2 * 4 and rep["arg_bad"] == 0, rep
    assert rep["rule_bad"] == 0, rep
    assert rep["sorts"] == 7 * 9 and rep["sort_bad"] == 0, rep
    assert rep["words"] == 9 * (1 + 63 + 65 + 2047 + 2048 + 2049 + 4099), rep
    assert rep["order_cost"] == 3 and rep["buckets"] == 65536, rep


def test_argument_rules_are_answered_before_the_handle_is_used(rtx):
    """Every RTX_ERR_INVALID case of rtx_trace_paths_keyed that does not need
    the world, on a handle that is an opaque block of zero bytes and no
    context: no GPU is needed, and nothing writes to the block. And
    rtx_trace_paths still refuses order 3."""
    lib = rtx.load_library()
    block = C.create_string_buffer(1 << 16)
    h = C.cast(block, C.c_void_p)
    p = C.c_void_p(C.addressof(block))  # a non-null buffer; never read or written
    # (d_queries, n, samples, flags, d_keys, probe, d_results, d_segments)
    cases = [((None, 5, 6, 0, None, 0, p, p), "d_queries"), ((p, 5, 6, 0, None, 0, None, p), "d_results"),
             ((None, 5, 6, 0, p, 2, None, None), "d_queries"),        # the first rule that fails answers
             ((p, 5, 6, 0, p, 2, None, None), "d_results"),
             ((p, 5, 0, 0, None, 0, p, None), "samples"), ((p, 0, 0, 0, None, 0, p, None), "samples"),  # an empty batch too
             ((None, 0, 0, 4, p, 1, None, None), "samples"),
             ((p, 5, 6, 4, None, 0, p, p), "flags"), ((p, 5, 6, 0x80000001, None, 2, p, p), "flags"),
             ((p, 5, 6, 0xFFFFFFFF, p, 2, p, p), "flags"),
             ((p, 5, 6, 0, p, 1, p, p), "probe"), ((p, 5, 6, 3, p, 0xFFFFFFFF, p, p), "probe"),
             ((None, 0, 1, 2, p, 7, None, None), "probe")]
    for args, word in cases:
        assert lib.rtx_trace_paths_keyed(h, *args) == INVALID, args
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_trace_paths_keyed:") and word in msg, msg
    assert lib.rtx_trace_paths_keyed(None, p, 5, 6, 0, None, 0, p, p) == INVALID and b"null ctx" in lib.rtx_last_error()
    assert lib.rtx_last_error().startswith(b"rtx_trace_paths_keyed:")
    host = (C.c_uint32 * 4)()
    assert lib.rtx_debug_paths_order(None, host, 16) == INVALID and b"rtx_debug_paths_order" in lib.rtx_last_error()
    assert lib.rtx_debug_paths_order(h, None, 16) == INVALID and b"rtx_debug_paths_order" in lib.rtx_last_error()
    # the plain entry point keeps its rule: 3 is no order of rtx_trace_paths
    assert lib.rtx_trace_paths(h, p, 5, 6, 0, 3, p, p) == INVALID
    msg = lib.rtx_last_error().decode()
    assert msg.startswith("rtx_trace_paths:") and "order" in msg, msg
    assert bytes(block.raw) == bytes(1 << 16)


def test_header_exports_and_upper_layers(rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    lib = rtx.load_library()
    flat = text.replace("*", " ")
    exported = subprocess.run(["nm", "-D", "--defined-only", rtx.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    for name in NAMES:
        assert f" {name}(" in flat, name
        assert hasattr(lib, name), name
        assert f" T {name}\n" in exported, name
    assert 'dlsym "rtx_trace_paths_keyed"' in text and "#define RTX_VERSION 145" in text and lib.rtx_version() == 145
    assert "enum { RTX_PATHS_ORDER_COST = 3 };" in text
    # additive: the plain entry point's declarations are as they were
    assert "enum { RTX_PATHS_LAMBERT_GUARD = 1, RTX_PATHS_CONTINUE = 2 };" in text
    assert "uint32_t flags, uint32_t order, void *d_results, void *d_segments);" in text
    assert rtx.PATHS_ORDER_COST == 3 and rtx.CAST_ORDERS == {"auto": 0, "given": 1, "coherent": 2}
    for method in ("trace_paths_keyed", "paths_order", "paths_last_order"):
        assert callable(getattr(rtx.Context, method)), method
    app = open(os.path.join(ROOT, "include", "rtx_app.hpp")).read()
    assert "bool TracePathsKeyed(const std::vector<rtx_path_query> &queries, uint32_t samples" in app
    cli = open(os.path.join(ROOT, "raytrace-we-gpu_amd", "csrc", "rtx_cli.cpp")).read()
    for option in ("--paths-order", "--paths-probe", "--paths-keys"):
        assert option in cli, option
    assert "rtx_trace_paths_keyed" in open(os.path.join(ROOT, "README.md")).read().split("What a ray sees")[1]
