"""The chain seed of a pixel and the zero-film twin of a path query
(include/rtx.h rtx_path_seed), CPU only.

The seed rule lives in a HIP-free header
(raytrace-we-gpu_amd/csrc/rtx_paths.h) that the host and tests/paths_check.cpp
compile; the checker runs it plain and as a stand-alone program under ASan and
UBSan. paths_cases.py builds a ray's twin frame and its queries; the oracle
shows here what makes the twin usable as an expectation: a twin's pixels do
not depend on its film size, and the cases do bounce."""
import json
import os
import subprocess

import numpy as np
import pytest

import paths_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "paths_check.cpp")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_rules_header(tmp_path, flags):
    """rtx_paths.h on the CPU: the seed of 50,000 pixels at four frame indices
    equals a restatement of the reference's baseHash chain and lies in [0, 1];
    samples * depth is accepted just below 2^32 and refused from it."""
    exe = str(tmp_path / "paths_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-o", exe, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout, out.stderr)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["seed_checks"] == 200000 and rep["seed_bad"] == rep["range_bad"] == rep["count_bad"] == 0, rep
    assert rep["ray_bytes"] == 32 and rep["seed_float"] == 3 and rep["d_float"] == 4


def test_path_seed_is_the_oracles_chain(rtx, oracle):
    """rtx_path_seed against oracle.base_hash chained as the render's
    pixel_seed does, for 1,000 pixels at frame_index 0, 1 and 0x7fffffff."""
    lib = rtx.load_library()
    rng = np.random.default_rng(5)
    xy = np.c_[rng.integers(0, 4096, 1000), rng.integers(0, 2304, 1000)]
    xy[:4] = [(0, 0), (1, 0), (0, 1), (4095, 2303)]
    for f in (0, 1, 0x7FFFFFFF):
        for x, y in xy:
            h = oracle.base_hash(int(x), int(y))
            if f:
                h = oracle.base_hash(h, 0x80000000 | f)
            want = np.float32(np.float32(h) / np.float32(4294967296.0))
            got = np.float32(lib.rtx_path_seed(int(x), int(y), f))
            assert got.view(np.uint32) == want.view(np.uint32), (x, y, f, got, want)
            assert rtx.path_seed(int(x), int(y), f).view(np.uint32) == want.view(np.uint32)
            assert pc.seed(x, y, f).view(np.uint32) == want.view(np.uint32)
    assert rtx.path_seed(3, 2) == rtx.path_seed(3, 2, 0) != rtx.path_seed(3, 2, 1)


def test_header_and_export(rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    lib = rtx.load_library()
    exported = subprocess.run(["nm", "-D", "--defined-only", rtx.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    assert "RTX_API float rtx_path_seed(uint32_t x, uint32_t y, uint32_t frame_index);" in text
    assert hasattr(lib, "rtx_path_seed") and " T rtx_path_seed\n" in exported
    assert 'dlsym "rtx_path_seed"' in text and "#define RTX_VERSION 145" in text and lib.rtx_version() == 145


def test_twin_frames_stand_for_their_ray(oracle):
    """The twin on the CPU oracle: at most a quarter of a case's rays see only
    sky (paths_cases.expect asserts it, and refuses a case that does not
    bounce), the sums are finite, a twin's pixels and its queries do not depend
    on its film size, and a query's seed is the twin pixel's."""
    import regime_cases as rc
    case = rc.world("rtiow11")
    o, L = pc.ray_recipe(48, 4100 + len("rtiow11"))
    e = pc.expect(case, o, L)
    assert np.isfinite(e.sums).all() and len(e.rays) == 48 * 32
    assert 2.0 < e.twin_segs.mean() / (32 * pc.SAMPLES) < pc.DEPTH
    big = pc.expect(case, o[:6], L[:6], w=16, h=8)
    small = e.sums.reshape(48, pc.H, pc.W, 3)[:6]
    assert (big.sums.reshape(6, 8, 16, 3)[:, :pc.H, :pc.W].view(np.uint32) == small.view(np.uint32)).all()
    assert (big.rays.reshape(6, 8, 16, 8)[:, :pc.H, :pc.W] == e.rays.reshape(48, pc.H, pc.W, 8)[:6])[..., :7].all()
    assert e.rays[2 * pc.W + 3, 3] == pc.seed(3, 2) and (e.rays[:32, 4:7] == (L[0] - o[0]).astype(np.float32)).all()
    with pytest.raises(AssertionError, match="only sky"):
        pc.expect(case, o[:4] + np.float32([0, 50, 0]), L[:4] + np.float32([0, 90, 0]))
    # hostile twins render: a zero direction and a NaN target
    hostile_o, hostile_L = o[:2].copy(), L[:2].copy()
    hostile_L[0] = hostile_o[0]
    hostile_L[1, 1] = np.nan
    h = pc.expect(case, hostile_o, hostile_L, all_sky_max=None)
    assert (h.twin_segs >= 32 * pc.SAMPLES).all()
