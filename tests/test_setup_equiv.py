"""The straight-line segment set-up against the early-return form it replaced,
on the CPU.

grid_stretch (rtx_grid.h) computes every output for every ray and decides the
outcome once at the end; the lane-mode render runs it, after line_test_setup
(rtx_prefilter.h), once per path segment. tests/setup_equiv_check.cpp keeps
the replaced form verbatim as the specification (and a copy of the line test,
which keeps its early return) and compares, with the headers' own host builds,
on the adversarial ray families of grid_check.cpp / grid_coop_check.cpp plus
level rays inside the slab, origins at the grid's range limit, signed zeros
and every hostile class: the same gives-up / never enters / n outcome for
every ray, bit-identical outputs for every ray with items, identical
grid_mask_items, and a bit-identical line test for every ray.
The GPU side is test_gpu_segment_setup.py.
"""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "setup_equiv_check.cpp")
GXX = ["g++", "-std=c++17", "-ffp-contract=off", "-mfma"]
SAN = ["-O1", "-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined"]


def _run(tmp_path, name, flags, args):
    exe = str(tmp_path / name)
    subprocess.run(GXX + flags + ["-o", exe, SRC], check=True)
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    print(rep)
    return out, rep


def test_straight_line_set_up_equals_the_early_return_form(tmp_path):
    """150 layers x 4,000 draws, every 7th ray hostile: no difference, and at
    least 1,000 rays of every outcome (safe and unsafe line tests; stretches
    with items, without, given up; level rays inside the slab; origins within
    a few ulps of the range limit)."""
    out, rep = _run(tmp_path, "setup_equiv_check", ["-O2"], ["150", "4000", "1000", "7"])
    assert out.returncode == 0, (rep, out.stderr)
    assert rep["failures"] == 0 and rep["line_differ"] == 0 and rep["stretch_differ"] == 0 and rep["mask_differ"] == 0
    assert rep["rays"] > 400_000
    for k in ("line_safe", "line_unsafe", "stretch_items", "stretch_none", "stretch_gave_up", "dy0_inside_slab",
              "near_omax"):
        assert rep[k] >= 1000, (k, rep)


def test_set_up_check_under_sanitizers(tmp_path):
    """The same stand-alone checker built with -fsanitize=address,undefined and
    float-cast-overflow: the straight-line form runs its conversions for rays
    the early returns kept away from them (NaN, infinite, far), and they must
    stay defined. No report, same verdict."""
    out, rep = _run(tmp_path, "setup_equiv_check_san", SAN, ["40", "2000", "200", "3"])
    assert out.returncode == 0, (rep, out.stderr[-2000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-2000:]
    assert rep["failures"] == 0
