"""The wave-cooperative walk of the layer grid, checked on the CPU.

The lane-mode render needs only the union of its lanes' grid masks, so the
wave cuts every lane's stretch of the slab into independent items (one per
column of cells) and shares them evenly (rtx_grid.h "the wave-cooperative
walk", rtx_kernels.hip grid_wave_mask). The DDA (grid_walk) stays the
specification whose sufficiency the header proves: the items' cells must
contain the DDA's for every ray. tests/grid_coop_check.cpp checks that with
the header's own code, and emulates the wave's sharing on the host. The GPU
side is test_gpu_grid_coop.py.
"""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "grid_coop_check.cpp")
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"]


def test_items_contain_the_dda_and_the_wave_shares_them(tmp_path):
    """RTIOW and random layers, the adversarial ray families of grid_check.cpp
    (near-tangent at every slope down to grazing, through cell corners, along
    the axes, leaving a sphere's surface, origins on the slab's and the box's
    faces, d components of 0) plus random rays: over at least 1,000,000 rays
    where the DDA applies, no cell of the DDA is missing from the items
    (the checker fails below that count). The host emulation of the 64-lane
    distribution (prefix, owner marks, rounds) reproduces the OR of the
    per-ray masks on every wave shape: no items, one lane holding every item
    over several rounds, totals of 63, 64, 65 and 128, inactive lanes in
    between, a give-up lane (~0). The block-mask bloat over the DDA stays
    small."""
    exe = str(tmp_path / "grid_coop_check")
    subprocess.run(GXX + ["-o", exe, SRC], check=True)
    out = subprocess.run([exe, "400", "4000", "1000000"], capture_output=True, text=True, timeout=120)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    print(rep)
    assert out.returncode == 0, (rep, out.stderr)
    assert rep["missed_rays"] == 0 and rep["checked"] >= 1_000_000, rep
    assert rep["waves"] > 10_000 and rep["waves_wrong"] == 0, rep
    # the items rarely give up where the DDA does not, and cost few extra blocks
    assert rep["items_every_block"] < 0.01 * rep["checked"], rep
    assert 0.99 < rep["block_mask_bloat"] < 1.05, rep


def test_checker_fails_without_the_epsilon(tmp_path):
    """Sensitivity: with the epsilon at 0 (the minor interval and the column
    range unpadded) the same run must find DDA cells outside the items."""
    exe = str(tmp_path / "grid_coop_check_eps0")
    subprocess.run(GXX + ["-DRTX_GRID_COOP_EPS=0.0f", "-o", exe, SRC], check=True)
    out = subprocess.run([exe, "400", "4000", "1000000"], capture_output=True, text=True, timeout=120)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 1 and rep["missed_rays"] > 0 and rep["waves_wrong"] == 0, rep
