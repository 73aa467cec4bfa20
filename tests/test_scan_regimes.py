"""Do the cases of regime_cases.py reach the branches they are meant for?
(CPU; the frames themselves: test_gpu_scan_regimes.py.)

tests/regime_check.cpp builds each world's layout, or the grid over its
scene-order flat run, with the headers' own code, as rtx_upload_world chooses
between them, and classifies the 2,304 pixel-centre primary rays of every
camera with grid_stretch. The assertions are conditions on the inputs: a
frame test "through the long shared walks" means something only while its
camera does send rays down them. If a seed or a camera misses one, change the
seed or the camera, not the bound.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import regime_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "regime_check.cpp"),
        os.path.join(ROOT, "raytrace-we-gpu_amd", "csrc", "rtx_host.cpp")]
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"]
NRAYS = rc.W * rc.H


def _build(dirname, name, flags):
    exe = os.path.join(str(dirname), name)
    subprocess.run(GXX + flags + ["-o", exe] + SRCS, check=True)
    return exe


def _case_file(dirname, oracle, world, camera):
    w = rc.world(world)
    rays = rc.primary_rays(oracle.camera_look_at(**rc.camera_args(camera)))
    assert rays.shape == (NRAYS, 6)
    path = os.path.join(str(dirname), f"{world}-{camera}.bin")
    with open(path, "wb") as f:
        f.write(np.array([w.count, len(rays), rc.expected_info(world)["layout"], 0], np.uint32).tobytes())
        f.write(w.spheres.tobytes())
        f.write(rays.tobytes())
    return path


def _run(exe, path):
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    lines = out.stdout.strip().splitlines()
    assert lines, (out.returncode, out.stderr[-2000:])
    return out, json.loads(lines[-1])


@pytest.fixture(scope="module")
def reports(tmp_path_factory, oracle):
    """regime_check's report for every (world, camera): computed once."""
    d = tmp_path_factory.mktemp("regime")
    exe = _build(d, "regime_check", [])
    out = {}
    for world in rc.WORLDS:
        for camera in rc.CAMERAS:
            res, rep = _run(exe, _case_file(d, oracle, world, camera))
            assert res.returncode == 0 and rep["failures"] == 0, (world, camera, rep, res.stderr[-2000:])
            assert rep["rays"] == NRAYS
            out[world, camera] = rep
    return out


def test_cameras_are_the_librarys(rtx, oracle):
    """The GPU tests build their frames with rtx.camera_look_at, this file with
    the oracle's: the same bytes, so the same primary rays."""
    for camera in rc.CAMERAS:
        a = rtx.camera_look_at(**rc.camera_args(camera))
        b = oracle.camera_look_at(**rc.camera_args(camera))
        assert bytes(a) == bytes(b), camera


@pytest.mark.parametrize("world", list(rc.WORLDS))
def test_layout_and_grid_as_the_regime_table_says(reports, world):
    """What the headers build for a world is its row of the regime table:
    whether it has a layout, its padded position count, the flat run, the
    grid and, for the strips, the grid's size."""
    rep = reports[world, "default"]
    want = rc.expected_info(world)
    w = rc.world(world)
    # the layer the headers find is the one the construction laid down
    usable = rc.LAYER_MIN <= w.layer <= rc.LAYER_MAX
    assert rep["valid"] == int(usable) and rep["n_layer"] == (w.layer if usable else 0), rep
    for k in ("layout", "layout_positions", "flat_lo", "flat_hi", "grid", "grid_nx", "grid_nz"):
        if k in want:
            assert rep[k] == want[k], (world, k, rep, want)
    if rep["grid"]:
        # (two_layers: the set whose first sphere comes first)
        assert np.float32(rep["flat_cy"]) == np.float32(rc.LAYER_Y), rep


GRID_WORLDS = [w for w in rc.WORLDS if rc.expected_info(w)["grid"]]


def test_which_worlds_have_a_grid():
    assert set(GRID_WORLDS) == set(rc.WORLDS) - {"layer15", "no_layer"}


@pytest.mark.parametrize("world", GRID_WORLDS)
def test_far_camera_gives_up_by_distance(reports, world):
    assert reports[world, "far"]["far"] == NRAYS, reports[world, "far"]


@pytest.mark.parametrize("world", ["rtiow11", "lds_full", "r3_small", "r3_full", "strip"])
def test_grazing_camera_walks_17_columns_or_more(reports, world):
    assert reports[world, "grazing"]["items_17_48"] >= 100, reports[world, "grazing"]


@pytest.mark.parametrize("world", ["strip", "strip_r3"])
def test_along_strip_passes_the_step_limit(reports, world):
    rep = reports[world, "along_strip"]
    assert rep["gave_up"] >= 50 and rep["items_17_48"] >= 300, rep
    assert rep["far"] == 0, rep


@pytest.mark.parametrize("world", GRID_WORLDS)
def test_top_down_camera_has_short_walks_only(reports, world):
    rep = reports[world, "top_down"]
    assert rep["far"] == 0 and rep["gave_up"] == 0, rep
    assert rep["items_5_16"] == 0 and rep["items_17_48"] == 0, rep
    assert rep["items_1_4"] + rep["none"] == NRAYS and rep["items_1_4"] > 0, rep


@pytest.mark.parametrize("world", GRID_WORLDS)
def test_default_camera_mixes_misses_and_short_walks(reports, world):
    rep = reports[world, "default"]
    assert rep["none"] >= 300, rep
    assert rep["items_1_4"] + rep["items_5_16"] >= 1000, rep


def test_in_plane_frame_meets_reversed_ties(oracle):
    """No camera_look_at frame has a ray exactly in the plane z = 0, so the
    six cameras meet `twins`' ties only at its coincident duplicates, where
    position order is scene order. rc.in_plane's frame does: every primary
    ray has o.z = d.z = 0, more than 300 of the 2,304 hit one of a column's
    mirror twins, and the oracle's winner is the later scene index, which is
    the twin at z = -0.25: the one that comes *first* in position order (the
    median split sorts a column by z)."""
    w = rc.world("twins")
    rays = rc.primary_rays(rc.in_plane(oracle.camera_look_at(**rc.camera_args("default"))))
    assert (rays[:, 2] == 0).all() and (rays[:, 5] == 0).all()
    hit = oracle.hit_world_f32(w, rays)
    idx = hit[:, 9].astype(int)
    sph = w.spheres
    big = (hit[:, 0] == 1) & (sph[np.clip(idx, 0, len(sph) - 1), 3] == np.float32(0.4))
    assert big.sum() > 300, big.sum()
    for i in np.unique(idx[big]):
        same = np.flatnonzero((sph[:, 0] == sph[i, 0]) & (np.abs(sph[:, 2]) == 0.25) & (sph[:, 3] == np.float32(0.4)))
        assert len(same) >= 2 and i == same.max() and sph[i, 2] == -0.25, (i, same)
    assert len(np.unique(idx[big])) >= 10  # many columns, not one


def test_in_plane_frame_shows_the_tie_choice(oracle):
    """A frame test of the tie rule must change when the rule is broken. With
    each column's twins swapped in scene order (geometry and materials move
    together, so the scene is the same set of spheres) every tie goes to the
    other twin: the oracle's in-plane frame then differs in more than 1,000
    of its 2,304 pixels, and its frame from the `default` camera in none."""
    w = rc.world("twins")
    sph, mt, mv = w.spheres.copy(), w.mat_types.copy(), w.mat_values.copy()
    big = np.flatnonzero(sph[:, 3] == np.float32(0.4))
    for a, b in zip(big[0::2], big[1::2]):  # a column's first and last sphere
        assert sph[a, 0] == sph[b, 0] and sph[a, 2] == -sph[b, 2]
        for arr in (sph, mt, mv):
            arr[[a, b]] = arr[[b, a]]
    swapped = rc.Case(sph, mt, mv, w.layer, w.depth, 3)
    rows = np.arange(rc.H)
    differ = {}
    for name in ("in_plane", "default"):
        frame = oracle.camera_look_at(**rc.camera_args("default"))
        if name == "in_plane":
            rc.in_plane(frame)
        a, _ = oracle.render_rows(w.at_spp(3), frame, rows, nthreads=min(8, os.cpu_count() or 1))
        b, _ = oracle.render_rows(swapped, frame, rows, nthreads=min(8, os.cpu_count() or 1))
        differ[name] = int((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).sum())
    assert differ["in_plane"] > 1000 and differ["default"] == 0, differ


def test_regime_check_under_sanitizers(tmp_path, oracle):
    """The same stand-alone checker built with -fsanitize=address,undefined on
    the step limit (strip, along_strip), the largest layout (r3_full, grazing)
    and a scene with no layer (no_layer, default): no report, same verdict."""
    exe = _build(tmp_path, "regime_check_san", ["-g", "-fsanitize=address,undefined",
                                                "-fno-sanitize-recover=undefined"])
    plain = _build(tmp_path, "regime_check", [])
    for world, camera in (("strip", "along_strip"), ("r3_full", "grazing"), ("no_layer", "default")):
        path = _case_file(tmp_path, oracle, world, camera)
        out, rep = _run(exe, path)
        assert out.returncode == 0, (world, camera, rep, out.stderr[-2000:])
        assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-2000:]
        assert rep["failures"] == 0 and rep == _run(plain, path)[1], (world, camera, rep)
