"""Are the culled layouts of cull_cases.py's worlds what DESIGN.md §3e says,
are their bounds conservative at all three sizes, and do the cameras reach
the sections and branches the frame tests are meant for? (CPU; the frames
themselves: test_gpu_cull_regimes.py.)

tests/cull_check.cpp builds each world's layout with rtx_cull.h's own code,
as rtx_upload_world does, checks its invariants, checks every sphere the
reference accepts against its own prefilter test and its three bounds with
the kernels' ops, and walks the layout as one lane of scan_culled does. The
assertions on what the walks and the oracle's first hits reach are conditions
on the inputs: if a seed or a camera misses one, change the seed or the
camera, not the bound.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import cull_cases as cc
from cases import grazing_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cull_check.cpp")]
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"]
NRAYS = cc.W * cc.H
NTHREADS = min(8, os.cpu_count() or 1)
GRAZING = 1500  # cases.grazing_rays per world


def _build(dirname, name, flags):
    exe = os.path.join(str(dirname), name)
    subprocess.run(GXX + flags + ["-o", exe] + SRCS, check=True)
    return exe


def _primary(oracle, camera):
    return cc.primary_rays(oracle.camera_look_at(**cc.camera_args(camera)))


_HITS = {}


def first_hits(oracle, world, camera):
    """The oracle's first hits of the camera's 2,304 primary rays: computed once."""
    if (world, camera) not in _HITS:
        hit = oracle.hit_world_f32(cc.world(world), _primary(oracle, camera))
        hit.setflags(write=False)
        _HITS[world, camera] = hit
    return _HITS[world, camera]


def bounce_rays(rays, hit, seed):
    """The rays that leave the first hits: from the hit point, half mirrored
    about the normal, half along the normal plus a random unit vector."""
    rng = np.random.default_rng(seed)
    on = hit[:, 0] == 1
    p, nrm, d = hit[on, 2:5].astype(np.float64), hit[on, 5:8].astype(np.float64), rays[on, 3:6].astype(np.float64)
    mirror = d - 2.0 * (d * nrm).sum(axis=1, keepdims=True) * nrm
    rnd = rng.normal(size=p.shape)
    diffuse = nrm + rnd / np.linalg.norm(rnd, axis=1, keepdims=True)
    out = np.where((np.arange(len(p)) % 2 == 0)[:, None], mirror, diffuse)
    return np.ascontiguousarray(np.c_[p, out], np.float32)


def _case_file(dirname, oracle, world, camera):
    """camera: one of cc.CAMERAS (its primary rays, then the bounce rays off
    their first hits), or "grazing_rays" (cases.grazing_rays over the world)."""
    w = cc.world(world)
    if camera == "grazing_rays":
        rays, nprim = grazing_rays(w.spheres, GRAZING, np.random.default_rng(len(world)), xaxis_frac=0.05), 0
    else:
        prim = _primary(oracle, camera)
        assert prim.shape == (NRAYS, 6)
        rays, nprim = np.concatenate([prim, bounce_rays(prim, first_hits(oracle, world, camera), 77)]), NRAYS
    path = os.path.join(str(dirname), f"{world}-{camera}.bin")
    with open(path, "wb") as f:
        f.write(np.array([w.count, len(rays), nprim, 0], np.uint32).tobytes())
        f.write(w.spheres.tobytes())
        f.write(np.ascontiguousarray(rays, np.float32).tobytes())
    return path


def _run(exe, path, *more):
    out = subprocess.run([exe, path, *more], capture_output=True, text=True, timeout=300)
    lines = out.stdout.strip().splitlines()
    assert lines, (out.returncode, out.stderr[-2000:])
    return out, json.loads(lines[-1])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("cull")
    return d, _build(d, "cull_check", [])


_REPORTS = {}


@pytest.fixture(scope="module")
def report_of(checker, oracle):
    """cull_check's report for a (world, batch), computed once; every report
    must be free of layout failures and of misses."""
    d, exe = checker

    def get(world, camera):
        if (world, camera) not in _REPORTS:
            res, rep = _run(exe, _case_file(d, oracle, world, camera))
            assert res.returncode == 0 and rep["failures"] == 0, (world, camera, rep, res.stderr[-2000:])
            _REPORTS[world, camera] = rep
        return _REPORTS[world, camera]
    return get


def test_cameras_are_the_librarys(rtx, oracle):
    for camera in cc.CAMERAS:
        a = rtx.camera_look_at(**cc.camera_args(camera))
        b = oracle.camera_look_at(**cc.camera_args(camera))
        assert bytes(a) == bytes(b), camera


@pytest.mark.parametrize("world", list(cc.WORLDS))
def test_layout_is_the_tables_row(report_of, world):
    """What rtx_cull.h builds for a world is its row: sections, positions, the
    flat section's first block, the level counts; and the layout's invariants
    hold (cull_check.cpp, part 1)."""
    rep = report_of(world, "default")
    want = cc.expected_info(world)
    assert (rep["large"], rep["other"], rep["flat"]) == cc.SECTIONS[world], rep
    assert rep["positions"] == want["cull_positions"] and rep["flat_lo"] == want["cull_flat_lo"], rep
    assert (rep["nblk"], rep["ngrp"], rep["nsg"], rep["nhg"]) == cc.levels(world), rep
    assert rep["has_flat"] == int(cc.SECTIONS[world][2] > 0), rep
    if rep["has_flat"]:
        assert np.float32(rep["flat_cy"]) == np.float32(cc.LAYER_Y), rep
    for k in ("bad_size", "bad_perm", "bad_pad", "bad_record", "bad_bound", "bad_flat_lo", "bad_height"):
        assert rep[k] == 0, (k, rep)
    lo = rep["flat_lo"]
    assert lo == 0 or lo == rep["nblk"] or lo % cc.CULL_ALIGN == 0


def test_the_shapes_the_worlds_are_for():
    """Each world has the structure its row of cull_cases.py's table names."""
    lv = {w: cc.levels(w) for w in cc.WORLDS}
    flat_lo = {w: cc.LAYOUT[w][1] for w in cc.WORLDS}
    # mixed: two bnd3 rows, the second a partial one; no level count is a multiple of 8
    assert lv["mixed"][3] == 2 and lv["mixed"][2] - 8 == 3 and all(c % 8 for c in lv["mixed"][:3])
    assert flat_lo["mixed"] == 512
    # no flat section: flat_lo = nblk, one partial bnd3 row
    for w, live in (("no_flat", 4), ("layer_no_run", 3)):
        assert flat_lo[w] == lv[w][0] and lv[w][2:] == (live, 1)
    assert (cc.world("layer_no_run").spheres[:, 1] == np.float32(cc.LAYER_Y)).sum() > 900  # ... though a layer exists
    assert flat_lo["all_flat"] == 0 and cc.SECTIONS["all_flat"][:2] == (0, 0)
    assert flat_lo["ground_flat"] == 512 and cc.SECTIONS["ground_flat"][:2] == (1, 0)  # 1 real block, 511 of padding
    assert flat_lo["wide"] == 1024 and lv["wide"][3] == 3
    # bimodal: a large section of many blocks that holds layer-height spheres too
    w = cc.world("bimodal")
    sec = cc.sections(w.spheres)
    assert (sec == 0).sum() > 64 * 8 and ((sec == 0) & (w.spheres[:, 1] == np.float32(cc.LAYER_Y))).sum() > 100
    # two_layers: the second equal-height set is in the non-flat section
    w = cc.world("two_layers")
    assert ((cc.sections(w.spheres) == 1) & (w.spheres[:, 1] == np.float32(0.75))).sum() == 450


@pytest.mark.parametrize("world", list(cc.WORLDS))
def test_bounds_are_conservative_on_the_real_layout(report_of, world):
    """Every sphere the reference accepts is flagged by its own prefilter test
    and passed by its block, group and super-group bounds, line test and half
    test, at t_min 1e-3 and 1e-6: the primary rays of every camera, the bounce
    rays off their first hits, and grazing rays over the world."""
    accepted = 0
    for camera in list(cc.CAMERAS) + ["grazing_rays"]:
        rep = report_of(world, camera)
        for k in ("sphere_missed", "block_missed", "group_missed", "super_missed"):
            assert rep[k] == 0, (world, camera, k, rep)
        assert rep["accepted"] > 0, (world, camera)
        accepted += rep["accepted"]
    assert accepted > 10000, accepted
    assert report_of(world, "grazing_rays")["unsafe_rays"] > 0  # (rays outside the safe range are among them)


@pytest.mark.parametrize("world", list(cc.WORLDS))
def test_every_section_is_hit(oracle, world):
    """Summed over the five cameras, each non-empty section's spheres are the
    first hit of at least 100 primary rays."""
    sec = cc.sections(cc.world(world).spheres)
    hits = np.zeros(3, int)
    for camera in cc.CAMERAS:
        hit = first_hits(oracle, world, camera)
        hits += np.bincount(sec[hit[hit[:, 0] == 1, 9].astype(int)], minlength=3)
    for k in range(3):
        if cc.SECTIONS[world][k]:
            assert hits[k] >= 100, (world, k, hits)


@pytest.mark.parametrize("world", ["all_flat", "ground_flat"])
def test_in_slab_camera_hits_the_layer(oracle, world):
    sec = cc.sections(cc.world(world).spheres)
    hit = first_hits(oracle, world, "in_slab")
    assert (sec[hit[hit[:, 0] == 1, 9].astype(int)] == 2).sum() >= 300


def test_both_bimodal_sections_are_hit(oracle):
    w = cc.world("bimodal")
    sec = cc.sections(w.spheres)
    hit = first_hits(oracle, "bimodal", "default")
    idx = hit[hit[:, 0] == 1, 9].astype(int)
    assert (w.spheres[idx, 3] == np.float32(0.41)).sum() >= 300  # the large radius
    assert (sec[idx] == 2).sum() >= 300


@pytest.mark.parametrize("world", list(cc.WORLDS))
def test_every_level_rejects_and_accepts(report_of, world):
    """For every camera, every level (all have more than one live entry) has
    at least one failed and one passed bound in one lane's walk."""
    assert min(cc.levels(world)[:3]) > 1
    for camera in cc.CAMERAS:
        rep = report_of(world, camera)
        for lv in ("block", "group", "super"):
            # (padding bounds, which fail for every ray, are not counted: *_failed_padding)
            assert rep[f"{lv}_failed"] + rep[f"{lv}_failed_flat"] > 0, (world, camera, lv, rep)
            assert rep[f"{lv}_passed"] + rep[f"{lv}_passed_flat"] > 0, (world, camera, lv, rep)
        # the walk tests flat bounds exactly where the layout has a flat section
        flat = sum(rep[f"{lv}_{r}_flat"] for lv in ("block", "group", "super") for r in ("failed", "passed"))
        assert (flat > 0) == (cc.SECTIONS[world][2] > 0), (world, camera, rep)


@pytest.mark.parametrize("world", list(cc.WORLDS))
def test_half_test_alone_rejects_bounds(report_of, world):
    """From inside the scene some bound passes the line test and fails the
    half test: the branch that separates the line test from the ray test."""
    for camera in ("in_slab", "grazing"):
        assert report_of(world, camera)["half_only_failed"] >= 1, (world, camera)


@pytest.mark.parametrize("world", ["mixed", "rtiow20"])
def test_grazing_camera_fills_a_default_list(report_of, world):
    """More than 24 blocks stepped for at least 50 rays: a list of the default
    build (24 entries) fills and the scan resumes inside a group."""
    assert report_of(world, "grazing")["rays_over_24_blocks"] >= 50, report_of(world, "grazing")


@pytest.mark.parametrize("world", list(cc.WORLDS))
def test_oracle_frames_are_finite(oracle, world):
    """NaN == NaN never decides a frame comparison: every frame is finite."""
    w = cc.world(world).at_spp(10)
    for camera in cc.CAMERAS:
        img, segs = oracle.render_rows(w, oracle.camera_look_at(**cc.camera_args(camera)), np.arange(cc.H),
                                       nthreads=NTHREADS)
        assert np.isfinite(img).all() and segs > 0, (world, camera)


def test_a_skipped_partial_entry_would_show(checker, oracle):
    """A frame test of the walk must change when the walk is broken. Without
    the spheres of one of `mixed`'s flat bnd3 entries (positions 512 * k on:
    k = 8 and 9, the second row's first two, or k = 10, its short last one
    with 76 spheres) the oracle's frame differs in more than 50 pixels: the
    `default` frame for 8 and 9, the `far` one for 10, which lies in the corner
    of the scene behind the `default` camera (where that camera's rays fail
    its bound: test_every_level_rejects_and_accepts)."""
    d, exe = checker
    w = cc.world("mixed")
    perm_path = os.path.join(str(d), "mixed.perm")
    res, rep = _run(exe, _case_file(d, oracle, "mixed", "default"), perm_path)
    assert res.returncode == 0 and rep["nsg"] == 11 and rep["flat_lo"] == 512, rep
    raw = np.fromfile(perm_path, np.uint8)
    npos = rep["positions"]
    perm, pad = raw[:4 * npos].view(np.uint32), raw[4 * npos:]
    assert len(pad) == npos
    rows = np.arange(cc.H)
    for entry, camera in ((8, "default"), (9, "default"), (10, "far")):
        frame = oracle.camera_look_at(**cc.camera_args(camera))
        full, _ = oracle.render_rows(w.at_spp(3), frame, rows, nthreads=NTHREADS)
        gone = np.unique(perm[512 * entry:512 * (entry + 1)][pad[512 * entry:512 * (entry + 1)] == 0])
        assert len(gone) == (76 if entry == 10 else 512) and 0 not in gone, (entry, len(gone))
        keep = np.setdiff1d(np.arange(w.count), gone)
        less = cc.Case(w.spheres[keep], w.mat_types[keep], w.mat_values[keep], 0, w.depth, 3)
        img, _ = oracle.render_rows(less, frame, rows, nthreads=NTHREADS)
        differ = int((img.view(np.uint32) != full.view(np.uint32)).any(axis=2).sum())
        assert differ > 50, (entry, camera, differ)


def test_cull_check_under_sanitizers(tmp_path, checker, oracle):
    """The same stand-alone checker built with -fsanitize=address,undefined on
    the flat-first layout from inside the slab, the widest layout, and the one
    with 511 padding blocks: no report, same JSON."""
    exe = _build(tmp_path, "cull_check_san", ["-g", "-fsanitize=address,undefined",
                                              "-fno-sanitize-recover=undefined"])
    _, plain = checker
    for world, camera in (("all_flat", "in_slab"), ("wide", "grazing"), ("ground_flat", "default")):
        path = _case_file(tmp_path, oracle, world, camera)
        out, rep = _run(exe, path)
        assert out.returncode == 0, (world, camera, rep, out.stderr[-2000:])
        assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-2000:]
        assert rep["failures"] == 0 and rep == _run(plain, path)[1], (world, camera, rep)
