"""Do the hostile inputs of hostile_cases.py do what they are meant to?
(CPU; the GPU side: test_gpu_hostile_inputs.py.)

A GPU test "about non-finite roots" means something only while the oracle
says its rays have them, and a frame test "with NaN rays mid-path" only while
the paths do meet them. The first half of this file asserts those conditions
from the oracle alone; if a seed misses one, change the seed, not the bound.

The second half runs the host halves of the scan (the prefilter's line test,
the layer grid's walks, the layout builder) over the same ray classes and
degenerate worlds, as the stand-alone checkers they already are, built once
plain and once with -fsanitize=address,undefined,float-cast-overflow: a NaN or
infinite coordinate must never reach a float-to-int conversion or an index.
"""
import json
import os
import subprocess

import numpy as np
import pytest

import hostile_cases as hc
import regime_cases as rc
from cases import grazing_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 36


# ---- ray conditions -----------------------------------------------------------
def _shares(oracle, world, rays, t_min=0.001):
    rec = oracle.hit_world_f32(world, rays, t_min)
    nonfinite = (rec[:, 0] == 1) & ~np.isfinite(rec[:, 1])
    other = nonfinite & (rec[:, 9] != world.count - 1)
    return nonfinite.mean(), (other.sum() / nonfinite.sum() if nonfinite.any() else 0.0)


@pytest.mark.parametrize("ext,n", [(4, 66), (11, 486), (25, 2500)])
def test_ray_classes_have_the_roots_they_are_meant_to(oracle, ext, n):
    world, exact, classes = hc.degenerate_world(ext)
    assert world.count == n and len(exact) >= 2
    assert len(classes) == 36 and all(r.shape == (64, 6) for r in classes.values())
    for name in hc.ALWAYS_NONFINITE:
        share, other = _shares(oracle, world, classes[name])
        print(f"ext {ext} {name}: non-finite hits {share:.2f}, winner not n-1 {other:.2f}")
        assert share >= 0.9, (name, share)
    for name in hc.ORDER_DEPENDENT:
        share, other = _shares(oracle, world, classes[name])
        print(f"ext {ext} {name}: non-finite hits {share:.2f}, winner not n-1 {other:.2f}")
        assert share >= 0.4 and other >= 0.5, (name, share, other)


@pytest.mark.parametrize("ext", [4, 11, 25])
def test_grazing_rays_meet_the_degenerate_spheres(oracle, ext):
    world, _, _ = hc.degenerate_world(ext)
    rays = grazing_rays(world.spheres, 3000, np.random.default_rng(300 + ext), xaxis_frac=0.05)
    rec = oracle.hit_world_f32(world, rays)
    hit = rec[:, 0] == 1
    radius = world.spheres[rec[hit, 9].astype(int), 3]
    print(f"ext {ext}: grazing hits {hit.mean():.3f}, winners with r = 0: {(radius == 0).sum()}, r < 0: {(radius < 0).sum()}")
    assert hit.mean() >= 0.5
    assert (radius == 0).any() and (radius < 0).any()


def test_degenerate_worlds_take_the_scan_paths_they_are_meant_for():
    """The shares of degenerate_spheres, the sphere counts the GPU tests'
    scan forms hang on, and the minimal divergence case's arithmetic."""
    for ext, n in ((4, 66), (11, 486), (25, 2500)):
        world, exact, _ = hc.degenerate_world(ext)
        base = hc.oracle.random_world(ext)[0]
        sph = world.spheres
        changed = (sph.view(np.uint32) != base.view(np.uint32)).any(axis=1)
        assert not changed[0] and 0.15 * n <= changed.sum() <= 0.27 * n, changed.sum()
        k = len(exact)
        assert (sph[:, 3] == 0).sum() == 2 * k and (np.signbit(sph[:, 3]) & (sph[:, 3] == 0)).sum() == k
        assert (sph[:, 3] < 0).sum() == k and (sph[:, 3] == np.float32(1e-30)).sum() == k
        assert ((sph[1:, :3] == sph[:-1, :3]).all(axis=1)).sum() >= k
        assert (sph[exact] * 8 == np.round(sph[exact] * 8)).all() and (sph[exact, 3] >= 0.125).all()
    assert 66 % 8 == 2  # the plain scan's padded last block
    for name, v in hc.large_variants(hc.degenerate_world(25)[0].spheres).items():
        assert np.abs(v).max() == np.float32(1e15), name
    sph, rays, k = hc.divergence_case()
    o, d, c, r = rays[0, :3], rays[0, 3:], sph[:, :3], sph[:, 3]
    with np.errstate(over="ignore", invalid="ignore"):
        a = np.float32(d[1] * d[1])
        oc = o[None] - c
        cc = (oc[:, 0] * oc[:, 0] - r * r).astype(np.float32)  # oc.y = oc.z = 0: exact
        disc = np.float32(0.0) - a * cc
    assert np.isinf(a) and (oc[:, 1:] == 0).all() and cc[k] == 0 and (np.delete(cc, k) > 0).all()
    assert np.isnan(disc[k]) and (np.delete(disc, k) == -np.inf).all()
    assert k // 8 == 1 and len(sph) == 21  # a whole batch of 8 around it, and a padded last one after


# ---- frame conditions -----------------------------------------------------------
def _frame(oracle):
    return oracle.camera_look_at(W, H, aspect=W / H)


@pytest.mark.parametrize("ext", [4, 11, 25])
def test_hostile_materials_put_nan_rays_mid_path(oracle, ext):
    """With a scattering last sphere the NaN rays a hostile material makes
    re-hit sphere n - 1 until `depth`; with an unknown material there the path
    ends at once. The difference is the number of NaN segments traced."""
    rows, seed = np.arange(H), hc.MATERIAL_SEED[ext]
    nt = min(8, os.cpu_count() or 1)
    img, lam = oracle.render_rows(hc.hostile_materials(ext, "lambert", seed), _frame(oracle), rows, nthreads=nt)
    _, unk = oracle.render_rows(hc.hostile_materials(ext, "unknown", seed), _frame(oracle), rows, nthreads=nt)
    plain, _ = oracle.render_rows(hc.hostile_materials(ext, "lambert", seed, untouched=True), _frame(oracle), rows,
                                  nthreads=nt)
    differ = (img.view(np.uint32) != plain.view(np.uint32)).any(axis=2).mean()
    print(f"ext {ext}: segments {lam} (last = lambert) vs {unk} (unknown): {(lam - unk) / lam:.3f} extra; "
          f"{differ:.3f} of the pixels differ from the untouched materials")
    assert lam - unk >= 0.15 * lam, (lam, unk)
    assert differ >= 0.25, differ


def test_hostile_frames_are_what_they_say(oracle):
    """nan_origin: every primary ray has a NaN o.x and d.x, every sample runs to `depth` on
    sphere n - 1 (Lambertian) and is black; zero_d: every direction is 0, the
    same; huge_d: |d|^2 overflows over most of the frame."""
    world = hc.hostile_materials(11, "lambert", hc.MATERIAL_SEED[11])
    full = W * H * world.spp * world.depth
    for kind in ("nan_origin", "zero_d"):
        frame = hc.hostile_frame(_frame(oracle), kind)
        rays = rc.primary_rays(frame)
        assert np.isnan(rays[:, [0, 3]]).all() if kind == "nan_origin" else (rays[:, 3:] == 0).all()
        img, segs = oracle.render_rows(world, frame, np.arange(H), nthreads=min(8, os.cpu_count() or 1))
        assert segs == full and (img[..., :3] == 0).all(), (kind, segs)
    rays = rc.primary_rays(hc.hostile_frame(_frame(oracle), "huge_d"))
    with np.errstate(over="ignore"):
        a = (rays[:, 3:] * rays[:, 3:]).sum(axis=1, dtype=np.float32)
    assert np.isinf(a).mean() >= 0.5 and np.isfinite(rays).all()


# ---- the host halves of the scan under sanitizers ----------------------------------
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-mfma"]
SAN = ["-g", "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=undefined"]
HOST = os.path.join(ROOT, "raytrace-we-gpu_amd", "csrc", "rtx_host.cpp")


def _build_both(tmp_path, name, extra=()):
    srcs = [os.path.join(ROOT, "tests", name + ".cpp")] + list(extra)
    exes = []
    for tag, flags in (("plain", []), ("san", SAN)):
        exe = str(tmp_path / f"{name}_{tag}")
        subprocess.run(GXX + flags + ["-o", exe] + srcs, check=True)
        exes.append(exe)
    return exes


def _report(exe, args):
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    lines = out.stdout.strip().splitlines()
    assert lines, (out.returncode, out.stderr[-2000:])
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-2000:]
    return out, json.loads(lines[-1])


def _both_agree(tmp_path, name, args, extra=()):
    plain, san = _build_both(tmp_path, name, extra)
    out, rep = _report(san, args)
    assert out.returncode == 0 and rep["failures"] == 0, (rep, out.stderr[-2000:])
    pout, prep = _report(plain, args)
    assert pout.returncode == 0 and prep == rep, (prep, rep)
    print(rep)
    return rep


def test_prefilter_check_hostile_under_sanitizers(tmp_path):
    """Every 7th case a hostile ray, the next a degenerate radius: no
    discriminant that is not negative, NaN included, goes unflagged."""
    rep = _both_agree(tmp_path, "prefilter_check", ["400000", "7"])
    assert rep["missed"] == 0 and rep["hostile_rays"] > 50_000 and rep["hostile_radii"] > 50_000, rep
    assert rep["hostile_nan_discs"] > 20_000 and rep["hostile_reference_candidates"] > rep["hostile_nan_discs"], rep


def test_grid_check_hostile_under_sanitizers(tmp_path):
    """Degenerate layers, every 5th ray hostile; the rays the line test sends
    away are still walked (grid_walk, grid_stretch), most of them to a give-up
    exit."""
    rep = _both_agree(tmp_path, "grid_check", ["60", "2000", "5"])
    assert rep["missed"] == 0 and rep["far_missed"] == 0, rep
    assert rep["hostile_rays"] > 15_000 and rep["hostile_walked"] > 10_000 and rep["hostile_gave_up"] > 10_000, rep


def test_grid_coop_check_hostile_under_sanitizers(tmp_path):
    """The wave's items over degenerate layers with hostile lanes: no cell
    index outside the grid, a wave with a hostile lane gives up."""
    rep = _both_agree(tmp_path, "grid_coop_check", ["60", "2000", "50000", "5"])
    assert rep["missed_rays"] == 0 and rep["waves_wrong"] == 0 and rep["hostile_cells_outside"] == 0, rep
    assert rep["hostile_rays"] > 15_000 and rep["hostile_walked"] > 10_000 and rep["hostile_gave_up"] > 10_000, rep


def test_layout_check_hostile_under_sanitizers(tmp_path):
    """The layout builder and the grid over position blocks on degenerate
    versions of the RTIOW worlds and the interleaved scenes, every 5th ray
    hostile."""
    rep = _both_agree(tmp_path, "layout_check", ["600", "400", "5"], [HOST])
    assert rep["missed"] == 0 and rep["layouts"] >= 90, rep
    assert rep["hostile_rays"] > 15_000 and rep["hostile_walked"] > 10_000, rep


def _regime_file(dirname, tag, world, rays, use_layout):
    path = os.path.join(str(dirname), f"{tag}.bin")
    with open(path, "wb") as f:
        f.write(np.array([world.count, len(rays), use_layout, 0], np.uint32).tobytes())
        f.write(np.ascontiguousarray(world.spheres, np.float32).tobytes())
        f.write(np.ascontiguousarray(rays, np.float32).tobytes())
    return path


def test_regime_check_hostile_under_sanitizers(tmp_path, oracle):
    """regime_check reads a case file: the degenerate worlds the GPU tests
    upload (66 and 486 spheres, r3_full) with every hostile class and the
    primary rays of the three hostile frames. The layouts and grids are the
    ones the GPU tests rely on; every NaN, infinite, zero and far ray leaves
    grid_stretch by a give-up exit, and no item names a cell outside the grid
    (std::vector::at)."""
    plain, san = _build_both(tmp_path, "regime_check", [HOST])
    frames = np.concatenate([rc.primary_rays(hc.hostile_frame(_frame(oracle), k)) for k in hc.HOSTILE_FRAMES])
    for key, layout in ((4, 1), (11, 1), ("r3_full", 1)):
        world, _, classes = hc.degenerate_world(key)
        rays, where = hc.grouped(classes)
        path = _regime_file(tmp_path, f"hostile-{key}", world, np.concatenate([rays, frames]), layout)
        out, rep = _report(san, [path])
        assert out.returncode == 0 and rep["failures"] == 0, (key, rep, out.stderr[-2000:])
        assert rep == _report(plain, [path])[1], key
        print(key, rep)
        assert rep["rays"] == len(rays) + len(frames)
        assert rep["valid"] == 1 and rep["layout"] == 1 and rep["grid"] == 1, (key, rep)
        # |o|^2 not <= 64^2 (a NaN or infinite origin component, the four |o| classes, the
        # NaN-origin frame) leaves by the distance exit, a NaN or infinite direction component
        # by the other one; a zero direction is "parallel and outside" or has no end
        assert rep["far"] >= 9 * 64 + 4 * 64 + W * H and rep["gave_up"] >= 9 * 64, (key, rep)
