"""rtx_trace_film (include/rtx.h), CPU only: the HIP-free rules of
raytrace-we-gpu_amd/csrc/rtx_film.h that the entry point, its kernel and the
generators run — checked by tests/film_check.cpp, a stand-alone program, plain
and under ASan and UBSan — the header, the exported symbols and the record
layouts, the argument rules that are answered before the context is looked at,
the set-up conditions of the GPU cases on the CPU oracle (film_cases.py), and
rtx_film_camera against a numpy fp64 restatement of its two models. The GPU
side is test_gpu_film.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import film_cases as fc
import hostile_cases as hc
import paths_cases as pc
import regime_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "film_check.cpp")
NAMES = ("rtx_trace_film", "rtx_film_last_order", "rtx_film_from_frame", "rtx_film_camera")
INVALID = -1
f32 = np.float32

# (rays, recipe seed, recipe scale) and the all-sky frames counted on the CPU oracle, without a lens and with
# lens_r = 0.05 in every frame; the first five are test_gpu_paths.RECIPES' tuples
RECIPES = {"test_world": (16, 4110, 0.25), "rtiow11": (48, 4107, 1.0), "r2_mixed": (48, 4108, 1.0),
           "r3_small": (48, 4108, 1.0), "no_layer": (48, 4108, 1.0), "rw25": (16, 4125, 25 / 11)}
ALL_SKY = {"test_world": (0, 0), "rtiow11": (3, 3), "r2_mixed": (3, 3), "r3_small": (2, 2), "no_layer": (2, 2),
           "rw25": (2, 1)}


def case_of(oracle, name):
    if name == "test_world":
        return hc.Case(*oracle.test_world())
    if name == "rw25":
        return hc.Case(*oracle.random_world(25))
    return rc.world(name)


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_argument_launch_and_generator_rules(tmp_path, flags):
    """rtx_film.h on the CPU: film_args over 4,608 argument tuples equals the
    rule as include/rtx.h words it, first failure first; the record offsets at
    the ends of 32 bits in both record sizes; 48 launches (the given order, a
    permutation, arbitrary perm words; 64- and 96-byte records) played on host
    buffers of exactly n records, where every record is written once and none
    outside; rtx_film_from_frame's records against the frame's bytes, and its
    refusals in their order."""
    exe = str(tmp_path / "film_check")
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, (out.stdout, out.stderr)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["arg_checks"] == 2 * 2 * 4 * 4 * 12 * 6 and rep["arg_bad"] == 0, rep
    assert rep["offset_bad"] == 0, rep
    assert rep["launches"] == 48 and rep["play_bad"] == 0 and rep["lanes"] > 2 * 3 * 4099, rep
    assert rep["frame_records"] == 70 and rep["frame_bad"] == 0 and rep["refusal_bad"] == 0, rep
    assert rep["query_bytes"] == 64 and rep["lens_query_bytes"] == 96 and rep["flag_mask"] == 7, rep
    assert rep["struct_bytes"] == [64, 96], rep


def test_argument_rules_are_answered_before_the_handle_is_used(rtx):
    """Every RTX_ERR_INVALID case of rtx_trace_film that does not need the
    world, on a handle that is an opaque block of zero bytes and no context: no
    GPU is needed, and nothing writes to the block."""
    lib = rtx.load_library()
    block = C.create_string_buffer(1 << 16)
    h = C.cast(block, C.c_void_p)
    p = C.c_void_p(C.addressof(block))  # a non-null buffer; never read or written
    # (d_queries, n, samples, img_w, img_h, flags, order, d_results, d_segments)
    cases = [((None, 5, 6, 8, 4, 0, 1, p, p), "d_queries"), ((p, 5, 6, 8, 4, 0, 1, None, p), "d_results"),
             ((None, 5, 6, 8, 4, 0, 1, None, None), "d_queries"),       # the first rule that fails answers
             ((p, 5, 0, 8, 4, 0, 1, p, None), "samples"), ((None, 0, 0, 8, 4, 0, 0, None, None), "samples"),
             ((p, 5, 6, 8, 4, 8, 1, p, p), "flags"), ((p, 5, 6, 8, 4, 0x80000001, 0, p, p), "flags"),
             ((p, 5, 6, 8, 4, 0xFFFFFFFF, 2, p, p), "flags"),
             ((p, 5, 6, 8, 4, 0, 2, p, p), "coherent"), ((p, 5, 6, 8, 4, 7, 4, p, p), "order"),
             ((None, 0, 1, 8, 4, 2, 0xFFFFFFFF, None, None), "order")]
    for args, word in cases:
        assert lib.rtx_trace_film(h, *args) == INVALID, args
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_trace_film:") and word in msg, msg
    assert lib.rtx_trace_film(None, p, 5, 6, 8, 4, 0, 1, p, p) == INVALID and b"null ctx" in lib.rtx_last_error()
    assert lib.rtx_film_last_order(None) == INVALID and b"rtx_film_last_order" in lib.rtx_last_error()
    assert bytes(block.raw) == bytes(1 << 16)


def test_header_exports_and_dtypes(tmp_path, rtx):
    text = open(os.path.join(ROOT, "include", "rtx.h")).read()
    lib = rtx.load_library()
    flat = text.replace("*", " ")
    exported = subprocess.run(["nm", "-D", "--defined-only", rtx.LIB_PATH], capture_output=True, text=True,
                              check=True).stdout
    for name in NAMES:
        assert f" {name}(" in flat, name
        assert hasattr(lib, name), name
        assert f" T {name}\n" in exported, name
    assert 'dlsym "rtx_trace_film"' in text and "#define RTX_VERSION 145" in text and lib.rtx_version() == 145
    assert "enum { RTX_FILM_LENS = 4 };" in text and "enum { RTX_FILM_EQUIRECT = 0, RTX_FILM_FISHEYE = 1 };" in text
    names = ("o", "seed", "lower_left", "tag", "horizontal", "fx", "vertical", "fy")
    lens_names = ("lens_u", "lens_r", "lens_v", "reserved")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rtx.h"\nint main(void) {\n'
                   '    printf("[%zu, %zu", sizeof(rtx_film_query), sizeof(rtx_film_lens_query));\n'
                   + "".join(f'    printf(", %zu", offsetof(rtx_film_query, {k}));\n' for k in names)
                   + "".join(f'    printf(", %zu", offsetof(rtx_film_lens_query, {k}));\n' for k in lens_names)
                   + '    printf("]\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "sizes")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    got = json.loads(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    q, ql = rtx.FILM_QUERY_DTYPE, rtx.FILM_LENS_QUERY_DTYPE
    assert got == [q.itemsize, ql.itemsize, *(q.fields[k][1] for k in names), *(ql.fields[k][1] for k in lens_names)]
    assert got == [64, 96, 0, 12, 16, 28, 32, 44, 48, 60, 64, 76, 80, 92] and ql.fields["q"][1] == 0
    assert rtx.FILM_LENS == 4 and rtx.FILM_ORDERS == {"auto": 0, "given": 1, "coherent": 2, "cost": 3}
    for method in ("trace_film", "film_last_order", "film_image"):
        assert callable(getattr(rtx.Context, method)), method
    app = open(os.path.join(ROOT, "include", "rtx_app.hpp")).read()
    assert "bool TraceFilm(" in app


@pytest.mark.parametrize("name", list(RECIPES))
def test_recipes_meet_the_cap(oracle, name):
    """film_cases.expect's cap on all-sky frames holds for every recipe the GPU
    tests use, with the counts recorded above; every sum is finite."""
    n, seed, scale = RECIPES[name]
    o, L, hor, ver, lu, lv = fc.recipe(n, seed, scale)
    case = case_of(oracle, name)
    for lens, want in ((None, ALL_SKY[name][0]), ((lu, lv, np.full(n, fc.LENS_R)), ALL_SKY[name][1])):
        e = fc.expect(case, o, L, hor, ver, lens=lens)
        assert int((e.frame_segs == e.per * fc.SAMPLES).sum()) == want, name
        assert np.isfinite(e.sums).all()
        assert e.recs.shape == (n * e.per, 16 if lens is None else 24)


def test_the_footprint_matters(oracle):
    """rtiow11: 2.27 segments per sample, and in every frame all 32 pixels
    differ from the zero-film twin's (a kernel that ignores H, V, fx, fy fails);
    with a lens every frame differs from the lens-less one."""
    n, seed, scale = RECIPES["rtiow11"]
    o, L, hor, ver, lu, lv = fc.recipe(n, seed, scale)
    case = case_of(oracle, "rtiow11")
    e = fc.expect(case, o, L, hor, ver)
    assert abs(float(e.frame_segs.sum()) / (n * e.per * fc.SAMPLES) - 2.27) < 0.005
    twin = pc.expect(case, o, L, all_sky_max=None)
    differ = (twin.sums.view(np.uint32) != e.sums.view(np.uint32)).any(1).reshape(n, e.per)
    assert differ.all()
    el = fc.expect(case, o, L, hor, ver, lens=(lu, lv, np.full(n, fc.LENS_R)))
    assert (el.sums.view(np.uint32) != e.sums.view(np.uint32)).any(1).reshape(n, e.per).any(1).all()
    zero = fc.expect(case, o, L, np.zeros_like(hor), np.zeros_like(ver), all_sky_max=None)
    assert (zero.sums.view(np.uint32) == twin.sums.view(np.uint32)).all()  # H = V = 0: the twin, bit for bit
    assert (zero.frame_segs == twin.twin_segs).all()


def test_unit_form_identity(oracle):
    """The unit form on the oracle: pixel (0, 0) of a 1 x 1 frame with img_w =
    img_h = 2 has u = h0 * 1.1f and v = g1 * 1.1f exactly (0 + h and h / 1 are
    exact). So the same frame with img_w = img_h = 3 and doubled rows (u / 2
    and 2 H: powers of two, exact) is the same pixel, bit for bit, and one with
    img_w = img_h = 2.5 is not."""
    n, seed, scale = RECIPES["rtiow11"]
    o, L, hor, ver, _, _ = fc.recipe(n, seed, scale)
    case = case_of(oracle, "rtiow11")
    unit = fc.expect(case, o, L, hor, ver, w=1, h=1, img_w=2, img_h=2)
    same = fc.expect(case, o, L, 2 * hor, 2 * ver, w=1, h=1, img_w=3, img_h=3)
    other = fc.expect(case, o, L, hor, ver, w=1, h=1, img_w=2.5, img_h=2.5, all_sky_max=None)
    assert (unit.sums.view(np.uint32) == same.sums.view(np.uint32)).all() and (unit.frame_segs == same.frame_segs).all()
    assert (unit.sums.view(np.uint32) != other.sums.view(np.uint32)).any()
    assert (unit.recs[:, 11] == 0).all() and (unit.recs[:, 15] == 0).all()


# ---------------------------------------------------------------------------
# rtx_film_camera against numpy in fp64
# ---------------------------------------------------------------------------
FROM, AT, VUP = (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)


def basis():
    o, at, up = (np.asarray(f32(v), np.float64) for v in (FROM, AT, VUP))
    w = at - o
    w = w / np.sqrt((w * w).sum())
    u = np.cross(w, up)
    u = u / np.sqrt((u * u).sum())
    return o, u, np.cross(u, w), w


def model_dir(model, fov, width, height, cx, cy):
    """The model's unit direction at corner (cx, cy), fp64; None outside a fisheye's image circle."""
    _, u, v, w = basis()
    if model == "equirect":
        lon = (cx / width - 0.5) * (2.0 * np.pi)
        lat = (cy / height - 0.5) * np.pi
        a, b, c = np.cos(lat) * np.sin(lon), np.sin(lat), np.cos(lat) * np.cos(lon)
    else:
        half = 0.5 * min(width, height)
        px, py = (cx - 0.5 * width) / half, (cy - 0.5 * height) / half
        r = np.sqrt(px * px + py * py)
        if r > 1.0:
            return None
        theta = r * (fov * np.pi / 360.0)
        s = np.sin(theta) / r if r > 0 else 0.0
        a, b, c = s * px, s * py, np.cos(theta)
    return a * u + b * v + c * w


def within_one_ulp(got, model, what):
    """Every stored float within 1 fp32 ulp of float32(model): both sides round
    one fp64 value, and the two libm's may differ in that value's last bit."""
    want = np.asarray(model, np.float64).astype(f32)
    got = np.asarray(got, f32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= np.spacing(np.abs(want)).astype(np.float64)).all(), (what, got, want)


@pytest.mark.parametrize("model,fov,width,height", [("equirect", 0.0, 16, 8), ("fisheye", 200.0, 12, 9),
                                                    ("fisheye", 360.0, 5, 8)])
def test_film_camera_against_the_models(rtx, model, fov, width, height):
    q = rtx.film_camera(model, width, height, FROM, AT, VUP, fov_deg=fov, frame_index=2)
    assert q.dtype == rtx.FILM_QUERY_DTYPE and q.shape == (width * height,)
    o = basis()[0]
    outside = 0
    for y in range(height):
        for x in range(width):
            r = q[y * width + x]
            assert r["fx"] == 0 and r["fy"] == 0 and r["tag"] == 0
            assert r["seed"] == rtx.path_seed(x, y, 2) == pc.seed(x, y, 2)
            assert (r["o"] == np.asarray(FROM, f32)).all()
            c0, cx, cy = (model_dir(model, fov, width, height, *p) for p in ((x, y), (x + 1, y), (x, y + 1)))
            if c0 is None or cx is None or cy is None:
                outside += 1
                assert (r["lower_left"] == r["o"]).all() and not r["horizontal"].any() and not r["vertical"].any()
                continue
            within_one_ulp(r["lower_left"], o + c0, (x, y, "L"))
            within_one_ulp(r["horizontal"], (cx - c0) / 1.1, (x, y, "H"))
            within_one_ulp(r["vertical"], (cy - c0) / 1.1, (x, y, "V"))
    assert (outside > 0) == (model == "fisheye")
    assert outside < width * height  # (which pixels lie outside is the model's say, checked pixel by pixel above)


@pytest.mark.parametrize("model,fov,width,height", [("equirect", 0.0, 16, 8), ("fisheye", 200.0, 12, 9)])
def test_neighbouring_corners_meet(rtx, model, fov, width, height):
    """L(x, y) + 1.1 H(x, y) is L(x + 1, y), and L(x, y) + 1.1 V(x, y) is
    L(x, y + 1), within the stored floats' rounding: each stored float lies
    within 1 ulp of its model value, so the two sides differ by at most
    ulp(L) + ulp(L') + 1.1 ulp(H) per component."""
    q = rtx.film_camera(model, width, height, FROM, AT, VUP, fov_deg=fov)
    inside = lambda r: bool(r["horizontal"].any() or r["vertical"].any())  # noqa: E731
    pairs = 0
    for y in range(height):
        for x in range(width):
            r = q[y * width + x]
            if not inside(r):
                continue
            for nx, ny, edge in ((x + 1, y, "horizontal"), (x, y + 1, "vertical")):
                if nx >= width or ny >= height or not inside(q[ny * width + nx]):
                    continue
                a, b, e = (np.asarray(v, np.float64) for v in (r["lower_left"], q[ny * width + nx]["lower_left"], r[edge]))
                bound = (np.spacing(np.abs(r["lower_left"])) + np.spacing(np.abs(q[ny * width + nx]["lower_left"]))
                         + 1.1 * np.spacing(np.abs(r[edge]))).astype(np.float64)
                assert (np.abs(a + 1.1 * e - b) <= bound).all(), (x, y, edge)
                pairs += 1
    assert pairs == 2 * width * height - width - height if model == "equirect" else pairs > 0


def test_film_camera_and_film_from_frame_refusals(rtx):
    for kw in (dict(model="fisheye", fov_deg=0.0), dict(model="fisheye", fov_deg=360.5), dict(model="equirect", width=0),
               dict(model="equirect", look_at=FROM), dict(model="equirect", vup=(13.0, 2.0, 3.0))):
        args = dict(width=4, height=4, look_from=FROM, look_at=AT, vup=VUP, fov_deg=90.0)
        args.update(kw)
        with pytest.raises(rtx.RtxError):
            rtx.film_camera(args.pop("model"), args.pop("width"), args.pop("height"), **args)
    frame = rtx.camera_look_at(8, 4, aspect=2.0)
    q, w, h = rtx.film_from_frame(frame, [0, 7], [0, 3], frame_index=5)
    assert q.dtype == rtx.FILM_QUERY_DTYPE and (w, h) == (frame.img_w, frame.img_h)
    assert q["seed"].tolist() == [rtx.path_seed(0, 0, 5), rtx.path_seed(7, 3, 5)] and q["fx"].tolist() == [0, 7]
    assert (q["lower_left"] == np.asarray(frame.lower_left[:3], f32)).all()
    for xs, ys in (([8], [0]), ([0], [4])):
        with pytest.raises(rtx.RtxError):
            rtx.film_from_frame(frame, xs, ys)
    rtx.set_aperture(frame, 0.1)
    with pytest.raises(rtx.RtxError):
        rtx.film_from_frame(frame, [0], [0], lens=False)
    ql, _, _ = rtx.film_from_frame(frame, [1], [2])
    assert ql.dtype == rtx.FILM_LENS_QUERY_DTYPE and ql["lens_r"][0] == f32(0.05) and ql["q"]["fy"][0] == 2
    frame.rng_mode = 1
    with pytest.raises(rtx.RtxError):
        rtx.film_from_frame(frame, [0], [0])
