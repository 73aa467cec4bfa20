"""The shading arithmetic pinned to an independent restatement (CPU only).

shading_spec.py restates ShaderCompute.hlsl in numpy without a look at the
oracle's shading. Here it is first pinned itself -- its geometry to the
compiled reference's records (tests/golden/hit_*), its RNG to the known
answers of test_kat.py, its vector formulas to closed forms -- and then the
oracle is held to it on every case of shading_cases.py under that module's
rule. test_spec_mutants_are_rejected shows that the rule would notice the
misreadings the oracle and the kernel could share.
"""
import numpy as np
import pytest

import paths_cases as pc
import shading_cases as sc
import shading_spec as spec
from golden_cases import load_case
from test_kat import KAT, base_hash_py, hash2_py
from tolerance import ill_conditioned

f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------
# the restatement pinned
# ---------------------------------------------------------------------------
def _golden_ids():
    import json
    import os
    from golden_cases import GOLDEN
    ids = []
    for name in ("hit_test_world.json", "hit_rtiow9.json"):
        ids += [(name, k) for k in range(len(json.load(open(os.path.join(GOLDEN, name)))["cases"]))]
    return ids + [("hit_rtiow11.npz", 0)]


@pytest.mark.parametrize("name,k", _golden_ids())
def test_spec_hit_world_against_the_compiled_reference(oracle, name, k):
    """The restatement's fp64 hit_world (HLSL :155-205) against the records
    of the reference's compiled Hittable_list::hit: hit / miss, the winning
    sphere and front_face identical, t, p and the normal within 1e-12
    relative; rays that tolerance.ill_conditioned marks are left out."""
    c = load_case(name, k, lambda ext, cap: oracle.random_world(ext, cap)[0])
    rays, e = np.asarray(c["rays"], f64), np.asarray(c["expected"], f64)
    well = ~ill_conditioned(c["spheres"], rays, c["t_min"], c["t_max"])
    assert well.sum() >= 0.9 * len(rays)
    rays, e = rays[well], e[well]
    hit, index, t, p, normal, front = spec.hit_world(c["spheres"].astype(f64), rays[:, :3], rays[:, 3:], f64(c["t_min"]),
                                                     f64(c["t_max"]))
    assert (hit == (e[:, 0] == 1)).all()
    h = hit
    assert h.any() and (~h).any() or len(rays) < 8
    assert (index[h] == e[h, 9]).all() and (front[h] == (e[h, 8] == 1)).all()

    def rel(got, want, scale=None):
        got, want = got.reshape(len(got), -1), want.reshape(len(want), -1)
        scale = np.abs(want).max(1) if scale is None else scale
        return float((np.abs(got - want).max(1) / np.maximum(scale, 1e-300)).max(initial=0.0))

    # Relative to what: the operands of the operation that forms the value, where the rounding happens. t is the
    # difference of -half_b / a and sqrt(d) / a, both of the size of the centre's distance |oc| / |d| in units of
    # t; p = o + t d; the normal is the difference of p and c, divided by r. Relative to the values themselves the
    # literal length(oc) * length(oc) of :162 (a square root squared again, where Sphere.cpp has length_squared)
    # is 6.5e-12 off in t on the ground sphere, whose c cancels six digits, and a 0.2 sphere's normal 6.5e-12 at
    # |p| = 10: conditioning, not a misreading (both are printed).
    sph = c["spheres"].astype(f64)[index[h]]
    o, d = rays[h, :3], rays[h, 3:]
    reach = np.maximum(np.abs(e[h, 1]), np.linalg.norm(o - sph[:, :3], axis=1) / np.linalg.norm(d, axis=1))
    p_scale = np.maximum(np.abs(o).max(1), np.abs(e[h, 2:5]).max(1))
    n_scale = np.maximum(1.0, np.maximum(np.abs(e[h, 2:5]).max(1), np.abs(sph[:, :3]).max(1)) / np.abs(sph[:, 3]))
    worst = {"t": rel(t[h], e[h, 1], reach), "p": rel(p[h], e[h, 2:5], p_scale), "normal": rel(normal[h], e[h, 5:8], n_scale)}
    print(f"{name}-{k}: {int(h.sum())} hits of {len(rays)} rays, {int((~well).sum())} left out, worst relative {worst}; "
          f"relative to the values themselves t {rel(t[h], e[h, 1]):.1e}, normal {rel(normal[h], e[h, 5:8]):.1e}")
    assert max(worst.values()) <= 1e-12, worst


def test_spec_rng_known_answers():
    for (x, y), h in KAT.items():
        assert int(spec.base_hash(x, y)) == h
    xy = np.random.default_rng(1).integers(0, 2**32, size=(2000, 2), dtype=np.uint64)
    got = spec.base_hash(xy[:, 0], xy[:, 1])
    assert [int(g) for g in got] == [base_hash_py(int(x), int(y)) for x, y in xy]
    # pixel (0, 0): seed 0, first hash2 = (0.89364517, 0.14578328), seed -> 0.2; pixel (1, 0): 0.93445665
    x, y, s = spec.hash2(np.zeros(1, f32))
    assert abs(x[0] - 0.89364517) < 1e-7 and abs(y[0] - 0.14578328) < 1e-7 and s[0] == f32(0.2)
    assert spec.pixel_seed(0, 0) == 0 and abs(spec.pixel_seed(1, 0) - 0.93445665) < 1e-7
    seeds = np.random.default_rng(2).uniform(0, 1, 500).astype(f32)
    x, y, s = spec.hash2(seeds)
    for i, sd in enumerate(seeds):
        assert (x[i], y[i], s[i]) == hash2_py(float(sd))
    assert f32(0xFFFFFFFF) == f32(2.0 ** 32) and f32(0x7FFFFFFF) == f32(2.0 ** 31)  # what :33 and :40 divide by


def math_seeds():
    rng = np.random.default_rng(4096)
    return np.concatenate([rng.uniform(0, 1, 3072), rng.uniform(0, 40, 1024)]).astype(f32)


def check_device_math(math):
    """hash1 and hash3 of `math` (oracle.math or a context's debug_math)
    bit-equal to the restatement's, the seed after hash1 too; its
    random_in_unit_sphere within 4 x the restatement's own fp32 - fp64
    spread."""
    seeds = math_seeds()
    h, s = spec.hash1(seeds)
    got = math("hash1", seeds)
    assert sc.same_bits(got[:, 0], h).all() and sc.same_bits(got[:, 1], s).all()
    got = math("hash3", seeds)
    for k, want in enumerate(spec.hash3(seeds)[:3]):
        assert sc.same_bits(got[:, k], want).all(), f"hash3 component {k}"
    r32, r64 = spec.random_in_unit_sphere(seeds, f32)[0], spec.random_in_unit_sphere(seeds, f64)[0]
    spread = np.abs(r32 - r64).max()
    err = np.abs(math("rius", seeds) - r64).max()
    print(f"random_in_unit_sphere: fp32 - fp64 spread {spread:.2e}, under test {err:.2e}")
    assert 0 < spread < 2e-6 and err <= 4 * spread
    assert (np.linalg.norm(r64, axis=1) <= 1).all()


def test_spec_hashes_and_rius_against_the_oracle(oracle):
    check_device_math(oracle.math)


def test_spec_closed_forms():
    rng = np.random.default_rng(5)
    v = rng.normal(size=(1000, 3)) * rng.uniform(0.1, 10, (1000, 1))
    n = spec.normalize(rng.normal(size=(1000, 3)))
    r = spec.reflect(v, n)
    assert np.abs(spec.length(r) / spec.length(v) - 1).max() < 1e-12          # |reflect(v, n)| = |v|
    assert np.abs(spec.dot(r, n) + spec.dot(v, n)).max() < 1e-12 * 10         # the normal part is mirrored
    # Snell: sin t' = ratio * sin t, for unit directions against the normal and every ratio with a refracted ray
    uv = spec.normalize(v)
    n = np.where(spec.col(spec.dot(uv, n) < 0), n, -n)
    for ratio in (1 / 1.5, 1 / 1.33, 1.0, 1.5):
        sin_in = np.sqrt(1 - spec.dot(-uv, n) ** 2)
        ok = ratio * sin_in < 0.999
        out = spec.refract(uv[ok], n[ok], np.full(ok.sum(), ratio))
        assert np.abs(spec.length(out) - 1).max() < 1e-12
        sin_out = spec.length(np.cross(out, n[ok]))
        assert np.abs(sin_out - ratio * sin_in[ok]).max() < 1e-12
        assert (spec.dot(out, n[ok]) < 0).all()                                # and it goes on through the surface
    for ir in (1.5, 1 / 1.5, 1.33):
        one, zero = spec.reflectance(np.ones(1), np.full(1, ir)), spec.reflectance(np.zeros(1), np.full(1, ir))
        assert abs(one[0] - ((1 - ir) / (1 + ir)) ** 2) < 1e-15 and abs(zero[0] - 1) < 1e-15


def test_trace_one_query_and_draw_count():
    """trace() is one row of trace_batch, and the seed moves by exactly the
    draws counted: 0.2 per draw in float32, one addition of 0.1 at a time."""
    c, (_, s64) = sc.case("mix"), sc.specs("mix")
    w = c.world
    for i in (0, 9, 500):
        q = c.queries[i]
        total, end, segs, draws = spec.trace(w.spheres, w.mat_types, w.mat_values, q[0:3], q[4:7], q[3], c.samples,
                                             c.depth)
        assert (total == s64.sums[i]).all() and end == s64.seeds[i] and segs == s64.segments[i]
        assert draws == s64.tally.draws[i]
        s = f32(q[3])
        for _ in range(2 * draws):
            s = f32(s + f32(0.1))
        assert s == end
    # 2 samples of at most `depth` segments, each hit but an unknown material's drawing once
    assert (s64.tally.draws >= 2 * c.samples).all() and (s64.tally.draws <= s64.segments + 2 * c.samples).all()


# ---------------------------------------------------------------------------
# the oracle against the restatement
# ---------------------------------------------------------------------------
_ORACLE = {}


def oracle_paths(oracle, name):
    """The oracle's sums per query and segments per ray for case `name`: each
    ray's zero-film twin (paths_cases.twin_frame) of SEEDS x 2 pixels, row 0
    rendered (a twin needs img_h != 1: v divides by img_h - 1)."""
    if name not in _ORACLE:
        c = sc.case(name)
        sums, segs = [], []
        for o, L in zip(c.o, c.L):
            img, s = oracle.render_rows_linear(c.world, pc.twin_frame(o, L, sc.SEEDS, 2), [0])
            sums.append(img.reshape(-1, 4)[:, :3])
            segs.append(s)
        assert (np.concatenate([pc.probes(o, L, sc.SEEDS, 2)[:sc.SEEDS] for o, L in zip(c.o, c.L)]) == c.queries).all()
        _ORACLE[name] = (np.concatenate(sums), np.array(segs, np.int64))
        for a in _ORACLE[name]:
            a.setflags(write=False)
    return _ORACLE[name]


@pytest.mark.parametrize("name", sc.NAMES)
def test_oracle_paths_against_spec(oracle, name):
    tol = sc.checked_tolerance(name)
    _, s64 = sc.specs(name)
    sums, segs = oracle_paths(oracle, name)
    if name in sc.BLACK:
        sc.assert_black(f"oracle, {name}", s64, sums, group_segments=segs)
        return
    v = sc.accept(f"oracle, {name}", tol, s64, sums, group_segments=segs)
    assert not v.ratio > 2, f"{v}: the oracle lies further from fp64 than twice the fp32 restatement does"


def oracle_frame(oracle, name, spp=sc.FSPP):
    return oracle.render_rows(sc.frame_world(name, spp), sc.frame_of(name), np.arange(sc.FH))


@pytest.mark.parametrize("name", sc.FRAMES)
def test_oracle_frames_against_spec(oracle, name):
    tol = sc.frame_tolerance(name)
    tol.assert_reference_within_half_cap(name)
    img, segs = oracle_frame(oracle, name)
    assert (img[..., 3] == 1).all()                                            # :314
    v = sc.judge_frame(f"oracle, frame {name}", tol, sc.frame_specs(name)[1], img, segs)
    assert v.ok, str(v)


# ---------------------------------------------------------------------------
# the rule has teeth
# ---------------------------------------------------------------------------
def _rius(seed, dtype, exponent=f32(1.0) / f32(3.0), swap=False):
    x, y, z, seed = spec.hash3(seed)
    hx, phi = x.astype(dtype) * dtype(2) - dtype(1), y.astype(dtype) * spec.lit(6.28318530718, dtype)
    r, s = np.power(z.astype(dtype), dtype(exponent)), np.sqrt(dtype(1) - hx * hx)
    a, b = (np.cos(phi), np.sin(phi)) if swap else (np.sin(phi), np.cos(phi))
    return spec.col(r) * np.stack([s * a, s * b, hx], -1), seed


def _schlick(cosine, ref_idx, exponent=5, square=True):
    r0 = (1 - ref_idx) / (1 + ref_idx)
    r0 = r0 * r0 if square else r0
    return r0 + (1 - r0) * np.power(1 - cosine, cosine.dtype.type(exponent))


def _reflects_short_circuit(cant, refl, seed):
    h, drawn = spec.hash1(seed)
    return cant | (refl > h.astype(refl.dtype)), np.where(cant, seed, drawn), (~cant).astype(np.int64)


def _jitter_first_y(x, y, seed, img_w, img_h):
    T = img_w.dtype.type
    first_x, first_y, seed = spec.hash2(seed)
    _, _, seed = spec.hash2(seed)
    return ((x.astype(T) + first_x.astype(T) * spec.lit(1.1, T)) / (img_w - T(1)),
            (y.astype(T) + first_y.astype(T) * spec.lit(1.1, T)) / (img_h - T(1)), seed)


def _sky_swapped(d):
    T = d.dtype.type
    t = T(0.5) * (spec.normalize(d)[:, 1] + T(1))
    return spec.col(t) * np.ones(3, T) + spec.col(T(1) - t) * np.array([0.5, spec.lit(0.7, T), 1.0], T)


# what is replaced, by what, and the cases it is tried on (an isolating world and `mix`; "frame:" a frame)
MUTANTS = {
    "Schlick exponent 4": ("reflectance", lambda c, r: _schlick(c, r, exponent=4), ("glass_ball", "mix")),
    "r0 not squared": ("reflectance", lambda c, r: _schlick(c, r, square=False), ("glass_ball", "mix")),
    "refraction ratio inverted": ("refraction_ratio", lambda front, ir: np.where(front, ir, 1 / ir),
                                  ("glass_ball", "mix")),
    "reflect with factor 1": ("reflect", lambda v, n: v - spec.col(spec.dot(v, n)) * n, ("mirror", "mix")),
    "square root in rius": ("random_in_unit_sphere", lambda s, T: _rius(s, T, exponent=0.5),
                            ("lambert_ball_d2", "mix")),
    "sin and cos swapped in rius": ("random_in_unit_sphere", lambda s, T: _rius(s, T, swap=True),
                                    ("lambert_ball_d2", "mix")),
    "v from the first hash2's .y": ("jitter", _jitter_first_y, ("frame:test_world", "frame:mix")),
    "hash1 not drawn when cant": ("reflects", _reflects_short_circuit, ("hollow_glass", "bubble", "mix")),
    "sky weights swapped": ("sky", _sky_swapped, ("lambert_ball_d2", "mix")),
    "attenuation applied after the sky": ("at_miss", lambda before, now, sky: before * sky, ("lambert_ball_d2", "mix")),
}


def test_spec_mutants_are_rejected(oracle, monkeypatch):
    """Each misreading, put into the restatement one at a time, makes the rule
    reject the oracle on the mutant's isolating case (the first named; the
    others are printed): a later relaxation of the cap or the tolerance that
    let one through fails here. Measured (RESULTS.md): Schlick's exponent is
    the weak one, it flips 21 of glass_ball's 1,024 paths and 6 of mix's (the
    cap is 5). The draw skipped when cant is true shows in hollow_glass's sums
    (36 paths: total reflection inside the shell, and the path goes on) but
    not in bubble's, where a ray that cannot enter sees the sky whatever its
    seed: there only the end seed tells, which the GPU test has."""
    assert (_rius(sc.case("mix").queries[:64, 3], f64)[0] ==
            spec.random_in_unit_sphere(sc.case("mix").queries[:64, 3], f64)[0]).all()  # the unmutated copy is the spec's
    for what, (attr, fn, names) in MUTANTS.items():
        verdicts = []
        with monkeypatch.context() as m:
            m.setattr(spec, attr, fn)
            for name in names:
                if name.startswith("frame:"):
                    name = name[6:]
                    img, segs = oracle_frame(oracle, name)
                    verdicts.append(sc.judge_frame(f"[{what}] frame {name}", sc.frame_tolerance(name, fresh=True),
                                                   sc.frame_specs(name, fresh=True)[1], img, segs))
                else:
                    sums, segs = oracle_paths(oracle, name)
                    tol = sc.tolerance(name, fresh=True)
                    verdicts.append(sc.judge(f"[{what}] {name}", tol, sc.specs(name, fresh=True)[1], sums,
                                             group_segments=segs))
        assert not verdicts[0].ok, f"{what}: the rule accepts the oracle against this mutant on {names[0]}"
    # and nothing of a mutant is left behind
    assert sc.accept("oracle, mix again", sc.tolerance("mix", fresh=True), sc.specs("mix", fresh=True)[1],
                     oracle_paths(oracle, "mix")[0], group_segments=oracle_paths(oracle, "mix")[1]).diverged == 0
