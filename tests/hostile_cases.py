"""Inputs the library accepts but no well-behaved scene produces: rays with
NaN, infinite, zero, tiny and huge components, spheres of zero or negative
radius, concentric and exactly representable spheres, materials with NaN,
infinite or negative parameters, frames with a NaN origin or every direction
zero. Shared by the CPU checks that the inputs do what they are meant to
(test_hostile_inputs.py) and the GPU parity tests
(test_gpu_hostile_inputs.py). Pure numpy and the oracle; every generator is
seeded and deterministic.

Why order matters for these inputs: the reference accepts a root with
`!(root < t_min || best < root)`, so a NaN root is accepted, and after it
every later sphere whose discriminant is not negative. What such a ray
"hits" is then a property of scene order, which every reordered scan (the
spatial layout, the culled order, wrapped starts, a ray split over lanes)
has to reproduce.
"""
import numpy as np

import oracle
from cases import grazing_rays

f32 = np.float32

COMPONENTS = ("ox", "oy", "oz", "dx", "dy", "dz")
NONFINITE = (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf))
TINY_D = (("1e-19", 1e-19), ("1e-20", 1e-20), ("1e-23", 1e-23), ("3e-39", 3e-39))
HUGE_D = (("1e10", 1e10), ("1.5e19", 1.5e19), ("3e19", 3e19), ("1e25", 1e25), ("1e38", 1e38))
HUGE_O = (("1e8", 1e8), ("1e20", 1e20), ("1e30", 1e30), ("3e38", 3e38))

# classes whose every ray the oracle reports as a hit with a non-finite t
ALWAYS_NONFINITE = tuple(f"{c}_{v}" for c in COMPONENTS for v, _ in NONFINITE) + ("d_zero", "d_negzero", "o_3e38")
# classes with a share of such hits, and with winners other than sphere n - 1
ORDER_DEPENDENT = ("d_1e-20", "d_3e19", "surface_d_3e19")
# classes that are also compared at t_min = 1e-30 (their finite roots are tiny or huge)
TINY_CLASSES = tuple(f"d_{name}" for name, _ in TINY_D)


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _origins(rng, n):
    """Origins around the scene; about 60 % lie below y = 0, inside the ground
    sphere (sphere 0), where |o - c|^2 - r^2 < 0: with a = |d|^2 = inf that is
    the one sphere whose discriminant is +inf instead of -inf."""
    return np.c_[rng.uniform(-14, 14, n), rng.uniform(-6.0, 4.0, n), rng.uniform(-14, 14, n)]


def _aimed(sph, o, rng):
    """Directions from `o` to a random sphere's centre each, with 0.1 jitter
    (not normalised: |d| is the distance)."""
    c = sph[rng.integers(0, len(sph), len(o)), :3]
    return c + rng.normal(scale=0.1, size=(len(o), 3)) - o


def hostile_rays(spheres, exact_ids, rng, per=64):
    """{class name: (per, 6) float32 rays (origin, direction)}. Unless a class
    fixes it, an origin lies around the scene and a direction is aimed at a
    random sphere with 0.1 jitter (an |o| class aims from its far origin, so
    its |d| is about |o|). exact_ids: spheres whose centre and radius
    are multiples of 1/8 (degenerate_spheres), so that c + (r, 0, 0) is exact
    in fp32 and |o - c|^2 - r^2 is exactly 0 there."""
    sph = np.asarray(spheres, np.float64)
    exact_ids = np.asarray(exact_ids, np.int64)
    assert len(exact_ids) > 0
    out = {}

    def base(length=None):
        o = _origins(rng, per)
        d = _aimed(sph, o, rng)
        return np.c_[o, d if length is None else _unit(d) * length]

    with np.errstate(over="ignore", invalid="ignore"):
        for k, comp in enumerate(COMPONENTS):
            for vname, v in NONFINITE:
                r = base()
                r[:, k] = v
                out[f"{comp}_{vname}"] = r
        for name, z in (("d_zero", 0.0), ("d_negzero", -0.0)):
            r = base()
            r[:, 3:] = z
            out[name] = r
        for name, length in TINY_D + HUGE_D:
            out[f"d_{name}"] = base(length)
        for name, length in HUGE_O:
            o = _unit(rng.normal(size=(per, 3))) * length
            out[f"o_{name}"] = np.c_[o, _aimed(sph, o, rng)]
        e = sph[exact_ids[rng.integers(0, len(exact_ids), per)]]
        out["at_centre"] = np.c_[e[:, :3], _aimed(sph, e[:, :3], rng)]
        for name, length in (("surface", None), ("surface_d_3e19", 3e19)):
            e = sph[exact_ids[rng.integers(0, len(exact_ids), per)]]
            o = e[:, :3] + np.c_[e[:, 3], np.zeros(per), np.zeros(per)]
            d = _aimed(sph, o, rng)
            out[name] = np.c_[o, d if length is None else _unit(d) * length]
        out = {k: np.ascontiguousarray(v, f32) for k, v in out.items()}
    for v in out.values():
        assert v.shape == (per, 6)
        v.setflags(write=False)
    return out


def degenerate_spheres(spheres, rng, frac=0.25):
    """About `frac` of the spheres, never sphere 0, rewritten in six equal
    shares: radius 0, radius -0.0, radius negated, radius 1e-30 (r * r is 0
    in fp32), the centre of the previous sphere (concentric), and "exact"
    spheres: centre rounded to 1/8, radius a multiple of 1/8 plus 1/8.
    Returns (the new (n, 4) float32 array, the ids of the exact spheres)."""
    sph = np.array(spheres, f32)
    n = len(sph)
    k = max(6, int(round(frac * n)) // 6 * 6)
    ids = 1 + rng.permutation(n - 1)[:k]
    share = np.array_split(ids, 6)
    sph[share[0], 3] = 0.0
    sph[share[1], 3] = -0.0
    sph[share[2], 3] = -sph[share[2], 3]
    sph[share[3], 3] = 1e-30
    exact = np.sort(share[5])
    sph[exact, :3] = np.round(sph[exact, :3] * 8) / 8
    sph[exact, 3] = np.floor(np.abs(sph[exact, 3]) * 8) / 8 + 0.125
    for i in np.sort(share[4]):  # last, in index order: concentric with what sphere i - 1 has become
        sph[i, :3] = sph[i - 1, :3]
    return sph, exact


def large_variants(spheres):
    """Two further versions of a large degenerate scene, for the culled
    layout's bounds: sphere n // 2 with radius 1e15, and sphere n // 3 with
    centre x = 1e15 (the largest values rtx_upload_world accepts)."""
    big_r, far_x = np.array(spheres, f32), np.array(spheres, f32)
    big_r[len(big_r) // 2, 3] = 1e15
    far_x[len(far_x) // 3, 0] = 1e15
    return {"radius_1e15": big_r, "centre_x_1e15": far_x}


class Case:
    """A world: what oracle.render_rows, oracle.hit_world_f32 and rtx.World take."""

    def __init__(self, spheres, mat_types=None, mat_values=None, depth=12, spp=4):
        n = len(spheres)
        self.spheres = np.ascontiguousarray(spheres, f32)
        self.mat_types = np.zeros(n, f32) if mat_types is None else np.ascontiguousarray(mat_types, f32)
        self.mat_values = np.zeros((n, 4), f32) if mat_values is None else np.ascontiguousarray(mat_values, f32)
        for a in (self.spheres, self.mat_types, self.mat_values):
            a.setflags(write=False)
        self.depth, self.spp = depth, spp

    @property
    def count(self):
        return len(self.spheres)

    def at_spp(self, spp, depth=None):
        return Case(self.spheres, self.mat_types, self.mat_values, self.depth if depth is None else depth, spp)


# seeds of hostile_materials per random_world extent, chosen so that the frame
# conditions of test_hostile_inputs.py hold (which spheres are rewritten, the
# three large ones above all, decides how much of the frame changes)
MATERIAL_SEED = {4: 10, 11: 5, 25: 8}
DEGENERATE_SEED = 1000  # + ext: degenerate_spheres and hostile_rays of random_world(ext)
LAST_KINDS = {"lambert": (0.0, (0.5, 0.5, 0.5, 0.0)), "metal": (1.0, (0.7, 0.6, 0.5, 0.1)),
              "glass": (2.0, (1.0, 1.0, 1.0, 1.5)), "unknown": (5.0, (0.5, 0.5, 0.5, 0.0))}
MATERIAL_REWRITES = ("glass_ir_nan", "glass_ir_0", "glass_ir_neg", "metal_fuzz_inf", "metal_fuzz_1e30",
                     "metal_fuzz_nan", "lambert_albedo_bad", "radius_negated")


def hostile_materials(ext, last, seed, depth=12, spp=4, untouched=False):
    """The oracle's random_world(ext) with about 30 % of its spheres, never
    sphere 0 or the last one, given one of MATERIAL_REWRITES each, and the
    last sphere's material set to `last` (a key of LAST_KINDS): a NaN ray
    hits sphere n - 1, so that material decides what the path does next.
    untouched: the same world with only the last sphere's material set."""
    sph, mt, mv = oracle.random_world(ext)
    n = len(sph)
    rng = np.random.default_rng(seed)
    ids = 1 + rng.permutation(n - 2)[:int(round(0.3 * n))]
    kind = rng.integers(0, len(MATERIAL_REWRITES), len(ids))
    if not untouched:
        for i, k in zip(ids, kind):
            name = MATERIAL_REWRITES[k]
            if name.startswith("glass"):
                mt[i] = 2.0
                mv[i, 3] = {"glass_ir_nan": np.nan, "glass_ir_0": 0.0, "glass_ir_neg": -1.5}[name]
            elif name.startswith("metal"):
                mt[i] = 1.0
                mv[i, 3] = {"metal_fuzz_inf": np.inf, "metal_fuzz_1e30": 1e30, "metal_fuzz_nan": np.nan}[name]
            elif name == "lambert_albedo_bad":
                mt[i] = 0.0
                mv[i, :3] = (np.inf, -1.0, np.nan)
            else:
                sph[i, 3] = -sph[i, 3]
    mt[n - 1], mv[n - 1] = LAST_KINDS[last]
    return Case(sph, mt, mv, depth, spp)


def grouped(classes):
    """Every class as a run of rays starting at a multiple of 64 (a short
    class is padded with its own rays): whole waves are one class, so a
    wave-wide ballot cannot hide a lane's mistake behind its neighbours.
    Returns (rays, {class: slice})."""
    runs, where, at = [], {}, 0
    for name, r in classes.items():
        pad = -len(r) % 64
        r = np.concatenate([r, r[np.arange(pad) % len(r)]]) if pad else r
        runs.append(r)
        where[name] = slice(at, at + len(r))
        at += len(r)
    return np.ascontiguousarray(np.concatenate(runs), f32), where


def mixed(classes, spheres, rng):
    """The same rays shuffled 1:1 among grazing_rays over `spheres`.
    Returns (rays, hostile: bool per ray)."""
    h = np.concatenate(list(classes.values()))
    g = grazing_rays(spheres, len(h), rng, xaxis_frac=0.05)
    order = rng.permutation(2 * len(h))
    rays = np.concatenate([h, g])[order]
    return np.ascontiguousarray(rays, f32), order < len(h)


def _set(frame, name, v):
    for k in range(3):
        getattr(frame, name)[k] = v[k]


def hostile_frame(frame, kind):
    """`frame` (rtx's or the oracle's look-at frame) turned hostile, in place:
    "nan_origin": origin.x = NaN, so every primary ray has a NaN origin and
    direction; "huge_d": horizontal scaled to length 6e19, so |d| is about
    3e19 at mid frame and |d|^2 overflows over the frame's right two thirds;
    "zero_d": horizontal = vertical = 0 and lower_left = origin, so every
    direction is exactly 0."""
    if kind == "nan_origin":
        frame.origin[0] = float("nan")
    elif kind == "huge_d":
        h = np.array(frame.horizontal[:3], np.float64)
        _set(frame, "horizontal", (h * (6e19 / np.linalg.norm(h))).astype(f32))
    elif kind == "zero_d":
        _set(frame, "horizontal", (0.0, 0.0, 0.0))
        _set(frame, "vertical", (0.0, 0.0, 0.0))
        _set(frame, "lower_left", frame.origin[:3])
    else:
        raise KeyError(kind)
    return frame


HOSTILE_FRAMES = ("nan_origin", "huge_d", "zero_d")


def divergence_case():
    """The minimal case of a batch of 8 discriminants mixing NaN and -inf: 21
    spheres with centres (k / 2, 0, 0) - all at height 0 - and radius 1/8, and
    the ray from exactly on sphere 10's surface, c + (r, 0, 0), along y with
    |d| = 3e19. a = |d|^2 = inf; o.y - c.y = 0 for every sphere, so hb = 0 and
    disc = 0 - inf * cc: NaN for sphere 10 (cc = 0 exactly), -inf for every
    other (cc > 0). The reference takes the NaN discriminant (`if (d < 0)
    return false` does not fire) and its NaN root; no later sphere is accepted.
    Returns (spheres, 64 copies of the ray, 10)."""
    k = np.arange(21)
    sph = np.c_[k / 2.0, np.zeros(21), np.zeros(21), np.full(21, 0.125)].astype(f32)
    ray = np.array([sph[10, 0] + sph[10, 3], 0.0, 0.0, 0.0, 3e19, 0.0], f32)
    return sph, np.repeat(ray[None], 64, 0), 10


_WORLDS = {}


def degenerate_world(key):
    """(Case, exact ids, hostile ray classes) of the degenerate version of
    random_world(key) for an int key, or of regime_cases.world(key) for a
    name; built once, read-only. Geometry only: the materials are all
    Lambertian (hit_world does not read them)."""
    if key not in _WORLDS:
        if isinstance(key, int):
            base, seed = oracle.random_world(key)[0], DEGENERATE_SEED + key
        else:
            import regime_cases
            base, seed = regime_cases.world(key).spheres, DEGENERATE_SEED + sum(map(ord, key))
        rng = np.random.default_rng(seed)
        sph, exact = degenerate_spheres(base, rng)
        _WORLDS[key] = (Case(sph), exact, hostile_rays(sph, exact, rng))
    return _WORLDS[key]
