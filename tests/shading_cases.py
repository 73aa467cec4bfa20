"""Worlds, rays and the acceptance rule for the shading checks: what the CPU
oracle (test_shading_spec.py) and the GPU (test_gpu_shading_spec.py) are held
to against the independent restatement of the compute shader in
shading_spec.py.

Worlds are the smallest that isolate a formula. Rays come from fixed-seed
default_rng recipes: for the one-ball worlds, origins on a shell of radius 4-6
round the ball and targets at impact parameters 0 .. 0.98 r, so no ray grazes
on purpose. Every ray is traced with the 8 chain seeds of the pixels of an
8 x 1 strip (paths_cases.seed) and 2 samples, so that the seed's carry across
a sample boundary is covered.

The rule (one for the CPU and the GPU tests)
    A path agrees with the reference when its segment count is the
    reference's, its end seed is the reference's bit for bit (which pins the
    number and kind of RNG draws), and
        |sum - spec64|inf <= tol * max(1, |spec64|inf).
    Otherwise it diverged: an ulp flips a hit or a reflect / refract choice
    and the two paths decorrelate, which is legitimate and rare. At most
    CAP of a case's paths may diverge.
    tol is measured on the reference alone, never on what is under test:
    FACTOR x the largest such distance between the restatement run in fp32
    and in fp64, over the paths on which those two agree on segments and
    seed, with floor FLOOR. The factor 4 covers an fp32 implementation whose
    operation order is not the restatement's (fma forms, * (1 / a), its own
    transcendentals at 3e-7), and the fact that a maximum over ~1,000 paths
    is a sample from a heavy tail. The reference alone must stay within half
    the cap: fp32 and fp64 restatements may disagree on at most CAP / 2 of
    the paths. If a recipe seed breaks that, another seed is chosen and the
    tried ones are named beside it; the cap does not move.
    The oracle reports no end seed and its segments per ray (the 8 seeds
    together), so there a path diverged when its sum is off, and a ray whose
    segment total differs with no sum off counts as one more.
"""
import numpy as np

import hostile_cases as hc
import oracle
import paths_cases as pc
import shading_spec as spec

f32 = np.float32
SEEDS = 8            # per ray: the pixels of an 8 x 1 strip
SAMPLES = 2
CAP = 0.005          # share of a case's paths that may diverge
FACTOR, FLOOR = 4.0, 1e-6
# A set-up condition on the reference alone, like the cap: a case whose measured tolerance is wider than 2 % of a
# white sample has a path among its "agreeing" ones that is in truth another path, and checks little.
TOL_MAX = 2e-2
GLASS_MIN = 0.25     # glass_ball: share of paths with a reflection, and with a refraction

BALL = [[0, 0, 0, 1]]
MIX = dict(
    spheres=[[0, -1000, 0, 1000], [0, 1, 0, 1], [-2.2, 1, 0, 1], [2.2, 1, 0, 1], [0, .4, 2, .4], [1.2, .3, 2.2, .3],
             [-1.2, .3, 2.2, .3], [0, 1, 0, -.9]],
    types=[0, 2, 0, 1, 1, 2, 0, 2],
    values=[[.5, .5, .5, 0], [1, 1, 1, 1.5], [.4, .2, .1, 0], [.7, .6, .5, 0], [.8, .8, .9, .3], [1, 1, 1, 1.33],
            [.2, .6, .3, 0], [1, 1, 1, 1.5]])

# name: (spheres, types, values, depth, rays, recipe seed). Recipe seeds are 7300 + the row, and no case but
# rtiow11 needed another. rtiow11 did: at depth 12 among 486 spheres the fp32 and fp64 restatements part on 2 .. 17
# of the 2,048 paths (median 9, seeds 7312 .. 7371 tried), mostly above half the cap (5), and on most seeds one
# path or more lands on another sphere of the same material, which keeps segments and seed and moves the sum by
# tenths, so the measured tolerance would check nothing (TOL_MAX). Within half the cap: 7312, 7336, 7338, 7341,
# 7342, 7353, 7356, 7361, 7362, 7364, 7366; of these 7361 (tol 3.5e-2 > TOL_MAX) and 7364 have no such path;
# 7364 it is.
_TABLE = {
    "lambert_ball_d2": (BALL, [0], [[.2, .5, .8, 0]], 2, 128, 7301),
    "lambert_ball_d3": (BALL, [0], [[.2, .5, .8, 0]], 3, 128, 7302),
    "mirror": (BALL, [1], [[.7, .6, .5, 0]], 3, 128, 7303),
    "fuzzy": (BALL, [1], [[.7, .6, .5, .4]], 3, 128, 7304),
    "bright_metal": (BALL, [1], [[1.25, 1.0, 1.5, 0]], 3, 128, 7305),
    "glass_ball": (BALL, [2], [[1, 1, 1, 1.5]], 6, 128, 7306),
    "bubble": (BALL, [2], [[1, 1, 1, 1 / 1.5]], 6, 128, 7307),
    "hollow_glass": ([[0, 0, 0, 1], [0, 0, 0, -.9]], [2, 2], [[1, 1, 1, 1.5]] * 2, 8, 128, 7308),
    "black_code3": (BALL, [3], [[.2, .5, .8, 0]], 4, 128, 7309),
    "black_depth1": (BALL, [0], [[.2, .5, .8, 0]], 1, 128, 7310),
    "mix": (MIX["spheres"], MIX["types"], MIX["values"], 12, 128, 7311),
    "rtiow11": (None, None, None, 12, 256, 7364),
}
SMALL = [k for k in _TABLE if k != "rtiow11"]
BLACK = ("black_code3", "black_depth1")
NAMES = list(_TABLE)


def ball_rays(n, rng_seed, radius=1.0):
    """n (origin, target) pairs round a ball at the origin: the origin on a
    shell of radius 4 .. 6, the target in the plane through the centre across
    the line of sight, 0 .. 0.98 radius from the centre (the ray's impact
    parameter, but for the target's rounding to float32)."""
    rng = np.random.default_rng(rng_seed)
    w = rng.normal(size=(n, 3))
    w /= np.linalg.norm(w, axis=1)[:, None]
    t = np.cross(w, rng.normal(size=(n, 3)))
    t /= np.linalg.norm(t, axis=1)[:, None]
    o = (w * rng.uniform(4, 6, (n, 1))).astype(f32)
    L = (t * 0.98 * np.sqrt(rng.uniform(0, 1, (n, 1))) * radius).astype(f32)  # uniform over the disc the rays see
    return o, (L + f32(0.0)).astype(f32)  # no negative zero in a target (paths_cases.ray_recipe)


class PathCase:
    def __init__(self, name):
        sph, mt, mv, depth, n, rng_seed = _TABLE[name]
        if name == "rtiow11":
            sph, mt, mv = oracle.random_world(11)
        self.name, self.depth, self.samples = name, depth, SAMPLES
        self.world = hc.Case(sph, mt, mv, depth, SAMPLES)
        if name == "mix":
            self.o, self.L = pc.ray_recipe(n, rng_seed, 0.4)
        elif name == "rtiow11":
            self.o, self.L = pc.ray_recipe(n, rng_seed, 1.0)
        else:
            self.o, self.L = ball_rays(n, rng_seed)
        # (n * SEEDS, 8) rows (o, seed, d, tag), a ray's SEEDS queries together
        self.queries = np.concatenate([pc.probes(o, L, SEEDS, 1) for o, L in zip(self.o, self.L)])
        self.queries.setflags(write=False)
        assert len(self.queries) >= 1024


class Spec:
    """What the restatement gives for a case's queries in one float type."""

    def __init__(self, case, dtype):
        q, w = case.queries, case.world
        self.sums, self.seeds, self.tally = spec.trace_batch(w.spheres, w.mat_types, w.mat_values, q[:, 0:3], q[:, 4:7],
                                                             q[:, 3], case.samples, case.depth, dtype)
        self.segments = self.tally.segments


_CASES, _SPECS = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = PathCase(name)
    return _CASES[name]


def specs(name, fresh=False):
    """(fp32, fp64) restatements of case `name`, computed once and, with them,
    the set-up conditions of the case; fresh: computed now and not kept (for
    a test that has replaced part of the restatement)."""
    if fresh:
        return Spec(case(name), np.float32), Spec(case(name), np.float64)
    if name not in _SPECS:
        s32, s64 = Spec(case(name), np.float32), Spec(case(name), np.float64)
        n = len(s64.sums)
        if name in SMALL and name != "mix":  # the one-ball worlds: every sample starts with a hit
            assert (s64.tally.hits == SAMPLES).all(), f"{name}: a ray misses its ball"
        if name in BLACK:
            assert not s64.sums.any() and not s32.sums.any(), f"{name}: the reference is not black"
        if name == "glass_ball":
            refl, refr = (s64.tally.reflections > 0).mean(), (s64.tally.refractions > 0).mean()
            assert refl >= GLASS_MIN and refr >= GLASS_MIN, f"glass_ball: {refl:.1%} reflect, {refr:.1%} refract"
        _SPECS[name] = (s32, s64)
    return _SPECS[name]


# ---------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------
def distance(got, want):
    """|got - want|inf / max(1, |want|inf) per row; NaN counts as infinite."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = np.abs(got - want).max(-1) / np.maximum(1.0, np.abs(want).max(-1))
    return np.where(np.isnan(d), np.inf, d)


def same_bits(a, b):
    return np.ascontiguousarray(a, f32).view(np.uint32) == np.ascontiguousarray(b, f32).view(np.uint32)


class Tolerance:
    """The reference alone: tol, the largest fp32 - fp64 distance behind it,
    and the paths on which the two restatements part."""

    def __init__(self, sums32, segs32, seeds32, sums64, segs64, seeds64):
        together = (segs32 == segs64) & same_bits(seeds32, seeds64)
        self.n = len(together)
        self.parted = int((~together).sum())
        self.spread = float(distance(sums32, sums64)[together].max(initial=0.0))
        self.tol = max(FLOOR, FACTOR * self.spread)

    def assert_reference_within_half_cap(self, what):
        assert self.parted <= CAP / 2 * self.n, \
            f"{what}: the fp32 and fp64 restatements part on {self.parted} of {self.n} paths, over half the cap"


def tolerance(name, fresh=False):
    s32, s64 = specs(name, fresh)
    return Tolerance(s32.sums, s32.segments, s32.seeds, s64.sums, s64.segments, s64.seeds)


def checked_tolerance(name):
    """The case's Tolerance, after the set-up conditions on the reference alone."""
    tol = tolerance(name)
    tol.assert_reference_within_half_cap(name)
    assert tol.tol <= TOL_MAX, f"{name}: a tolerance of {tol.tol:.2e} checks little; another recipe seed"
    return tol


def assert_black(what, want, sums, seeds=None, segments=None, group_segments=None, group=SEEDS):
    """The black cases: exactly 0.0, no tolerance and no cap."""
    sums = np.asarray(sums)
    assert not want.sums.any()
    assert not sums.any() and not np.signbit(sums).any(), f"{what}: a sum is not exactly 0.0"
    if seeds is not None:
        assert same_bits(seeds, want.seeds).all(), f"{what}: end seeds"
    if segments is not None:
        assert (np.asarray(segments, np.int64) == want.segments).all(), f"{what}: segments"
    if group_segments is not None:
        assert (np.asarray(group_segments, np.int64) == want.segments.reshape(-1, group).sum(1)).all(), what


class Verdict:
    def __init__(self, what, diverged, n, worst, tol, spread):
        self.what, self.diverged, self.n, self.worst, self.tol = what, int(diverged), n, float(worst), tol
        self.ratio = worst / spread if spread > 0 else float("nan")  # under test / fp32 restatement, agreeing paths
        self.ok = self.diverged <= CAP * n

    def __str__(self):
        return (f"{self.what}: {self.diverged} of {self.n} diverged, tol {self.tol:.2e}, worst agreeing "
                f"{self.worst:.2e}, ratio to the fp32 restatement {self.ratio:.2f}")


def judge(what, tol, want, sums, seeds=None, segments=None, group_segments=None, group=SEEDS):
    """The rule. want: the fp64 Spec (or anything with sums, seeds, segments);
    tol: the case's Tolerance. seeds and segments per path where the thing
    under test reports them (the GPU); group_segments: segments summed over
    each `group` consecutive paths where that is all there is (the oracle)."""
    dist = distance(sums, want.sums)
    off = dist > tol.tol
    if seeds is not None:
        off |= ~same_bits(seeds, want.seeds)
    if segments is not None:
        off |= np.asarray(segments, np.int64) != want.segments
    diverged = int(off.sum())
    if group_segments is not None:
        wrong = np.asarray(group_segments, np.int64) != want.segments.reshape(-1, group).sum(1)
        diverged += int((wrong & ~off.reshape(-1, group).any(1)).sum())
    v = Verdict(what, diverged, len(dist), dist[~off].max(initial=0.0), tol.tol, tol.spread)
    print(v)
    return v


def accept(*args, **kw):
    v = judge(*args, **kw)
    assert v.ok, f"{v} -- more than {CAP:.1%}"
    return v


# ---------------------------------------------------------------------------
# frames
# ---------------------------------------------------------------------------
FW, FH, FSPP, FDEPTH = 16, 9, 4, 12
FRAMES = ("mix", "test_world")


def frame_world(name, spp=FSPP):
    if name == "mix":
        return hc.Case(MIX["spheres"], MIX["types"], MIX["values"], FDEPTH, spp)
    return hc.Case(*oracle.test_world(), FDEPTH, spp)


def frame_of(name):
    if name == "mix":
        return oracle.camera_look_at(FW, FH, look_from=(4, 1.5, 6), look_at=(0, .8, .5), vfov=40.0, aspect=FW / FH)
    return oracle.camera_simple(FW, FH)


class FrameSpec:
    def __init__(self, name, spp, dtype):
        ys, xs = np.mgrid[0:FH, 0:FW]
        c, self.segments, self.seeds = spec.pixels(frame_world(name, spp), frame_of(name), xs.ravel(), ys.ravel(), dtype)
        self.sums = c  # gamma colours, row-major like the image


_FRAMES = {}


def frame_specs(name, spp=FSPP, fresh=False):
    if fresh:
        return FrameSpec(name, spp, np.float32), FrameSpec(name, spp, np.float64)
    if (name, spp) not in _FRAMES:
        _FRAMES[name, spp] = (FrameSpec(name, spp, np.float32), FrameSpec(name, spp, np.float64))
    return _FRAMES[name, spp]


def frame_tolerance(name, spp=FSPP, fresh=False):
    s32, s64 = frame_specs(name, spp, fresh)
    return Tolerance(s32.sums, s32.segments, s32.seeds, s64.sums, s64.segments, s64.seeds)


def judge_frame(what, tol, want, image, segments):
    """The rule on a frame: per pixel on the gamma colours, and the frame's
    total segment count, which can differ only where a pixel diverged."""
    v = judge(what, tol, want, np.asarray(image)[..., :3].reshape(-1, 3))
    if int(segments) != int(want.segments.sum()) and v.diverged == 0:
        v.diverged, v.ok = 1, 1 <= CAP * v.n
        print(f"{what}: {segments} segments, the reference {int(want.segments.sum())}")
    return v
