"""Path queries along rays of the caller's choosing and what they must give
(include/rtx.h rtx_path_seed), for the CPU checks (test_paths_host.py) and for
GPU tests of an entry point that traces such queries. Only numpy and the
oracle: nothing here touches the GPU library.

The expectation is the zero-film twin. In a frame whose horizontal and vertical
rows are zero, get_ray gives every pixel the ray (origin, fl(lower_left -
origin)) whatever the jitter, so pixel (x, y) differs from its neighbours by
its seed alone: a query with that ray and that pixel's seed is, by the
contract, that pixel. oracle.render_rows_linear renders the twin.
"""
import numpy as np

import oracle

f32 = np.float32
W, H = 8, 4          # seeds per ray: the twin's pixels
SAMPLES, DEPTH = 6, 8
ALL_SKY_MAX = 0.25   # at most this share of a case's rays may see nothing but sky


def twin_frame(o, L, w=W, h=H, frame_index=0, flags=0):
    """The oracle's camera_simple frame of w x h pixels with origin = o,
    lower_left = L, horizontal = vertical = 0 (no lens: camera_simple has
    none), img_w, img_h = w, h."""
    f = oracle.camera_simple(w, h)
    o, L = np.asarray(o, f32), np.asarray(L, f32)
    for k in range(3):
        f.origin[k] = float(o[k])
        f.lower_left[k] = float(L[k])
        f.horizontal[k] = 0.0
        f.vertical[k] = 0.0
    f.img_w, f.img_h = float(w), float(h)
    f.rng_mode, f.frame_index, f.flags = 0, frame_index, flags
    assert f.lens_u[3] == 0.0
    return f


def seed_hash(x, y, frame_index=0):
    """The hash behind pixel (x, y)'s chain seed: the chain-mode rule of the
    render's pixel_seed, from oracle.base_hash."""
    h = oracle.base_hash(int(x), int(y))
    if frame_index != 0:
        h = oracle.base_hash(h, 0x80000000 | int(frame_index))
    return h


def seed(x, y, frame_index=0):
    return f32(f32(seed_hash(x, y, frame_index)) / f32(4294967296.0))


def probes(o, L, w=W, h=H, frame_index=0):
    """The w * h queries of a ray's twin, row-major like the twin's pixels:
    (w * h, 8) float32 rows (o, seed, d, tag) with d = float32(L) - float32(o)."""
    o, L = np.asarray(o, f32), np.asarray(L, f32)
    d = (L - o).astype(f32)
    out = np.empty((w * h, 8), f32)
    out[:, 0:3], out[:, 4:7] = o, d
    out[:, 3] = [seed(x, y, frame_index) for y in range(h) for x in range(w)]
    out.view(np.uint32)[:, 7] = 0xFACADE00 + np.arange(w * h, dtype=np.uint32)
    return out


def ray_recipe(n, rng_seed, scale=1.0):
    """n (origin, target) pairs: the origin uniform in x, z in +-12 * scale and
    y in 0.05 .. 3, the target L uniform in x, z in +-10 * scale and y in
    -0.5 .. 1; no component of L is a negative zero (L + 0 + 0 - o would make
    it +0 in the twin, and d = L - o would not)."""
    rng = np.random.default_rng(rng_seed)
    o = np.c_[rng.uniform(-12, 12, n) * scale, rng.uniform(0.05, 3.0, n), rng.uniform(-12, 12, n) * scale].astype(f32)
    L = np.c_[rng.uniform(-10, 10, n) * scale, rng.uniform(-0.5, 1.0, n), rng.uniform(-10, 10, n) * scale].astype(f32)
    L = (L + f32(0.0)).astype(f32)  # -0 + +0 = +0
    assert not np.signbit(L[L == 0]).any()
    return o, L


class Expect:
    """A case's queries and what they must give: rays (n_rays * w * h, 8), sums
    (the same rows, 3) and, per twin, the oracle's segment count."""

    def __init__(self, rays, sums, twin_segs, per, o, L):
        self.rays, self.sums, self.twin_segs, self.per = rays, sums, twin_segs, per
        self.o, self.L = np.array(o, f32), np.array(L, f32)  # the rays' origins and targets
        for a in (self.rays, self.sums, self.twin_segs, self.o, self.L):
            a.setflags(write=False)


def expect(case, o, L, samples=SAMPLES, depth=DEPTH, w=W, h=H, frame_index=0, flags=0, all_sky_max=ALL_SKY_MAX):
    """The queries of rays (o[i], L[i]) and the oracle's answer: every ray's
    twin rendered at spp = samples and `depth`. all_sky_max: the set-up
    condition — at most that share of the rays may have an all-sky twin (the
    oracle's segments == w * h * samples); None: not asked (hostile rays)."""
    world = type("World", (), dict(spheres=case.spheres, mat_types=case.mat_types, mat_values=case.mat_values,
                                   depth=depth, spp=samples))
    rays, sums, segs = [], [], []
    for oi, Li in zip(np.asarray(o, f32), np.asarray(L, f32)):
        img, s = oracle.render_rows_linear(world, twin_frame(oi, Li, w, h, frame_index, flags), np.arange(h))
        rays.append(probes(oi, Li, w, h, frame_index))
        sums.append(img.reshape(w * h, 4)[:, :3])
        segs.append(s)
    segs = np.array(segs, np.uint64)
    if all_sky_max is not None:
        sky = int((segs == w * h * samples).sum())
        assert sky <= all_sky_max * len(segs), f"{sky} of {len(segs)} rays see only sky: the case exercises no bounce"
    return Expect(np.concatenate(rays), np.ascontiguousarray(np.concatenate(sums), f32), segs, w * h, o, L)
