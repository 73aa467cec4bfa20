"""Film queries (include/rtx.h rtx_trace_film) and what they must give, for the
CPU checks (test_film_host.py) and the GPU tests (test_gpu_film.py). Only numpy
and the oracle: nothing here touches the GPU library.

A film query is a pixel of a frame of its own, so the expectation needs no new
oracle: a case is paths_cases.ray_recipe's (o, L) per ray with a footprint (H,
V) per ray, uniform in +-0.5 per component, and ray i's frame — origin o,
lower_left L, horizontal H, vertical V, 8 x 4 pixels, img_w, img_h = 8, 4 — is
rendered by oracle.render_rows_linear. Its 32 pixels are the ray's 32 queries:
fx = x, fy = y, seed = the chain seed of pixel (x, y).
"""
import numpy as np

import oracle
import paths_cases as pc

f32 = np.float32
W, H = pc.W, pc.H
SAMPLES, DEPTH = pc.SAMPLES, pc.DEPTH
ALL_SKY_MAX = pc.ALL_SKY_MAX
LENS_R = f32(0.05)


def footprints(n, recipe_seed):
    """n footprints (H, V), uniform in +-0.5 per component, and n lens bases
    (lens_u, lens_v), uniform in +-1 per component, from default_rng(recipe
    seed + 1), drawn in that order."""
    rng = np.random.default_rng(recipe_seed + 1)
    hor = rng.uniform(-0.5, 0.5, (n, 3)).astype(f32)
    ver = rng.uniform(-0.5, 0.5, (n, 3)).astype(f32)
    lu = rng.uniform(-1.0, 1.0, (n, 3)).astype(f32)
    lv = rng.uniform(-1.0, 1.0, (n, 3)).astype(f32)
    return hor, ver, lu, lv


def film_frame(o, L, hor, ver, w=W, h=H, img_w=None, img_h=None, frame_index=0, flags=0, lens=None):
    """paths_cases.twin_frame with the rows filled in: horizontal = hor,
    vertical = ver, img_w, img_h (the pixel counts when None) and, with lens =
    (lens_u, lens_v, lens_r), the thin lens."""
    f = pc.twin_frame(o, L, w, h, frame_index, flags)
    hor, ver = np.asarray(hor, f32), np.asarray(ver, f32)
    for k in range(3):
        f.horizontal[k] = float(hor[k])
        f.vertical[k] = float(ver[k])
    f.img_w = float(f32(w if img_w is None else img_w))
    f.img_h = float(f32(h if img_h is None else img_h))
    if lens is not None:
        lu, lv, r = lens
        for k in range(3):
            f.lens_u[k] = float(f32(lu[k]))
            f.lens_v[k] = float(f32(lv[k]))
        f.lens_u[3] = float(f32(r))
    return f


def records(o, L, hor, ver, w=W, h=H, frame_index=0, lens=None, seeds=None):
    """The w * h film records of one ray's frame, row-major like its pixels:
    (w * h, 16) float32 rows (o, seed, L, tag, H, fx, V, fy), or (w * h, 24)
    with lens = (lens_u, lens_v, lens_r): (.., lens_u, lens_r, lens_v, 0)."""
    out = np.zeros((w * h, 16 if lens is None else 24), f32)
    out[:, 0:3], out[:, 4:7] = np.asarray(o, f32), np.asarray(L, f32)
    out[:, 8:11], out[:, 12:15] = np.asarray(hor, f32), np.asarray(ver, f32)
    xy = [(x, y) for y in range(h) for x in range(w)]
    out[:, 3] = [pc.seed(x, y, frame_index) for x, y in xy] if seeds is None else seeds
    out[:, 11] = [f32(x) for x, _ in xy]
    out[:, 15] = [f32(y) for _, y in xy]
    out.view(np.uint32)[:, 7] = 0xF11A0000 + np.arange(w * h, dtype=np.uint32)
    if lens is not None:
        lu, lv, r = lens
        out[:, 16:19], out[:, 19], out[:, 20:23] = np.asarray(lu, f32), f32(r), np.asarray(lv, f32)
    return out


class Expect:
    """A case's records and what they must give: recs (n_rays * w * h, 16 or
    24), sums (the same rows, 3) and, per frame, the oracle's segment count."""

    def __init__(self, recs, sums, frame_segs, per, o, L, hor, ver):
        self.recs, self.sums, self.frame_segs, self.per = recs, sums, frame_segs, per
        self.o, self.L, self.hor, self.ver = (np.array(a, f32) for a in (o, L, hor, ver))
        for a in (self.recs, self.sums, self.frame_segs, self.o, self.L, self.hor, self.ver):
            a.setflags(write=False)


def expect(case, o, L, hor, ver, samples=SAMPLES, depth=DEPTH, w=W, h=H, img_w=None, img_h=None, frame_index=0,
           flags=0, lens=None, all_sky_max=ALL_SKY_MAX):
    """The records of rays (o[i], L[i]) with footprints (hor[i], ver[i]) and the
    oracle's answer: every ray's frame rendered at spp = samples and `depth`.
    lens: None, or (lens_u (n, 3), lens_v (n, 3), lens_r (n,)): 24-float
    records, each frame with its own lens (radius 0: none). all_sky_max: the
    set-up condition — at most that share of the frames may be all sky (the
    oracle's segments == w * h * samples); None: not asked (hostile records)."""
    world = type("World", (), dict(spheres=case.spheres, mat_types=case.mat_types, mat_values=case.mat_values,
                                   depth=depth, spp=samples))
    o, L, hor, ver = (np.asarray(a, f32) for a in (o, L, hor, ver))
    recs, sums, segs = [], [], []
    for i in range(len(o)):
        ln = None if lens is None else (lens[0][i], lens[1][i], lens[2][i])
        frame = film_frame(o[i], L[i], hor[i], ver[i], w, h, img_w, img_h, frame_index, flags, ln)
        img, s = oracle.render_rows_linear(world, frame, np.arange(h))
        recs.append(records(o[i], L[i], hor[i], ver[i], w, h, frame_index, ln))
        sums.append(img.reshape(w * h, 4)[:, :3])
        segs.append(s)
    segs = np.array(segs, np.uint64)
    if all_sky_max is not None:
        sky = int((segs == w * h * samples).sum())
        assert sky <= all_sky_max * len(segs), f"{sky} of {len(segs)} frames are all sky: the case exercises no bounce"
    return Expect(np.concatenate(recs), np.ascontiguousarray(np.concatenate(sums), f32), segs, w * h, o, L, hor, ver)


def recipe(n, rng_seed, scale=1.0):
    """paths_cases.ray_recipe's rays with their footprints and lens bases."""
    o, L = pc.ray_recipe(n, rng_seed, scale)
    return (o, L) + footprints(n, rng_seed)
