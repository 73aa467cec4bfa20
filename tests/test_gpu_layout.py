"""GPU side of the small-scene spatial layout (rtx_layout.h; CPU side:
test_layout.py). A small scene with a sphere layer is scanned in the layout's
block order — off-layer spheres first, the layer in spatially compact blocks —
with list entries holding positions that the resolve maps back to scene
indices. Nothing a caller can see may change: frames and hit_world answers
are bit for bit the fp32 oracle's, from every start block, and a tie between
equal roots still goes to the later *scene* index, whichever block order the
scan met the two spheres in. Both builds: the product's, and the stress build
whose one-entry candidate lists make every resolve round resume inside the
layout.
"""
import os

import numpy as np
import pytest

from test_gpu_parity import stress_ctx  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 160, 90
NRAYS = 1000  # not a multiple of 64: the last wave is partly empty
CTXS = ["gpu_ctx", "stress_ctx"]


def assert_bits_equal(a, b, what=""):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    assert same.all(), f"{what}: {(~same).sum()} of {same.size} values differ; first at {np.argwhere(~same)[:5].tolist()}"


@pytest.fixture(scope="module")
def frames(rtx, oracle):
    """random_world(11) at 160x90, spp 4, depth 50, and the oracle's frame for
    each RNG mode: computed once, shared, never changed."""
    world = rtx.random_world(11, depth=50, spp=4)
    out = {}
    for rng_mode in (0, 1):
        frame = rtx.camera_look_at(W, H, aspect=W / H)
        frame.rng_mode = rng_mode
        want, segs = oracle.render_rows(world, frame, np.arange(H), nthreads=min(8, os.cpu_count() or 1))
        want.setflags(write=False)
        out[rng_mode] = (frame, want, segs)
    return world, out


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("rng_mode", [0, 1], ids=["chain", "per-sample"])
def test_frame_bit_exact_auto_and_linear(request, frames, ctx_name, rng_mode):
    """AUTO (the layout) and LINEAR (scene order, every block) give the
    oracle's frame and segment count."""
    ctx = request.getfixturevalue(ctx_name)
    world, per_mode = frames
    frame, want, segs = per_mode[rng_mode]
    try:
        for mode in ("auto", "linear"):
            ctx.set_scan_mode(mode)
            ctx.upload_world(world)
            ctx.set_frame(frame)
            ctx.stats_reset()
            img = ctx.render_image()
            st = ctx.stats()
            assert_bits_equal(img, want, f"{ctx_name} {mode} rng {rng_mode}")
            assert st.segments == segs, (ctx_name, mode, rng_mode)
    finally:
        ctx.set_scan_mode("auto")


def _world(rtx, sph):
    sph = np.ascontiguousarray(sph, np.float32)
    n = len(sph)
    return rtx.World(sph, np.zeros(n, np.float32), np.zeros((n, 4), np.float32), 1, 1)


def _interleaved(rng, layer, off, y0):
    """`layer` spheres at height y0 mixed at random, in scene order, with `off`
    spheres at other heights (the CPU checker's construction)."""
    n = layer + off
    sph = np.c_[rng.uniform(-9, 9, n), np.full(n, y0), rng.uniform(-9, 9, n), rng.uniform(0.05, 0.5, n)]
    where = rng.permutation(n)[:off]
    sph[where, 1] = y0 + 1.0 + np.arange(off) / 1024.0
    return sph.astype(np.float32)


def _twins(flip):
    """17 columns along x, each a pair of mirror twins at z = -+0.25 (r 0.4)
    with 14 small fillers between them. A ray in the plane z = 0 meets both
    twins at bit-equal roots (o.z - c.z = +-0.25, d.z = 0: the same hb, cc and
    discriminant). The median split orders a column by z, so the -z twin comes
    15 positions — more than a block — before the +z twin; in the columns
    where the -z twin has the later scene index (every column when `flip`,
    else every second one) position order is the reverse of scene order.
    Exactly coincident spheres cannot be reversed: the split breaks their tie
    by scene index; they are in here too (the last two columns repeat)."""
    rows = []
    for c in range(17):
        x = float(c - 8)
        fill = [(x, 0.2, s * (0.02 + 0.025 * k), 0.01) for k in range(7) for s in (1.0, -1.0)]
        first, last = ((x, 0.2, 0.25, 0.4), (x, 0.2, -0.25, 0.4))
        if not (flip or c % 2 == 0):
            first, last = last, first
        rows += [first] + fill + [last]
    rows += rows[-32:]  # exact duplicates of the last two columns
    rows = [(0.0, -1000.0, 0.0, 1000.0)] + rows  # the ground, off the layer
    return np.array(rows, np.float32)


def _twin_rays(rng, n):
    """Rays in the plane z = 0 (o.z = 0, d.z = 0 exactly) over the columns:
    dropping from above and grazing along x."""
    x = rng.uniform(-9, 9, n)
    steep = rng.random(n) < 0.5
    o = np.c_[x, np.where(steep, rng.uniform(1, 3, n), rng.uniform(0.05, 0.5, n)), np.zeros(n)]
    d = np.c_[np.where(steep, rng.normal(scale=0.2, size=n), rng.choice([-1.0, 1.0], n)),
              np.where(steep, -1.0, rng.normal(scale=0.02, size=n)), np.zeros(n)]
    return np.c_[o, d * rng.uniform(0.5, 2, (n, 1))].astype(np.float32)


def _rays(rng, sph, n):
    """Aimed at and near the silhouettes of random spheres, from around and
    above the scene; every eighth leaves a sphere's surface."""
    c = sph[rng.integers(0, len(sph), n)].astype(np.float64)
    tgt = c[:, :3] + c[:, 3:4] * rng.normal(scale=0.7, size=(n, 3))
    o = np.c_[rng.uniform(-14, 14, n), rng.uniform(0.0, 5.0, n), rng.uniform(-14, 14, n)]
    d = (tgt - o) * rng.uniform(0.2, 3.0, (n, 1))
    leave = np.arange(n) % 8 == 0
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o[leave] = (c[:, :3] + c[:, 3:4] * nrm)[leave]
    d[leave] = rng.normal(size=(int(leave.sum()), 3))
    return np.c_[o, d].astype(np.float32)


def _crafted(rtx):
    rng = np.random.default_rng(77)
    w11, w5 = rtx.random_world(11, depth=1, spp=1), rtx.random_world(5, depth=1, spp=1)
    two = np.c_[rng.uniform(-8, 8, 48), np.where(np.arange(48) % 2, 1.5, -0.25), rng.uniform(-8, 8, 48),
                np.full(48, 0.3)]
    none = np.c_[rng.uniform(-8, 8, 100), np.arange(100) / 64.0, rng.uniform(-8, 8, 100), np.full(100, 0.3)]
    worlds = {"rtiow11": w11.spheres, "rtiow5": w5.spheres, "two equal layers": two, "no layer": none}
    # (512 and 513 spheres: with and without room for the LDS position map
    # beside the sphere copy; 641 and 712: no sphere copy, the map in memory)
    for layer, off in ((15, 9), (16, 0), (19, 30), (67, 5), (259, 21), (500, 12), (500, 13), (512, 37), (513, 3),
                       (500, 141), (512, 200)):
        worlds[f"layer {layer} + {off}"] = _interleaved(rng, layer, off, 0.5)
    return {k: np.ascontiguousarray(v, np.float32).reshape(-1, 4) for k, v in worlds.items()}


@pytest.fixture(scope="module")
def crafted(rtx, oracle):
    """The CPU test's worlds with 1,000 rays each and the oracle's answers."""
    rng = np.random.default_rng(78)
    out = {}
    for name, sph in _crafted(rtx).items():
        world = _world(rtx, sph)
        rays = _rays(rng, sph, NRAYS)
        want = oracle.hit_world_f32(world, rays)
        want.setflags(write=False)
        out[name] = (world, rays, want)
    return out


@pytest.mark.parametrize("ctx_name", CTXS)
def test_hit_world_crafted_worlds_every_start(request, crafted, ctx_name):
    """rtx_debug_hit_world and rtx_debug_hit_world_from (start blocks 0, 1, one
    inside the flat run, the last one, one far past the count) on every
    crafted world: the oracle's answer, bit for bit."""
    ctx = request.getfixturevalue(ctx_name)
    hits = 0
    for name, (world, rays, want) in crafted.items():
        ctx.upload_world(world)
        nblk = (world.count + 7) // 8
        for start in (None, 0, 1, nblk // 2, nblk, 1_000_003):
            got = ctx.debug_hit_world(rays, start_block=start)
            assert_bits_equal(got, want, f"{ctx_name} {name} start {start}")
        hits += int((want[:, 0] == 1).sum())
    assert hits > 2000  # the rays do hit


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("flip", [False, True])
def test_ties_go_to_the_later_scene_index(request, rtx, oracle, ctx_name, flip):
    """Mirror twins met at bit-equal roots, in different blocks of the layout,
    with position order the reverse of scene order: the hit is the twin with
    the later scene index, from every start block."""
    ctx = request.getfixturevalue(ctx_name)
    sph = _twins(flip)
    world = _world(rtx, sph)
    rays = _twin_rays(np.random.default_rng(5 + flip), NRAYS)
    want = oracle.hit_world_f32(world, rays)
    idx = want[:, 9].astype(int)
    big = (want[:, 0] == 1) & (sph[np.clip(idx, 0, len(sph) - 1), 3] == np.float32(0.4))
    assert big.sum() > 300
    # the oracle's winner is the later twin of its column (or of its duplicate column)
    x, z = sph[:, 0], sph[:, 2]
    for i in idx[big][:200]:
        same = np.flatnonzero((x == x[i]) & (np.abs(z) == 0.25) & (sph[:, 3] == np.float32(0.4)))
        assert i == same.max(), (i, same)
    ctx.upload_world(world)
    nblk = (world.count + 7) // 8
    for start in (None, 0, 1, 3, nblk // 2, nblk - 1):
        got = ctx.debug_hit_world(rays, start_block=start)
        assert_bits_equal(got, want, f"{ctx_name} twins flip={flip} start {start}")
