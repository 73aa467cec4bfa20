"""Worlds and cameras for the large-scene culled layout,
shared by the GPU frame tests (test_gpu_cull_regimes.py) and the CPU check of
the layouts and of what the cameras reach in them (test_cull_cases.py). Only
numpy and the oracle: nothing here touches the GPU library.

rtx_upload_world gives every scene with n_pad > 1024 the culled layout of
rtx_cull.h: up to three sections (large spheres, the other non-flat ones, the
flat ones), each padded to whole blocks of 8, the flat section starting at a
multiple of 512 blocks unless it is the first, and three levels of bounds
(8, 64 and 512 spheres) above the blocks. The worlds below have each shape of
it, each the smallest that also meets test_cull_cases.py's conditions on what
the five cameras reach (below 1,500 spheres the `grazing` camera stands so
near the scene's edge that no bound lies wholly behind it, and a world whose
bnd3 entries all hold 512 spheres has none that any ray from inside the scene
fails: every size here leaves a short last entry):

  mixed         ground, 399 off-layer spheres interleaved with 1100 layer
                spheres, the last 16 of the scene on the layer: the RTIOW
                shape; two bnd3 rows, the second with 3 live entries; the
                block, group and super-group counts are no multiples of 8
  no_flat       1700, no two spheres at one height: no flat section,
                flat_lo = nblk, one bnd3 row with 4 live entries
  layer_no_run  1100, sphere i off-layer iff i % 8 == 0: a layer, but no
                scene-order block of 8 is flat, so the upload finds no flat run
                and the layer is tested with the 7-op bounds
  all_flat      1600, every sphere on the layer and no ground: the flat section
                is the first one, flat_lo = 0
  ground_flat   ground + 1599 layer spheres: one real block, 511 padding blocks
                (bounds with R = -inf), then the flat section
  wide          4400: more than 512 non-flat blocks, flat_lo = 1024, three bnd3
                rows
  bimodal       2400, mixed's recipe (1400 layer, 1000 off) with radii 0.05
                (53 %, so the median), 0.39 (24 %) or 0.41 (23 %, above 8 x the
                median): the large section has 68 blocks, more than one
                super-group, and holds layer-height spheres too. (With only
                0.05 and 0.5 over 1300 spheres the default camera's 2,304 rays
                hit 7 spheres of the flat section: r = 0.05 is below a pixel
                and behind the large ones. The 0.39 spheres are what the
                cameras see of the other two sections.)
  two_layers    1500: ground, 599 at y = 0.2 and 450 at y = 0.75, one run each,
                450 at heights of their own: only the longer run is the flat
                section
  rtiow20       oracle.random_world(20): the shape every other large-scene
                frame test uses, as the control

expected_info() states a world's row as Context.scene_info()'s fields, from a
numpy restatement of the sectioning rule, never read back from the library.
"""
import numpy as np

import oracle
import regime_cases as rc
from regime_cases import GROUND, LAYER_Y, Case, H, W, _extent, _materials, camera_args, primary_rays  # noqa: F401

SMALL_MAX_PAD = rc.SMALL_MAX_PAD  # scenes padded to more than this take the culled layout
CULL_ALIGN = 512                  # blocks: where a flat section that is not the first one starts
BIG_FACTOR = 8.0                  # large: |r| > 8 x the median |r|

CAMERAS = {k: v for k, v in rc.CAMERAS.items() if k != "along_strip"}
assert list(CAMERAS) == ["default", "grazing", "far", "top_down", "in_slab"]


def _scattered(seed, n, layer_at, ground=True, radii=None, heights=None):
    """n spheres over x, z in +-_extent(n), radii 0.1..0.3 unless given;
    `layer_at`: bool [n], True where the sphere lies on the layer (y = 0.2);
    every other sphere has a height of its own, 0.5 + k / 1024, unless
    `heights` gives them; sphere 0 is the ground if asked."""
    rng = np.random.default_rng(seed)
    ex = _extent(n)
    r = rng.uniform(0.1, 0.3, n) if radii is None else radii(rng, n)
    sph = np.c_[rng.uniform(-ex, ex, n), np.full(n, LAYER_Y), rng.uniform(-ex, ex, n), r]
    off = np.flatnonzero(~layer_at)
    sph[off, 1] = 0.5 + rng.permutation(len(off)) / 1024.0 if heights is None else heights[off]
    if ground:
        sph[0] = GROUND
    mt, mv = _materials(rng, n)
    return Case(sph, mt, mv, int(layer_at.sum()))


def _mixed_mask(seed, layer, off, tail=16):
    """`layer` layer spheres and `off` off-layer ones (the ground among them)
    mixed at random in scene order, the last `tail` of the scene on the layer."""
    n = layer + off
    rng = np.random.default_rng(seed + 1000)
    at = np.ones(n, bool)
    at[0] = False
    at[1 + rng.permutation(n - 1 - tail)[:off - 1]] = False
    assert at.sum() == layer and at[-tail:].all()
    return at


def _mixed(seed, layer, off, **kw):
    return _scattered(seed, layer + off, _mixed_mask(seed, layer, off), **kw)


def _no_flat():
    return _scattered(202, 1700, np.zeros(1700, bool))


def _layer_no_run():
    return _scattered(203, 1100, np.arange(1100) % 8 != 0)


def _two_layers():
    """ground; 1..599 at y = 0.2; 600..1049 at y = 0.75; 1050..1499 at heights of their own."""
    n = 1500
    k = np.arange(n)
    h = np.where(k < 1050, 0.75, 1.0 + (k - 1050) / 1024.0)
    return _scattered(208, n, (k >= 1) & (k < 600), heights=h)


def _bimodal_radii(rng, n):
    u = rng.random(n)
    return np.where(u < 0.53, 0.05, np.where(u < 0.77, 0.39, 0.41))


def _rtiow20():
    sph, mt, mv = oracle.random_world(20)
    return Case(sph, mt, mv, int((sph[:, 1] == np.float32(LAYER_Y)).sum()))


WORLDS = {
    "mixed": lambda: _mixed(201, 1100, 400),
    "no_flat": _no_flat,
    "layer_no_run": _layer_no_run,
    "all_flat": lambda: _scattered(204, 1600, np.ones(1600, bool), ground=False),
    "ground_flat": lambda: _scattered(205, 1600, np.arange(1600) >= 1),
    "wide": lambda: _mixed(206, 215, 4185),
    "bimodal": lambda: _mixed(209, 1400, 1000, radii=_bimodal_radii),
    "two_layers": _two_layers,
    "rtiow20": _rtiow20,
}
# (large, other, flat) spheres of each world, by its construction where the
# construction fixes them; bimodal's are what its seed gave
SECTIONS = {"mixed": (1, 399, 1100), "no_flat": (1, 1699, 0), "layer_no_run": (1, 1099, 0), "all_flat": (0, 0, 1600),
            "ground_flat": (1, 0, 1599), "wide": (1, 4184, 215), "bimodal": (540, 776, 1084), "two_layers": (1, 900, 599),
            "rtiow20": (1, 3, 1597)}
# the layout's padded position count and the flat section's first block
LAYOUT = {"mixed": (5200, 512), "no_flat": (1712, 214), "layer_no_run": (1112, 139), "all_flat": (1600, 0),
          "ground_flat": (5696, 512), "wide": (8408, 1024), "bimodal": (5184, 512), "two_layers": (4696, 512),
          "rtiow20": (5696, 512)}

_CACHE = {}


def world(name):
    """The world `name`, built once; its arrays are read-only."""
    if name not in _CACHE:
        _CACHE[name] = WORLDS[name]()
    return _CACHE[name]


def sections(spheres):
    """The sectioning rule of rtx_cull.h restated: the section (0 large, 1
    other, 2 flat) of every sphere. Large: |r| > 8 x the median |r| (the
    element n // 2 of the sorted radii); flat: the scene has a scene-order run
    of flat blocks and the height's bits equal those of the longest one."""
    sph = np.ascontiguousarray(spheres, np.float32)
    n = len(sph)
    r = np.abs(sph[:, 3])
    big = np.float32(BIG_FACTOR) * np.sort(r)[n // 2]
    lo, hi = rc.scene_order_flat_run(sph)
    sec = np.ones(n, int)
    if hi > lo:
        yb = sph[:, 1].view(np.uint32)
        sec[yb == yb[min(8 * lo, n - 1)]] = 2
    sec[r > big] = 0
    return sec


def layout_shape(spheres):
    """(positions, flat_lo) of the culled layout: each section padded to 8,
    the flat section at a multiple of CULL_ALIGN blocks unless it is first;
    flat_lo = the block count when there is no flat section."""
    cnt = np.bincount(sections(spheres), minlength=3)
    blocks = [(int(c) + 7) // 8 for c in cnt]
    before = blocks[0] + blocks[1]
    if cnt[2] == 0:
        return 8 * before, before
    flat_lo = (before + CULL_ALIGN - 1) // CULL_ALIGN * CULL_ALIGN
    return 8 * (flat_lo + blocks[2]), flat_lo


def levels(name):
    """(nblk, ngrp, nsg, nhg): the entries of each level of world `name`'s layout."""
    nblk = LAYOUT[name][0] // 8
    ngrp = (nblk + 7) // 8
    nsg = (ngrp + 7) // 8
    return nblk, ngrp, nsg, (nsg + 7) // 8


def expected_info(name, linear=False):
    """The world's row as Context.scene_info()'s fields (those the row
    fixes). linear: after set_scan_mode("linear"), where no scene has a culled
    layout."""
    w = world(name)
    n = w.count
    n_pad = (n + 7) // 8 * 8
    assert n_pad > SMALL_MAX_PAD, name
    # the tables above follow from the arrays: a mistake in them shows here
    cnt = tuple(int(c) for c in np.bincount(sections(w.spheres), minlength=3))
    assert cnt == SECTIONS[name], (name, cnt)
    assert layout_shape(w.spheres) == LAYOUT[name], (name, layout_shape(w.spheres))
    want = dict(count=n, n_pad=n_pad, kernels=2 if linear else 1, sphere_copy_lds=0, layout=0, layout_positions=0,
                map_in_lds=0, grid=0, grid_nx=0, grid_nz=0)
    pos, flat_lo = (0, 0) if linear else LAYOUT[name]
    run_lo, run_hi = rc.scene_order_flat_run(w.spheres)  # (the scene-order `pre` keeps its own flat run)
    want.update(cull_positions=pos, cull_flat_lo=flat_lo, flat_lo=run_lo, flat_hi=run_hi)
    return want
