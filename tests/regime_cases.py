"""Worlds and cameras for the small-scene scan regimes,
shared by the GPU frame tests (test_gpu_scan_regimes.py) and the CPU check
that the cases reach the branches they are meant for (test_scan_regimes.py).
Only numpy and the oracle: nothing here touches the GPU library.

rtx_upload_world sends a scene with n_pad <= 1024 down one of four paths:

  R1  n <= 512, layer 16..512: sphere copy in LDS, a layout, the position map
      in LDS (uint16), the layer grid over position blocks
  R2  n 513..640: sphere copy in LDS, never a layout (copy and map do not fit
      the render's LDS together); a grid over the scene-order flat run, if
      there is one
  R3  n 641.., layer 16..512: no sphere copy, a layout, the position map in
      memory (cperm), the grid over position blocks
  R0  layer below 16 or above 512, or no two equal heights: no layout; the
      sphere copy by n; a scene-order run or none

expected_info() states a world's row as those fields, from the counts of its
construction, for comparison with Context.scene_info().
"""
import numpy as np

import oracle
from test_gpu_layout import _twins

W, H = 64, 36
GROUND = (0.0, -1000.0, 0.0, 1000.0)
LAYER_Y = 0.2

# the constants the regimes hang on, as DESIGN.md §3f states them: a test's
# expectation is written with these, never read back from the library
COOP_LDS = 640       # spheres up to which the render keeps the LDS sphere copy
LAYER_MIN, LAYER_MAX = 16, 512
SMALL_MAX_PAD = 1024
GRID_MAX_BLOCKS = 64


class Case:
    """A world: what oracle.render_rows and rtx.World take."""

    def __init__(self, spheres, mat_types, mat_values, layer, depth=50, spp=10):
        self.spheres = np.ascontiguousarray(spheres, np.float32)
        self.mat_types = np.ascontiguousarray(mat_types, np.float32)
        self.mat_values = np.ascontiguousarray(mat_values, np.float32)
        for a in (self.spheres, self.mat_types, self.mat_values):
            a.setflags(write=False)
        self.layer = layer  # spheres of the layer by construction (0: none of a usable size)
        self.depth, self.spp = depth, spp

    @property
    def count(self):
        return len(self.spheres)

    def at_spp(self, spp):
        return Case(self.spheres, self.mat_types, self.mat_values, self.layer, self.depth, spp)


def _materials(rng, n):
    """Types from {0, 1, 2}; albedo 0.2..1; metal fuzz 0..0.3, ir 1.3..1.6.
    Sphere 0 (the ground) is Lambertian grey."""
    mt = rng.integers(0, 3, n).astype(np.float32)
    mv = np.c_[rng.uniform(0.2, 1.0, (n, 3)), np.where(mt == 1, rng.uniform(0.0, 0.3, n), rng.uniform(1.3, 1.6, n))]
    if n:
        mt[0] = 0.0
        mv[0] = (0.5, 0.5, 0.5, 0.0)
    return mt, mv.astype(np.float32)


def _extent(n):
    return 11.0 * np.sqrt(n / 486.0)


def _scattered(seed, n, layer_at, ext_x=None, ext_z=None, radius=(0.1, 0.3)):
    """n spheres, sphere 0 the ground; `layer_at`: bool [n], True where the
    sphere lies on the layer (y = 0.2); every other sphere has a height of its
    own, 0.5 + k / 1024."""
    rng = np.random.default_rng(seed)
    ex = _extent(n) if ext_x is None else ext_x
    ez = _extent(n) if ext_z is None else ext_z
    sph = np.c_[rng.uniform(-ex, ex, n), np.full(n, LAYER_Y), rng.uniform(-ez, ez, n), rng.uniform(*radius, n)]
    off = np.flatnonzero(~layer_at)
    sph[off, 1] = 0.5 + rng.permutation(len(off)) / 1024.0
    sph[0] = GROUND
    mt, mv = _materials(rng, n)
    return Case(sph, mt, mv, int(layer_at.sum()))


def _interleaved(seed, layer, off):
    """`layer` layer spheres mixed at random, in scene order, with `off`
    off-layer ones, the ground among them."""
    n = layer + off
    rng = np.random.default_rng(seed + 1000)
    at = np.ones(n, bool)
    at[0] = False
    at[1 + rng.permutation(n - 1)[:off - 1]] = False
    return _scattered(seed, n, at)


def _run(seed, off, layer):
    """`off` off-layer spheres (the ground first), then `layer` layer spheres
    contiguous in scene order."""
    at = np.arange(off + layer) >= off
    return _scattered(seed, off + layer, at)


def _strip(seed, layer, off):
    """The layer in x +-30, z +-2 (a 64 x 8 grid of unit cells): the same
    layer spheres for every `off`, interleaved in scene order with `off`
    off-layer ones over the same strip."""
    n = layer + off
    rl, ro = np.random.default_rng(seed), np.random.default_rng(seed + 1000 + off)
    at = np.ones(n, bool)
    at[0] = False
    at[1 + ro.permutation(n - 1)[:off - 1]] = False
    sph = np.empty((n, 4))
    sph[at] = np.c_[rl.uniform(-30, 30, layer), np.full(layer, LAYER_Y), rl.uniform(-2, 2, layer),
                    rl.uniform(0.1, 0.3, layer)]
    sph[~at] = np.c_[ro.uniform(-30, 30, off), 0.5 + ro.permutation(off) / 1024.0, ro.uniform(-2, 2, off),
                     ro.uniform(0.1, 0.3, off)]
    sph[0] = GROUND
    mt, mv = _materials(ro, n)
    return Case(sph, mt, mv, layer)


def _rtiow11():
    sph, mt, mv = oracle.random_world(11)
    return Case(sph, mt, mv, len(sph) - 4)


def _twins_world():
    sph = _twins(True)
    mt, mv = _materials(np.random.default_rng(31), len(sph))
    return Case(sph, mt, mv, len(sph) - 1)


def _two_layers():
    """24 + 24 spheres alternating between two heights, plus the ground: two
    sets of equal size, the layer is the one whose first sphere comes first
    (sphere 1, y = 0.2)."""
    n = 49
    rng = np.random.default_rng(41)
    ex = _extent(n)
    k = np.arange(n)
    sph = np.c_[rng.uniform(-ex, ex, n), np.where(k % 2 == 1, LAYER_Y, 0.75), rng.uniform(-ex, ex, n),
                rng.uniform(0.1, 0.3, n)]
    sph[0] = GROUND
    mt, mv = _materials(rng, n)
    return Case(sph, mt, mv, 24)


def _no_layer():
    """100 spheres, no two at one height: sphere k at k / 64."""
    n = 100
    rng = np.random.default_rng(51)
    ex = _extent(n)
    sph = np.c_[rng.uniform(-ex, ex, n), np.arange(n) / 64.0, rng.uniform(-ex, ex, n), rng.uniform(0.1, 0.3, n)]
    sph[0] = GROUND
    mt, mv = _materials(rng, n)
    return Case(sph, mt, mv, 0)


WORLDS = {
    "rtiow11": _rtiow11,
    "lds_full": lambda: _interleaved(101, 500, 12),
    "twins": _twins_world,
    "two_layers": _two_layers,
    "r2_run": lambda: _run(102, 40, 512),
    "r2_mixed": lambda: _interleaved(103, 512, 37),
    "r3_small": lambda: _interleaved(104, 500, 141),
    "r3_full": lambda: _interleaved(105, 512, 500),
    "r3_tiny_layer": lambda: _interleaved(106, 16, 700),
    "strip": lambda: _strip(108, 480, 24),
    "strip_r3": lambda: _strip(108, 480, 200),
    "layer15": lambda: _interleaved(108, 15, 9),
    "no_layer": _no_layer,
}
# the regime of each, from the table of DESIGN.md §3f
REGIME = {"rtiow11": "R1", "lds_full": "R1", "twins": "R1", "two_layers": "R1", "r2_run": "R2", "r2_mixed": "R2",
          "r3_small": "R3", "r3_full": "R3", "r3_tiny_layer": "R3", "strip": "R1", "strip_r3": "R3",
          "layer15": "R0", "no_layer": "R0"}
# the layout's padded position count, from the construction: each section
# (off-layer, layer) padded to whole blocks of 8
LAYOUT_POSITIONS = {"rtiow11": 8 + 488, "lds_full": 16 + 504, "twins": 8 + 304, "two_layers": 32 + 24,
                    "r3_small": 144 + 504, "r3_full": 504 + 512, "r3_tiny_layer": 704 + 16, "strip": 24 + 480,
                    "strip_r3": 200 + 480}
GRID_SIZE = {"strip": (64, 8), "strip_r3": (64, 8)}
# r2_run: 40 off-layer spheres fill blocks 0..4, the 512 layer spheres blocks 5..68
FLAT_RUN = {"r2_run": (5, 69)}

_CACHE = {}


def world(name):
    """The world `name`, built once; its arrays are read-only."""
    if name not in _CACHE:
        _CACHE[name] = WORLDS[name]()
    return _CACHE[name]


# "default" is camera_look_at's defaults (from (13, 2, 3), at the origin) but
# for vfov 16 instead of 20: at 20 only 899 of the 2,304 primary rays have 1-16
# items on `twins`, whose layer is a band 17 long and 1 wide, and
# test_scan_regimes.py asks 1,000 of every world with a grid.
CAMERAS = {
    "default": dict(vfov=16.0),
    "grazing": dict(look_from=(-12.0, 0.3, 0.5), look_at=(12.0, 0.2, 0.0)),
    "far": dict(look_from=(70.0, 12.0, 20.0), look_at=(0.0, 0.0, 0.0), vfov=10.0),
    "top_down": dict(look_from=(0.0, 20.0, 0.0), look_at=(0.0, 0.0, 0.0), vup=(0.0, 0.0, 1.0), vfov=40.0),
    "in_slab": dict(look_from=(0.3, 0.2, 0.3), look_at=(5.0, 0.2, 5.0), vfov=60.0),
    "along_strip": dict(look_from=(-31.0, 0.25, 0.1), look_at=(31.0, 0.2, 0.0), vfov=8.0),
}


def camera_args(name):
    """Keyword arguments of camera_look_at (rtx's or the oracle's) for camera `name` at 64 x 36."""
    return dict(width=W, height=H, aspect=W / H, **CAMERAS[name])


def in_plane(frame):
    """`frame` (rtx's or the oracle's) turned into a fan of rays that lie in
    the plane z = 0 exactly, for `twins`: from (0, 6, 0) down onto x in +-9,
    y in 0..0.6. horizontal and vertical have no z and lower_left's z is the
    origin's, so every sample's direction, jittered or not, has d.z = 0 bit
    for bit and meets a column's mirror twins (z = -+0.25) at bit-equal
    roots."""
    for name, v in (("origin", (0.0, 6.0, 0.0)), ("horizontal", (18.0, 0.0, 0.0)), ("vertical", (0.0, 0.6, 0.0)),
                    ("lower_left", (-9.0, 0.0, 0.0))):
        for k in range(3):
            getattr(frame, name)[k] = v[k]
    return frame


def primary_rays(frame):
    """The pixel-centre primary rays of a frame, [H * W, 6] float32 (origin,
    direction), with the render's ops: u = (x + 0.5) / (img_w - 1),
    d = ((llc + u hor) + v ver) - org."""
    f32 = np.float32
    x = np.arange(frame.width, dtype=f32)
    y = np.arange(frame.height, dtype=f32)
    u = ((x + f32(0.5)) / (f32(frame.img_w) - f32(1.0))).astype(f32)
    v = ((y + f32(0.5)) / (f32(frame.img_h) - f32(1.0))).astype(f32)
    org = np.array(frame.origin[:3], f32)
    hor = np.array(frame.horizontal[:3], f32)
    ver = np.array(frame.vertical[:3], f32)
    llc = np.array(frame.lower_left[:3], f32)
    d = (llc[None, None, :] + u[None, :, None] * hor[None, None, :]).astype(f32)
    d = (d + v[:, None, None] * ver[None, None, :]).astype(f32)
    d = (d - org[None, None, :]).astype(f32).reshape(-1, 3)
    return np.ascontiguousarray(np.c_[np.broadcast_to(org, d.shape), d], f32)


def scene_order_flat_run(spheres):
    """The longest run of flat 8-sphere blocks in scene order, as (lo, hi)
    (rtx_internal.h KScene::flat_lo, flat_hi; the first of equal length;
    (0, 0): none): a block is flat when its 8 centre heights are equal bit for
    bit, the last block padded with copies of the last sphere, and a run keeps
    one height."""
    n = len(spheres)
    if n == 0:
        return 0, 0
    yb = np.ascontiguousarray(spheres[:, 1], np.float32).view(np.uint32)
    yb = np.r_[yb, np.full(-n % 8, yb[-1], np.uint32)].reshape(-1, 8)
    flat = (yb == yb[:, :1]).all(axis=1)
    best, b, nblk = (0, 0), 0, len(yb)
    while b < nblk:
        if not flat[b]:
            b += 1
            continue
        e = b + 1
        while e < nblk and flat[e] and yb[e, 0] == yb[b, 0]:
            e += 1
        if e - b > best[1] - best[0]:
            best = (b, e)
        b = e
    return best


def expected_info(name, linear=False):
    """The world's row of the regime table as Context.scene_info()'s fields
    (those the row fixes). linear: after set_scan_mode("linear"), where no
    small scene has a layout or a grid."""
    w = world(name)
    n = w.count
    regime = REGIME[name]
    n_pad = (n + 7) // 8 * 8
    assert n_pad <= SMALL_MAX_PAD
    want = dict(count=n, n_pad=n_pad, kernels=0, sphere_copy_lds=int(n <= COOP_LDS))
    # the regime follows from the counts: a mistake in the table above shows here
    has_layer = LAYER_MIN <= w.layer <= LAYER_MAX
    assert regime == ("R0" if not has_layer else "R1" if n <= 512 else "R2" if n <= COOP_LDS else "R3"), name
    if regime in ("R1", "R3") and not linear:
        off_pad = (n - w.layer + 7) // 8 * 8
        pos = off_pad + (w.layer + 7) // 8 * 8
        assert pos == LAYOUT_POSITIONS[name], name
        want.update(layout=1, layout_positions=pos, map_in_lds=int(regime == "R1"),
                    flat_lo=off_pad // 8, flat_hi=pos // 8, grid=1)
        if name in GRID_SIZE:
            want.update(grid_nx=GRID_SIZE[name][0], grid_nz=GRID_SIZE[name][1])
    else:
        lo, hi = scene_order_flat_run(w.spheres)
        assert (lo, hi) == FLAT_RUN.get(name, (lo, hi)), name
        grid = int(not linear and hi > lo and hi - lo <= GRID_MAX_BLOCKS)
        want.update(layout=0, layout_positions=0, map_in_lds=0, flat_lo=lo, flat_hi=hi, grid=grid)
        if not grid:
            want.update(grid_nx=0, grid_nz=0)
    return want
