"""GPU side of the walk's item prefix (rtx_kernels.hip grid_wave_mask,
rtx_grid.h grid_item_prefix; the arithmetic itself and the conditions on these
inputs: test_walk_prefix.py on the CPU).

The batches are walk_prefix_cases.py's: rays chosen on the host by their
grid_stretch item count, so that a wave provably has no lane with an item, one
lane with the largest count (48, the walk's limit, on the strip's 64 x 8 grid)
and the rest none, every lane with it, every lane with 1..7 (the prefix skips
bits 3..5), 7 and 8 side by side, or a mix; each as a full wave and as a last
wave of 1, 17 or 64 active lanes; no lane gives up, so the prefix runs. The
counts of every wave are asserted here again before anything is launched.

The wave's block mask itself cannot be compared with the OR of
grid_mask_items: the C-ABI has no output for it (rtx_debug_hit_world returns
hit records). What is compared is what the mask is for. Every hit of the
oracle on a layer sphere lies in a block of the hitting ray's own host mask
(asserted), so a start or total that is wrong hands a slot the wrong item or
none, the block leaves the wave's union wherever no other lane marks it (in
"one lane big, the rest 0" no other lane marks anything), and the hit is
lost: the answers must be the oracle's and the LINEAR upload's, bit for bit.
A mask that is too large scans more blocks and changes no answer; that side is
the frame time's to show.
"""
import numpy as np
import pytest

import regime_cases as rc
import walk_prefix_cases as wp
from test_gpu_grid_coop import assert_bits_equal
from test_gpu_parity import stress_ctx  # noqa: F401

pytestmark = pytest.mark.gpu

CTXS = ["gpu_ctx", "stress_ctx"]


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("walk_items")


@pytest.mark.parametrize("ctx_name", CTXS)
@pytest.mark.parametrize("name", wp.WORLDS)
def test_waves_chosen_by_item_count(request, rtx, oracle, workdir, ctx_name, name):
    ctx = request.getfixturevalue(ctx_name)
    c = wp.cases(name, workdir)
    assert c.big == wp.MAX_ITEMS if name == "strip" else 17 <= c.big < wp.MAX_ITEMS
    c.check_shapes()
    case = rc.world(name)
    world = rtx.World(case.spheres, case.mat_types, case.mat_values, 1, 1)
    got = {}
    try:
        for mode in ("linear", "auto"):
            ctx.set_scan_mode(mode)
            ctx.upload_world(world)
            info = ctx.scene_info()
            assert info["kernels"] == 0 and info["grid"] == int(mode == "auto"), info
            if mode == "auto":  # the host's layout is the library's
                assert (info["flat_lo"], info["flat_hi"], info["layout_positions"]) == (c.flat_lo, c.flat_hi,
                                                                                       len(c.perm)), info
            got[mode] = {k: ctx.debug_hit_world(b[0]) for k, b in c.batches.items()}
    finally:
        ctx.set_scan_mode("auto")
    in_mask = 0
    for key, (rays, _, _) in c.batches.items():
        want = oracle.hit_world_f32(world, rays)
        in_mask += c.check_hits_in_masks(key, want)
        assert_bits_equal(got["auto"][key], want, f"{ctx_name} {name} {key}: grid vs oracle")
        assert_bits_equal(got["auto"][key], got["linear"][key], f"{ctx_name} {name} {key}: grid vs linear")
    assert in_mask > 500  # hits that depend on the wave's mask
