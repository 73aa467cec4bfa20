"""The item prefix of the wave-cooperative walk, checked on the CPU
(rtx_grid.h grid_item_prefix; the GPU side: test_gpu_walk_prefix.py). The
kernel numbers a wave's items with one ballot per bit of the lanes' counts
and skips bits 3..5 where no lane has 8 items or more;
tests/walk_prefix_check.cpp runs the header's own code over 64-lane vectors
against a plain prefix sum (beside grid_coop_check.cpp's emulation of the
sharing that follows it).
"""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "walk_prefix_check.cpp")


def test_prefix_equals_a_plain_prefix_sum(tmp_path):
    """1, 17 and 64 active lanes and masks with gaps; every n 0, every n 48,
    one lane with 48, counts below 8, of 7 and 8, random ones; 200,000 random
    waves: start and total are the plain sums in every active lane, and waves
    without a count of 8 or more (the high bits skipped) do occur."""
    exe = str(tmp_path / "walk_prefix_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, SRC], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    print(rep)
    assert out.returncode == 0, (rep, out.stderr)
    assert rep["waves_wrong"] == 0 and rep["waves"] > 200_000, rep
    assert rep["waves_without_high_bits"] > 50_000 and rep["max_items"] == 48, rep


import pytest  # noqa: E402

import walk_prefix_cases as wp  # noqa: E402


@pytest.mark.parametrize("name", wp.WORLDS)
def test_waves_have_the_item_counts_they_are_named_for(tmp_path_factory, oracle, name):
    """The batches test_gpu_walk_prefix.py sends to the GPU, classified with
    grid_stretch on the host: no lane with an item; one lane with the largest
    count (48, the walk's limit, on the strip) and the rest none; every lane
    with it; every lane with 1..7 (the prefix skips its high bits); 7 and 8
    side by side; a mix with a count of 8 or more. No lane of any of them
    gives up, so the wave does run the prefix. And every hit of the oracle on
    a layer sphere lies in a block of the hitting ray's own grid_mask_items
    mask: conditions on the inputs, not on the kernel."""
    c = wp.cases(name, tmp_path_factory.mktemp("walk_items"))
    print(name, c.big, c.available)
    assert c.big == wp.MAX_ITEMS if name == "strip" else 17 <= c.big < wp.MAX_ITEMS, c.big
    for k in ("zero", "big", "low", "seven", "eight", "high"):
        assert c.available[k] >= 20, (k, c.available)  # enough distinct rays of every kind
    if name == "strip":  # the pool reaches past the limit: 48 is the last count that does not give up
        assert c.available["gave_up"] > 0 and c.pool_items.max() == wp.MAX_ITEMS, c.available
    c.check_shapes()
    w = rc_world(name)
    hits = {}
    for key, (rays, _, _) in c.batches.items():
        hits[key] = c.check_hits_in_masks(key, oracle.hit_world_f32(w, rays))
    print(hits)
    # the long stretches do end on layer spheres: the hits a dropped item would lose
    assert sum(v for k, v in hits.items() if k.startswith("every lane big")) >= 40, hits
    assert sum(v for k, v in hits.items() if k.startswith("one lane big")) >= 1, hits


def rc_world(name):
    import regime_cases as rc
    return rc.world(name)
