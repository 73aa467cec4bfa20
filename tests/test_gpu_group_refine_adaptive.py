"""rtx_group_refine_adaptive and rtx_refine_adaptive_rows: adaptive refinement
on row parts and across a group's members, on the box's one MI355X through
one-device rehearsal groups (every member on device 0, one after another).

The expectation is test_gpu_refine_adaptive.py's whole-frame plan, built from
the CPU oracle alone. A group, and the parts of a frame each driven on a
context of its own, must reproduce it bit for bit (NaN == NaN): the image, the
counts, the errors, the exported sums, the active count (and pending before
the call), every member's stats.samples against its own rows of the mask, and
the members' summed stats.segments. More than one RCCL rank and peer copies
have never run anywhere; nothing here claims they have."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_refine import stress_ctx  # noqa: F401
from test_gpu_refine_adaptive import (FIVE_OF_8, INF, assert_bits_equal, c1_inputs, check_shares, cost_at, dilate,
                                      plan, precompute_costs)

pytestmark = pytest.mark.gpu

RTX_ERR_INVALID, RTX_ERR_STATE = -1, -3


def halo_only(steps, i, T):
    """Pixels of step i that are active only through a noisy neighbour across
    a tile edge: active, but not when every tile dilates its own rows alone."""
    st = steps[i]
    assert i > 0
    err = steps[i - 1]["err"]
    with np.errstate(invalid="ignore"):
        noisy = err >= np.float32(st["thr"])
    inside = np.zeros_like(noisy)
    for y0 in range(0, noisy.shape[0], T):
        inside[y0:y0 + T] = dilate(noisy[y0:y0 + T])
    return st["mask"] & ~inside


def member_rows(rtx, H, T, n):
    return [rtx.part_row_ids(H, T, m, n) for m in range(n)]


def step_segments(ctx, key, st):
    m = st["mask"]
    cost = np.zeros(m.shape, np.int64)
    for n0 in np.unique(st["old"][m]) if m.any() else ():
        sel = m & (st["old"] == n0)
        cost[sel] = (cost_at(ctx, key, int(n0) + st["samples"]) - cost_at(ctx, key, int(n0)))[sel]
    return int(cost.sum())


def check_group_state(g, st, where):
    assert_bits_equal(g.download()[..., :3], st["image"][..., :3], f"{where}: image")
    assert (g.refine_counts() == st["counts"]).all(), f"{where}: counts"
    assert_bits_equal(g.refine_error(), st["err"], f"{where}: errors")
    assert_bits_equal(g.refine_export()[..., :3], st["sums"], f"{where}: chain sums")


def run_group_plan(g, cost_ctx, rtx, key, steps, T, what, reset_first=True, before=None):
    """The calls of a plan on a group, everything compared after each.
    cost_ctx: a context with the same world and frame, for debug_pixel_cost.
    before(i): called before call i (after pending)."""
    precompute_costs(cost_ctx, key, steps)
    n = len(g)
    H = g.frame.height
    rows = member_rows(rtx, H, T, n)
    for i, st in enumerate(steps):
        want = int(st["mask"].sum())
        first = i == 0 and reset_first
        where = f"{what}: call {i} ({st['samples']} samples, threshold {st['thr']!r}, cap {st['cap']}, {want} active)"
        if not first:
            assert g.refine_pending(st["samples"], st["thr"], st["cap"], tile_rows=T) == want, f"{where}: pending"
        if before:
            before(i)
        total = 0 if first else g.refined_samples
        member_n = [0 if first else g.ctx(m).refined_samples for m in range(n)]
        for m in range(n):
            g.ctx(m).stats_reset()
        got = g.refine_adaptive(st["samples"], st["thr"], st["cap"], tile_rows=T, reset=first)
        image = g.download()
        stats = [g.ctx(m).stats() for m in range(n)]
        assert got == want, f"{where}: active count {got}"
        own = [int(st["mask"][r].sum()) if len(r) else 0 for r in rows]
        assert [s.samples for s in stats] == [a * st["samples"] for a in own], f"{where}: members' stats.samples"
        assert [s.launches for s in stats] == [1 if a else 0 for a in own], f"{where}: members' launches"
        assert sum(s.segments for s in stats) == step_segments(cost_ctx, key, st), f"{where}: stats.segments"
        assert g.refined_samples == total + (st["samples"] if want else 0), where
        assert [g.ctx(m).refined_samples for m in range(n)] == \
            [member_n[m] + (st["samples"] if own[m] else 0) for m in range(n)], f"{where}: members' N"
        assert_bits_equal(image[..., :3], st["image"][..., :3], f"{where}: image")
        assert (image[..., 3] == 1.0).all(), f"{where}: w"
        check_group_state(g, st, where)


def a162(oracle, rtx, calls=FIVE_OF_8, start=0):
    world, frame = c1_inputs(rtx)
    return world, frame, plan(oracle, rtx, "a162", world, frame, calls, start=start)


def setup(target, world, frame):
    target.upload_world(world)
    target.set_frame(frame)


@pytest.mark.parametrize("devices,T", [([0, 0, 0], 4), ([0, 0], 1), ([0], 5)], ids=["3xT4", "2xT1", "direct"])
def test_five_steps(gpu_ctx, oracle, rtx, devices, T):
    """162 x 91, 486 spheres, five steps of 8: 23 tiles of 4 rows (the last
    ragged) on three members; tiles of one row on two (both halos of every row
    from the same neighbour); one member (the direct path)."""
    world, frame, steps = a162(oracle, rtx)
    assert steps[0]["mask"].all() and steps[1]["mask"].all()
    check_shares(steps, (2, 3, 4))
    n = len(devices)
    if n > 1:
        rows = member_rows(rtx, frame.height, T, n)
        for i in (2, 3, 4):
            k = int(halo_only(steps, i, T).sum())
            assert k > 0, f"inputs: step {i} has no pixel that is active only across a tile edge (T {T})"
            assert all(steps[i]["mask"][r].any() for r in rows), f"inputs: step {i}: an idle member"
    setup(gpu_ctx, world, frame)
    with rtx.Group(devices, "copy") as g:
        setup(g, world, frame)
        run_group_plan(g, gpu_ctx, rtx, "a162", steps, T, f"{devices} T {T}")


def test_mixed_steps(gpu_ctx, oracle, rtx):
    """Steps (3, 9, 12, 5, 8) on three members: mixed per-pixel counts and
    pixels that are re-activated."""
    calls = [(3, 0.0, 0), (9, 0.0, 0), (12, "q", 0), (5, "q", 0), (8, "q", 0)]
    world, frame, steps = a162(oracle, rtx, calls)
    check_shares(steps, (2, 3, 4))
    for i in (2, 3, 4):
        assert halo_only(steps, i, 4).any(), f"inputs: step {i}"
    assert len(np.unique(steps[-1]["counts"])) >= 3
    setup(gpu_ctx, world, frame)
    with rtx.Group([0, 0, 0], "copy") as g:
        setup(g, world, frame)
        run_group_plan(g, gpu_ctx, rtx, "a162", steps, 4, "mixed steps")


def test_a_member_without_rows(gpu_ctx, oracle, rtx):
    """160 x 20 in tiles of 8 for four members: three tiles (8, 8 and a ragged
    4 rows), so member 3 owns nothing."""
    W, H, T = 160, 20, 8
    world, _ = c1_inputs(rtx)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    assert [rtx.part_rows(H, T, m, 4) for m in range(4)] == [8, 8, 4, 0]
    steps = plan(oracle, rtx, "a160x20", world, frame, [(8, INF, 0), (8, INF, 0), (8, "q", 0), (8, "q", 0)])
    check_shares(steps, (2, 3))
    for i in (2, 3):
        assert halo_only(steps, i, T).any(), f"inputs: step {i}"
    setup(gpu_ctx, world, frame)
    with rtx.Group([0, 0, 0, 0], "copy") as g:
        setup(g, world, frame)
        run_group_plan(g, gpu_ctx, rtx, "a160x20", steps, T, "four members, three tiles")
        assert g.ctx(3).refined_samples == 0


def test_edges(gpu_ctx, oracle, rtx):
    """test_edges' calls on three members: a +inf threshold changes nothing and
    launches nothing anywhere; at the largest finite E as the threshold (at
    most 9 pixels, so at most 3 adjacent rows, so at most 2 of 3 members at
    T 4) some row-owning member traces nothing, launches nothing, and the image
    is still right everywhere; then the capped steps."""
    calls = [(8, INF, 0), (8, INF, 0), (8, INF, 0), (8, "max", 0), (8, "q", 24), (8, "q", 24), (8, "q", 32)]
    world, frame, steps = a162(oracle, rtx, calls)
    T = 4
    assert steps[2]["mask"].sum() == 0 and 1 <= steps[3]["mask"].sum() <= 9
    rows = member_rows(rtx, frame.height, T, 3)
    assert any(not steps[3]["mask"][r].any() for r in rows), "inputs: the 'max' step reaches every member"
    check_shares(steps, (4, 6))
    assert steps[5]["mask"].any() and steps[6]["mask"].any()
    setup(gpu_ctx, world, frame)
    with rtx.Group([0, 0, 0], "copy") as g:
        setup(g, world, frame)
        kept = {}

        def before(i):
            if i == 2:
                kept["image"] = g.download()
        run_group_plan(g, gpu_ctx, rtx, "a162", steps, T, "edges", before=before)
    # (run_group_plan compared call 2's image with the plan's, which is call 1's; and bit for bit with w:)
    assert_bits_equal(kept["image"][..., :3], steps[2]["image"][..., :3], "the +inf step changed nothing")


def test_a_plain_frame_in_between(gpu_ctx, oracle, rtx):
    """A plain group frame overwrites the members' row buffers and the image;
    the next selective step must still leave the plan's image at every pixel,
    so the pixels it does not trace are rewritten from the state."""
    world, frame, steps = a162(oracle, rtx)
    setup(gpu_ctx, world, frame)
    for devices, T in (([0, 0, 0], 4), ([0], 5)):
        with rtx.Group(devices, "copy") as g:
            setup(g, world, frame)

            def before(i):
                if i == 2:
                    plain = g.render_image(T)
                    assert not (plain[..., :3].view(np.uint32) == steps[1]["image"][..., :3].view(np.uint32)).all()
                    assert g.refined_samples == 16
            run_group_plan(g, gpu_ctx, rtx, "a162", steps[:3], T, f"{devices}: plain frame before call 2", before=before)


def test_transitions(gpu_ctx, oracle, rtx):
    """Group.refine 8 + 8, then adaptive (the first call traces everything);
    Group.refine on the non-uniform state is refused; export, import into
    another group shape, adaptive again; a member refined behind the group's
    back is refused by name."""
    world, frame = c1_inputs(rtx)
    W, H, T = frame.width, frame.height, 4
    after = plan(oracle, rtx, "a162", world, frame, [(8, INF, 0), (8, "q", 0), (8, "q", 0)], start=16)
    assert after[0]["mask"].all()
    check_shares(after, (1, 2))
    setup(gpu_ctx, world, frame)
    with rtx.Group([0, 0, 0], "copy") as g:
        lib = g._lib
        setup(g, world, frame)
        g.refine(8, tile_rows=T, reset=True)
        assert g.refine(8, tile_rows=T) == 16
        state16 = g.refine_export()
        assert (g.refine_counts() == 16).all() and np.isposinf(g.refine_error()).all()
        assert g.refine_pending(8, after[1]["thr"], tile_rows=T) == W * H
        assert g.refine_pending(8, after[1]["thr"], 23, tile_rows=T) == 0
        run_group_plan(g, gpu_ctx, rtx, "a162", after, T, "after refine 8 + 8", reset_first=False)
        # a non-uniform state: rtx_group_refine is refused and names the way on, nothing is launched
        for m in range(3):
            g.ctx(m).stats_reset()
        assert lib.rtx_group_refine(g._h, 8, T, 0) == RTX_ERR_STATE
        assert b"rtx_group_refine_adaptive" in lib.rtx_last_error()
        assert [g.ctx(m).stats().launches for m in range(3)] == [0, 0, 0] and g.refined_samples == 40
        check_group_state(g, after[2], "after the refused rtx_group_refine")
        # a member's own rtx_refine_rows on its non-uniform part state is refused too
        member = g.ctx(1)
        out = member.alloc((rtx.part_rows(H, T, 1, 3), W, 4))
        try:
            assert lib.rtx_refine_rows(member._h, T, 1, 3, 8, 0, C.c_void_p(out.ptr)) == RTX_ERR_STATE
            assert b"rtx_refine_adaptive" in lib.rtx_last_error()
            # ... and a restart of its own puts it out of step with the group
            n = C.c_uint32(0)
            assert member.refine_adaptive_rows(T, 1, 3, 8, 0.1, reset=True, d_out=out.ptr) == \
                rtx.part_rows(H, T, 1, 3) * W
        finally:
            out.free()
        for fn, rc in (("rtx_group_refine_adaptive", lib.rtx_group_refine_adaptive(g._h, 8, 0.1, 0, T, 0, C.byref(n))),
                       ("rtx_group_refine_pending", lib.rtx_group_refine_pending(g._h, 8, 0.1, 0, T, C.byref(n)))):
            assert rc == RTX_ERR_STATE, fn
        assert lib.rtx_group_refine_adaptive(g._h, 8, 0.1, 0, T, 0, C.byref(n)) == RTX_ERR_STATE
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_group_refine_adaptive: member 1:"), msg
    # the uniform state of 16 into a group of another shape, then adaptive: the plan from 16
    with rtx.Group([0, 0], "copy") as g2:
        setup(g2, world, frame)
        g2.refine_import(state16, 16, tile_rows=5)
        assert (g2.refine_counts() == 16).all() and np.isposinf(g2.refine_error()).all()
        run_group_plan(g2, gpu_ctx, rtx, "a162", after, 5, "imported into [0,0] T 5", reset_first=False)
        # the non-uniform state still exports its sums; an import is uniform again
        g2.refine_import(g2.refine_export(), 16, tile_rows=5)
        assert g2.refine(8, tile_rows=5) == 24


def drive_parts(ctxs, rtx, key, cost_ctx, steps, T, what):
    """Every part of a frame on a context of its own through
    rtx_refine_adaptive_rows, the halos moved by hand from the other parts'
    rtx_refine_edges (through the host), each part's rows against the plan."""
    n = len(ctxs)
    frame = ctxs[0].frame
    W, H = frame.width, frame.height
    rows = member_rows(rtx, H, T, n)
    tiles = [-(-len(r) // T) for r in rows]
    ntiles = -(-H // T)
    outs = [c.alloc((len(r), W, 4)) for c, r in zip(ctxs, rows)]
    edges = [c.alloc((2, t, W)) for c, t in zip(ctxs, tiles)]
    halos = [c.alloc((2, t, W)) for c, t in zip(ctxs, tiles)]
    precompute_costs(cost_ctx, key, steps)
    try:
        for i, st in enumerate(steps):
            first = i == 0
            if not first:
                # tile k's halo: the last err row of tile k - 1, the first of tile k + 1
                packed = []
                for c, e, t in zip(ctxs, edges, tiles):
                    c.refine_edges(e.ptr)
                    packed.append(e.numpy())  # (a copy is ordered on the context stream)
                for m, (c, h, t) in enumerate(zip(ctxs, halos, tiles)):
                    halo = np.full((2, t, W), np.nan, np.float32)
                    for j in range(t):
                        k = m + j * n
                        if k > 0:
                            halo[0, j] = packed[(k - 1) % n][1, (k - 1) // n]
                        if k + 1 < ntiles:
                            halo[1, j] = packed[(k + 1) % n][0, (k + 1) // n]
                    h.upload(halo)
            segs = 0
            for m, c in enumerate(ctxs):
                own = st["mask"][rows[m]]
                where = f"{what}: call {i}, part {m}"
                if not first:
                    assert c.refine_pending_rows(T, m, n, st["samples"], st["thr"], st["cap"], d_halo=halos[m].ptr) == \
                        own.sum(), f"{where}: pending"
                c.stats_reset()
                got = c.refine_adaptive_rows(T, m, n, st["samples"], st["thr"], st["cap"], reset=first,
                                             d_halo=0 if first else halos[m].ptr, d_out=outs[m].ptr)
                c.sync()
                stats = c.stats()
                assert got == own.sum() and stats.samples == own.sum() * st["samples"], where
                segs += stats.segments
                img = outs[m].numpy()
                assert_bits_equal(img[..., :3], st["image"][rows[m]][..., :3], f"{where}: rows")
                assert (c.refine_counts_rows() == st["counts"][rows[m]]).all(), f"{where}: counts"
                assert_bits_equal(c.refine_error_rows(), st["err"][rows[m]], f"{where}: errors")
                assert_bits_equal(c.refine_export()[..., :3], st["sums"][rows[m]], f"{where}: sums")
                assert c.refine_shape() == (T, m, n)
            assert segs == step_segments(cost_ctx, key, st), f"{what}: call {i}: segments"
    finally:
        for b in outs + edges + halos:
            b.free()


def test_parts_on_contexts(gpu_ctx, oracle, rtx):
    """Three parts of 160 x 90 at T 4, no group."""
    W, H, T = 160, 90, 4
    world, _ = c1_inputs(rtx)
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    steps = plan(oracle, rtx, "a160", world, frame, [(8, INF, 0), (8, INF, 0), (8, "q", 0), (8, "q", 0)])
    check_shares(steps, (2, 3))
    for i in (2, 3):
        assert halo_only(steps, i, T).any()
    setup(gpu_ctx, world, frame)
    ctxs = [rtx.Context(0) for _ in range(3)]
    try:
        for c in ctxs:
            setup(c, world, frame)
        drive_parts(ctxs, rtx, "a160", gpu_ctx, steps, T, "three contexts")
        # a part state: d_halo is needed now, and the whole-frame readers name the _rows ones
        lib, h = ctxs[0]._lib, ctxs[0]._h
        n = C.c_uint32(0)
        out = ctxs[0].alloc((rtx.part_rows(H, T, 0, 3), W, 4))
        try:
            assert lib.rtx_refine_adaptive_rows(h, T, 0, 3, 8, 0.1, 0, 0, None, C.c_void_p(out.ptr),
                                                C.byref(n)) == RTX_ERR_INVALID
            assert b"d_halo" in lib.rtx_last_error()
            assert lib.rtx_refine_pending_rows(h, T, 0, 3, 8, 0.1, 0, None, C.byref(n)) == RTX_ERR_INVALID
        finally:
            out.free()
        buf = np.empty((H, W), np.uint32)
        assert lib.rtx_refine_counts(h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), buf.nbytes) == RTX_ERR_STATE
        assert b"rtx_refine_counts_rows" in lib.rtx_last_error() and b"row part" in lib.rtx_last_error()
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("ctx_name", ["gpu_ctx", "stress_ctx"])
def test_large_scene_parts(request, oracle, rtx, ctx_name):
    """Above 1,024 spheres (the kPF instances) at 96 x 54, two parts at T 4 on
    two contexts of the same build (product and stress)."""
    ctx = request.getfixturevalue(ctx_name)
    world = rtx.random_world(20, depth=50, spp=60)
    assert world.count > 1024
    W, H, T = 96, 54, 4
    frame = rtx.camera_look_at(W, H, aspect=W / H)
    steps = plan(oracle, rtx, "abig96", world, frame, [(8, INF, 0), (8, INF, 0), (8, "q", 0)])
    check_shares(steps, (2,))
    assert halo_only(steps, 2, T).any()
    setup(ctx, world, frame)
    second = rtx.Context(0, lib=ctx._lib)
    try:
        setup(second, world, frame)
        drive_parts([ctx, second], rtx, "abig96", ctx, steps, T, f"{ctx_name} large scene")
    finally:
        second.close()


def test_group_refusals(rtx):
    """Decided before anything is launched: no world, depth 0, a per-sample
    frame, a null `active` for pending; the group stays as it was."""
    world, frame = c1_inputs(rtx)
    n = C.c_uint32(77)
    with rtx.Group([0, 0], "copy") as g:
        lib = g._lib
        g.set_frame(frame)
        assert lib.rtx_group_refine_adaptive(g._h, 8, 0.1, 0, 4, 0, C.byref(n)) == RTX_ERR_STATE  # no world
        g.upload_world(rtx.World(world.spheres, world.mat_types, world.mat_values, 0, 4))
        assert lib.rtx_group_refine_adaptive(g._h, 8, 0.1, 0, 4, 1, C.byref(n)) == RTX_ERR_INVALID
        msg = lib.rtx_last_error().decode()
        assert msg.startswith("rtx_group_refine_adaptive: member 0:") and "depth is 0" in msg, msg
        g.upload_world(world)
        for m in range(2):
            g.ctx(m).stats_reset()
        assert lib.rtx_group_refine_pending(g._h, 8, 0.1, 0, 4, None) == RTX_ERR_INVALID
        buf = np.zeros((frame.height, frame.width), np.uint32)
        assert lib.rtx_group_refine_counts(g._h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), buf.nbytes) == RTX_ERR_STATE
        ps = rtx.camera_look_at(frame.width, frame.height, aspect=frame.width / frame.height)
        ps.rng_mode = rtx.RNG_PER_SAMPLE
        g.set_frame(ps)
        assert lib.rtx_group_refine_adaptive(g._h, 8, 0.1, 0, 4, 0, C.byref(n)) == RTX_ERR_INVALID
        assert b"per-sample" in lib.rtx_last_error()
        assert n.value == 77 and g.refined_samples == 0
        assert [g.ctx(m).stats().launches for m in range(2)] == [0, 0]
        # a fresh group answers pending for a fresh state: every pixel
        g.set_frame(frame)
        assert g.refine_pending(8, 0.1, tile_rows=4) == frame.width * frame.height
        assert g.refine_adaptive(8, 0.1, tile_rows=4) == frame.width * frame.height
        assert lib.rtx_group_refine_counts(g._h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), buf.nbytes - 4) == \
            RTX_ERR_INVALID
        assert (g.refine_counts() == 8).all()
