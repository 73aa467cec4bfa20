"""Shared by test_gpu_refine_rows.py and test_gpu_group_refine.py: the scene, the
oracle's frames at each N (computed once per (frame, N) for the whole session
and never modified) and the bit-exact comparison."""
import numpy as np

DEPTH = 50
_WORLD = {}
_ORACLE = {}


def world_of(rtx, spp=4):
    """random_world(11), 486 spheres, depth 50 (spp: the plain render's only)."""
    if spp not in _WORLD:
        w = rtx.random_world(11, depth=DEPTH, spp=spp)
        assert w.count == 486
        _WORLD[spp] = w
    return _WORLD[spp]


def frame_of(rtx, W, H, **kw):
    return rtx.camera_look_at(W, H, aspect=W / H, **kw)


def oracle_at(oracle, rtx, frame, n):
    """(image, segments) of the oracle's full frame at spp = n."""
    k = (bytes(frame), n)
    if k not in _ORACLE:
        base = world_of(rtx)
        w = rtx.World(base.spheres, base.mat_types, base.mat_values, DEPTH, n)
        img, segs = oracle.render_rows(w, frame, np.arange(frame.height), nthreads=8)
        img.setflags(write=False)
        _ORACLE[k] = (img, segs)
    return _ORACLE[k]


def assert_bits_equal(a, b, what=""):
    """uint32 views equal, NaN == NaN."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    same = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    if not same.all():
        bad = np.argwhere(~same)
        raise AssertionError(f"{what}: {(~same).sum()} of {same.size} values differ; first at "
                             f"{bad[:5].tolist()}: got {a[tuple(bad[0])]} want {b[tuple(bad[0])]}")
