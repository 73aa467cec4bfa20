"""rtx — Python host binding of librtx.so (the MI355X path tracer's C-ABI).

Thin ctypes layer over ``include/rtx.h``; the compute path is the HIP kernel
in ``raytrace-we-gpu_amd/csrc``. There is deliberately no CPU fallback: if
``librtx.so`` is missing, importing the GPU entry points raises.

Host surface mirrors the reference app (CSVersion/DxCSApp.cpp):
  * :func:`random_world` / :func:`test_world`  ~ WorldDef::random_world /
    test_world (DxCSApp.cpp:72-157)
  * :func:`camera_look_at`                    ~ PerFrame::ComputeViewVals
    (DxCSApp.cpp:39-61) + focus distance (:488)
  * :class:`Context`                           ~ CDx11Base + DxCSApp resource
    lifetime (upload_world = WorldDef cbuffer, set_frame = PerFrame cbuffer,
    render_rows = Dispatch, DxCSApp.cpp:524)
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("RTX_LIB", os.path.join(_PKG_DIR, "lib", "librtx.so"))

RTX_OK = 0
RTX_ERR_INCOMPLETE = -5  # a render launch left pixels unwritten (ABI 1.3)
SCHEDULE_ABI = 140  # the rtx_schedule layout this module passes (ABI 1.4.0)
DEBUG_CULLED = 0xFFFFFFFF  # rtx_debug_hit_world_from: the culled scan (include/rtx.h RTX_DEBUG_CULLED)


def DEBUG_CULLED_COOP(q: int) -> int:
    """rtx_debug_hit_world_from: the culled group coop, q rays per wave (RTX_DEBUG_CULLED_COOP)."""
    if not 1 <= q <= 64:
        raise ValueError("q must be in 1..64")
    return 0xFFFFFF00 | q


def DEBUG_CULLED_COOP_LANE(q: int) -> int:
    """rtx_debug_hit_world_from: the culled group coop with the per-lane walk
    (the per-sample kernel's form), q rays per wave (RTX_DEBUG_CULLED_COOP_LANE)."""
    if not 1 <= q <= 64:
        raise ValueError("q must be in 1..64")
    return 0xFFFFFE00 | q
MAT_LAMBERT, MAT_METAL, MAT_DIELECTRIC = 0, 1, 2
RNG_CHAIN, RNG_PER_SAMPLE = 0, 1
SCAN_MODES = {"auto": 0, "linear": 1}  # rtx_set_scan_mode (RTX_SCAN_AUTO / RTX_SCAN_LINEAR)
FN = dict(sqrt=0, div=1, sin=2, cos=3, log2=4, exp2=5, pow=6, basehash=7,
          hash1=8, hash2=9, hash3=10, rius=11, lambert_dir=12, lambert_dir_guard=13)
FRAME_LAMBERT_GUARD = 1  # rtx_frame.flags bit (RTX_FRAME_LAMBERT_GUARD)
# rtx_refine_set_keys / rtx_refine_last_keys (RTX_REFINE_KEYS_*; "unscheduled": last_keys only)
REFINE_KEYS = {"prepass": 0, "carried": 1, "unscheduled": 2}
CAST_ORDERS = {"auto": 0, "given": 1, "coherent": 2}  # rtx_cast_rays (RTX_CAST_ORDER_*)
# rtx_ray / rtx_ray_hit (include/rtx.h), 32 bytes each; a ray is also a row of 8 float32 (o, t_max, d, tag)
RAY_DTYPE = np.dtype([("o", "<f4", (3,)), ("t_max", "<f4"), ("d", "<f4", (3,)), ("tag", "<u4")])
RAY_HIT_DTYPE = np.dtype([("t", "<f4"), ("index", "<i4"), ("normal", "<f4", (3,)), ("front_face", "<u4"),
                          ("reserved", "<u4", (2,))])
# rtx_path_query (32 bytes; also a row of 8 float32: o, seed, d, tag) / rtx_path_result (16 bytes: a float4)
PATH_QUERY_DTYPE = np.dtype([("o", "<f4", (3,)), ("seed", "<f4"), ("d", "<f4", (3,)), ("tag", "<u4")])
PATH_RESULT_DTYPE = np.dtype([("sum", "<f4", (3,)), ("seed", "<f4")])
PATHS_LAMBERT_GUARD, PATHS_CONTINUE = 1, 2  # rtx_trace_paths flags (RTX_PATHS_*)
PATHS_ORDER_COST = 3  # RTX_PATHS_ORDER_COST: rtx_paths_last_order after rtx_trace_paths_keyed sorted
FILM_QUERY_DTYPE = np.dtype([("o", "<f4", (3,)), ("seed", "<f4"), ("lower_left", "<f4", (3,)), ("tag", "<u4"),
                             ("horizontal", "<f4", (3,)), ("fx", "<f4"), ("vertical", "<f4", (3,)), ("fy", "<f4")])
FILM_LENS_QUERY_DTYPE = np.dtype([("q", FILM_QUERY_DTYPE), ("lens_u", "<f4", (3,)), ("lens_r", "<f4"),
                                  ("lens_v", "<f4", (3,)), ("reserved", "<u4")])
FILM_LENS = 4  # rtx_trace_film flag (RTX_FILM_LENS): 96-byte records
FILM_ORDERS = {"auto": 0, "given": 1, "coherent": 2, "cost": 3}  # rtx_trace_film's `order` ("coherent" is refused)
FILM_CAMERAS = {"equirect": 0, "fisheye": 1}  # rtx_film_camera (RTX_FILM_*)
GATHER_MODES = {"auto": 0, "rccl": 1, "copy": 2}  # rtx_group_create (RTX_GATHER_*)
GROUP_MAX = 64  # RTX_GROUP_MAX


class RtxError(RuntimeError):
    pass


class rtx_world(C.Structure):
    _fields_ = [("count", C.c_uint32), ("depth", C.c_uint32), ("spp", C.c_uint32),
                ("reserved", C.c_uint32), ("spheres", C.POINTER(C.c_float)),
                ("mat_types", C.POINTER(C.c_float)), ("mat_values", C.POINTER(C.c_float))]


class rtx_frame(C.Structure):
    _fields_ = [("origin", C.c_float * 4), ("horizontal", C.c_float * 4),
                ("vertical", C.c_float * 4), ("lower_left", C.c_float * 4),
                ("img_w", C.c_float), ("img_h", C.c_float), ("width", C.c_uint32),
                ("height", C.c_uint32), ("rng_mode", C.c_uint32), ("frame_index", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("lens_u", C.c_float * 4), ("lens_v", C.c_float * 4)]


class rtx_schedule(C.Structure):
    """The chain render's schedule (include/rtx.h rtx_schedule)."""
    _fields_ = [("tier1_bar", C.c_float), ("tier1_bar_small", C.c_float), ("tier1_bar_low", C.c_float),
                ("tier2_bar_small", C.c_float), ("tier2_bar_medium", C.c_float), ("tier2_bar", C.c_float),
                ("small_share", C.c_float),
                ("low_share", C.c_float), ("medium_share", C.c_float), ("hot_fraction", C.c_float),
                ("occupancy_small", C.c_float), ("occupancy_low", C.c_float), ("occupancy_normal", C.c_float),
                ("trace_small", C.c_float), ("trace_low", C.c_float), ("trace_medium", C.c_float),
                ("trace_large", C.c_float), ("promote_small", C.c_float), ("promote_low", C.c_float),
                ("promote_medium", C.c_float), ("promote_large", C.c_float), ("promote_big_scene", C.c_float),
                ("trace_solo_bar", C.c_float),
                ("tail_coop_max", C.c_uint32), ("tail_coop_max_large", C.c_uint32), ("tier1_priority", C.c_uint32), ("tier2_priority", C.c_uint32),
                ("hot_priority", C.c_uint32), ("refill_chunk", C.c_uint32), ("trace_group", C.c_uint32),
                ("prepass_cap_split", C.c_uint32), ("prio_bar1", C.c_float), ("prio_bar2", C.c_float),
                ("prio_bar3", C.c_float), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class rtx_stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("launches", C.c_uint64), ("samples", C.c_uint64),
                ("segments", C.c_uint64), ("sphere_tests", C.c_uint64)]


class rtx_scene_info(C.Structure):
    """What rtx_upload_world built (include/rtx.h rtx_scene_info)."""
    _fields_ = [("count", C.c_uint32), ("n_pad", C.c_uint32), ("kernels", C.c_uint32),
                ("sphere_copy_lds", C.c_uint32), ("layout", C.c_uint32), ("layout_positions", C.c_uint32),
                ("map_in_lds", C.c_uint32), ("flat_lo", C.c_uint32), ("flat_hi", C.c_uint32),
                ("grid", C.c_uint32), ("grid_nx", C.c_uint32), ("grid_nz", C.c_uint32),
                ("cull_positions", C.c_uint32), ("cull_flat_lo", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class rtx_hit(C.Structure):
    """What a pixel shows (include/rtx.h rtx_hit)."""
    _fields_ = [("hit", C.c_uint32), ("index", C.c_int32), ("front_face", C.c_uint32), ("material", C.c_uint32),
                ("t", C.c_float), ("depth", C.c_float), ("p", C.c_float * 3), ("normal", C.c_float * 3),
                ("albedo", C.c_float * 3), ("mat_param", C.c_float), ("reserved", C.c_uint32 * 2)]


_lib = None


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load librtx.so (raises RtxError if it was not built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RtxError(f"librtx.so not found at {p}: build it first (python -c "
                       "'import __graft_entry__ as g; g.build()' or make)")
    lib = C.CDLL(p)
    f, u32, i32, vp = C.POINTER(C.c_float), C.c_uint32, C.c_int32, C.c_void_p
    ctx = C.c_void_p
    sig = {
        "rtx_version": (C.c_int, []),
        "rtx_build_info": (C.c_char_p, []),
        "rtx_last_error": (C.c_char_p, []),
        "rtx_device_count": (C.c_int, [C.POINTER(C.c_int)]),
        "rtx_create": (C.c_int, [C.c_int, C.POINTER(ctx)]),
        "rtx_destroy": (None, [ctx]),
        "rtx_set_stream": (C.c_int, [ctx, vp]),
        "rtx_use_own_stream": (C.c_int, [ctx]),
        "rtx_upload_world": (C.c_int, [ctx, C.POINTER(rtx_world)]),
        "rtx_set_scan_mode": (C.c_int, [ctx, C.c_int]),
        "rtx_set_frame": (C.c_int, [ctx, C.POINTER(rtx_frame)]),
        "rtx_render_rows": (C.c_int, [ctx, u32, u32, u32, vp]),
        "rtx_render": (C.c_int, [ctx]),
        "rtx_accumulate": (C.c_int, [ctx, C.c_int]),
        "rtx_accumulated_frames": (u32, [ctx]),
        "rtx_render_sum": (C.c_int, [ctx, u32, vp]),
        "rtx_fold_frames": (C.c_int, [ctx, vp, vp, u32, C.c_size_t, C.c_size_t, u32, vp]),
        "rtx_refine": (C.c_int, [ctx, u32, C.c_int]),
        "rtx_refined_samples": (u32, [ctx]),
        "rtx_refine_state": (vp, [ctx]),
        "rtx_refine_export": (C.c_int, [ctx, f, C.c_size_t]),
        "rtx_refine_import": (C.c_int, [ctx, f, C.c_size_t, u32]),
        "rtx_refine_rows": (C.c_int, [ctx, u32, u32, u32, u32, C.c_int, vp]),
        "rtx_refine_import_rows": (C.c_int, [ctx, u32, u32, u32, f, C.c_size_t, u32, vp]),
        "rtx_refine_shape": (C.c_int, [ctx, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]),
        "rtx_refine_set_keys": (C.c_int, [ctx, C.c_int]),
        "rtx_refine_last_keys": (C.c_int, [ctx]),
        "rtx_refine_cost": (C.c_int, [ctx, C.POINTER(u32), C.c_size_t, C.POINTER(u32)]),
        "rtx_adaptive_error": (C.c_float, [f, u32, f, u32]),
        "rtx_refine_adaptive": (C.c_int, [ctx, u32, C.c_float, u32, C.c_int, C.POINTER(u32)]),
        "rtx_refine_pending": (C.c_int, [ctx, u32, C.c_float, u32, C.POINTER(u32)]),
        "rtx_refine_counts": (C.c_int, [ctx, C.POINTER(u32), C.c_size_t]),
        "rtx_refine_error": (C.c_int, [ctx, f, C.c_size_t]),
        "rtx_refine_adaptive_rows": (C.c_int, [ctx, u32, u32, u32, u32, C.c_float, u32, C.c_int, vp, vp,
                                               C.POINTER(u32)]),
        "rtx_refine_pending_rows": (C.c_int, [ctx, u32, u32, u32, u32, C.c_float, u32, vp, C.POINTER(u32)]),
        "rtx_refine_edges": (C.c_int, [ctx, vp]),
        "rtx_refine_counts_rows": (C.c_int, [ctx, C.POINTER(u32), C.c_size_t]),
        "rtx_refine_error_rows": (C.c_int, [ctx, f, C.c_size_t]),
        "rtx_features": (C.c_int, [ctx, vp, vp]),
        "rtx_features_rows": (C.c_int, [ctx, u32, u32, u32, vp, vp]),
        "rtx_pick": (C.c_int, [ctx, u32, u32, C.POINTER(rtx_hit)]),
        "rtx_mask_from_ids": (C.c_int, [ctx, vp, C.POINTER(u32), u32, u32, vp, C.POINTER(u32)]),
        "rtx_refine_masked": (C.c_int, [ctx, u32, vp, u32, C.POINTER(u32)]),
        "rtx_cast_rays": (C.c_int, [ctx, vp, u32, C.c_float, u32, vp, vp]),
        "rtx_cast_last_order": (C.c_int, [ctx]),
        "rtx_path_seed": (C.c_float, [u32, u32, u32]),
        "rtx_trace_paths": (C.c_int, [ctx, vp, u32, u32, u32, u32, vp, vp]),
        "rtx_paths_last_order": (C.c_int, [ctx]),
        "rtx_trace_paths_keyed": (C.c_int, [ctx, vp, u32, u32, u32, vp, u32, vp, vp]),
        "rtx_debug_paths_order": (C.c_int, [ctx, C.POINTER(u32), C.c_size_t]),
        "rtx_trace_film": (C.c_int, [ctx, vp, u32, u32, C.c_float, C.c_float, u32, u32, vp, vp]),
        "rtx_film_last_order": (C.c_int, [ctx]),
        "rtx_film_from_frame": (C.c_int, [C.POINTER(rtx_frame), C.POINTER(u32), C.POINTER(u32), u32, u32, vp, C.c_int,
                                          f, f]),
        "rtx_film_camera": (C.c_int, [C.c_int, f, f, f, C.c_float, u32, u32, u32, vp]),
        "rtx_camera_set_aperture": (C.c_int, [C.POINTER(rtx_frame), C.c_float]),
        "rtx_part_rows": (u32, [u32, u32, u32, u32]),
        "rtx_deinterleave_rows": (C.c_int, [ctx, vp, u32, u32, u32, u32, vp]),
        "rtx_sync": (C.c_int, [ctx]),
        "rtx_framebuffer": (vp, [ctx]),
        "rtx_download": (C.c_int, [ctx, f, C.c_size_t]),
        "rtx_alloc": (C.c_int, [ctx, C.c_size_t, C.POINTER(C.c_void_p)]),
        "rtx_free": (C.c_int, [ctx, vp]),
        "rtx_copy_to_host": (C.c_int, [ctx, vp, vp, C.c_size_t]),
        "rtx_copy_to_device": (C.c_int, [ctx, vp, vp, C.c_size_t]),
        "rtx_stats_reset": (C.c_int, [ctx]),
        "rtx_get_stats": (C.c_int, [ctx, C.POINTER(rtx_stats)]),
        "rtx_scene_random_world": (C.c_int, [i32, u32, f, f, f, C.POINTER(u32)]),
        "rtx_scene_test_world": (C.c_int, [f, f, f, C.POINTER(u32)]),
        "rtx_scene_ps_world": (C.c_int, [f, f, f, C.POINTER(u32)]),
        "rtx_camera_look_at": (C.c_int, [f, f, f, C.c_float, C.c_float, C.c_float, C.c_float,
                                         u32, u32, C.POINTER(rtx_frame)]),
        "rtx_camera_simple": (C.c_int, [u32, u32, C.POINTER(rtx_frame)]),
        "rtx_world_from_worlddef": (C.c_int, [vp, C.c_size_t, f, f, f, C.POINTER(rtx_world)]),
        "rtx_frame_from_perframe": (C.c_int, [vp, C.c_size_t, u32, u32, C.POINTER(rtx_frame)]),
        "rtx_schedule_defaults": (C.c_int, [C.POINTER(rtx_schedule)]),
        "rtx_set_schedule": (C.c_int, [ctx, C.POINTER(rtx_schedule)]),
        "rtx_get_schedule": (C.c_int, [ctx, C.POINTER(rtx_schedule)]),
        "rtx_debug_hit_world": (C.c_int, [ctx, f, u32, C.c_float, C.c_float, f]),
        "rtx_debug_hit_world_from": (C.c_int, [ctx, f, u32, C.c_float, C.c_float, u32, f]),
        "rtx_debug_math": (C.c_int, [ctx, C.c_int, f, f, u32, f]),
        "rtx_debug_wave_times": (C.c_int, [ctx, C.c_size_t, C.POINTER(C.c_uint64)]),
        "rtx_debug_pixel_cost": (C.c_int, [ctx, u32, C.POINTER(C.c_uint32)]),
        "rtx_debug_scan_rate": (C.c_int, [ctx, u32, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]),
        "rtx_debug_scene_info": (C.c_int, [ctx, C.POINTER(rtx_scene_info)]),
        "rtx_group_create": (C.c_int, [C.POINTER(C.c_int), u32, C.c_int, C.POINTER(C.c_void_p)]),
        "rtx_group_destroy": (None, [vp]),
        "rtx_group_size": (u32, [vp]),
        "rtx_group_ctx": (ctx, [vp, u32]),
        "rtx_group_gather_mode": (C.c_int, [vp]),
        "rtx_group_rccl_version": (C.c_int, [vp]),
        "rtx_group_upload_world": (C.c_int, [vp, C.POINTER(rtx_world)]),
        "rtx_group_set_frame": (C.c_int, [vp, C.POINTER(rtx_frame)]),
        "rtx_group_render": (C.c_int, [vp, u32]),
        "rtx_group_sync": (C.c_int, [vp]),
        "rtx_group_image": (vp, [vp]),
        "rtx_group_download": (C.c_int, [vp, f, C.c_size_t]),
        "rtx_group_get_times": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_double)]),
        "rtx_group_accumulate": (C.c_int, [vp, u32, C.c_int]),
        "rtx_group_accumulated_frames": (u32, [vp]),
        "rtx_group_get_accumulate_times": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                     C.POINTER(C.c_double)]),
        "rtx_group_refine": (C.c_int, [vp, u32, u32, C.c_int]),
        "rtx_group_refined_samples": (u32, [vp]),
        "rtx_group_refine_export": (C.c_int, [vp, f, C.c_size_t]),
        "rtx_group_refine_import": (C.c_int, [vp, u32, f, C.c_size_t, u32]),
        "rtx_group_refine_adaptive": (C.c_int, [vp, u32, C.c_float, u32, u32, C.c_int, C.POINTER(u32)]),
        "rtx_group_refine_pending": (C.c_int, [vp, u32, C.c_float, u32, u32, C.POINTER(u32)]),
        "rtx_group_refine_counts": (C.c_int, [vp, C.POINTER(u32), C.c_size_t]),
        "rtx_group_refine_error": (C.c_int, [vp, f, C.c_size_t]),
    }
    # entry points added after 1.0 may be absent from older builds (A/B runs
    # of earlier libraries); calling one then fails with AttributeError
    optional = {"rtx_schedule_defaults", "rtx_set_schedule", "rtx_get_schedule", "rtx_debug_hit_world_from",
                "rtx_build_info", "rtx_debug_scan_rate", "rtx_set_scan_mode", "rtx_debug_scene_info"}
    optional |= {n for n in sig if n.startswith("rtx_group_")}  # arrived without a version bump
    optional |= {"rtx_render_sum", "rtx_fold_frames"}            # ... with rtx_group_accumulate
    optional |= {n for n in sig if n.startswith("rtx_refine")}   # ... probe "rtx_refine"
    optional |= {"rtx_adaptive_error"}                           # ... with rtx_refine_adaptive
    optional |= {"rtx_features", "rtx_features_rows", "rtx_pick", "rtx_mask_from_ids"}  # ... probe "rtx_features"
    optional |= {"rtx_cast_rays", "rtx_cast_last_order"}         # ... probe "rtx_cast_rays"
    optional |= {"rtx_path_seed"}                                # ... probe "rtx_path_seed"
    optional |= {"rtx_trace_paths", "rtx_paths_last_order"}      # ... probe "rtx_trace_paths"
    optional |= {"rtx_trace_paths_keyed", "rtx_debug_paths_order"}  # ... probe "rtx_trace_paths_keyed"
    optional |= {"rtx_trace_film", "rtx_film_last_order", "rtx_film_from_frame", "rtx_film_camera"}  # ... "rtx_trace_film"
    for name, (res, args) in sig.items():
        if name in optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _dev_ptr(x) -> int:
    """The device address of a pointer, a DeviceArray (.ptr) or a torch tensor (.data_ptr()); None: 0."""
    if x is None:
        return 0
    if isinstance(x, (int, np.integer)):
        return int(x)
    if hasattr(x, "ptr"):
        return int(x.ptr)
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    raise TypeError(f"not a device buffer: {type(x).__name__}")


def path_seed(x: int, y: int, frame_index: int = 0) -> np.float32:
    """The chain seed of pixel (x, y) in frame frame_index (rtx_path_seed; host, no GPU): the seed
    with which a ray (o, d) sees what that pixel sees in the frame with origin o, lower_left o + d and
    zero horizontal and vertical rows."""
    lib = load_library()
    if not hasattr(lib, "rtx_path_seed"):
        raise RtxError("this librtx has no rtx_path_seed")
    return np.float32(lib.rtx_path_seed(x, y, frame_index))


def path_queries(o, d, seeds, tags=None) -> np.ndarray:
    """n PATH_QUERY_DTYPE records from origins and directions ((n, 3), or one (3,) for all) and seeds
    ((n,), e.g. path_seed(x, y, f) per query); tags: the caller's words, 0 when None."""
    seeds = np.ascontiguousarray(seeds, np.float32).reshape(-1)
    q = np.zeros(seeds.size, PATH_QUERY_DTYPE)
    q["o"] = np.asarray(o, np.float32)
    q["d"] = np.asarray(d, np.float32)
    q["seed"] = seeds
    if tags is not None:
        q["tag"] = np.asarray(tags, np.uint32)
    return q


def film_from_frame(frame: "rtx_frame", xs, ys, frame_index: int = 0, lens: Optional[bool] = None):
    """The film records of the listed pixels (xs[i], ys[i]) of a frame (rtx_film_from_frame; host, no
    GPU): (queries, img_w, img_h), to be traced with Context.trace_film(queries, samples, img_w,
    img_h). lens: True for FILM_LENS_QUERY_DTYPE records, False for FILM_QUERY_DTYPE (refused for a
    frame with a lens), None: whichever the frame needs."""
    lib = load_library()
    if not hasattr(lib, "rtx_film_from_frame"):
        raise RtxError("this librtx has no rtx_film_from_frame")
    xs = np.ascontiguousarray(xs, np.uint32).reshape(-1)
    ys = np.ascontiguousarray(ys, np.uint32).reshape(-1)
    if xs.size != ys.size:
        raise RtxError("film_from_frame: xs and ys differ in length")
    if lens is None:
        lens = frame.lens_u[3] > 0.0
    q = np.zeros(xs.size, FILM_LENS_QUERY_DTYPE if lens else FILM_QUERY_DTYPE)
    w, h = C.c_float(), C.c_float()
    u32p = C.POINTER(C.c_uint32)
    _check(lib.rtx_film_from_frame(C.byref(frame), xs.ctypes.data_as(u32p), ys.ctypes.data_as(u32p), xs.size,
                                   frame_index, q.ctypes.data, 1 if lens else 0, C.byref(w), C.byref(h)),
           "rtx_film_from_frame")
    return q, np.float32(w.value), np.float32(h.value)


def film_camera(model: str, width: int, height: int, look_from=(13.0, 2.0, 3.0), look_at=(0.0, 0.0, 0.0),
                vup=(0.0, 1.0, 0.0), fov_deg: float = 180.0, frame_index: int = 0) -> np.ndarray:
    """width * height unit-form FILM_QUERY_DTYPE records of an "equirect" or "fisheye" camera
    (rtx_film_camera; host, no GPU), record y * width + x, row 0 at the bottom: trace them with
    Context.trace_film(queries, samples, 2, 2)."""
    lib = load_library()
    if not hasattr(lib, "rtx_film_camera"):
        raise RtxError("this librtx has no rtx_film_camera")
    a = [np.ascontiguousarray(v, np.float32) for v in (look_from, look_at, vup)]
    q = np.zeros(int(width) * int(height), FILM_QUERY_DTYPE)
    _check(lib.rtx_film_camera(FILM_CAMERAS[model], _fptr(a[0]), _fptr(a[1]), _fptr(a[2]), fov_deg, width, height,
                               frame_index, q.ctypes.data), "rtx_film_camera")
    return q


def _check(rc: int, what: str, lib: Optional[C.CDLL] = None):
    if rc != RTX_OK:
        msg = (lib or load_library()).rtx_last_error().decode(errors="replace")
        raise RtxError(f"{what} failed ({rc}): {msg}")


# ---------------------------------------------------------------------------
# Scene / camera producers (host-side, no GPU)
# ---------------------------------------------------------------------------
@dataclass
class World:
    """Scene ~ WorldDef (DxCSApp.cpp:64-71): spheres [n,4] (center, radius),
    mat_types [n] (0 Lambert, 1 metal, 2 dielectric), mat_values [n,4]."""
    spheres: np.ndarray
    mat_types: np.ndarray
    mat_values: np.ndarray
    depth: int = 50
    spp: int = 60

    @property
    def count(self) -> int:
        return int(self.spheres.shape[0])

    def as_struct(self):
        self.spheres = np.ascontiguousarray(self.spheres, dtype=np.float32)
        self.mat_types = np.ascontiguousarray(self.mat_types, dtype=np.float32)
        self.mat_values = np.ascontiguousarray(self.mat_values, dtype=np.float32)
        w = rtx_world()
        w.count, w.depth, w.spp, w.reserved = self.count, self.depth, self.spp, 0
        w.spheres, w.mat_types, w.mat_values = (_fptr(self.spheres), _fptr(self.mat_types),
                                                _fptr(self.mat_values))
        return w


def random_world(grid_half_extent: int = 9, capacity: Optional[int] = None, depth: int = 50,
                 spp: int = 60) -> World:
    """WorldDef::random_world (DxCSApp.cpp:72-134). 9 -> 326 spheres (the
    reference scene), 11 -> 486 (RTIOW final scene), 159 -> 101,124."""
    cap = capacity if capacity is not None else 4 + (2 * grid_half_extent) ** 2
    sph = np.zeros((cap, 4), np.float32)
    mt = np.zeros(cap, np.float32)
    mv = np.zeros((cap, 4), np.float32)
    n = C.c_uint32()
    _check(load_library().rtx_scene_random_world(grid_half_extent, cap, _fptr(sph), _fptr(mt),
                                                 _fptr(mv), C.byref(n)), "rtx_scene_random_world")
    k = n.value
    return World(sph[:k].copy(), mt[:k].copy(), mv[:k].copy(), depth, spp)


def test_world(depth: int = 50, spp: int = 50) -> World:
    """WorldDef::test_world (DxCSApp.cpp:136-157)."""
    sph = np.zeros((4, 4), np.float32)
    mt = np.zeros(4, np.float32)
    mv = np.zeros((4, 4), np.float32)
    n = C.c_uint32()
    _check(load_library().rtx_scene_test_world(_fptr(sph), _fptr(mt), _fptr(mv), C.byref(n)),
           "rtx_scene_test_world")
    return World(sph, mt, mv, depth, spp)


def ps_world(depth: int = 25, spp: int = 1) -> World:
    """The pixel-shader prototype's 7-sphere scene (Shader_RT.fx:300-335);
    its defaults depth 25, 1 sample (Shader_RT.fx:392, 430)."""
    sph = np.zeros((7, 4), np.float32)
    mt = np.zeros(7, np.float32)
    mv = np.zeros((7, 4), np.float32)
    n = C.c_uint32()
    _check(load_library().rtx_scene_ps_world(_fptr(sph), _fptr(mt), _fptr(mv), C.byref(n)),
           "rtx_scene_ps_world")
    return World(sph, mt, mv, depth, spp)


def camera_look_at(width: int, height: int, look_from=(13.0, 2.0, 3.0), look_at=(0.0, 0.0, 0.0),
                   vup=(0.0, 1.0, 0.0), vfov: float = 20.0, aspect: float = 16.0 / 9.0,
                   aperture: float = 2.0, focus_dist: float = 0.0) -> rtx_frame:
    """PerFrame::ComputeViewVals with DxCSApp's defaults (DxCSApp.cpp:176-179)."""
    f = rtx_frame()
    a = [np.asarray(v, np.float32) for v in (look_from, look_at, vup)]
    _check(load_library().rtx_camera_look_at(_fptr(a[0]), _fptr(a[1]), _fptr(a[2]), vfov,
                                             np.float32(aspect), aperture, focus_dist, width,
                                             height, C.byref(f)), "rtx_camera_look_at")
    return f


def set_aperture(frame: rtx_frame, aperture: float) -> rtx_frame:
    """Thin-lens defocus: lens radius = aperture / 2."""
    _check(load_library().rtx_camera_set_aperture(C.byref(frame), aperture), "rtx_camera_set_aperture")
    return frame


def camera_simple(width: int, height: int) -> rtx_frame:
    """Camera(width, height) of the CPU library (Camera.h:9-21)."""
    f = rtx_frame()
    _check(load_library().rtx_camera_simple(width, height, C.byref(f)), "rtx_camera_simple")
    return f


def part_rows(height: int, tile_rows: int, part: int, nparts: int) -> int:
    return int(load_library().rtx_part_rows(height, tile_rows, part, nparts))


def part_row_ids(height: int, tile_rows: int, part: int, nparts: int) -> np.ndarray:
    """Global rows owned by `part` (interleaved tiles), ascending."""
    y = np.arange(height, dtype=np.int64)
    return y[(y // tile_rows) % nparts == part].astype(np.uint32)


def _require_schedule_abi(lib: C.CDLL):
    """rtx_schedule grew in 1.2.0 (promote_big_scene, refill_chunk), 1.3.0
    (trace_solo_bar, trace_group) and 1.4.0 (prio_bar1..3): a library of
    another major.minor (older or newer) would read this module's struct at
    the wrong offsets, so it must match exactly (patch levels may differ)."""
    v = int(lib.rtx_version())
    if v // 10 != SCHEDULE_ABI // 10 or not hasattr(lib, "rtx_set_schedule"):
        raise RtxError(f"library ABI {v} does not match the rtx_schedule layout {SCHEDULE_ABI} this binding "
                       "passes (major.minor must be equal)")


def schedule_defaults() -> rtx_schedule:
    """The library's default schedule (no GPU)."""
    lib = load_library()
    _require_schedule_abi(lib)
    sch = rtx_schedule()
    _check(lib.rtx_schedule_defaults(C.byref(sch)), "rtx_schedule_defaults")
    return sch


def build_info(lib: Optional[C.CDLL] = None) -> dict:
    """rtx_build_info of the loaded library: {"src_sha16": ..., "arch": ...}
    (empty for libraries older than ABI 1.3)."""
    lib = lib or load_library()
    if not hasattr(lib, "rtx_build_info"):
        return {}
    return dict(kv.split("=", 1) for kv in lib.rtx_build_info().decode().split())


def device_count() -> int:
    n = C.c_int(0)
    rc = load_library().rtx_device_count(C.byref(n))
    return n.value if rc == RTX_OK else 0


def adaptive_error(sum_old, n_old: int, sum_new, n_new: int, lib: Optional[C.CDLL] = None) -> float:
    """The error estimate E of a step that took a pixel from n_old to n_new
    samples, from its linear sums (x, y, z) before and after: the kernels' own
    fp32 arithmetic on the host, no GPU (rtx_adaptive_error)."""
    a = np.ascontiguousarray(sum_old, np.float32).reshape(3)
    b = np.ascontiguousarray(sum_new, np.float32).reshape(3)
    return float((lib or load_library()).rtx_adaptive_error(_fptr(a), n_old, _fptr(b), n_new))


# ---------------------------------------------------------------------------
# GPU context
# ---------------------------------------------------------------------------
class Context:
    """One HIP device's renderer (~ CDx11Base::Initialize .. Terminate)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None,
                 lib: Optional[C.CDLL] = None):
        self._lib = lib or load_library()
        h = C.c_void_p()
        _check(self._lib.rtx_create(device, C.byref(h)), "rtx_create", self._lib)
        self._h = h
        self.device = device
        self.frame: Optional[rtx_frame] = None
        self.world: Optional[World] = None
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rtx_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream: Optional[int]):
        """Launch on `stream` (a hipStream_t handle; 0 = HIP's null stream,
        i.e. torch's default stream); None = the context's own stream."""
        if stream is None:
            _check(self._lib.rtx_use_own_stream(self._h), "rtx_use_own_stream", self._lib)
        else:
            _check(self._lib.rtx_set_stream(self._h, C.c_void_p(stream)), "rtx_set_stream", self._lib)

    def set_scan_mode(self, mode: str):
        """"auto" (layer grid / culled scan) or "linear" (every block of every
        segment, Hittable_list order): rtx_set_scan_mode, applied by the next
        upload_world."""
        _check(self._lib.rtx_set_scan_mode(self._h, SCAN_MODES[mode]), "rtx_set_scan_mode", self._lib)

    def upload_world(self, world: World):
        w = world.as_struct()
        _check(self._lib.rtx_upload_world(self._h, C.byref(w)), "rtx_upload_world", self._lib)
        self.world = world

    def set_frame(self, frame: rtx_frame):
        _check(self._lib.rtx_set_frame(self._h, C.byref(frame)), "rtx_set_frame", self._lib)
        self.frame = frame

    def render_rows(self, tile_rows: int, part: int, nparts: int, d_out: Optional[int] = None):
        _check(self._lib.rtx_render_rows(self._h, tile_rows, part, nparts,
                                         C.c_void_p(d_out or 0)), "rtx_render_rows", self._lib)

    def render(self):
        _check(self._lib.rtx_render(self._h), "rtx_render", self._lib)

    def accumulate(self, reset: bool = False) -> int:
        """Progressive accumulation; returns frames accumulated."""
        _check(self._lib.rtx_accumulate(self._h, 1 if reset else 0), "rtx_accumulate", self._lib)
        return int(self._lib.rtx_accumulated_frames(self._h))

    def render_sum(self, frame_index: int, d_sum: int):
        """One frame's linear per-pixel sample sums (what accumulate() adds for
        its frame number frame_index) into d_sum, width*height float4 with
        w = 0; the context's own accumulation is untouched."""
        _check(self._lib.rtx_render_sum(self._h, frame_index, C.c_void_p(d_sum or 0)), "rtx_render_sum", self._lib)

    def fold_frames(self, d_accum: int, d_sums: int, m: int, slot_pixels: int, pixels: int, divisor: int,
                    d_image: int):
        """Ordered fold: d_accum[p].xyz += d_sums[k * slot_pixels + p].xyz for
        k = 0 .. m-1 in that order, d_image[p] = toGamma(d_accum[p] / divisor)."""
        _check(self._lib.rtx_fold_frames(self._h, C.c_void_p(d_accum or 0), C.c_void_p(d_sums or 0), m, slot_pixels,
                                         pixels, divisor, C.c_void_p(d_image or 0)), "rtx_fold_frames", self._lib)

    def refine(self, samples: int, reset: bool = False) -> int:
        """`samples` more samples of every pixel along the reference's own RNG
        chain (rtx_refine): the framebuffer is then, bit for bit, the plain
        render at spp = the samples refined so far, which it returns."""
        _check(self._lib.rtx_refine(self._h, samples, 1 if reset else 0), "rtx_refine", self._lib)
        return int(self._lib.rtx_refined_samples(self._h))

    @property
    def refined_samples(self) -> int:
        """Samples per pixel in the chain state (0: none)."""
        return int(self._lib.rtx_refined_samples(self._h))

    def refine_rows(self, tile_rows: int, part: int, nparts: int, samples: int, reset: bool = False,
                    d_out: Optional[int] = None) -> int:
        """refine() for the rows of `part` of `nparts` (render_rows' partition)
        into d_out (device pointer, rows * width float4; None: the framebuffer,
        nparts == 1 only). The chain state then covers those rows only. With
        samples and reset bound it has render_rows' signature, so a rank of
        rtx.dist.FrameGather passes it as its render_part (rtx_refine_rows).
        Returns the samples refined so far."""
        _check(self._lib.rtx_refine_rows(self._h, tile_rows, part, nparts, samples, 1 if reset else 0,
                                         C.c_void_p(d_out or 0)), "rtx_refine_rows", self._lib)
        return int(self._lib.rtx_refined_samples(self._h))

    def refine_import_rows(self, tile_rows: int, part: int, nparts: int, state: np.ndarray, samples: int,
                           d_out: Optional[int] = None):
        """refine_import() for a part: `state` is (rows, W, 4) in the part's row
        order; its image rows go to d_out (None with nparts > 1: no image)
        (rtx_refine_import_rows)."""
        state = np.ascontiguousarray(state, np.float32)
        _check(self._lib.rtx_refine_import_rows(self._h, tile_rows, part, nparts, _fptr(state), state.nbytes, samples,
                                                C.c_void_p(d_out or 0)), "rtx_refine_import_rows", self._lib)

    def refine_shape(self) -> tuple:
        """(tile_rows, part, nparts) of the chain state; the whole frame is
        (1, 0, 1). RtxError when there is no state (rtx_refine_shape)."""
        t, p, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(self._lib.rtx_refine_shape(self._h, C.byref(t), C.byref(p), C.byref(n)), "rtx_refine_shape", self._lib)
        return int(t.value), int(p.value), int(n.value)

    def _state_rows(self) -> int:
        """Rows of the chain state: the frame's, or a part state's own."""
        t, p, n = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        if hasattr(self._lib, "rtx_refine_shape") and \
                self._lib.rtx_refine_shape(self._h, C.byref(t), C.byref(p), C.byref(n)) == RTX_OK:
            return int(self._lib.rtx_part_rows(self.frame.height, t.value, p.value, n.value))
        return int(self.frame.height)

    def refine_export(self) -> np.ndarray:
        """The chain state, (H, W, 4) float32: xyz the pixel's linear sample
        sum, w its seed after its last sample (rtx_refine_export). A part
        state (refine_rows): (rows, W, 4) in the part's row order."""
        f = self.frame
        out = np.empty((self._state_rows(), f.width, 4), np.float32)
        _check(self._lib.rtx_refine_export(self._h, _fptr(out), out.nbytes), "rtx_refine_export", self._lib)
        return out

    def refine_import(self, state: np.ndarray, samples: int):
        """Install a chain state of `samples` samples per pixel for the current
        world and frame and write its image (rtx_refine_import); the next
        refine() continues from it."""
        state = np.ascontiguousarray(state, np.float32)
        _check(self._lib.rtx_refine_import(self._h, _fptr(state), state.nbytes, samples), "rtx_refine_import",
               self._lib)

    def set_refine_keys(self, mode: str):
        """What orders a scheduled refine launch's pixel queue: "prepass" (a
        cost pre-pass per launch, the default) or "carried" (the previous
        launch's cost map where it is valid, no pre-pass). Results are the
        same either way (rtx_refine_set_keys)."""
        if mode not in ("prepass", "carried"):
            raise ValueError(f"refine keys {mode!r}: 'prepass' or 'carried'")
        _check(self._lib.rtx_refine_set_keys(self._h, REFINE_KEYS[mode]), "rtx_refine_set_keys", self._lib)

    @property
    def refine_last_keys(self) -> str:
        """What the last refine launch was keyed by: "prepass", "carried" or
        "unscheduled" (rtx_refine_last_keys)."""
        k = int(self._lib.rtx_refine_last_keys(self._h))
        _check(min(k, 0), "rtx_refine_last_keys", self._lib)
        return {v: n for n, v in REFINE_KEYS.items()}[k]

    def refine_cost(self):
        """The last refine launch's cost map and the samples it covers:
        ((H, W) uint32 ray segments per pixel, samples) (rtx_refine_cost); a
        part state's map is (rows, W) in the part's row order."""
        f = self.frame
        out = np.empty((self._state_rows(), f.width), np.uint32)
        n = C.c_uint32(0)
        _check(self._lib.rtx_refine_cost(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.nbytes, C.byref(n)),
               "rtx_refine_cost", self._lib)
        return out, int(n.value)

    def refine_adaptive(self, samples: int, threshold: float, max_samples: int = 0, reset: bool = False) -> int:
        """Trace `samples` more samples of every pixel that is still noisy:
        one whose 3 x 3 neighbourhood holds an error estimate >= threshold and
        whose count stays within max_samples (0: no cap). Every other pixel
        keeps its state and its framebuffer value. Returns the number of
        pixels traced (rtx_refine_adaptive)."""
        n = C.c_uint32(0)
        _check(self._lib.rtx_refine_adaptive(self._h, samples, threshold, max_samples, 1 if reset else 0, C.byref(n)),
               "rtx_refine_adaptive", self._lib)
        return int(n.value)

    def refine_pending(self, samples: int, threshold: float, max_samples: int = 0) -> int:
        """The number of pixels refine_adaptive with these arguments would
        trace now; nothing is traced or changed (rtx_refine_pending)."""
        n = C.c_uint32(0)
        _check(self._lib.rtx_refine_pending(self._h, samples, threshold, max_samples, C.byref(n)),
               "rtx_refine_pending", self._lib)
        return int(n.value)

    def refine_counts(self) -> np.ndarray:
        """(H, W) uint32: the samples in every pixel's sum (rtx_refine_counts)."""
        f = self.frame
        out = np.empty((f.height, f.width), np.uint32)
        _check(self._lib.rtx_refine_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.nbytes),
               "rtx_refine_counts", self._lib)
        return out

    def refine_error(self) -> np.ndarray:
        """(H, W) float32: the error estimate of every pixel's last step
        (+inf: none yet) (rtx_refine_error)."""
        f = self.frame
        out = np.empty((f.height, f.width), np.float32)
        _check(self._lib.rtx_refine_error(self._h, _fptr(out), out.nbytes), "rtx_refine_error", self._lib)
        return out

    def refine_adaptive_rows(self, tile_rows: int, part: int, nparts: int, samples: int, threshold: float,
                             max_samples: int = 0, reset: bool = False, d_halo: int = 0, d_out: int = 0) -> int:
        """refine_adaptive() for the rows of `part` of `nparts`: the state and
        its maps cover the part's rows. d_halo: the neighbours' edge rows of
        err, [2][tiles][W] float32 on the device (0: one part, or a fresh or
        uniform state); d_out: device pointer for the part's rows, every one
        of them written by a call that traces anything. Returns the number of
        pixels traced (rtx_refine_adaptive_rows)."""
        n = C.c_uint32(0)
        _check(self._lib.rtx_refine_adaptive_rows(self._h, tile_rows, part, nparts, samples, threshold, max_samples,
                                                  1 if reset else 0, C.c_void_p(d_halo or 0), C.c_void_p(d_out or 0),
                                                  C.byref(n)), "rtx_refine_adaptive_rows", self._lib)
        return int(n.value)

    def refine_pending_rows(self, tile_rows: int, part: int, nparts: int, samples: int, threshold: float,
                            max_samples: int = 0, d_halo: int = 0) -> int:
        """The number of pixels refine_adaptive_rows with these arguments would
        trace now (rtx_refine_pending_rows)."""
        n = C.c_uint32(0)
        _check(self._lib.rtx_refine_pending_rows(self._h, tile_rows, part, nparts, samples, threshold, max_samples,
                                                 C.c_void_p(d_halo or 0), C.byref(n)), "rtx_refine_pending_rows",
               self._lib)
        return int(n.value)

    def refine_edges(self, d_edges: int):
        """The first and last err row of each of the state's tiles into
        d_edges, [2][tiles][W] float32 on the device, asynchronously: what the
        neighbouring parts take their halos from (rtx_refine_edges)."""
        _check(self._lib.rtx_refine_edges(self._h, C.c_void_p(d_edges or 0)), "rtx_refine_edges", self._lib)

    def _state_rows(self) -> int:
        t, p, n = self.refine_shape()
        return part_rows(self.frame.height, t, p, n)

    def refine_counts_rows(self) -> np.ndarray:
        """refine_counts() for a state of any shape: (rows, W) uint32 in the
        part's row order (rtx_refine_counts_rows)."""
        out = np.empty((self._state_rows(), self.frame.width), np.uint32)
        _check(self._lib.rtx_refine_counts_rows(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.nbytes),
               "rtx_refine_counts_rows", self._lib)
        return out

    def refine_error_rows(self) -> np.ndarray:
        """refine_error() for a state of any shape: (rows, W) float32
        (rtx_refine_error_rows)."""
        out = np.empty((self._state_rows(), self.frame.width), np.float32)
        _check(self._lib.rtx_refine_error_rows(self._h, _fptr(out), out.nbytes), "rtx_refine_error_rows", self._lib)
        return out

    def features_rows(self, tile_rows: int, part: int, nparts: int, d_geom: int = 0, d_surf: int = 0):
        """The first-hit feature planes of the rows of `part` of `nparts` into
        device buffers of rows x W float4 (0: that plane is skipped),
        asynchronously (rtx_features_rows)."""
        _check(self._lib.rtx_features_rows(self._h, tile_rows, part, nparts, C.c_void_p(d_geom or 0),
                                           C.c_void_p(d_surf or 0)), "rtx_features_rows", self._lib)

    def features(self):
        """(geom, surf), two (H, W, 4) float32 arrays, row 0 = bottom: the first
        hit of every pixel's centre ray. geom = (normal, depth), (0, 0, 0, +inf)
        on a miss; surf = (albedo, sphere index), (0, 0, 0, -1) on a miss
        (rtx_features)."""
        f = self.frame
        g, s = self.alloc((f.height, f.width, 4)), self.alloc((f.height, f.width, 4))
        try:
            _check(self._lib.rtx_features(self._h, C.c_void_p(g.ptr), C.c_void_p(s.ptr)), "rtx_features", self._lib)
            return g.numpy(), s.numpy()
        finally:
            g.free()
            s.free()

    def pick(self, x: int, y: int) -> dict:
        """What is under pixel (x, y), y from the bottom row: the planes' entry
        of that pixel plus p, t, the material code and its parameter
        (rtx_pick)."""
        h = rtx_hit()
        _check(self._lib.rtx_pick(self._h, x, y, C.byref(h)), "rtx_pick", self._lib)
        return dict(hit=bool(h.hit), index=int(h.index), front_face=bool(h.front_face), material=int(h.material),
                    t=np.float32(h.t), depth=np.float32(h.depth), p=np.array(h.p[:], np.float32),
                    normal=np.array(h.normal[:], np.float32), albedo=np.array(h.albedo[:], np.float32),
                    mat_param=np.float32(h.mat_param))

    def mask_from_ids(self, d_surf, ids, grow: int = 0):
        """The pixels within Chebyshev distance `grow` of one that shows a
        sphere of `ids`, from a whole-frame surf plane on the device (a
        DeviceArray or a pointer). Returns (mask, set): an (H, W) uint8
        DeviceArray and the number of set pixels (rtx_mask_from_ids)."""
        f = self.frame
        a = np.ascontiguousarray(ids, np.uint32).reshape(-1)
        mask = self.alloc((f.height, f.width), np.uint8)
        n = C.c_uint32(0)
        _check(self._lib.rtx_mask_from_ids(self._h, C.c_void_p(getattr(d_surf, "ptr", d_surf) or 0),
                                           a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size, grow, C.c_void_p(mask.ptr),
                                           C.byref(n)), "rtx_mask_from_ids", self._lib)
        return mask, int(n.value)

    def refine_masked(self, samples: int, d_mask, max_samples: int = 0) -> int:
        """Trace `samples` more samples of every pixel whose mask byte is set
        (a DeviceArray or a device pointer of H x W bytes) and whose count stays
        within max_samples (0: no cap); every other pixel keeps its state.
        Needs a whole-frame chain state. Returns the number of pixels traced
        (rtx_refine_masked)."""
        n = C.c_uint32(0)
        _check(self._lib.rtx_refine_masked(self._h, samples, C.c_void_p(getattr(d_mask, "ptr", d_mask) or 0),
                                           max_samples, C.byref(n)), "rtx_refine_masked", self._lib)
        return int(n.value)

    def cast(self, rays, t_min: float = 0.001, order: str = "auto", hits=True, occluded=False,
             n: Optional[int] = None):
        """What `rays` hit in the uploaded world, each over (t_min, its own
        t_max): rtx_cast_rays. Returns (hits, occluded), None for an output
        that was not asked for.

        rays: a numpy array — (n, 8) float32 rows (o, t_max, d, tag) or n
        RAY_DTYPE records — is uploaded, and numpy arrays come back (n
        RAY_HIT_DTYPE records, n uint8), after a wait. A device pointer, a
        DeviceArray or a torch tensor is used in place, asynchronously on the
        context's stream, and DeviceArrays come back (`n`: the number of rays,
        when the object has no shape). hits / occluded: True (allocate one),
        False (skip it), or the caller's device buffer, which is filled and
        returned as it is. order: "auto", "given" or "coherent" — a schedule,
        never a different record."""
        if isinstance(rays, np.ndarray):
            host = np.ascontiguousarray(rays)
            if host.dtype != RAY_DTYPE:
                host = np.ascontiguousarray(host, np.float32).reshape(-1, 8)
            n = host.shape[0]
            d_rays = self.alloc((max(n, 1),), RAY_DTYPE)
            try:
                if n:
                    _check(self._lib.rtx_copy_to_device(self._h, C.c_void_p(d_rays.ptr), host.ctypes.data, 32 * n),
                           "rtx_copy_to_device", self._lib)
                got = self.cast(d_rays, t_min, order, hits, occluded, n)
                out = []
                for g, dt, asked in ((got[0], RAY_HIT_DTYPE, hits), (got[1], np.uint8, occluded)):
                    if g is None:
                        out.append(None)
                    elif asked is True:
                        out.append(g.numpy()[:n])
                        g.free()
                    else:
                        out.append(g)
                return tuple(out)
            finally:
                d_rays.free()
        if n is None:
            if not hasattr(rays, "shape"):
                raise RtxError("Context.cast: n is needed with a bare pointer")
            n = int(rays.shape[0])
        d_hits = self.alloc((max(n, 1),), RAY_HIT_DTYPE) if hits is True else (None if hits is False else hits)
        d_occ = self.alloc((max(n, 1),), np.uint8) if occluded is True else (None if occluded is False else occluded)
        _check(self._lib.rtx_cast_rays(self._h, C.c_void_p(_dev_ptr(rays)), n, t_min, CAST_ORDERS[order],
                                       C.c_void_p(_dev_ptr(d_hits)), C.c_void_p(_dev_ptr(d_occ))),
               "rtx_cast_rays", self._lib)
        return d_hits, d_occ

    def cast_last_order(self) -> str:
        """"given" or "coherent": what the last cast ran ("auto" resolved) (rtx_cast_last_order)."""
        code = self._lib.rtx_cast_last_order(self._h)
        for name, v in CAST_ORDERS.items():
            if v == code:
                return name
        raise RtxError(f"rtx_cast_last_order returned {code}")

    def trace_paths(self, queries, samples: int, flags: int = 0, order: str = "auto", results=None,
                    segments=False, cont: bool = False, n: Optional[int] = None):
        """What the rays of `queries` see: `samples` path-traced samples each,
        along the RNG chain from the query's seed, to the world's depth
        (rtx_trace_paths). Returns (results, segments), segments None when not
        asked for.

        queries: a numpy array — (n, 8) float32 rows (o, seed, d, tag) or n
        PATH_QUERY_DTYPE records (path_queries) — is uploaded, and numpy arrays
        come back (n PATH_RESULT_DTYPE records, n uint32), after a wait. A
        device pointer, a DeviceArray or a torch tensor is used in place,
        asynchronously on the context's stream, and the device buffers come
        back (`n`: the number of queries, when the object has no shape).
        results: None (allocate one), or the caller's buffer, which is filled
        and returned as it is; with numpy queries, a numpy array of n records
        (or (n, 4) float32) to continue from. segments: True (allocate one),
        False (none), or the caller's device buffer. cont: continue from what
        `results` holds (RTX_PATHS_CONTINUE; also as a bit of `flags`). order:
        "auto", "given" or "coherent" — a schedule, never a different
        record."""
        flags = int(flags) | (PATHS_CONTINUE if cont else 0)
        if not hasattr(self._lib, "rtx_trace_paths"):
            raise RtxError("this librtx has no rtx_trace_paths")
        if isinstance(queries, np.ndarray):
            host = np.ascontiguousarray(queries)
            if host.dtype != PATH_QUERY_DTYPE:
                host = np.ascontiguousarray(host, np.float32).reshape(-1, 8)
            n = host.shape[0]
            start = None
            if flags & PATHS_CONTINUE:
                if not isinstance(results, np.ndarray):
                    raise RtxError("Context.trace_paths: continuing numpy queries needs numpy results")
                start = np.ascontiguousarray(results)
                if start.dtype != PATH_RESULT_DTYPE:
                    start = np.ascontiguousarray(start, np.float32).reshape(-1, 4)
                if start.shape[0] != n:
                    raise RtxError("Context.trace_paths: results and queries differ in length")
            elif results is not None:
                raise RtxError("Context.trace_paths: numpy queries take results only to continue from")
            d_q = self.alloc((max(n, 1),), PATH_QUERY_DTYPE)
            d_r = self.alloc((max(n, 1),), PATH_RESULT_DTYPE)
            d_s = self.alloc((max(n, 1),), np.uint32) if segments is True else None
            try:
                if n:
                    _check(self._lib.rtx_copy_to_device(self._h, C.c_void_p(d_q.ptr), host.ctypes.data, 32 * n),
                           "rtx_copy_to_device", self._lib)
                    if start is not None:
                        _check(self._lib.rtx_copy_to_device(self._h, C.c_void_p(d_r.ptr), start.ctypes.data, 16 * n),
                               "rtx_copy_to_device", self._lib)
                self.trace_paths(d_q, samples, flags, order, d_r, d_s if d_s is not None else segments, False, n)
                return d_r.numpy()[:n], (d_s.numpy()[:n] if d_s is not None else (None if segments is False else segments))
            finally:
                d_q.free()
                d_r.free()
                if d_s is not None:
                    d_s.free()
        if n is None:
            if not hasattr(queries, "shape"):
                raise RtxError("Context.trace_paths: n is needed with a bare pointer")
            n = int(queries.shape[0])
        if results is None:
            if flags & PATHS_CONTINUE:
                raise RtxError("Context.trace_paths: continuing needs the results to continue from")
            results = self.alloc((max(n, 1),), PATH_RESULT_DTYPE)
        d_seg = self.alloc((max(n, 1),), np.uint32) if segments is True else (None if segments is False else segments)
        _check(self._lib.rtx_trace_paths(self._h, C.c_void_p(_dev_ptr(queries)), n, samples, flags, CAST_ORDERS[order],
                                         C.c_void_p(_dev_ptr(results)), C.c_void_p(_dev_ptr(d_seg))),
               "rtx_trace_paths", self._lib)
        return results, d_seg

    def trace_film(self, queries, samples: int, img_w: float, img_h: float, flags: int = 0, order: str = "auto",
                   results=None, segments=None, n: Optional[int] = None, cont: bool = False,
                   lens: Optional[bool] = None):
        """Path queries with a per-sample film footprint (rtx_trace_film): query
        i is a pixel (fx, fy) of the frame its record states, `samples`
        jittered samples each. Returns (results, segments), segments None when
        not asked for.

        queries: a numpy array — n FILM_QUERY_DTYPE or FILM_LENS_QUERY_DTYPE
        records (film_from_frame, film_camera), or (n, 16) / (n, 24) float32
        rows — is uploaded, and numpy arrays come back (n PATH_RESULT_DTYPE
        records, n uint32), after a wait. A device pointer, a DeviceArray or a
        torch tensor is used in place, asynchronously on the context's stream,
        and the device buffers come back (`n`: the number of queries, when the
        object has no shape). lens: whether the records are the 96-byte ones
        (RTX_FILM_LENS; also as a bit of `flags`); None: what a numpy array's
        dtype or row length says, and False for a device buffer. results,
        segments (True / None or False / a device buffer), cont: as in
        trace_paths. order: "auto", "given" or "cost" — a schedule, never a
        different record."""
        flags = int(flags) | (PATHS_CONTINUE if cont else 0)
        if not hasattr(self._lib, "rtx_trace_film"):
            raise RtxError("this librtx has no rtx_trace_film")
        if segments is None:
            segments = False
        if isinstance(queries, np.ndarray):
            host = np.ascontiguousarray(queries)
            if host.dtype == FILM_LENS_QUERY_DTYPE:
                rec_lens = True
            elif host.dtype == FILM_QUERY_DTYPE:
                rec_lens = False
            else:
                if host.ndim != 2 or host.shape[1] not in (16, 24):
                    raise RtxError("Context.trace_film: float rows are (n, 16) or (n, 24)")
                rec_lens = host.shape[1] == 24
                host = np.ascontiguousarray(host, np.float32)
            if (lens is not None and bool(lens) != rec_lens) or ((flags & FILM_LENS) and not rec_lens):
                raise RtxError("Context.trace_film: lens does not match the records")
            flags |= FILM_LENS if rec_lens else 0
            dt = FILM_LENS_QUERY_DTYPE if rec_lens else FILM_QUERY_DTYPE
            n = host.shape[0]
            start = None
            if flags & PATHS_CONTINUE:
                if not isinstance(results, np.ndarray):
                    raise RtxError("Context.trace_film: continuing numpy queries needs numpy results")
                start = np.ascontiguousarray(results)
                if start.dtype != PATH_RESULT_DTYPE:
                    start = np.ascontiguousarray(start, np.float32).reshape(-1, 4)
                if start.shape[0] != n:
                    raise RtxError("Context.trace_film: results and queries differ in length")
            elif results is not None:
                raise RtxError("Context.trace_film: numpy queries take results only to continue from")
            d_q = self.alloc((max(n, 1),), dt)
            d_r = self.alloc((max(n, 1),), PATH_RESULT_DTYPE)
            d_s = self.alloc((max(n, 1),), np.uint32) if segments is True else None
            try:
                if n:
                    _check(self._lib.rtx_copy_to_device(self._h, C.c_void_p(d_q.ptr), host.ctypes.data,
                                                        dt.itemsize * n), "rtx_copy_to_device", self._lib)
                    if start is not None:
                        _check(self._lib.rtx_copy_to_device(self._h, C.c_void_p(d_r.ptr), start.ctypes.data, 16 * n),
                               "rtx_copy_to_device", self._lib)
                self.trace_film(d_q, samples, img_w, img_h, flags, order, d_r,
                                d_s if d_s is not None else segments, n)
                return d_r.numpy()[:n], (d_s.numpy()[:n] if d_s is not None else (None if segments is False else segments))
            finally:
                d_q.free()
                d_r.free()
                if d_s is not None:
                    d_s.free()
        if lens:
            flags |= FILM_LENS
        elif lens is not None and (flags & FILM_LENS):
            raise RtxError("Context.trace_film: lens does not match the flags")
        if n is None:
            if not hasattr(queries, "shape"):
                raise RtxError("Context.trace_film: n is needed with a bare pointer")
            n = int(queries.shape[0])
        if results is None:
            if flags & PATHS_CONTINUE:
                raise RtxError("Context.trace_film: continuing needs the results to continue from")
            results = self.alloc((max(n, 1),), PATH_RESULT_DTYPE)
        d_seg = self.alloc((max(n, 1),), np.uint32) if segments is True else (None if segments is False else segments)
        _check(self._lib.rtx_trace_film(self._h, C.c_void_p(_dev_ptr(queries)), n, samples, np.float32(img_w),
                                        np.float32(img_h), flags, FILM_ORDERS[order], C.c_void_p(_dev_ptr(results)),
                                        C.c_void_p(_dev_ptr(d_seg))), "rtx_trace_film", self._lib)
        return results, d_seg

    def film_last_order(self) -> str:
        """"given" or "cost": what the last trace_film ran (rtx_film_last_order)."""
        code = self._lib.rtx_film_last_order(self._h)
        for name in ("given", "cost"):
            if FILM_ORDERS[name] == code:
                return name
        raise RtxError(f"rtx_film_last_order returned {code}")

    def film_image(self, results, samples: int, width: int, height: int) -> np.ndarray:
        """The image of a film batch: (height, width, 4) float32, toGamma(sum /
        samples) per record and alpha 1, record y * width + x (rtx_fold_frames
        on a zeroed accumulator; a wait). results: width * height
        PATH_RESULT_DTYPE records, numpy or a device buffer."""
        npix = int(width) * int(height)
        own = None
        if isinstance(results, np.ndarray):
            host = np.ascontiguousarray(results)
            if host.dtype != PATH_RESULT_DTYPE:
                host = np.ascontiguousarray(host, np.float32).reshape(-1, 4)
            if host.shape[0] != npix:
                raise RtxError("Context.film_image: results are not width * height records")
            own = self.alloc((npix,), PATH_RESULT_DTYPE)
            _check(self._lib.rtx_copy_to_device(self._h, C.c_void_p(own.ptr), host.ctypes.data, 16 * npix),
                   "rtx_copy_to_device", self._lib)
            results = own
        acc = self.alloc((npix, 4), np.float32)
        img = self.alloc((npix, 4), np.float32)
        try:
            acc.upload(np.zeros((npix, 4), np.float32))
            self.fold_frames(acc.ptr, _dev_ptr(results), 1, npix, npix, samples, img.ptr)
            return img.numpy().reshape(height, width, 4)
        finally:
            acc.free()
            img.free()
            if own is not None:
                own.free()

    def paths_last_order(self) -> str:
        """"given" or "coherent": what the last trace_paths ran; "cost" after a
        trace_paths_keyed that sorted (rtx_paths_last_order)."""
        code = self._lib.rtx_paths_last_order(self._h)
        if code == PATHS_ORDER_COST:
            return "cost"
        for name, v in CAST_ORDERS.items():
            if v == code:
                return name
        raise RtxError(f"rtx_paths_last_order returned {code}")

    def trace_paths_keyed(self, queries, samples: int, keys=None, probe: int = 0, flags: int = 0, results=None,
                          segments=False, cont: bool = False, n: Optional[int] = None):
        """trace_paths in cost order, the longest queries first
        (rtx_trace_paths_keyed): the records are trace_paths(order="given")'s,
        bit for bit; only the schedule differs. Returns (results, segments).

        keys: None — the library probes (`probe` samples in the given order,
        0: its default; their segment counts are the keys) — or n uint32, one
        per query, larger for longer (`probe` must then be 0). With numpy
        queries keys is a numpy array; with device queries a device buffer,
        which may be the `segments` buffer itself (the keys are read before
        the trace writes it). queries, results, segments, cont, n: as
        trace_paths takes them."""
        flags = int(flags) | (PATHS_CONTINUE if cont else 0)
        if not hasattr(self._lib, "rtx_trace_paths_keyed"):
            raise RtxError("this librtx has no rtx_trace_paths_keyed")
        if isinstance(queries, np.ndarray):
            host = np.ascontiguousarray(queries)
            if host.dtype != PATH_QUERY_DTYPE:
                host = np.ascontiguousarray(host, np.float32).reshape(-1, 8)
            n = host.shape[0]
            start = None
            if flags & PATHS_CONTINUE:
                if not isinstance(results, np.ndarray):
                    raise RtxError("Context.trace_paths_keyed: continuing numpy queries needs numpy results")
                start = np.ascontiguousarray(results)
                if start.dtype != PATH_RESULT_DTYPE:
                    start = np.ascontiguousarray(start, np.float32).reshape(-1, 4)
                if start.shape[0] != n:
                    raise RtxError("Context.trace_paths_keyed: results and queries differ in length")
            elif results is not None:
                raise RtxError("Context.trace_paths_keyed: numpy queries take results only to continue from")
            host_keys = None
            if keys is not None:
                if not isinstance(keys, np.ndarray):
                    raise RtxError("Context.trace_paths_keyed: numpy queries take numpy keys")
                host_keys = np.ascontiguousarray(keys, np.uint32).reshape(-1)
                if host_keys.shape[0] != n:
                    raise RtxError("Context.trace_paths_keyed: keys and queries differ in length")
            d_q = self.alloc((max(n, 1),), PATH_QUERY_DTYPE)
            d_r = self.alloc((max(n, 1),), PATH_RESULT_DTYPE)
            d_s = self.alloc((max(n, 1),), np.uint32) if segments is True else None
            d_k = self.alloc((max(n, 1),), np.uint32) if host_keys is not None else None
            try:
                if n:
                    for d, h, size in ((d_q, host, 32), (d_r, start, 16), (d_k, host_keys, 4)):
                        if h is not None:
                            _check(self._lib.rtx_copy_to_device(self._h, C.c_void_p(d.ptr), h.ctypes.data, size * n),
                                   "rtx_copy_to_device", self._lib)
                self.trace_paths_keyed(d_q, samples, d_k, probe, flags, d_r, d_s if d_s is not None else segments,
                                       False, n)
                return d_r.numpy()[:n], (d_s.numpy()[:n] if d_s is not None else (None if segments is False else segments))
            finally:
                for d in (d_q, d_r, d_s, d_k):
                    if d is not None:
                        d.free()
        if n is None:
            if not hasattr(queries, "shape"):
                raise RtxError("Context.trace_paths_keyed: n is needed with a bare pointer")
            n = int(queries.shape[0])
        if results is None:
            if flags & PATHS_CONTINUE:
                raise RtxError("Context.trace_paths_keyed: continuing needs the results to continue from")
            results = self.alloc((max(n, 1),), PATH_RESULT_DTYPE)
        d_seg = self.alloc((max(n, 1),), np.uint32) if segments is True else (None if segments is False else segments)
        _check(self._lib.rtx_trace_paths_keyed(self._h, C.c_void_p(_dev_ptr(queries)), n, samples, flags,
                                               C.c_void_p(_dev_ptr(keys)), probe, C.c_void_p(_dev_ptr(results)),
                                               C.c_void_p(_dev_ptr(d_seg))),
               "rtx_trace_paths_keyed", self._lib)
        self._paths_keyed_n = n
        return results, d_seg

    def paths_order(self, n: Optional[int] = None) -> np.ndarray:
        """The permutation the last trace_paths_keyed ran, one uint32 per
        query: lane g took query perm[g] (rtx_debug_paths_order; a wait). n:
        that call's number of queries (None: what this object's last
        trace_paths_keyed had). RtxError (RTX_ERR_STATE, -3) when the last
        path call did not sort by cost or the scratch has been reused since."""
        perm = np.empty(int(getattr(self, "_paths_keyed_n", 0) if n is None else n), np.uint32)
        _check(self._lib.rtx_debug_paths_order(self._h, perm.ctypes.data_as(C.POINTER(C.c_uint32)), perm.nbytes),
               "rtx_debug_paths_order", self._lib)
        return perm

    def deinterleave(self, d_gathered: int, width: int, height: int, tile_rows: int, nparts: int,
                     d_image: int):
        _check(self._lib.rtx_deinterleave_rows(self._h, C.c_void_p(d_gathered), width, height,
                                               tile_rows, nparts, C.c_void_p(d_image)),
               "rtx_deinterleave_rows", self._lib)

    def sync(self):
        _check(self._lib.rtx_sync(self._h), "rtx_sync", self._lib)

    def framebuffer_ptr(self) -> int:
        return int(self._lib.rtx_framebuffer(self._h) or 0)

    def download(self) -> np.ndarray:
        f = self.frame
        out = np.empty((f.height, f.width, 4), np.float32)
        _check(self._lib.rtx_download(self._h, _fptr(out), out.nbytes), "rtx_download", self._lib)
        return out

    def render_image(self) -> np.ndarray:
        self.render()
        return self.download()

    def alloc(self, shape, dtype=np.float32) -> "DeviceArray":
        return DeviceArray(self, shape, dtype)

    def stats_reset(self):
        _check(self._lib.rtx_stats_reset(self._h), "rtx_stats_reset", self._lib)

    def stats(self) -> rtx_stats:
        s = rtx_stats()
        _check(self._lib.rtx_get_stats(self._h, C.byref(s)), "rtx_get_stats", self._lib)
        return s

    def set_schedule(self, schedule: Optional[rtx_schedule] = None, **fields):
        """Install a schedule (rtx_set_schedule): `schedule`, or the current
        one with `fields` replaced; no arguments = the defaults."""
        _require_schedule_abi(self._lib)
        if schedule is None and not fields:
            _check(self._lib.rtx_set_schedule(self._h, None), "rtx_set_schedule", self._lib)
            return
        sch = schedule if schedule is not None else self.get_schedule()
        for k, v in fields.items():
            if k not in dict(rtx_schedule._fields_):
                raise RtxError(f"unknown schedule field {k}")
            setattr(sch, k, v)
        _check(self._lib.rtx_set_schedule(self._h, C.byref(sch)), "rtx_set_schedule", self._lib)

    def get_schedule(self) -> rtx_schedule:
        _require_schedule_abi(self._lib)
        sch = rtx_schedule()
        _check(self._lib.rtx_get_schedule(self._h, C.byref(sch)), "rtx_get_schedule", self._lib)
        return sch

    def debug_hit_world(self, rays: np.ndarray, t_min: float = 0.001,
                        t_max: float = float("inf"), start_block: Optional[int] = None) -> np.ndarray:
        """hit_world on the GPU (rtx_debug_hit_world); start_block: the scan
        starts at that 8-sphere block and wraps round (rtx_debug_hit_world_from);
        DEBUG_CULLED: the culled scan (worlds of more than 1,024 spheres)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((rays.shape[0], 10), np.float32)
        if start_block is None:
            _check(self._lib.rtx_debug_hit_world(self._h, _fptr(rays), rays.shape[0], t_min, t_max,
                                                 _fptr(out)), "rtx_debug_hit_world", self._lib)
        else:
            _check(self._lib.rtx_debug_hit_world_from(self._h, _fptr(rays), rays.shape[0], t_min, t_max,
                                                      start_block, _fptr(out)), "rtx_debug_hit_world_from",
                   self._lib)
        return out

    def scene_info(self) -> dict:
        """What upload_world built and which path the launches take for it
        (rtx_debug_scene_info): count, n_pad, kernels (0 small, 1 large culled,
        2 large linear), sphere_copy_lds, layout, layout_positions, map_in_lds,
        flat_lo, flat_hi, grid, grid_nx, grid_nz, and the culled layout's
        cull_positions and cull_flat_lo (0 unless kernels == 1). Nothing is launched."""
        info = rtx_scene_info()
        _check(self._lib.rtx_debug_scene_info(self._h, C.byref(info)), "rtx_debug_scene_info", self._lib)
        return {name: int(getattr(info, name)) for name, _ in rtx_scene_info._fields_ if name != "reserved"}

    def arm_wave_times(self, max_waves: int):
        _check(self._lib.rtx_debug_wave_times(self._h, max_waves, None), "rtx_debug_wave_times", self._lib)

    def wave_times(self, max_waves: int) -> np.ndarray:
        out = np.zeros((max_waves, 2), np.uint64)
        _check(self._lib.rtx_debug_wave_times(self._h, max_waves, out.ctypes.data_as(C.POINTER(C.c_uint64))),
               "rtx_debug_wave_times", self._lib)
        return out

    def debug_scan_rate(self, reps: int) -> tuple:
        """hit_world alone at the render's occupancy (rtx_debug_scan_rate):
        (launch ms, wave-segments)."""
        ms, ws = C.c_float(0.0), C.c_uint64(0)
        _check(self._lib.rtx_debug_scan_rate(self._h, reps, C.byref(ms), C.byref(ws)), "rtx_debug_scan_rate", self._lib)
        return float(ms.value), int(ws.value)

    def debug_pixel_cost(self, spp: int = 0) -> np.ndarray:
        """Per-pixel ray-segment counts of the current frame, (H, W) uint32."""
        f = self.frame
        out = np.zeros((f.height, f.width), np.uint32)
        _check(self._lib.rtx_debug_pixel_cost(self._h, spp, out.ctypes.data_as(C.POINTER(C.c_uint32))),
               "rtx_debug_pixel_cost", self._lib)
        return out

    def debug_math(self, fn: str, in0: np.ndarray, in1: Optional[np.ndarray] = None) -> np.ndarray:
        a = np.ascontiguousarray(in0, np.float32)
        b = None if in1 is None else np.ascontiguousarray(in1, np.float32)
        out = np.zeros(3 * a.size, np.float32)
        _check(self._lib.rtx_debug_math(self._h, FN[fn], _fptr(a),
                                        _fptr(b) if b is not None else None, a.size, _fptr(out)),
               "rtx_debug_math", self._lib)
        return out.reshape(a.size, 3) if FN[fn] >= FN["hash1"] else out[:a.size]

    def debug_lambert_dir(self, p: np.ndarray, nrm: np.ndarray, rius: np.ndarray, guard: bool) -> np.ndarray:
        """The kernel's diffuse direction, normalize(((p + normal) + rius) - p),
        optionally near-zero guarded (RTX_FN_LAMBERT_DIR[_GUARD]); (n, 3) arrays."""
        a = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
        b = np.ascontiguousarray(np.concatenate([np.reshape(nrm, (-1, 3)), np.reshape(rius, (-1, 3))], 1),
                                 np.float32)
        out = np.zeros_like(a)
        fn = FN["lambert_dir_guard" if guard else "lambert_dir"]
        _check(self._lib.rtx_debug_math(self._h, fn, _fptr(a), _fptr(b), a.shape[0], _fptr(out)),
               "rtx_debug_math", self._lib)
        return out


class _MemberContext(Context):
    """A group member's context, borrowed (rtx_group_ctx): the group owns and
    destroys it, so close() only lets go of the handle."""

    def __init__(self, lib: C.CDLL, handle: int, device: int):
        self._lib = lib
        self._h = C.c_void_p(handle)
        self.device = device
        self.frame = None
        self.world = None

    def close(self):
        self._h = None


class Group:
    """One frame across several devices in one process (rtx_group, include/rtx.h):
    member i of `devices` renders part i of the interleaved row tiles, member 0
    gathers and assembles the image. `devices` all distinct, or all equal for
    the one-GPU rehearsal (the members then render one after another).
    gather: "auto", "rccl" or "copy". Mirrors :class:`Context`."""

    def __init__(self, devices, gather: str = "auto", lib: Optional[C.CDLL] = None):
        self._lib = lib or load_library()
        if not hasattr(self._lib, "rtx_group_create"):
            raise RtxError("this librtx.so has no rtx_group entry points")
        if gather not in GATHER_MODES:
            raise ValueError(f"gather must be one of {sorted(GATHER_MODES)}")
        self.devices = [int(d) for d in devices]
        arr = (C.c_int * max(1, len(self.devices)))(*self.devices)
        h = C.c_void_p()
        _check(self._lib.rtx_group_create(arr, len(self.devices), GATHER_MODES[gather], C.byref(h)),
               "rtx_group_create", self._lib)
        self._h = h
        self.frame: Optional[rtx_frame] = None
        self.world: Optional[World] = None
        self._members = [_MemberContext(self._lib, self._lib.rtx_group_ctx(h, i), d)
                         for i, d in enumerate(self.devices)]

    def close(self):
        if getattr(self, "_h", None):
            for m in self._members:
                m.close()
            self._lib.rtx_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return int(self._lib.rtx_group_size(self._h))

    def ctx(self, member: int) -> Context:
        """Member's context (borrowed): schedule, scan mode, stats."""
        return self._members[member]

    @property
    def gather(self) -> str:
        """The transport in use: "rccl" or "copy"."""
        return "rccl" if self._lib.rtx_group_gather_mode(self._h) == GATHER_MODES["rccl"] else "copy"

    @property
    def rccl_version(self) -> Optional[int]:
        return int(self._lib.rtx_group_rccl_version(self._h)) or None

    def upload_world(self, world: World):
        w = world.as_struct()
        _check(self._lib.rtx_group_upload_world(self._h, C.byref(w)), "rtx_group_upload_world", self._lib)
        self.world = world
        for m in self._members:
            m.world = world

    def set_frame(self, frame: rtx_frame):
        _check(self._lib.rtx_group_set_frame(self._h, C.byref(frame)), "rtx_group_set_frame", self._lib)
        self.frame = frame
        for m in self._members:
            m.frame = frame

    def render(self, tile_rows: int = 5):
        _check(self._lib.rtx_group_render(self._h, tile_rows), "rtx_group_render", self._lib)

    def sync(self):
        _check(self._lib.rtx_group_sync(self._h), "rtx_group_sync", self._lib)

    def image_ptr(self) -> int:
        return int(self._lib.rtx_group_image(self._h) or 0)

    def download(self) -> np.ndarray:
        f = self.frame
        out = np.empty((f.height, f.width, 4), np.float32)
        _check(self._lib.rtx_group_download(self._h, _fptr(out), out.nbytes), "rtx_group_download", self._lib)
        return out

    def render_image(self, tile_rows: int = 5) -> np.ndarray:
        self.render(tile_rows)
        return self.download()

    def accumulate(self, frames: int, reset: bool = False) -> int:
        """`frames` more progressive frames, whole frames dealt to the members
        (frame j to member j % n), folded in frame order on the root: the image
        of as many Context.accumulate calls, bit for bit. Returns the frames
        accumulated."""
        _check(self._lib.rtx_group_accumulate(self._h, frames, 1 if reset else 0), "rtx_group_accumulate",
               self._lib)
        return self.accumulated_frames

    @property
    def accumulated_frames(self) -> int:
        return int(self._lib.rtx_group_accumulated_frames(self._h))

    def refine(self, samples: int, tile_rows: int = 5, reset: bool = False) -> int:
        """`samples` more samples of every pixel along the reference's own RNG
        chain, each member refining its own rows (Context.refine_rows), then the
        gather and the de-interleave: the image of as many Context.refine
        calls, bit for bit. Returns the samples refined so far
        (rtx_group_refine)."""
        _check(self._lib.rtx_group_refine(self._h, samples, tile_rows, 1 if reset else 0), "rtx_group_refine",
               self._lib)
        return self.refined_samples

    @property
    def refined_samples(self) -> int:
        """Samples per pixel in the group's chain state (0: none)."""
        return int(self._lib.rtx_group_refined_samples(self._h))

    def refine_export(self) -> np.ndarray:
        """The group's chain state as one whole-frame state, (H, W, 4) float32:
        what Context.refine_export gives on one context at the same N
        (rtx_group_refine_export)."""
        f = self.frame
        out = np.empty((f.height, f.width, 4), np.float32)
        _check(self._lib.rtx_group_refine_export(self._h, _fptr(out), out.nbytes), "rtx_group_refine_export",
               self._lib)
        return out

    def refine_import(self, state: np.ndarray, samples: int, tile_rows: int = 5):
        """Install a whole-frame chain state of `samples` samples per pixel,
        every member its rows, and assemble its image; the next refine() with
        this tile_rows continues from it (rtx_group_refine_import)."""
        state = np.ascontiguousarray(state, np.float32)
        _check(self._lib.rtx_group_refine_import(self._h, tile_rows, _fptr(state), state.nbytes, samples),
               "rtx_group_refine_import", self._lib)

    def refine_adaptive(self, samples: int, threshold: float, max_samples: int = 0, tile_rows: int = 5,
                        reset: bool = False) -> int:
        """Context.refine_adaptive across the members: each refines the noisy
        pixels of its own rows after the members exchanged their tiles' edge
        rows of the error map, so the image, counts, errors and state are those
        of one context, bit for bit. Returns the number of pixels traced
        (rtx_group_refine_adaptive)."""
        n = C.c_uint32(0)
        _check(self._lib.rtx_group_refine_adaptive(self._h, samples, threshold, max_samples, tile_rows,
                                                   1 if reset else 0, C.byref(n)), "rtx_group_refine_adaptive",
               self._lib)
        return int(n.value)

    def refine_pending(self, samples: int, threshold: float, max_samples: int = 0, tile_rows: int = 5) -> int:
        """The number of pixels refine_adaptive with these arguments would
        trace now; nothing is traced (rtx_group_refine_pending)."""
        n = C.c_uint32(0)
        _check(self._lib.rtx_group_refine_pending(self._h, samples, threshold, max_samples, tile_rows, C.byref(n)),
               "rtx_group_refine_pending", self._lib)
        return int(n.value)

    def refine_counts(self) -> np.ndarray:
        """(H, W) uint32: the samples in every pixel's sum (rtx_group_refine_counts)."""
        f = self.frame
        out = np.empty((f.height, f.width), np.uint32)
        _check(self._lib.rtx_group_refine_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.nbytes),
               "rtx_group_refine_counts", self._lib)
        return out

    def refine_error(self) -> np.ndarray:
        """(H, W) float32: the error estimate of every pixel's last step
        (rtx_group_refine_error)."""
        f = self.frame
        out = np.empty((f.height, f.width), np.float32)
        _check(self._lib.rtx_group_refine_error(self._h, _fptr(out), out.nbytes), "rtx_group_refine_error", self._lib)
        return out

    def accumulate_times(self) -> dict:
        """HIP-event times of the last round of the last accumulate(), after
        sync() / download(): {"render_ms": [per member, 0 for one that took no
        frame in it], "gather_ms", "fold_ms"}. No scaling figure either."""
        n = len(self.devices)
        r = (C.c_double * n)()
        g, d = C.c_double(0.0), C.c_double(0.0)
        _check(self._lib.rtx_group_get_accumulate_times(self._h, r, C.byref(g), C.byref(d)),
               "rtx_group_get_accumulate_times", self._lib)
        return {"render_ms": list(r), "gather_ms": g.value, "fold_ms": d.value}

    def times(self) -> dict:
        """HIP-event times of the last synced frame: {"render_ms": [per member],
        "gather_ms", "deinterleave_ms"}. Members on one device run one after
        another: no scaling figure."""
        n = len(self.devices)
        r = (C.c_double * n)()
        g, d = C.c_double(0.0), C.c_double(0.0)
        _check(self._lib.rtx_group_get_times(self._h, r, C.byref(g), C.byref(d)), "rtx_group_get_times",
               self._lib)
        return {"render_ms": list(r), "gather_ms": g.value, "deinterleave_ms": d.value}


class DeviceArray:
    """Device buffer owned by a Context (rtx_alloc/rtx_free), no torch needed."""

    def __init__(self, ctx: Context, shape, dtype=np.float32):
        self.ctx, self.shape, self.dtype = ctx, tuple(shape), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        _check(ctx._lib.rtx_alloc(ctx._h, self.nbytes, C.byref(p)), "rtx_alloc", ctx._lib)
        self.ptr = int(p.value)

    def numpy(self) -> np.ndarray:
        out = np.empty(self.shape, self.dtype)
        _check(self.ctx._lib.rtx_copy_to_host(self.ctx._h, out.ctypes.data, C.c_void_p(self.ptr),
                                              self.nbytes), "rtx_copy_to_host", self.ctx._lib)
        return out

    def upload(self, a: np.ndarray):
        a = np.ascontiguousarray(a, self.dtype)
        assert a.nbytes == self.nbytes
        _check(self.ctx._lib.rtx_copy_to_device(self.ctx._h, C.c_void_p(self.ptr), a.ctypes.data,
                                                self.nbytes), "rtx_copy_to_device", self.ctx._lib)

    def free(self):
        if self.ptr and self.ctx._h:
            _check(self.ctx._lib.rtx_free(self.ctx._h, C.c_void_p(self.ptr)), "rtx_free", self.ctx._lib)
        self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
