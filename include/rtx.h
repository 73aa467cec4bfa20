/*
 * rtx.h — C-ABI of the MI355X-native sphere path tracer (librtx.so).
 *
 * This is the drop-in boundary for the reference's GPU path. In
 * Brochu/RayTrace-WE-GPU the host app (CSVersion/DxCSApp.cpp) talks to the
 * GPU through D3D11 objects owned by CDx11Base (CSVersion/Dx11Base.h:11-40):
 *   - cbuffer b1 `WorldDef`   (DxCSApp.cpp:64-71, ShaderCompute.hlsl:12-19),
 *     IMMUTABLE, uploaded once in LoadContent (DxCSApp.cpp:393-413);
 *   - cbuffer b0 `PerFrame`   (DxCSApp.cpp:30-37, ShaderCompute.hlsl:3-10),
 *     DYNAMIC, Map/memcpy/Unmap every Update (DxCSApp.cpp:481-496);
 *   - UAV slot 0 RWTexture2D<float4> (DxCSApp.cpp:326-356, :519) written by
 *     `CSMain` (ShaderCompute.hlsl:291-315);
 *   - Dispatch(32,32,1) (DxCSApp.cpp:524).
 * Every entry point below names the reference call it replaces.
 *
 * Conventions: plain C types only; no exceptions cross the ABI; every
 * function returns RTX_OK (0) or a negative RTX_ERR_* code and then
 * rtx_last_error() (thread-local) describes the failure. A context is bound
 * to one HIP device and is not thread-safe (the reference drives one D3D11
 * immediate context from the UI thread). Framebuffers are linear
 * float4[rows * width], row 0 = image bottom (the reference's DTid.y,
 * ShaderCompute.hlsl:306-307 with the display quad's texcoords,
 * DxCSApp.cpp:297-303).
 */
#ifndef RTX_H_
#define RTX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define RTX_API __attribute__((visibility("default")))
#else
#define RTX_API
#endif

#define RTX_VERSION 145 /* 1.4.5 */
/* ABI notes.
 *  1.4.5 (later builds, no version bump): rtx_trace_film (rtx_film_query,
 *         rtx_film_lens_query, RTX_FILM_LENS), rtx_film_last_order and the
 *         host generators rtx_film_from_frame and rtx_film_camera
 *         (RTX_FILM_EQUIRECT, RTX_FILM_FISHEYE): path queries whose every
 *         sample is jittered over a film footprint of the query's own, and
 *         goes through its lens; purely additive again: probe for the symbol
 *         (dlsym "rtx_trace_film").
 *  1.4.5 (later builds, no version bump): rtx_trace_paths_keyed
 *         (RTX_PATHS_ORDER_COST) and rtx_debug_paths_order (path queries in
 *         cost order, by the caller's keys or the library's own probe; the
 *         records are rtx_trace_paths'); purely additive again: probe for the
 *         symbol (dlsym "rtx_trace_paths_keyed").
 *  1.4.5 (later builds, no version bump): rtx_trace_paths (rtx_path_query,
 *         rtx_path_result, RTX_PATHS_*) and rtx_paths_last_order (what rays of
 *         the caller's choosing see: path-traced sample sums along the RNG
 *         chain, on device buffers); purely additive again: probe for the
 *         symbol (dlsym "rtx_trace_paths").
 *  1.4.5 (later builds, no version bump): rtx_path_seed (the chain seed of a
 *         pixel, on the host; groundwork for path queries along rays of the
 *         caller's choosing); purely additive again: probe for the symbol
 *         (dlsym "rtx_path_seed").
 *  1.4.5 (later builds, no version bump): rtx_cast_rays (rtx_ray, rtx_ray_hit,
 *         RTX_CAST_ORDER_*) and rtx_cast_last_order (batched closest-hit ray
 *         queries on device buffers, each ray with its own t_max); purely
 *         additive again: probe for the symbol (dlsym "rtx_cast_rays").
 *  1.4.5 (later builds, no version bump): rtx_features, rtx_features_rows,
 *         rtx_pick (rtx_hit), rtx_mask_from_ids and rtx_refine_masked (the
 *         first hit of every pixel's centre ray as feature buffers, picking,
 *         and refinement of the pixels that show chosen objects); purely
 *         additive again: probe for the symbol (dlsym "rtx_features").
 *  1.4.5 (later builds, no version bump): rtx_debug_scene_info (what
 *         rtx_upload_world built; dlsym "rtx_debug_scene_info").
 *  1.4.5 (later builds, no version bump): rtx_refine_adaptive_rows,
 *         rtx_refine_pending_rows, rtx_refine_edges, rtx_refine_counts_rows and
 *         rtx_refine_error_rows (adaptive refinement of a row part on a
 *         context), rtx_group_refine_adaptive, rtx_group_refine_pending,
 *         rtx_group_refine_counts and rtx_group_refine_error (... across a
 *         group's members); purely additive again: probe for the symbol
 *         (dlsym "rtx_refine_adaptive_rows").
 *  1.4.5 (later builds, no version bump): rtx_refine_rows,
 *         rtx_refine_import_rows and rtx_refine_shape (refinement of a row
 *         part on a context), rtx_group_refine, rtx_group_refined_samples,
 *         rtx_group_refine_export and rtx_group_refine_import (progressive
 *         refinement across a group's members, and its checkpoint); purely
 *         additive again: probe for the symbol (dlsym "rtx_group_refine").
 *  1.4.5 (later builds, no version bump): rtx_refine, rtx_refined_samples,
 *         rtx_refine_state, rtx_refine_export and rtx_refine_import
 *         (progressive samples along the reference's own RNG chain, and its
 *         checkpoint); purely additive again: probe for the symbol
 *         (dlsym "rtx_refine"). rtx_refine_set_keys, rtx_refine_last_keys and
 *         rtx_refine_cost (the cost map a refine launch records, and queue keys
 *         carried from it: dlsym "rtx_refine_set_keys"). rtx_refine_adaptive,
 *         rtx_refine_pending, rtx_refine_counts, rtx_refine_error and
 *         rtx_adaptive_error (refinement of the pixels that are still noisy:
 *         dlsym "rtx_refine_adaptive").
 *  1.4.5 (later builds, no version bump): rtx_render_sum, rtx_fold_frames
 *         (RTX_FOLD_MAX), rtx_group_accumulate, rtx_group_accumulated_frames
 *         and rtx_group_get_accumulate_times (progressive frames dealt across
 *         a group's members); purely additive again: probe for the symbol
 *         (dlsym "rtx_group_accumulate").
 *  1.4.5 (later builds, no version bump): the rtx_group entry points (one
 *         frame across several devices); purely additive — no struct and no
 *         earlier entry point changed — so a caller probes for the symbol
 *         (dlsym "rtx_group_create") rather than for a version.
 *  1.4.5: schedule defaults tier1_bar_low 2.0 -> 1.8, promote_low 300 ->
 *         500 (the R = 4 share with the layer grid, S6k-S6l) and
 *         refill_chunk 16 -> 64 (the queue in pixel tiles, S6t-S6u); private
 *         runs (at most 16 slots) also for large scenes and medium shares;
 *         no layout change.
 *  1.4.4: rtx_set_scan_mode (RTX_SCAN_AUTO / RTX_SCAN_LINEAR; a new entry
 *         point, no layout change).
 *  1.4.3: RTX_DEBUG_CULLED_COOP_LANE(q) (the culled coop's per-lane walk);
 *         RTX_ERR_INCOMPLETE's message names which promotion wait fired and
 *         what the server saw (no layout change).
 *  1.4.2: rtx_debug_hit_world_from's start_block RTX_DEBUG_CULLED and
 *         RTX_DEBUG_CULLED_COOP(q) (the culled scan, lane mode and group
 *         coop; no layout change).
 *  1.4.1: rtx_debug_scan_rate (a diagnostic; no layout change).
 *  1.4.0: rtx_schedule.prio_bar1..3 (after prepass_cap_split, before
 *         `reserved`): dynamic lane-mode wave priority; the struct grew by
 *         12 bytes.
 *  1.3.0: rtx_schedule.trace_solo_bar (after promote_big_scene),
 *         trace_group and prepass_cap_split (after refill_chunk): the
 *         struct grew by 12 bytes;
 *         rtx_build_info; RTX_ERR_INCOMPLETE: rtx_sync, rtx_download, rtx_get_stats and
 *         rtx_stats_reset report a render launch that left pixels unwritten
 *         (the promotion service's safety valve fired) instead of returning
 *         the image as if it were complete.
 *  1.2.0: rtx_schedule.promote_big_scene (after promote_large) and
 *         refill_chunk (before `reserved`): the struct grew by 8 bytes.
 *  1.1.0: rtx_schedule_defaults / rtx_set_schedule / rtx_get_schedule (the
 *         chain-RNG schedule, formerly an undocumented environment variable
 *         of the library: the library now reads no environment);
 *         rtx_debug_hit_world_from; rtx_debug_hit_world rejects t_min <= 0.
 *  1.0.x: rtx_set_stream(ctx, NULL) selects HIP's null (legacy default)
 *         stream, which implicitly synchronises with every blocking stream;
 *         the context's own non-blocking stream is rtx_use_own_stream. (The
 *         first 1.0 builds treated NULL as "own stream".) */

enum {
    RTX_OK = 0,
    RTX_ERR_INVALID = -1, /* bad argument (null pointer, size mismatch, ...) */
    RTX_ERR_HIP = -2,     /* a HIP runtime call failed */
    RTX_ERR_STATE = -3,   /* call out of order (no world / no frame yet) */
    RTX_ERR_NOMEM = -4,   /* host or device allocation failed */
    RTX_ERR_INCOMPLETE = -5 /* a render launch since the last check left pixels
                               unwritten (reported once, by the next rtx_sync,
                               rtx_download, rtx_get_stats or rtx_stats_reset) */
};

/* Material type codes, as the reference stores them in WorldDef::matTypes
 * (DxCSApp.cpp:11-17 SetFloat4Cmpt; ShaderCompute.hlsl:209,219,229). */
enum { RTX_MAT_LAMBERT = 0, RTX_MAT_METAL = 1, RTX_MAT_DIELECTRIC = 2 };

/* RNG modes. CHAIN is the reference: ONE fp32 seed per pixel carried through
 * all samples (ShaderCompute.hlsl:295, 304-309). PER_SAMPLE re-seeds every
 * (pixel, sample) so samples are independent of each other (needed to split
 * one pixel's samples across lanes/GPUs); it is an extension, not reference
 * behaviour. */
enum { RTX_RNG_CHAIN = 0, RTX_RNG_PER_SAMPLE = 1 };

/* rtx_frame.flags. RTX_FRAME_LAMBERT_GUARD (an extension):
 * a diffuse scatter direction whose three components are all below 1e-9 in
 * magnitude is replaced by the normal before it is normalised — the guard of
 * the pixel-shader prototype's lambert (Shader_RT.fx:219-225) with the
 * compute shader's own unused near_zero (ShaderCompute.hlsl:70-74). The
 * compute shader has no guard (:209-217) and normalises a zero vector to
 * NaN; 0 keeps that. */
enum { RTX_FRAME_LAMBERT_GUARD = 1 };

/* Scene (~ cbuffer b1 WorldDef, DxCSApp.cpp:64-71). Arrays are read during
 * rtx_upload_world and copied; the caller keeps ownership. Unlike the
 * reference's fixed 512-sphere cbuffer the count is unbounded. */
typedef struct rtx_world {
    uint32_t count;           /* sceneValues.x : number of spheres           */
    uint32_t depth;           /* sceneValues.y : max ray segments per sample */
    uint32_t spp;             /* sceneValues.z : samples per pixel           */
    uint32_t reserved;        /* must be 0                                   */
    const float *spheres;     /* 4*count : center.xyz, radius  (spheres[])   */
    const float *mat_types;   /* count   : RTX_MAT_* as float  (matTypes[])  */
    const float *mat_values;  /* 4*count : albedo.rgb, fuzz-or-ir (matValues[]) */
} rtx_world;

/* Per-frame constants (~ cbuffer b0 PerFrame, DxCSApp.cpp:30-37). The four
 * rows are the reference's viewVals as the shader reads them
 * (ShaderCompute.hlsl:122-123): origin, horizontal, vertical, lower-left. */
typedef struct rtx_frame {
    float origin[4];          /* viewVals[0] */
    float horizontal[4];      /* viewVals[1] */
    float vertical[4];        /* viewVals[2] */
    float lower_left[4];      /* viewVals[3] */
    float img_w;              /* img_dim.x = perspectiveVals.w               (ShaderCompute.hlsl:294) */
    float img_h;              /* img_dim.y = perspectiveVals.w / perspectiveVals.y */
    uint32_t width;           /* framebuffer width in pixels  (texture Width,  DxCSApp.cpp:331) */
    uint32_t height;          /* framebuffer height in pixels (texture Height, DxCSApp.cpp:330) */
    uint32_t rng_mode;        /* RTX_RNG_*; 0 = reference                     */
    uint32_t frame_index;     /* seed offset for progressive frames; 0 = reference (time unused, :296) */
    uint32_t flags;           /* RTX_FRAME_* bits; 0 = reference              */
    uint32_t reserved;        /* must be 0 */
    /* Thin-lens defocus (an extension: the reference's compute
     * shader passes aperture but ignores it, DxCSApp.cpp:179 /
     * ShaderCompute.hlsl:118-127). lens_u/lens_v = camera u/v axes, lens_u[3]
     * = lens radius (aperture/2); 0 = pinhole (reference behaviour). Per
     * sample: rd = radius * random_in_unit_disk (ShaderCompute.hlsl:50-57),
     * offset = u*rd.x + v*rd.y, origin += offset, dir -= offset
     * (Shader_RT.fx:288-298). */
    float lens_u[4];
    float lens_v[4];
} rtx_frame;

/* Counters of the last launches since rtx_stats_reset (measurement, §8d). */
typedef struct rtx_stats {
    double kernel_ms;         /* summed HIP-event duration of the render kernels */
    uint64_t launches;        /* render kernel launches                          */
    uint64_t samples;         /* pixel-samples traced (pixels * spp)             */
    uint64_t segments;        /* hit_world calls (ray segments)                  */
    uint64_t sphere_tests;    /* segments * sphere count (ray-sphere tests)      */
} rtx_stats;

typedef struct rtx_ctx rtx_ctx;

/* ---- library / device ------------------------------------------------- */
RTX_API int rtx_version(void);
/* Build provenance (1.3.0): "src_sha16=<hash of the sources the library was
 * compiled from> arch=gfx950" (static string). */
RTX_API const char *rtx_build_info(void);
/* Thread-local text of the last failure on this thread ("" if none). */
RTX_API const char *rtx_last_error(void);
/* Number of visible HIP devices. */
RTX_API int rtx_device_count(int *count);

/* ---- context lifecycle (~ CDx11Base::Initialize / Terminate) ------------
 * rtx_create replaces D3D11CreateDeviceAndSwapChain (CSVersion/Dx11Base.cpp:75)
 * + the resource creation in LoadContent; rtx_destroy replaces
 * CDx11Base::Terminate -> DxCSApp::UnloadContent (Dx11Base.cpp:134-152,
 * DxCSApp.cpp:420-456). */
RTX_API int rtx_create(int hip_device, rtx_ctx **out);
RTX_API void rtx_destroy(rtx_ctx *ctx);
/* Use an external hipStream_t (e.g. torch's current stream) for every later
 * launch and copy. NULL is HIP's null (legacy default) stream — the handle
 * torch reports for its default stream — so that work orders with the
 * caller's other work on it. */
RTX_API int rtx_set_stream(rtx_ctx *ctx, void *hip_stream);
/* Back to the context's own non-blocking stream (the state after rtx_create). */
RTX_API int rtx_use_own_stream(rtx_ctx *ctx);

/* ---- schedule of the chain-RNG render ------------------
 * The reference's RNG chain makes a pixel's samples sequential, so the render
 * schedules PIXELS: a 2-spp cost pre-pass gives every pixel a cost key (its
 * 3x3 neighbourhood's segments), the persistent render takes pixels most
 * expensive first, and the heaviest are traced by groups of lanes. With
 * share = (sum of the keys) / (resident lanes) and "pixels per lane" = the
 * part's pixels / resident lanes:
 *   - tier 1 (one pixel per wave, 64 lanes per ray): keys above
 *     tier1_bar x share; for a SMALL part (pixels per lane < small_share,
 *     e.g. one rank of an 8-way split) tier1_bar_small, for a LOW part
 *     (< low_share) tier1_bar_low;
 *   - tier 2 (eight pixels per wave): a small part's keys above
 *     tier2_bar_small x share, a MEDIUM part's (< medium_share) above
 *     tier2_bar_medium x share, a larger part's above tier2_bar x share
 *     (tier-2 bars above the tier-1 bar select no tier 2);
 *   - hot_fraction x resident lanes of the normal queue's first slots run at
 *     wave priority hot_priority; tier-1 waves at tier1_priority, tier-2
 *     waves at tier2_priority (s_setprio 0..3: issue arbitration among the
 *     waves of a SIMD);
 *   - occupancy_*: the fraction of the resident waves launched for a small /
 *     low / larger part;
 *   - tail_coop_max: once the queue is empty a wave with at most this many
 *     pixels left traces them with several lanes per ray (1..64);
 *     tail_coop_max_large for scenes above 640 spheres (no LDS copy of the
 *     scene: the group's sphere reads go to L2/HBM);
 *   - trace_*: for scenes up to 640 spheres tier 1 runs in its own kernel
 *     beside the render (one pixel per wave, all 64 lanes on its ray), with
 *     this fraction of the resident waves for a small / low / medium /
 *     larger part (0: tier 1 stays in the render kernel); trace_group
 *     pixels per wave of it (each traced by 64 / trace_group lanes: more
 *     chains for about the same issue, a little longer per segment), except
 *     keys above trace_solo_bar x share, traced one per wave; the kernel also
 *     serves the promotion queue once tier 1 is done;
 *   - promote_*: once the pixel queue is empty, a lane whose pixel is
 *     projected to need more than this many further ray segments hands it
 *     over at a sample boundary to a wave with nothing else to do (an idle
 *     render wave, or the tier-1 kernel), which traces it with all 64 lanes
 *     (0: never); promote_big_scene replaces them for scenes above 640
 *     spheres (no LDS copy: a segment is a long scan there, so a far
 *     shorter remaining chain is worth handing to a whole wave);
 *   - refill_chunk: for a part of at least medium_share pixels per lane (a
 *     whole frame) of a scene up to 1,024 spheres, each wave takes its pixels
 *     from a private run of this many consecutive slots of the cost-ordered
 *     queue (at most 16 for a larger scene or a part of low_share to
 *     medium_share pixels per lane; none below), re-stocked when
 *     empty, so its lanes hold pixels from few runs (coherent rays) rather
 *     than one slot per refill from wherever the queue head is; the last
 *     eighth of the queue is taken slot by slot;
 *   - prio_bar1..3: a lane-mode wave runs at priority 1, 2 or 3 while some
 *     lane's pixel is projected (its segments per sample so far, the cost
 *     pre-pass's included, times the samples left) to need more than
 *     prio_barK x the mean pixel's segments (the pre-pass's estimate), else
 *     at 0: the longest remaining chains get the SIMDs' issue, whatever their
 *     key said; prio_bar1 = 0 selects the static scheme instead (hot_fraction
 *     of the queue's first slots at hot_priority).
 * Results never depend on the schedule (every pixel's operations are the
 * same whichever lanes trace it); only the time does. The defaults are the
 * measured best. A context starts with the defaults. */
typedef struct rtx_schedule {
    float tier1_bar;          /* default 1.7 */
    float tier1_bar_small;    /* default 1.6 */
    float tier1_bar_low;      /* default 1.8 (2.0 before 1.4.5) */
    float tier2_bar_small;    /* default 2.0 */
    float tier2_bar_medium;   /* default 1e30 (none; 1.2 in earlier builds) */
    float tier2_bar;          /* default 1e30 (no tier 2 for a larger part) */
    float small_share;        /* default 1.2 pixels per resident lane */
    float low_share;          /* default 2.5 */
    float medium_share;       /* default 3.5 */
    float hot_fraction;       /* default 0.2 */
    float occupancy_small;    /* default 1.0; each occupancy in (0, 1] */
    float occupancy_low;      /* default 1.0 */
    float occupancy_normal;   /* default 1.0 */
    float trace_small;        /* default 0.35; each trace_* in [0, 0.5] */
    float trace_low;          /* default 0.3 */
    float trace_medium;       /* default 0.15 */
    float trace_large;        /* default 0 */
    float promote_small;      /* default 400; each promote_* in [0, 1e9] */
    float promote_low;        /* default 500 (300 before 1.4.5) */
    float promote_medium;     /* default 400 */
    float promote_large;      /* default 400 */
    float promote_big_scene;  /* default 60: every part of a scene above 640 spheres */
    float trace_solo_bar;     /* default 6: tier-1 keys above this x share are traced one pixel per wave
                                 even when trace_group > 1 */
    uint32_t tail_coop_max;   /* default 32 */
    uint32_t tail_coop_max_large; /* default 8: the same for scenes above 640 spheres */
    uint32_t tier1_priority;  /* default 3 */
    uint32_t tier2_priority;  /* default 2 */
    uint32_t hot_priority;    /* default 3 */
    uint32_t refill_chunk;    /* default 64 (16 before 1.4.5); 0..4096 (0, 1: one refill per need) */
    uint32_t trace_group;     /* default 4: tier-1 pixels per wave of the tier-1 kernel (1, 2, 4 or 8; 8 since 1.4.1) */
    uint32_t prepass_cap_split; /* default 0 (none): a row-split part's cost pre-pass stops a pixel past this
                                   many segments (0..4096); it goes to the top of the queue (tier 1) and the
                                   render traces it from sample 0 */
    float prio_bar1;          /* default 0.5 (0: static hot slots, hot_fraction / hot_priority) */
    float prio_bar2;          /* default 1.0 */
    float prio_bar3;          /* default 1.5 */
    uint32_t reserved;        /* must be 0 */
} rtx_schedule;
/* The library's defaults (no context, no GPU). */
RTX_API int rtx_schedule_defaults(rtx_schedule *out);
/* Validates and installs a schedule for later launches of `ctx` (NULL =
 * the defaults): bars and shares finite and > 0, hot_fraction in [0, 1],
 * occupancies in (0, 1], trace_* in [0, 0.5], promote_* in [0, 1e9],
 * tail_coop_max and tail_coop_max_large in 1..64,
 * priorities in 0..3, refill_chunk in 0..4096, trace_group 1, 2, 4 or 8,
 * trace_solo_bar > 0, prepass_cap_split in 0..4096, prio_bar1 = 0 or
 * 0 < prio_bar1 <= prio_bar2 <= prio_bar3 <= 1e30, reserved 0. */
RTX_API int rtx_set_schedule(rtx_ctx *ctx, const rtx_schedule *schedule);
RTX_API int rtx_get_schedule(rtx_ctx *ctx, rtx_schedule *out);

/* ---- scene / frame upload ----------------------------------------------
 * ~ CreateBuffer(WorldDef, IMMUTABLE) (DxCSApp.cpp:393-413).
 * What rtx_upload_world accepts: every sphere component (centre and radius)
 * finite with |value| <= 1e15, nothing more. A radius may be 0, -0 or
 * negative: the reference reads it as r * r in the discriminant and as 1 / r
 * in the normal, and so does the library (a negative radius turns the normal
 * and front_face round, a zero one makes them infinite or NaN). mat_types and
 * mat_values are not looked at: a code other than 0, 1, 2 does not scatter,
 * and a NaN, infinite, zero or negative albedo, fuzz or refraction index
 * enters the path arithmetic as it stands. rtx_set_frame does not check that
 * the camera vectors are finite either. Every such input renders what the
 * reference's arithmetic gives, bit for bit (tests/test_gpu_hostile_inputs.py). */
RTX_API int rtx_upload_world(rtx_ctx *ctx, const rtx_world *world);
/* How hit_world finds its candidates (the answer is the reference's in both):
 * RTX_SCAN_AUTO (the default): the flat layer's blocks through the layer grid
 * (scenes up to 1,024 spheres) and the culled scan over a spatially ordered
 * copy (larger scenes); RTX_SCAN_LINEAR: every block of the scene for every
 * ray segment, in Hittable_list order (Hittable_list.cpp:3-20,
 * ShaderCompute.hlsl:194), with the prefilter — large scenes stream it
 * through a per-wave LDS tile of 64 blocks. Takes effect at the next
 * rtx_upload_world. */
enum { RTX_SCAN_AUTO = 0, RTX_SCAN_LINEAR = 1 };
RTX_API int rtx_set_scan_mode(rtx_ctx *ctx, int mode);
/* ~ Map(WRITE_DISCARD)/memcpy/Unmap of PerFrame (DxCSApp.cpp:494-496).
 * Host-side only: constants travel as kernel arguments. */
RTX_API int rtx_set_frame(rtx_ctx *ctx, const rtx_frame *frame);

/* ---- render (~ Dispatch(32,32,1), DxCSApp.cpp:524) ------------------------
 * Renders the rows owned by partition `part` of `nparts`: image rows are
 * cut into tiles of `tile_rows` rows and tile k belongs to part k % nparts
 * (interleaved row tiles). The part's rows are written in
 * ascending order, contiguously, to d_out (device pointer, at least
 * rtx_part_rows(...) * width float4s). d_out == NULL renders into the
 * context's own framebuffer (whole image only: part 0 of 1).
 * Asynchronous on the context stream. */
RTX_API int rtx_render_rows(rtx_ctx *ctx, uint32_t tile_rows, uint32_t part,
                            uint32_t nparts, void *d_out);
/* Whole frame into the context framebuffer (= rtx_render_rows(ctx,1,0,1,NULL)). */
RTX_API int rtx_render(rtx_ctx *ctx);
/* Progressive accumulation (the reference's intended
 * interactive mode: sampleCount/currSamples DxCSApp.cpp:491-492, frame loop
 * CSVersion/main.cpp:51-52, seed hook ShaderCompute.hlsl:296). reset != 0
 * clears the accumulator. Each call renders one frame of spp samples per
 * pixel with frame_index = frames accumulated so far (distinct seeds), adds
 * each pixel's linear sample sum into a float4 accumulator, and writes
 * toGamma(sum / (frames * spp)) into the context framebuffer. */
RTX_API int rtx_accumulate(rtx_ctx *ctx, int reset);
/* Frames accumulated since the last reset. */
RTX_API uint32_t rtx_accumulated_frames(rtx_ctx *ctx);
/* One whole frame's LINEAR per-pixel sample sums for seed offset frame_index
 * (what rtx_accumulate adds to its accumulator for its frame number
 * frame_index), into d_sum: width*height float4, xyz = sum, w = 0.
 * Device pointer; asynchronous on the context stream. The context's own
 * accumulator and rtx_accumulated_frames are untouched (its framebuffer is
 * overwritten). frame_index <= 0x7fffffff. */
RTX_API int rtx_render_sum(rtx_ctx *ctx, uint32_t frame_index, void *d_sum);
/* Ordered fold. For each pixel p < pixels:
 *   a = d_accum[p];
 *   for k = 0 .. m-1: a.xyz = a.xyz + d_sums[k * slot_pixels + p].xyz   (this order)
 *   d_accum[p] = a (w unchanged);
 *   d_image[p] = (toGamma(a.x / n), toGamma(a.y / n), toGamma(a.z / n), 1), n = (float)divisor.
 * 1 <= m <= RTX_FOLD_MAX, slot_pixels >= pixels >= 1, divisor >= 1; the three
 * buffers must not overlap. With the sums of rtx_render_sum for frame_index
 * F .. F+m-1 and divisor (F + m) * spp this is m calls of rtx_accumulate, bit
 * for bit. Device pointers; asynchronous on the context stream. */
#define RTX_FOLD_MAX 64
RTX_API int rtx_fold_frames(rtx_ctx *ctx, void *d_accum, const void *d_sums, uint32_t m,
                            size_t slot_pixels, size_t pixels, uint32_t divisor, void *d_image);
/* Progressive refinement along the reference's own RNG chain (chain RNG only).
 * The reference counts sampleCount / currSamples every Update
 * (DxCSApp.cpp:491-492) but its frame loop and seed hook stayed commented out;
 * rtx_accumulate fills that gap with new seeds per frame, so its image after k
 * frames is no image the reference produces. rtx_refine instead CONTINUES
 * every pixel's chain: a pixel's whole future depends only on its linear
 * colour sum so far and its one fp32 seed, and the context keeps both.
 *
 * The context owns a chain state — width*height float4 in framebuffer order,
 * xyz = the pixel's linear sample sum, w = its seed after its last finished
 * sample — and the number N of samples in it. rtx_refine traces `samples`
 * more samples of every pixel of the current frame, writes
 * toGamma(sum / (float)(N + samples)), w = 1, into the context framebuffer and
 * updates the state and N. Asynchronous on the context stream, like
 * rtx_render. After calls adding s1..sk the framebuffer is, bit for bit (NaN
 * pixels included), what rtx_render writes for the same world and frame with
 * world.spp = s1 + ... + sk, whatever the steps: an image that sharpens in
 * steps and is the reference's image at every step, and "300 more samples"
 * at the cost of 300. world.spp is ignored; world.depth (0: zeros, as
 * rtx_render), frame_index, the thin lens and RTX_FRAME_LAMBERT_GUARD apply as
 * in rtx_render. The stats count pixels * samples samples and the launch's
 * segments.
 * The state restarts at N = 0 (every pixel's chain from its first seed) when
 * reset != 0, on a first call, after any rtx_upload_world, and after an
 * rtx_set_frame whose rtx_frame bytes differ from the frame the state was made
 * for (another size included). An rtx_set_frame of equal bytes keeps it (hosts
 * call it every Update, as the reference maps PerFrame every Update).
 * rtx_set_schedule and rtx_set_scan_mode keep it (results never depend on
 * them); rtx_render, rtx_render_rows, rtx_accumulate and rtx_render_sum
 * between two calls overwrite the framebuffer but not the state.
 * RTX_ERR_INVALID, before any HIP call: a null ctx, samples == 0, N + samples
 * not representable in uint32, or a frame with rng_mode RTX_RNG_PER_SAMPLE —
 * under a nonzero frame_index that mode's seeds depend on the frame's total
 * spp (frame_index * spp + s), so "continue" has no single meaning there;
 * rtx_accumulate is that mode's progressive form. RTX_ERR_STATE: no world or
 * no frame.
 * Row parts: rtx_refine_rows below; a group-wide refine: rtx_group_refine;
 * adaptive refinement of a part and of a group: rtx_refine_adaptive_rows and
 * rtx_group_refine_adaptive.
 * The pixel queue's order: see rtx_refine_set_keys below. */
RTX_API int rtx_refine(rtx_ctx *ctx, uint32_t samples, int reset);
/* rtx_refine for the rows of partition `part` of `nparts` (rtx_render_rows'
 * partition; later builds, no version bump: probe with dlsym
 * "rtx_group_refine" or "rtx_refine_rows"). rtx_refine(ctx, s, reset) is
 * rtx_refine_rows(ctx, 1, 0, 1, s, reset, NULL).
 * The chain state and the cost map then cover the part's rows only:
 * rtx_part_rows(...) * width entries in the part's row order (ascending,
 * contiguous: d_out's order). d_out: device pointer to at least rows * width
 * float4; it receives toGamma(sum / (float)(N + samples)), w = 1, for those
 * rows. d_out == NULL is allowed only with nparts == 1 and selects the context
 * framebuffer, as rtx_refine does. A pixel's seed depends only on its global
 * position, so the parts of a frame, each refined on its own state, hold the
 * rows of the one-context image and state bit for bit.
 * A state has a shape (tile_rows, part, nparts); every shape with nparts == 1
 * is the same whole-frame shape whatever tile_rows (reported as (1, 0, 1)).
 * The state restarts at N = 0 under rtx_refine's rules and also when the call's
 * shape differs from the state's. rtx_refine_export, rtx_refine_cost and
 * rtx_refine_state serve a state of any shape: their `bytes` must match the
 * state's own pixel count (rows * width). Carried keys (rtx_refine_set_keys)
 * work on a part unchanged, the map in part order; the key's 3 x 3 window runs
 * over the part's local rows, which affects the queue's order only.
 * Adaptive refinement of a part state goes through the _rows entry points
 * (rtx_refine_adaptive_rows below): on a context whose state has nparts > 1,
 * the whole-frame rtx_refine_adaptive with reset == 0, rtx_refine_pending,
 * rtx_refine_counts and rtx_refine_error return RTX_ERR_STATE before any GPU
 * work; rtx_refine_adaptive with reset != 0 starts its whole-frame state. On a
 * part state whose counts differ after adaptive steps rtx_refine_rows without
 * reset returns RTX_ERR_STATE, as rtx_refine does on a whole frame.
 * RTX_ERR_INVALID, before any HIP call: a null ctx, samples == 0,
 * tile_rows == 0, nparts == 0, part >= nparts, d_out == NULL with nparts > 1,
 * N + samples above 2^32 - 1, a per-sample-RNG frame. RTX_ERR_STATE: no world
 * or no frame. A part that owns no rows returns RTX_OK, launches nothing and
 * leaves the state alone. */
RTX_API int rtx_refine_rows(rtx_ctx *ctx, uint32_t tile_rows, uint32_t part, uint32_t nparts,
                            uint32_t samples, int reset, void *d_out);
/* rtx_refine_import (below) for a part: bytes == rows*width*16, the state in
 * the part's row order; d_out receives the part's image rows
 * (toGamma(sum / (float)samples)); NULL with nparts > 1: no image is written,
 * NULL with nparts == 1: the context framebuffer. Synchronous. */
RTX_API int rtx_refine_import_rows(rtx_ctx *ctx, uint32_t tile_rows, uint32_t part, uint32_t nparts,
                                   const float *host_state, size_t bytes, uint32_t samples,
                                   void *d_out);
/* The shape of the chain state (NULL outputs are skipped); RTX_ERR_STATE when
 * there is no state, RTX_ERR_INVALID for a null ctx. */
RTX_API int rtx_refine_shape(rtx_ctx *ctx, uint32_t *tile_rows, uint32_t *part, uint32_t *nparts);
/* The cost map and the queue keys of a refine launch (1.4.5, later builds, no
 * version bump: probe with dlsym "rtx_refine_set_keys").
 * Every rtx_refine launch records, per pixel, the ray segments (hit_world
 * calls) it spent on that pixel — exact in every kernel path; the map's sum is
 * the launch's rtx_stats.segments. By default (RTX_REFINE_KEYS_PREPASS) every
 * scheduled launch still orders its pixel queue by a cost pre-pass of its own.
 * Under RTX_REFINE_KEYS_CARRIED the next launch builds the queue from the
 * previous launch's map instead and runs no pre-pass, when it can: the map is
 * valid, this call has at least 8 samples (smaller steps are unscheduled), and
 * the map covers at least the samples a pre-pass would trace (2; 1 for scenes
 * of more than 1,024 spheres). Otherwise the launch takes the pre-pass as
 * before. Images, the chain state, the map and the segment counts are bit for
 * bit the same in either mode: results never depend on the schedule.
 * The map is valid after any rtx_refine that traced segments. It falls with
 * the chain state (reset, rtx_upload_world, an rtx_set_frame with other bytes
 * or another size), after rtx_refine_import (the state file holds no map: the
 * first step after a resume takes the pre-pass), after a depth == 0 step, and
 * when samples * depth >= 2^32 (a count could wrap). rtx_render,
 * rtx_render_rows, rtx_accumulate, rtx_render_sum, rtx_set_schedule,
 * rtx_set_scan_mode and rtx_refine_set_keys leave it alone. */
#define RTX_REFINE_KEYS_PREPASS 0     /* a cost pre-pass per launch (the default) */
#define RTX_REFINE_KEYS_CARRIED 1     /* the previous launch's cost map, where valid */
#define RTX_REFINE_KEYS_UNSCHEDULED 2 /* rtx_refine_last_keys only */
/* RTX_ERR_INVALID, before any HIP call, for a null ctx or another mode. Keeps
 * the chain state and the map. */
RTX_API int rtx_refine_set_keys(rtx_ctx *ctx, int mode);
/* What the last rtx_refine launch was keyed by: RTX_REFINE_KEYS_PREPASS,
 * RTX_REFINE_KEYS_CARRIED, or RTX_REFINE_KEYS_UNSCHEDULED (the exact grid of a
 * step below 8 samples, the depth == 0 launch, or no launch yet). A null ctx:
 * RTX_ERR_INVALID. */
RTX_API int rtx_refine_last_keys(rtx_ctx *ctx);
/* The cost map to host memory (synchronous, like rtx_download): width*height
 * uint32 in framebuffer order (row 0 = bottom), and in *samples the samples of
 * the step it covers. bytes == width*height*4; for a part state
 * (rtx_refine_rows) the part's rows * width * 4, in the part's row order.
 * RTX_ERR_STATE if there is no valid map; RTX_ERR_INVALID for a null argument
 * or other bytes. */
RTX_API int rtx_refine_cost(rtx_ctx *ctx, uint32_t *host_cost, size_t bytes, uint32_t *samples);
/* N: samples per pixel in the chain state (0 for NULL / none): the sum of the
 * steps since the state began. After adaptive steps (below) that is the count
 * of a pixel that took part in every step; rtx_refine_counts has each pixel's. */
RTX_API uint32_t rtx_refined_samples(rtx_ctx *ctx);

/* ---- adaptive refinement: only the pixels that are still noisy -------------
 * (later builds, no version bump: probe with dlsym "rtx_refine_adaptive").
 * Next to the chain state the context keeps, per pixel, `count` (the samples
 * in the pixel's sum) and `err` (the error estimate E of the pixel's last
 * step). rtx_refine_adaptive traces `samples` more samples of every ACTIVE
 * pixel along its chain and leaves every other pixel alone: its state, count,
 * err, cost-map entry and framebuffer value are not touched. So a pixel that
 * has taken n samples holds, bit for bit, what rtx_render writes for it at
 * world.spp = n — the image is a mosaic of the reference's pixels at per-pixel
 * spp — and which pixels were traced is a deterministic function of the sums.
 *
 * E of a step that took a pixel from n_old to n_new samples, from its linear
 * sums before and after (fp32, in this order, IEEE division and square root,
 * no fma):
 *   n_old == 0 -> +inf
 *   a = (float)n_old, b = (float)n_new, sf = (float)(n_new - n_old)
 *   m0.c = sum_old.c / a,  m1.c = sum_new.c / b          (c = x, y, z)
 *   d = (|m1.x - m0.x| + |m1.y - m0.y|) + |m1.z - m0.z|
 *   l = (m1.x + m1.y) + m1.z
 *   E = (d * sqrt(a / sf)) / sqrt(l + 0.01f)
 * NaN sums give a NaN E. rtx_adaptive_error is that function on the host (no
 * GPU, no context).
 *
 * Pixel p is active in a call (samples, threshold, max_samples) iff
 *   some pixel q of its 3 x 3 neighbourhood inside the image has
 *   E_q >= threshold (false for a NaN E: a NaN pixel stays NaN), and
 *   max_samples == 0 or count_p + samples <= max_samples.
 *
 * The maps begin and fall with the chain state (reset, rtx_upload_world,
 * rtx_set_frame with other bytes). The first adaptive call over a uniform
 * state of N samples (a fresh one: N = 0; after rtx_refine or
 * rtx_refine_import: their N) fills count with N and err with +inf, so that
 * call traces every pixel, and after a fresh start so does the second (E stays
 * +inf for n_old == 0).
 *
 * A call with active pixels is one scheduled launch over those pixels, keyed
 * by the cost map where it is valid (rtx_refine_set_keys does not affect it;
 * rtx_refine_last_keys reports CARRIED), and rtx_stats.samples counts
 * active * samples. The host reads the 4-byte active count back before it
 * sizes the launch: one small stream synchronisation per call. A call with no
 * active pixel launches no render and changes nothing (rtx_refine_last_keys:
 * UNSCHEDULED; rtx_refined_samples stays). *active (may be NULL) receives the
 * number of pixels traced. Inactive pixels keep their own last step's entry
 * of the cost map (rtx_refine_cost), whose *samples is the last call's.
 *
 * RTX_ERR_INVALID, before any GPU work: a null ctx, samples == 0, a NaN
 * threshold, max_samples nonzero and below samples, rtx_refined_samples +
 * samples above 2^32 - 1, samples * depth >= 2^32, depth == 0, a per-sample
 * RNG frame. RTX_ERR_STATE: no world or no frame.
 * After a call that left the counts non-uniform, rtx_refine without reset
 * returns RTX_ERR_STATE (continue with rtx_refine_adaptive); rtx_refine_export
 * still copies the state, rtx_refine_import installs a uniform one. Plain
 * renders and rtx_accumulate overwrite the framebuffer only, as for rtx_refine. */
RTX_API float rtx_adaptive_error(const float sum_old[3], uint32_t n_old,
                                 const float sum_new[3], uint32_t n_new);
RTX_API int rtx_refine_adaptive(rtx_ctx *ctx, uint32_t samples, float threshold,
                                uint32_t max_samples, int reset, uint32_t *active);
/* The number of pixels the same call would trace now: the mask only, nothing
 * is traced or changed (a context with no state answers for a fresh one:
 * every pixel). Synchronous. *active must not be NULL. */
RTX_API int rtx_refine_pending(rtx_ctx *ctx, uint32_t samples, float threshold,
                               uint32_t max_samples, uint32_t *active);
/* The count and err maps to host memory (synchronous, like rtx_download):
 * width*height uint32 / float in framebuffer order, bytes == width*height*4.
 * RTX_ERR_STATE if there is no chain state. A uniform state that no adaptive
 * call has touched yet reads as count N and err +inf. */
RTX_API int rtx_refine_counts(rtx_ctx *ctx, uint32_t *host_counts, size_t bytes);
RTX_API int rtx_refine_error(rtx_ctx *ctx, float *host_err, size_t bytes);
/* ---- adaptive refinement of a row part --------------------------------------
 * (later builds, no version bump: probe with dlsym "rtx_refine_adaptive_rows").
 * rtx_refine_adaptive for the rows of `part` of `nparts` (rtx_render_rows'
 * partition): the chain state, count, err and the cost map cover the part's
 * rows in its row order, and the state restarts under rtx_refine_rows' rules
 * (reset, other frame bytes, another shape, a new world). The parts of a
 * frame, each with its own state, hold bit for bit the rows of what
 * rtx_refine_adaptive gives on one context for the same calls — provided each
 * call sees its neighbours' edges: a pixel's 3 x 3 window crosses tile edges.
 *
 * d_halo: device pointer, two planes [2][tiles_of_part][width] fp32. Plane 0,
 * slot j: the err row just below local tile j's first row (the last err row
 * of tile k - 1, k = part + j * nparts); plane 1, slot j: the err row just
 * above its last row (the first err row of tile k + 1). A slot whose row lies
 * outside the image is never read. d_halo may be NULL only when nparts == 1
 * (the rule reads the local map), or when the state is fresh or uniform (every
 * err is +inf, so only max_samples decides; a non-NULL d_halo is not read).
 * rtx_refine_edges writes a state's own edges in the same layout — plane 0
 * each local tile's first err row, plane 1 its last (one row twice for a
 * 1-row tile; the ragged final tile's last row is the image's top row), +inf
 * for a uniform state whose maps are not filled yet — asynchronously on the
 * context stream; d_edges: 2 * tiles * width floats, tiles = the state's
 * ceil(rows / tile_rows) (a whole-frame state: tile_rows 1). The caller moves
 * edge rows into the neighbours' halos (rtx_group_refine_adaptive does).
 *
 * d_out receives the part's rows. Every pixel of the part is written by every
 * call that traces anything: the traced ones by the launch, the others from
 * the state (toGamma(sum / (float)count), w = 1), so whatever overwrote the
 * buffer between two calls does not matter. A call with no active pixel
 * launches no render, leaves the state, the maps and N alone and does not touch
 * d_out. d_out == NULL is allowed only with nparts == 1 and selects the
 * context framebuffer; the call is then exactly rtx_refine_adaptive (inactive
 * pixels untouched). A part that owns no rows returns RTX_OK with *active = 0.
 * RTX_ERR_INVALID, before any HIP call: rtx_refine_adaptive's rules,
 * tile_rows == 0, nparts == 0, part >= nparts, d_out == NULL with nparts > 1,
 * d_halo == NULL where it is needed. RTX_ERR_STATE: no world or no frame. */
RTX_API int rtx_refine_adaptive_rows(rtx_ctx *ctx, uint32_t tile_rows, uint32_t part, uint32_t nparts,
                                     uint32_t samples, float threshold, uint32_t max_samples, int reset,
                                     const void *d_halo, void *d_out, uint32_t *active);
/* rtx_refine_pending for a part: the mask only. *active must not be NULL. */
RTX_API int rtx_refine_pending_rows(rtx_ctx *ctx, uint32_t tile_rows, uint32_t part, uint32_t nparts,
                                    uint32_t samples, float threshold, uint32_t max_samples,
                                    const void *d_halo, uint32_t *active);
/* See above. RTX_ERR_STATE when there is no chain state; RTX_ERR_INVALID for
 * a null argument. */
RTX_API int rtx_refine_edges(rtx_ctx *ctx, void *d_edges);
/* rtx_refine_counts / rtx_refine_error for a state of any shape: bytes == the
 * state's rows * width * 4, in the part's row order (as rtx_refine_export). */
RTX_API int rtx_refine_counts_rows(rtx_ctx *ctx, uint32_t *host_counts, size_t bytes);
RTX_API int rtx_refine_error_rows(rtx_ctx *ctx, float *host_err, size_t bytes);
/* ---- first-hit feature buffers, picking, object-masked refinement ----------
 * (later builds, no version bump: probe with dlsym "rtx_features").
 * What a pixel shows: the first hit of the ray through the pixel's centre.
 * For pixel (x, y) of the current frame, y counted from the bottom row (fp32,
 * in this order, no fma):
 *   u = ((float)x + 0.5f) / (img_w - 1.0f),  v = ((float)y + 0.5f) / (img_h - 1.0f)
 *   origin o = frame.origin,  d = ((lower_left + u*horizontal) + v*vertical) - origin
 * — get_ray's operations (ShaderCompute.hlsl:118-127) without jitter and
 * without a lens offset even when the frame has a lens radius; rng_mode,
 * frame_index and flags do not enter. The hit is the render's hit_world with
 * t_min = 0.001 and t_max = +inf, its record rtx_debug_hit_world's: t, p, the
 * normal flipped to face the ray, front_face, the scene index (the largest
 * index among equal roots, as the reference's scan leaves it). Two planes of
 * float4, rows * width each, row 0 = bottom:
 *   geom  xyz = the record's normal, w = depth;          a miss: (0, 0, 0, +inf)
 *   surf  xyz = the sphere's mat_values rgb, w = (float)index;  a miss: (0, 0, 0, -1)
 * depth = t * sqrt((d.x*d.x + d.y*d.y) + d.z*d.z): the distance in world
 * units (plain fp32 multiplies and adds, a correctly rounded square root).
 * The kernel takes the scan path the render takes for the scene (the layout
 * and layer grid, the culled scan above 1,024 spheres, the linear scan under
 * RTX_SCAN_LINEAR); it reads the world and the frame and writes the planes,
 * nothing else: no stats, no framebuffer, no chain state.
 * rtx_features_rows: the rows of `part` of `nparts` in rtx_render_rows' part
 * order; rtx_features is rtx_features_rows(ctx, 1, 0, 1, ...). Device
 * pointers; either plane may be NULL (skipped). Asynchronous on the context
 * stream. RTX_ERR_INVALID, before any HIP call: a null ctx, both planes NULL,
 * tile_rows == 0, nparts == 0, part >= nparts. RTX_ERR_STATE: no world or no
 * frame. A part without rows returns RTX_OK and launches nothing.
 * With a group, call it on rtx_group_ctx(g, 0): it only reads the world and
 * the frame the group installed there (there is no group entry point). */
RTX_API int rtx_features(rtx_ctx *ctx, void *d_geom, void *d_surf);
RTX_API int rtx_features_rows(rtx_ctx *ctx, uint32_t tile_rows, uint32_t part, uint32_t nparts,
                              void *d_geom, void *d_surf);
/* What is under pixel (x, y): the planes' entry of that pixel, with the
 * record's p and t, the material code as the kernels hold it (RTX_MAT_*; 3: a
 * code that is none of them and scatters nothing) and mat_values.w.
 * Synchronous. A miss: hit = 0, index = -1, depth = +inf, the rest 0.
 * RTX_ERR_INVALID: a null argument, x >= width or y >= height; RTX_ERR_STATE:
 * no world or no frame. */
typedef struct rtx_hit {
    uint32_t hit; int32_t index; uint32_t front_face; uint32_t material;
    float t, depth, p[3], normal[3], albedo[3], mat_param;
    uint32_t reserved[2];
} rtx_hit;
RTX_API int rtx_pick(rtx_ctx *ctx, uint32_t x, uint32_t y, rtx_hit *out);
/* The pixels that show chosen objects. d_surf: a whole-frame surf plane of the
 * current frame's size (device); ids: host array of scene indices,
 * 1 <= n <= 256; grow: 0..8; d_mask: width*height bytes in framebuffer order
 * (device). mask[p] = 1 iff some pixel within Chebyshev distance `grow` of p,
 * inside the image, hit a sphere whose index is in ids; else 0. A miss is
 * never listed (an entry 0xffffffff names no sphere). *set (may be NULL)
 * receives the number of set pixels; the call is synchronous when set is
 * given, else asynchronous on the context stream. RTX_ERR_INVALID, before any
 * HIP call: a null ctx, d_surf, ids or d_mask, n == 0, n > 256, grow > 8;
 * RTX_ERR_STATE: no frame. */
RTX_API int rtx_mask_from_ids(rtx_ctx *ctx, const void *d_surf, const uint32_t *ids, uint32_t n,
                              uint32_t grow, void *d_mask, uint32_t *set);
/* rtx_refine_adaptive with the "noisy" test replaced by the caller's mask
 * (width*height bytes in framebuffer order, device; rtx_mask_from_ids writes
 * one): pixel p is traced iff mask[p] != 0 and (max_samples == 0 or
 * count_p + samples <= max_samples). Everything else is rtx_refine_adaptive's
 * contract: the count / err maps are filled from a uniform state (count N,
 * err +inf); each traced pixel's sum, seed, count, E, cost-map entry and
 * framebuffer value are updated, every other pixel is untouched; one scheduled
 * launch keyed by the cost map (rtx_refine_last_keys: CARRIED); no active
 * pixel launches nothing; rtx_refined_samples advances only when something was
 * traced; rtx_stats.samples counts active * samples. Whole frame only: it
 * continues an existing whole-frame chain state for the current world and
 * frame (from rtx_refine, rtx_refine_adaptive or rtx_refine_import) and never
 * starts one. RTX_ERR_INVALID, before any HIP call: a null ctx or mask, and
 * rtx_refine_adaptive's argument rules (samples == 0, max_samples nonzero and
 * below samples, rtx_refined_samples + samples above 2^32 - 1,
 * samples * depth >= 2^32, depth == 0, a per-sample RNG frame). RTX_ERR_STATE,
 * before any HIP call: no world, no frame, no chain state for them, or a part
 * state. Afterwards the counts are non-uniform: rtx_refine without reset
 * refuses as after adaptive steps; rtx_refine_adaptive continues from the maps. */
RTX_API int rtx_refine_masked(rtx_ctx *ctx, uint32_t samples, const void *d_mask,
                              uint32_t max_samples, uint32_t *active);
/* ---- batched closest-hit ray queries ----------------------------------------
 * (later builds, no version bump: probe with dlsym "rtx_cast_rays").
 * What n rays of the caller's choosing hit in the uploaded world: the render's
 * hit_world for every ray, each over its own range (t_min, t_max_i). d_rays
 * (n rtx_ray), d_hits (n rtx_ray_hit) and d_occluded (n bytes) are device
 * pointers; either output may be NULL, not both; the buffers must not overlap.
 * Asynchronous on the context stream. Reads the world and needs no frame.
 * Ray i: if !(t_max_i >= t_min) — a NaN, negative or too short t_max — it
 * misses without being scanned. Otherwise its record is rtx_debug_hit_world's
 * for that ray with (t_min, t_max_i), in every scan form the context selects
 * for the scene (the layout and layer grid, the culled scan above 1,024
 * spheres, the linear scan under RTX_SCAN_LINEAR): the reference's in-order
 * hit_world, the largest index among equal roots, a NaN ray "hitting" sphere
 * count - 1 with t = NaN.
 *   hit:   t, index, the normal flipped to face the ray, front_face (1 / 0),
 *          reserved 0
 *   miss:  t = +inf, index = -1, the rest 0
 *   occluded[i] = (index >= 0)
 * The hit point is not stored: o + t * d, one multiply then one add per
 * component, is the record's p. `tag` is the caller's and is ignored.
 * `order` is a schedule and nothing else; no record depends on it:
 *   GIVEN     lane i of the kernel casts ray i: a wave scans the union of its
 *             64 rays' candidate blocks, so rays that are neighbours in space
 *             should be neighbours in the buffer
 *   COHERENT  the rays are first sorted by a coarse key of their origin and
 *             direction (three small passes on the context's own scratch,
 *             which grows when a call needs more), and lane i casts the i-th
 *             ray of that order
 *   AUTO      one of the two, by the batch size and the scene's class
 * rtx_cast_last_order: what the last call ran, GIVEN or COHERENT (AUTO
 * resolved); GIVEN before any call.
 * RTX_ERR_INVALID, before any HIP call and before the context is looked at: a
 * null ctx; n > 0 with d_rays NULL or both outputs NULL; t_min not finite or
 * <= 0; an unknown order. RTX_ERR_STATE: no world. n == 0 returns RTX_OK and
 * launches nothing. The call touches nothing else: no stats, no framebuffer,
 * no chain state, no cost map. With a group, call it on rtx_group_ctx(g, 0),
 * as rtx_features. */
typedef struct rtx_ray     { float o[3]; float t_max; float d[3]; uint32_t tag; } rtx_ray;        /* 32 B */
typedef struct rtx_ray_hit { float t; int32_t index; float normal[3]; uint32_t front_face;
                             uint32_t reserved[2]; } rtx_ray_hit;                                  /* 32 B */
enum { RTX_CAST_ORDER_AUTO = 0, RTX_CAST_ORDER_GIVEN = 1, RTX_CAST_ORDER_COHERENT = 2 };
RTX_API int rtx_cast_rays(rtx_ctx *ctx, const void *d_rays, uint32_t n, float t_min, uint32_t order,
                          void *d_hits, void *d_occluded);
RTX_API int rtx_cast_last_order(rtx_ctx *ctx);   /* GIVEN or COHERENT: what the last call ran; AUTO resolved */
/* ---- the chain seed of a pixel ------------------------------------------------
 * (later builds, no version bump: probe with dlsym "rtx_path_seed").
 * Host, no GPU, no context. The seed pixel (x, y)'s RNG chain starts from in
 * a chain-mode frame with frame_index f: (float)h / 4294967296.0f, where h =
 * base_hash(x, y) and, for f != 0, then h = base_hash(h, 0x80000000 | f) (the
 * rule of the render's first sample and of rtx_refine's chain state, whose w
 * is this seed advanced by the samples taken).
 * What it is for: in a frame whose horizontal and vertical rows and lens are
 * zero, every pixel starts every sample on the one ray (origin, fl(lower_left -
 * origin)), whatever the jitter, and (x, y) enters through this seed alone. So
 * "what does the ray (o, d) see, with the random numbers of pixel (x, y)" is
 * pixel (x, y) of rtx_render_sum in the frame with origin = o, lower_left = L
 * where fl(L - o) == d, zero horizontal and vertical, any img_w, img_h != 1 —
 * the zero-film twin of a path query. */
RTX_API float rtx_path_seed(uint32_t x, uint32_t y, uint32_t frame_index);
/* ---- what a ray sees: path queries along rays of the caller's choosing ---------
 * (later builds, no version bump: probe with dlsym "rtx_trace_paths").
 * For each of n queries (o, d, seed): `samples` samples of the reference's
 * ray_color along the ray — bounces, materials, sky — with the random numbers
 * of the RNG chain that starts at `seed`, to the uploaded world's depth.
 * d_queries (n rtx_path_query), d_results (n rtx_path_result) and d_segments
 * (n uint32, or NULL) are device pointers; overlapping buffers are the
 * caller's business. Asynchronous on the context stream. Reads the world and
 * needs no frame; touches no stats, framebuffer, chain state or cost map. With
 * a group, call it on rtx_group_ctx(g, 0), as rtx_cast_rays.
 * The contract: query i with ray (o, d) and seed = rtx_path_seed(x, y, f)
 * gives, bit for bit (NaN sums included), pixel (x, y) of rtx_render_sum in
 * the zero-film twin frame of (o, d) (rtx_path_seed above) with frame_index f,
 * world.spp = samples, and RTX_FRAME_LAMBERT_GUARD set iff
 * RTX_PATHS_LAMBERT_GUARD is.
 *   result.sum   the linear sum of the samples' colours (divide by the number
 *                of samples taken for the mean)
 *   result.seed  the chain's seed after the last sample: with sum, the pixel's
 *                chain state as rtx_refine keeps it (rtx_refine_export's w)
 *   d_segments[i]  the hit_world calls this call spent on query i
 * `tag` is the caller's and is ignored.
 * RTX_PATHS_CONTINUE: query i starts from d_results[i] (sum and seed) instead
 * of (0, query.seed), whose seed is then not read: `samples` = s1 followed by
 * a continuing call with s2 equals one call with s1 + s2, bit for bit;
 * d_segments holds the continuing call's own segments.
 * `order` (RTX_CAST_ORDER_*) is a schedule and nothing else, as in
 * rtx_cast_rays, whose COHERENT passes and scratch it uses; only a query's
 * first segment follows the batch's order, so AUTO is GIVEN.
 * rtx_paths_last_order: what the last call ran; GIVEN before any call.
 * One kernel lane traces one query from its first sample to its last: a
 * wave takes as long as its longest query, so give neighbouring queries
 * similar work where there is a choice.
 * RTX_ERR_INVALID, before any HIP call and before the context is looked at: a
 * null ctx; n > 0 with d_queries or d_results NULL; samples == 0; unknown flag
 * bits; an unknown order. RTX_ERR_STATE: no world. RTX_ERR_INVALID once the
 * world is known: its depth is 0, or samples * depth >= 2^32. n == 0 returns
 * RTX_OK and launches nothing. */
typedef struct rtx_path_query  { float o[3]; float seed; float d[3]; uint32_t tag; } rtx_path_query;   /* 32 B */
typedef struct rtx_path_result { float sum[3]; float seed; } rtx_path_result;                          /* 16 B */
enum { RTX_PATHS_LAMBERT_GUARD = 1, RTX_PATHS_CONTINUE = 2 };
RTX_API int rtx_trace_paths(rtx_ctx *ctx, const void *d_queries, uint32_t n, uint32_t samples,
                            uint32_t flags, uint32_t order, void *d_results, void *d_segments);
RTX_API int rtx_paths_last_order(rtx_ctx *ctx);  /* GIVEN or COHERENT: what the last call ran */
/* ---- path queries in cost order -----------------------------------------------
 * (later builds, no version bump: probe with dlsym "rtx_trace_paths_keyed").
 * rtx_trace_paths with the schedule chosen by keys: every record — sum, end
 * seed, and the call's own segment count per query, NaN sums included,
 * RTX_PATHS_CONTINUE and RTX_PATHS_LAMBERT_GUARD honoured — is bit for bit
 * what rtx_trace_paths(ctx, d_queries, n, samples, flags, RTX_CAST_ORDER_GIVEN,
 * d_results, d_segments) writes. The order is a schedule and nothing else: the
 * longest queries first, so that the 64 lanes of a wave hold queries of
 * similar length. Asynchronous on the context stream; needs no frame; touches
 * no stats, framebuffer, chain state or cost map.
 * d_keys != NULL: n uint32 on the device, and probe must be 0. Lane g of the
 * one launch takes the g-th query in non-increasing order of min(key, 65535);
 * the order among equal keys is unspecified (a workgroup's queries of one key
 * stay together). d_keys may be d_segments: the keys are copied to the
 * context's scratch before the trace is enqueued, so "order this step by the
 * segments the last step wrote" works in place.
 * d_keys == NULL: the library probes. p = probe, or with probe == 0 the
 * default: 2, or 1 for a world of more than 1,024 spheres after padding. With
 * samples <= p the call is one plain launch in the given order. Otherwise p
 * samples run in the given order, their segment counts are the keys, and the
 * remaining samples - p follow in cost order as a continuing call;
 * d_segments[i] is the whole call's count.
 * rtx_paths_last_order returns RTX_PATHS_ORDER_COST after a call that sorted
 * and GIVEN after a samples <= p call. rtx_trace_paths itself still refuses
 * order 3.
 * rtx_debug_paths_order: the permutation the last sorted keyed call used, to
 * host memory (synchronous; bytes == n * 4). RTX_ERR_STATE when the last path
 * call did not sort by cost, or when a later rtx_cast_rays or COHERENT path
 * call has reused the scratch; RTX_ERR_INVALID for a null argument or a wrong
 * bytes.
 * RTX_ERR_INVALID, before any HIP call and before the context is looked at,
 * first failure first: a null ctx; n > 0 with d_queries NULL, then with
 * d_results NULL; samples == 0; unknown flag bits; d_keys != NULL with
 * probe != 0. RTX_ERR_STATE: no world. RTX_ERR_INVALID once the world is
 * known: its depth is 0, or samples * depth >= 2^32. n == 0 returns RTX_OK and
 * launches nothing. */
enum { RTX_PATHS_ORDER_COST = 3 };   /* reported by rtx_paths_last_order; rtx_trace_paths still refuses order 3 */
RTX_API int rtx_trace_paths_keyed(rtx_ctx *ctx, const void *d_queries, uint32_t n, uint32_t samples,
                                  uint32_t flags, const void *d_keys, uint32_t probe,
                                  void *d_results, void *d_segments);
RTX_API int rtx_debug_paths_order(rtx_ctx *ctx, uint32_t *host_perm, size_t bytes);
/* ---- film queries: path queries with a per-sample film footprint ---------------
 * (later builds, no version bump: probe with dlsym "rtx_trace_film").
 * rtx_trace_paths starts every sample of a query on one fixed ray. A film
 * query is a pixel of a frame of its own: the record carries that frame's
 * origin o, lower-left corner L, horizontal and vertical rows H and V, the
 * pixel's coordinates (fx, fy) and the seed of its RNG chain; img_w and img_h
 * are the call's. Every sample starts as the render's does, in fp32, in this
 * order, without fused multiply-adds:
 *   hash2(seed) -> h0, _ ;  u = (fx + h0 * 1.1f) / (img_w - 1.0f)
 *   hash2(seed) -> _, g1 ;  v = (fy + g1 * 1.1f) / (img_h - 1.0f)
 *   o' = o ;  d = ((L + u * H) + v * V) - o
 *   with RTX_FILM_LENS and lens_r > 0:
 *     rd = lens_r * random_in_unit_disk(seed); off = rd.x * lens_u + rd.y * lens_v;
 *     o' = o' + off; d = d - off
 * and is from there a sample of rtx_trace_paths along (o', d).
 * The contract: query i with fx = (float)x, fy = (float)y (x, y < 2^24) and
 * seed = rtx_path_seed(x, y, f) gives, bit for bit (NaN sums included), pixel
 * (x, y) of rtx_render_sum in the frame {origin o, lower_left L, horizontal H,
 * vertical V, img_w, img_h, lens_u = (lens_u, lens_r), lens_v, chain RNG,
 * frame_index f}, world.spp = samples, RTX_FRAME_LAMBERT_GUARD set iff
 * RTX_PATHS_LAMBERT_GUARD is. So it renders any subset of a frame's pixels, in
 * any order, at the cost of those pixels; and with one frame per record it
 * renders cameras that are no pinhole:
 *   H = V = 0 without a lens is rtx_trace_paths' query (o, fl(L - o), seed).
 *   The unit form: fx = fy = 0 with img_w = img_h = 2 gives u = h0 * 1.1f and
 *   v = g1 * 1.1f exactly; L is then the footprint's corner and H, V its
 *   edges divided by 1.1 (rtx_film_camera writes such records).
 * img_w, img_h, fx, fy and the vectors are not checked (rtx_set_frame checks
 * none either): whatever the arithmetic gives is the answer.
 * d_queries: n rtx_film_query (64 B), or with RTX_FILM_LENS n
 * rtx_film_lens_query (96 B; a record with lens_r <= 0 has no lens, record by
 * record). d_results (n rtx_path_result), d_segments (n uint32, or NULL),
 * RTX_PATHS_CONTINUE and RTX_PATHS_LAMBERT_GUARD: as in rtx_trace_paths.
 * Device pointers; asynchronous on the context stream; needs no frame; touches
 * no stats, framebuffer, chain state or cost map. `tag` is the caller's.
 * `order` is a schedule and nothing else: RTX_CAST_ORDER_AUTO and _GIVEN run
 * lane g on query g; RTX_PATHS_ORDER_COST is rtx_trace_paths_keyed's probe (the
 * first 2 samples, or 1 for a world of more than 1,024 spheres after padding,
 * in the given order; the rest in non-increasing order of their segment
 * counts; with samples <= that probe, one plain launch). RTX_CAST_ORDER_COHERENT
 * is refused: its key pass reads a direction where a film record holds L.
 * rtx_film_last_order: GIVEN or RTX_PATHS_ORDER_COST, what the last call ran;
 * GIVEN before any call. A film call that sorts reuses the scratch of
 * rtx_debug_paths_order, which then returns RTX_ERR_STATE.
 * The image of a batch: d_results is a row of linear sums, so
 * rtx_fold_frames(ctx, zeroed accum, d_results, 1, n, n, samples, d_image)
 * gives toGamma(sum / samples).
 * RTX_ERR_INVALID, before any HIP call and before the context is looked at,
 * first failure first: a null ctx; n > 0 with d_queries NULL, then with
 * d_results NULL; samples == 0; unknown flag bits; COHERENT or an unknown
 * order. RTX_ERR_STATE: no world. RTX_ERR_INVALID once the world is known: its
 * depth is 0, or samples * depth >= 2^32. n == 0 returns RTX_OK and launches
 * nothing. */
typedef struct rtx_film_query      { float o[3], seed, lower_left[3]; uint32_t tag;
                                     float horizontal[3], fx, vertical[3], fy; } rtx_film_query;       /* 64 B */
typedef struct rtx_film_lens_query { rtx_film_query q; float lens_u[3], lens_r, lens_v[3];
                                     uint32_t reserved; } rtx_film_lens_query;                          /* 96 B */
enum { RTX_FILM_LENS = 4 };   /* with RTX_PATHS_LAMBERT_GUARD = 1 and RTX_PATHS_CONTINUE = 2 */
RTX_API int rtx_trace_film(rtx_ctx *ctx, const void *d_queries, uint32_t n, uint32_t samples,
                           float img_w, float img_h, uint32_t flags, uint32_t order,
                           void *d_results, void *d_segments);
RTX_API int rtx_film_last_order(rtx_ctx *ctx);   /* GIVEN or RTX_PATHS_ORDER_COST: what the last call ran */
/* Host, no GPU, no context: the film records of the n listed pixels (xs[i],
 * ys[i]) of a frame, values copied, fx = (float)x, fy = (float)y, seed =
 * rtx_path_seed(x, y, frame_index), tag 0; *img_w and *img_h (either may be
 * NULL) receive the frame's. lens != 0 writes rtx_film_lens_query records with
 * the frame's lens_u, lens radius and lens_v. RTX_ERR_INVALID: a null frame or
 * (n > 0) list or buffer; a frame with rng_mode RTX_RNG_PER_SAMPLE; lens == 0
 * for a frame whose lens radius is > 0; a pixel outside width x height. The
 * frame's own frame_index and flags are not read. */
RTX_API int rtx_film_from_frame(const rtx_frame *frame, const uint32_t *xs, const uint32_t *ys, uint32_t n,
                                uint32_t frame_index, void *host_queries, int lens,
                                float *img_w, float *img_h);
/* Host, no GPU, no context: width * height unit-form records (trace them with
 * img_w = img_h = 2), one per pixel, record y * width + x, row 0 at the
 * bottom, of a camera at `from` looking at `at`: forward w = normalize(at -
 * from), right u = normalize(cross(w, vup)), up v = cross(u, w). With c(x, y)
 * the model's unit direction at pixel corner (x, y), in double: L = o + c(x,
 * y), H = (c(x + 1, y) - c(x, y)) / 1.1, V = (c(x, y + 1) - c(x, y)) / 1.1,
 * each rounded once; seed = rtx_path_seed(x, y, frame_index).
 *   RTX_FILM_EQUIRECT  longitude (x / width - 0.5) * 2 pi over the width (0:
 *       forward, positive to the right), latitude (y / height - 0.5) * pi over
 *       the height; c = cos(lat) sin(lon) u + sin(lat) v + cos(lat) cos(lon) w.
 *       fov_deg is unused.
 *   RTX_FILM_FISHEYE   equidistant, fov_deg (0 < fov <= 360) across the
 *       shorter side: p = ((x, y) - (width, height) / 2) / (min(width, height)
 *       / 2), r = |p|, theta = r * fov / 2, c = sin(theta) (p.x u + p.y v) / r
 *       + cos(theta) w. A pixel with a corner outside the image circle (r > 1)
 *       gets a zero direction (L = o, H = V = 0): every root of such a ray
 *       is NaN, each sample ends black at the world's depth, and the query
 *       returns the sum (0, 0, 0) with `depth` segments per sample — black
 *       in the image (an empty world has no root: there the sky colour of a
 *       zero direction is NaN).
 * RTX_ERR_INVALID: a null pointer, an unknown model, width or height 0 or
 * width * height >= 2^32, a fisheye fov outside (0, 360], from == at or vup
 * parallel to the view direction. */
enum { RTX_FILM_EQUIRECT = 0, RTX_FILM_FISHEYE = 1 };
RTX_API int rtx_film_camera(int model, const float from[3], const float at[3], const float vup[3],
                            float fov_deg, uint32_t width, uint32_t height, uint32_t frame_index,
                            rtx_film_query *host_queries);
/* Device pointer of the chain state (width*height float4; a part state: its
 * rows * width), NULL if none. */
RTX_API void *rtx_refine_state(rtx_ctx *ctx);
/* The chain state to host memory (synchronous, like rtx_download):
 * bytes == width*height*16 (a part state, rtx_refine_rows: its rows * width *
 * 16, in the part's row order; rtx_refine_shape names the part);
 * RTX_ERR_STATE if there is no state. With
 * rtx_refined_samples it is all a later session needs to resume. */
RTX_API int rtx_refine_export(rtx_ctx *ctx, float *host_state, size_t bytes);
/* Installs a chain state with N = samples (>= 1) for the current world and
 * frame (both needed; bytes == width*height*16) and writes the framebuffer
 * from it, toGamma(sum / (float)samples): a resumed session shows its image
 * before it traces anything. The next rtx_refine continues from it.
 * Synchronous. Whether the state belongs to this world and frame is the
 * caller's business (rtx_app.hpp's state file checks it). */
RTX_API int rtx_refine_import(rtx_ctx *ctx, const float *host_state, size_t bytes,
                              uint32_t samples);
/* Rows owned by `part` (host arithmetic, no GPU). */
RTX_API uint32_t rtx_part_rows(uint32_t height, uint32_t tile_rows, uint32_t part,
                               uint32_t nparts);
/* Gathered buffer [nparts][max_rows][width] (each part's rows, padded to
 * the largest part) -> image [height][width] in global row order. Device
 * pointers; asynchronous on the context stream. */
RTX_API int rtx_deinterleave_rows(rtx_ctx *ctx, const void *d_gathered,
                                  uint32_t width, uint32_t height,
                                  uint32_t tile_rows, uint32_t nparts,
                                  void *d_image);
/* Wait for all work on the context stream (~ the implicit sync of Present,
 * DxCSApp.cpp:551); RTX_ERR_INCOMPLETE if a launch left pixels unwritten. */
RTX_API int rtx_sync(rtx_ctx *ctx);
/* Device pointer of the context framebuffer (width*height float4) or NULL. */
RTX_API void *rtx_framebuffer(rtx_ctx *ctx);
/* Copy the context framebuffer to host memory (synchronous). The reference
 * never reads results back; this is the image-output contract (§8f-1). */
RTX_API int rtx_download(rtx_ctx *ctx, float *host_rgba, size_t bytes);

/* ---- one frame across several devices -------------------
 * A group owns n contexts ("members"), their buffers and the gather, in one
 * process driven by one host thread. Member i renders part i of n of
 * rtx_render_rows' partition; member 0 is the root: it holds the gathered
 * buffer [n][max_rows][width] and the image [height][width] on its device.
 * `devices` is either all distinct (one member per GPU) or all equal (a
 * rehearsal of the same partition, buffers and assembly on one GPU: the
 * members then share the root member's stream, so their renders run one after
 * another — the render is a persistent kernel sized to the device's resident
 * waves and two of them must not compete for it). Anything else, n == 0,
 * n > RTX_GROUP_MAX, a null pointer, a negative device or an unknown mode is
 * RTX_ERR_INVALID, decided before any HIP call.
 * Transport of the gather:
 *   RTX_GATHER_COPY  the root's stream waits for each member's "rendered"
 *                    event and pulls its rows (hipMemcpyPeerAsync; a
 *                    device-to-device copy on one device). Any valid list.
 *   RTX_GATHER_RCCL  one ncclGroupStart/End of every other member's ncclSend
 *                    (on its own stream) and the root's ncclRecv into the
 *                    gathered slots. Needs distinct devices. RCCL is loaded at
 *                    run time (dlopen "librccl.so.1": the library itself does
 *                    not link it); a failed load is RTX_ERR_STATE with the
 *                    loader's message.
 *   RTX_GATHER_AUTO  RCCL for members on more than one device, else copies
 *                    (one member: it renders straight into the image).
 * The image equals the one-context frame bit for bit (the seed depends only
 * on the global pixel). Not thread-safe, like a context. */
typedef struct rtx_group rtx_group;
enum { RTX_GATHER_AUTO = 0, RTX_GATHER_RCCL = 1, RTX_GATHER_COPY = 2 };
#define RTX_GROUP_MAX 64

RTX_API int rtx_group_create(const int *devices, uint32_t n, int gather_mode, rtx_group **out);
RTX_API void rtx_group_destroy(rtx_group *g);
/* Members (0 for NULL). */
RTX_API uint32_t rtx_group_size(rtx_group *g);
/* Member's context, borrowed: for its schedule, scan mode (before
 * rtx_group_upload_world), stats and refine keys (rtx_refine_set_keys: what
 * orders its rtx_group_refine launches). Its stream, world, frame and chain
 * state belong to the group. NULL if out of range. */
RTX_API rtx_ctx *rtx_group_ctx(rtx_group *g, uint32_t member);
/* The transport in use: RTX_GATHER_RCCL or RTX_GATHER_COPY (AUTO resolved). */
RTX_API int rtx_group_gather_mode(rtx_group *g);
/* ncclGetVersion's code of the RCCL the group loaded, 0 if it loaded none. */
RTX_API int rtx_group_rccl_version(rtx_group *g);
/* rtx_upload_world / rtx_set_frame on every member. */
RTX_API int rtx_group_upload_world(rtx_group *g, const rtx_world *w);
RTX_API int rtx_group_set_frame(rtx_group *g, const rtx_frame *f);
/* Every member's rows (tiles of tile_rows rows; a member that owns none
 * launches nothing), the gather, then the de-interleave on the root's
 * stream. Asynchronous: no host wait once the buffers fit the frame size and
 * tile_rows (they are resized like the context framebuffer when those change). */
RTX_API int rtx_group_render(rtx_group *g, uint32_t tile_rows);
/* Wait for every member. The first failing member's error (RTX_ERR_INCOMPLETE
 * included) is returned, its index in rtx_last_error(). */
RTX_API int rtx_group_sync(rtx_group *g);
/* Device pointer of the image (width*height float4) on member 0's device, or
 * NULL before the first rtx_group_render. */
RTX_API void *rtx_group_image(rtx_group *g);
/* rtx_group_sync, then the image to host memory. */
RTX_API int rtx_group_download(rtx_group *g, float *host_rgba, size_t bytes);
/* HIP-event times of the last frame (rendered by rtx_group_render or refined
 * by rtx_group_refine), after rtx_group_sync / _download:
 * render_ms[n] each member's render (0 for a member without rows), the gather
 * and the de-interleave on the root's stream. NULL outputs are skipped.
 * Members sharing a device run one after another: their times add up and say
 * nothing about scaling. */
RTX_API int rtx_group_get_times(rtx_group *g, double *render_ms, double *gather_ms,
                                double *deinterleave_ms);
/* Progressive accumulation with whole frames dealt to the members (the row
 * split above serves one frame's latency; this serves the throughput of a
 * converged image: a frame's seeds depend on (pixel, frame_index) only, so
 * frames are independent). Adds `frames` frames to the group's accumulator and
 * writes the image. With F frames accumulated so far, frame j of the call
 * (j = 0 .. frames-1) has frame_index F + j and goes to member j % n: a call
 * always starts at member 0, so the root renders in every round. The call runs
 * in rounds of up to n frames. In a round each taking member renders its
 * frame's sums with rtx_render_sum — the root straight into slot 0 of a
 * root-side buffer [n][width*height], the others into one sum buffer each,
 * gathered into their slots by the group's transport (stream-ordered copies /
 * hipMemcpyPeerAsync, or one ncclGroupStart/End of send/recv) — and one
 * rtx_fold_frames of the round's m sums (member order = frame order) follows
 * on the root's stream with divisor (frames accumulated after the round) * spp.
 * A member past the call's last frame launches nothing in that round. A
 * member's sum buffer is reused by the next round only after the gather that
 * read it (copies: its stream waits for the gather's end event; RCCL: the send
 * is ordered on its stream).
 * Asynchronous like rtx_group_render: no host wait once the buffers fit the
 * frame size. Afterwards rtx_group_image / rtx_group_download give the image;
 * it equals F + frames calls of rtx_accumulate on one context bit for bit.
 * reset != 0, a first call, or a frame size other than the accumulator's
 * restarts at F = 0 (the accumulator is zeroed), as rtx_accumulate does.
 * rtx_group_render between two calls overwrites the image but not the
 * accumulator: the next call continues and rewrites the image.
 * RTX_ERR_INVALID before any HIP call: a null group, frames == 0, spp == 0,
 * F + frames > 0x7fffffff (the seed uses 0x80000000 | frame_index), or
 * (F + frames) * spp not representable in uint32 (the fold's divisor). No
 * frame set or no world uploaded is RTX_ERR_STATE. F advances by the rounds
 * whose fold was enqueued; a failing member's error is returned with its index. */
RTX_API int rtx_group_accumulate(rtx_group *g, uint32_t frames, int reset);
/* Frames in the group's accumulator (0 for NULL). */
RTX_API uint32_t rtx_group_accumulated_frames(rtx_group *g);
/* HIP-event times of the LAST round of the last rtx_group_accumulate, after
 * rtx_group_sync: render_ms[n] (0 for a member that rendered nothing in it),
 * the gather and the fold on the root's stream. NULL outputs are skipped. */
RTX_API int rtx_group_get_accumulate_times(rtx_group *g, double *render_ms, double *gather_ms,
                                           double *fold_ms);
/* Progressive refinement along the reference's RNG chain across the members
 * (later builds, no version bump: probe with dlsym "rtx_group_refine"). A
 * pixel's chain is sequential, so frames cannot be dealt to members as
 * rtx_group_accumulate does; the row split is exact, because the seed depends
 * only on the global pixel. Each member that owns rows runs
 * rtx_refine_rows(ctx_i, tile_rows, i, n, samples, fresh, d_out_i) — its chain
 * state covers its own rows — into the buffers of rtx_group_render, followed
 * by the same gather and de-interleave (a one-member group with copies refines
 * straight into the image). Asynchronous like rtx_group_render. After calls
 * adding s1..sk rtx_group_image is bit for bit (NaN included) what rtx_refine
 * gives on one context, so what rtx_render gives at spp = s1 + ... + sk.
 * The group decides freshness itself and passes it to every member: its state
 * restarts at N = 0 on reset != 0, a first call, a tile_rows other than the
 * state's, rtx_group_upload_world, and rtx_group_set_frame with other bytes.
 * Before it launches anything the group checks that every row-owning member's
 * rtx_refined_samples and rtx_refine_shape agree with its own N and shape: a
 * mismatch (someone refined through a borrowed rtx_group_ctx) is RTX_ERR_STATE
 * naming the member. If a member's launch fails after earlier members were
 * enqueued, N becomes 0 (the next call restarts everyone) and the error
 * carries the member's index. rtx_group_render and rtx_group_accumulate between
 * two calls overwrite the image, not the states.
 * RTX_ERR_INVALID, before any HIP call: a null group, samples == 0,
 * tile_rows == 0, a per-sample-RNG frame, N + samples above 2^32 - 1.
 * RTX_ERR_STATE: no frame or no world. */
RTX_API int rtx_group_refine(rtx_group *g, uint32_t samples, uint32_t tile_rows, int reset);
/* N of the group's chain state (0 for NULL / none). */
RTX_API uint32_t rtx_group_refined_samples(rtx_group *g);
/* The group's chain state as ONE whole-frame state, [height][width] float4 in
 * framebuffer order, bytes == width*height*16: byte for byte what
 * rtx_refine_export gives on one context at the same N, so one state (file)
 * moves between a context and a group of any size and tile_rows. Synchronous.
 * RTX_ERR_STATE: no state, or a member that disagrees with the group. */
RTX_API int rtx_group_refine_export(rtx_group *g, float *host_state, size_t bytes);
/* The inverse: every member receives its rows (rtx_refine_import_rows), its
 * image rows go into its slot, then the gather and the de-interleave run: the
 * image is there before anything is traced, and N = samples with this
 * tile_rows. Synchronous. Errors as rtx_group_refine, and RTX_ERR_INVALID for
 * a null host_state or other bytes. */
RTX_API int rtx_group_refine_import(rtx_group *g, uint32_t tile_rows, const float *host_state,
                                    size_t bytes, uint32_t samples);
/* Adaptive refinement across the members (later builds, no version bump: probe
 * with dlsym "rtx_refine_adaptive_rows"): rtx_refine_adaptive with the rows
 * split as in rtx_group_refine. The image, the counts, the errors and the
 * chain state are bit for bit what rtx_refine_adaptive gives on one context
 * for the same calls, whatever n and tile_rows. Two phases from the calling
 * thread. Phase 1: every row-owning member packs its tiles' edge rows of err
 * (rtx_refine_edges), the edge rows travel into the neighbours' halo buffers
 * (stream-ordered copies on one device, hipMemcpyPeerAsync ordered by events
 * between devices, one ncclGroupStart/End of send/recv in an RCCL group), every
 * member computes its mask (rtx_refine_pending_rows) and *active (may be NULL)
 * receives the sum. If that is 0 nothing else happens: N, the image, the
 * states and the maps stay. Phase 2: every member with active pixels launches
 * (rtx_refine_adaptive_rows) into its slot; a member with rows but no active
 * pixel launches no render, writes its current rows from its state, and keeps
 * its own N; the usual gather and de-interleave follow. The call is
 * synchronous up to the masks' 4-byte readbacks, asynchronous after.
 * Freshness is the group's decision, as in rtx_group_refine; a fresh call
 * traces every pixel without an exchange. rtx_group_refined_samples is the sum
 * of the steps that traced anything. The group remembers each member's N and
 * refuses (RTX_ERR_STATE, naming the member) when one was refined through
 * rtx_group_ctx. After a call that left the counts non-uniform,
 * rtx_group_refine without reset returns RTX_ERR_STATE (continue with
 * rtx_group_refine_adaptive); rtx_group_refine_export still copies the sums
 * and seeds, rtx_group_refine_import installs a uniform state.
 * rtx_group_render between two calls overwrites the image, not the states.
 * RTX_ERR_INVALID, before any HIP call: a null group, rtx_refine_adaptive's
 * argument rules, tile_rows == 0. RTX_ERR_STATE: no frame or no world. */
RTX_API int rtx_group_refine_adaptive(rtx_group *g, uint32_t samples, float threshold,
                                      uint32_t max_samples, uint32_t tile_rows, int reset,
                                      uint32_t *active);
/* Phase 1 alone: the number of pixels the same call would trace now.
 * *active must not be NULL. */
RTX_API int rtx_group_refine_pending(rtx_group *g, uint32_t samples, float threshold,
                                     uint32_t max_samples, uint32_t tile_rows, uint32_t *active);
/* The members' count and err maps as whole-frame maps in framebuffer order,
 * bytes == width*height*4 (what rtx_refine_counts / rtx_refine_error give on
 * one context). Synchronous. RTX_ERR_STATE without a chain state. */
RTX_API int rtx_group_refine_counts(rtx_group *g, uint32_t *host_counts, size_t bytes);
RTX_API int rtx_group_refine_error(rtx_group *g, float *host_err, size_t bytes);

/* ---- device buffers (for callers without their own allocator) ----------
 * Ordered on the context stream; copies are synchronous. d_ptr from
 * rtx_alloc may be passed as d_out / d_gathered / d_image above. */
RTX_API int rtx_alloc(rtx_ctx *ctx, size_t bytes, void **d_ptr);
RTX_API int rtx_free(rtx_ctx *ctx, void *d_ptr);
RTX_API int rtx_copy_to_host(rtx_ctx *ctx, void *host, const void *d_src, size_t bytes);
RTX_API int rtx_copy_to_device(rtx_ctx *ctx, void *d_dst, const void *host, size_t bytes);

/* ---- measurement ------------------------------------------------------ */
RTX_API int rtx_stats_reset(rtx_ctx *ctx);
/* Synchronises the stream, then reports counters since the last reset. */
RTX_API int rtx_get_stats(rtx_ctx *ctx, rtx_stats *out);

/* ---- host-side producers (no GPU) ----------------------------------------
 * WorldDef::random_world (DxCSApp.cpp:72-134) with MSVC rand() (unseeded,
 * DxCSApp.cpp:6-9) emulated bit-exactly. grid_half_extent 9 = reference
 * (326 spheres), 11 = RTIOW final scene (486). At most `capacity` spheres
 * are written (the generator stops there); *count receives the number
 * written. Arrays: spheres 4*capacity, mat_types capacity, mat_values
 * 4*capacity. */
RTX_API int rtx_scene_random_world(int32_t grid_half_extent, uint32_t capacity,
                                   float *spheres, float *mat_types,
                                   float *mat_values, uint32_t *count);
/* WorldDef::test_world (DxCSApp.cpp:136-157): 4 spheres. */
RTX_API int rtx_scene_test_world(float *spheres, float *mat_types,
                                 float *mat_values, uint32_t *count);
/* The pixel-shader prototype's scene (Shader_RT.fx:300-335): 7 spheres
 * (ground, 3 small Lambert, glass, Lambert, metal); arrays of capacity 7. */
RTX_API int rtx_scene_ps_world(float *spheres, float *mat_types,
                               float *mat_values, uint32_t *count);
/* PerFrame::ComputeViewVals (DxCSApp.cpp:39-61) + the focus distance of
 * DxCSApp::Update (DxCSApp.cpp:488) with focus_dist <= 0 meaning
 * |from - at|. Fills the four view rows, img_w = width_px,
 * img_h = width_px / aspect (ShaderCompute.hlsl:294) and width/height. */
RTX_API int rtx_camera_look_at(const float from[3], const float at[3],
                               const float vup[3], float vfov_deg, float aspect,
                               float aperture, float focus_dist,
                               uint32_t width_px, uint32_t height_px,
                               rtx_frame *out);
/* Enable thin-lens defocus on a frame from rtx_camera_look_at: lens
 * radius = aperture / 2 (focus distance is already in the frame rows). */
RTX_API int rtx_camera_set_aperture(rtx_frame *frame, float aperture);
/* Camera(width, height) of the CPU library (Camera.h:9-21). */
RTX_API int rtx_camera_simple(uint32_t width_px, uint32_t height_px, rtx_frame *out);
/* Adapters from the reference's exact cbuffer byte layouts: WorldDef
 * (18,448 B, DxCSApp.cpp:64-71) and PerFrame (112 B, DxCSApp.cpp:30-37,
 * viewVals stored transposed, :60). The world adapter writes into
 * caller arrays of capacity 512 like rtx_scene_random_world. */
RTX_API int rtx_world_from_worlddef(const void *worlddef_bytes, size_t nbytes,
                                    float *spheres, float *mat_types,
                                    float *mat_values, rtx_world *out);
RTX_API int rtx_frame_from_perframe(const void *perframe_bytes, size_t nbytes,
                                    uint32_t width_px, uint32_t height_px,
                                    rtx_frame *out);

/* ---- debug entry points: the hot-path building blocks run on the GPU ----
 * (used by the parity tests; same device code as the render kernel).
 * rays: nrays * 6 floats (origin.xyz, dir.xyz) host memory. out: nrays * 10
 * floats: hit(0/1), t, p.xyz, normal.xyz, front_face(0/1), sphere index.
 * Uses the uploaded world. Synchronous. ~ hit_world, ShaderCompute.hlsl:188-205.
 * The rays may hold any bit patterns: NaN, infinities, zero directions, tiny
 * and huge lengths. The reference accepts a root with
 * !(root < t_min || t_max < root), so a NaN root is accepted and after it
 * every later sphere whose discriminant is not negative: a ray with a NaN
 * component "hits" sphere count - 1 with t = NaN, and what a ray with
 * |d|^2 = inf or 1 / |d|^2 = inf hits depends on the scene's order. The record
 * is the in-order scan's for such rays too, in every scan form below. The
 * render meets them in ordinary use (the unguarded Lambert direction
 * normalize(0), RTX_FN_LAMBERT_DIR): a NaN ray then goes on from sphere
 * count - 1 by that sphere's material. */
RTX_API int rtx_debug_hit_world(rtx_ctx *ctx, const float *rays, uint32_t nrays,
                                float t_min, float t_max, float *out);
/* Requirements of both: t_min finite and > 0 (the render's 0.001; the
 * kernel orders candidate roots by their bit patterns, which order like the
 * values only for positive roots), t_max not NaN. t_max < t_min: no ray
 * hits (no root lies in [t_min, t_max]).
 * rtx_debug_hit_world_from: the same, with the prefiltered scan starting at
 * 8-sphere block start_block % (its number of blocks) and wrapping round —
 * the start the large-scene kernels take from their workgroup's position
 * word (DESIGN.md §3 "pack start"). The blocks are counted in whichever
 * order the scan visits the spheres: scene order (ceil(count / 8) blocks),
 * or, for a small world with a sphere layer, the spatial layout built at
 * rtx_upload_world (off-layer spheres, then the layer in
 * compact blocks, each section padded to whole blocks). The answer does not
 * depend on it: the result is the in-order scan's for every start (ties
 * between spheres on either side of the wrap included), and the sphere index
 * reported is always the scene's.
 * start_block = RTX_DEBUG_CULLED: for a world of more than 1,024 spheres
 * (after padding to 8), the culled scan the render's lane mode runs on such
 * scenes (a spatially ordered copy of the spheres whose 8-sphere blocks are
 * skipped when no lane's line passes their bounding sphere, DESIGN.md §3e
 * "culled scan"); smaller worlds scan from block
 * RTX_DEBUG_CULLED % ceil(count / 8) as above. */
#define RTX_DEBUG_CULLED 0xFFFFFFFFu
/* start_block = RTX_DEBUG_CULLED_COOP(q), q in 1..64, for the same worlds:
 * the culled scan split over a wave's lanes as the render's frame tail and
 * heavy tiers run it, q rays per wave (64 / 2^ceil(log2 q) lanes per ray). */
#define RTX_DEBUG_CULLED_COOP(q) (0xFFFFFF00u | (unsigned)(q))
/* start_block = RTX_DEBUG_CULLED_COOP_LANE(q): the same split with each lane
 * walking its own subtree (the per-sample kernel's form; RTX_DEBUG_CULLED_COOP
 * walks one ray's levels breadth first). */
#define RTX_DEBUG_CULLED_COOP_LANE(q) (0xFFFFFE00u | (unsigned)(q))
RTX_API int rtx_debug_hit_world_from(rtx_ctx *ctx, const float *rays, uint32_t nrays,
                                     float t_min, float t_max, uint32_t start_block,
                                     float *out);
/* Evaluates device math function `fn` (RTX_FN_*) elementwise on host
 * arrays (in0, in1 may be unused); out receives n floats (hash functions
 * write 1, 2 or 3 floats per element: out must hold 3*n). The diffuse
 * direction functions take n cases: in0 = p[3n], in1 = (normal, rius)[6n],
 * out = normalize(((p + normal) + rius) - p)[3n] (ShaderCompute.hlsl:
 * 211-212), unguarded or with RTX_FRAME_LAMBERT_GUARD. Synchronous. */
enum {
    RTX_FN_SQRT = 0, RTX_FN_DIV = 1, RTX_FN_SIN = 2, RTX_FN_COS = 3,
    RTX_FN_LOG2 = 4, RTX_FN_EXP2 = 5, RTX_FN_POW = 6, RTX_FN_BASEHASH = 7,
    RTX_FN_HASH1 = 8, RTX_FN_HASH2 = 9, RTX_FN_HASH3 = 10, RTX_FN_RIUS = 11,
    RTX_FN_LAMBERT_DIR = 12, RTX_FN_LAMBERT_DIR_GUARD = 13
};
RTX_API int rtx_debug_math(rtx_ctx *ctx, int fn, const float *in0,
                           const float *in1, uint32_t n, float *out);
/* Wave timeline diagnostic: a call with a new max_waves (> 0) arms
 * recording of every render wave's (start, end) s_memrealtime (100 MHz)
 * into a device buffer of that many waves (0 disarms); a call with the same
 * max_waves and host_pairs != NULL copies the pairs back (synchronous). */
RTX_API int rtx_debug_wave_times(rtx_ctx *ctx, size_t max_waves, unsigned long long *host_pairs);
/* Per-pixel cost diagnostic: traces the whole current frame with `spp`
 * samples per pixel (0 = the world's spp), one lane per pixel, and writes
 * each pixel's ray-segment count (hit_world calls) into host_cost
 * (width * height uint32, row 0 = image bottom). Does not touch the
 * framebuffer or the stats. Synchronous. */
RTX_API int rtx_debug_pixel_cost(rtx_ctx *ctx, uint32_t spp, uint32_t *host_cost);
/* Issue-rate probe of hit_world's instruction mix (ABI 1.4.1): a
 * full-occupancy grid shaped like the render (same workgroups, register
 * budget and LDS) in which every lane runs the render's lane-mode hit_world
 * (prefiltered scan + resolve, ShaderCompute.hlsl:188-205) `reps` times on
 * one primary ray of the current frame, and nothing else. *ms: the launch's
 * HIP-event time; *wave_segments: waves x reps (one wave-segment = 64 ray
 * segments' hit_world). A profiler's SQ_INSTS_VALU over this launch gives
 * the VALU issue rate the scan-and-resolve mix sustains on its own — the
 * ceiling for the render's hit_world section. Scenes up to 640 spheres (the
 * render's LDS-copy scenes); needs a world and a frame. Synchronous. */
RTX_API int rtx_debug_scan_rate(rtx_ctx *ctx, uint32_t reps, float *ms, unsigned long long *wave_segments);
/* What rtx_upload_world built for the uploaded world, and which kernels and
 * scan path the launches will take for it (1.4.5, later builds, no version
 * bump: probe with dlsym "rtx_debug_scene_info"): the context's fields and
 * the predicates the launches themselves use, so a test can assert the path
 * a scene takes. Launches nothing, touches no device memory.
 * RTX_ERR_STATE without a world; RTX_ERR_INVALID for a null argument. */
typedef struct rtx_scene_info {
    uint32_t count, n_pad;        /* spheres, padded to 8 */
    uint32_t kernels;             /* 0 small (n_pad <= 1024), 1 large culled, 2 large linear */
    uint32_t sphere_copy_lds;     /* the render keeps the LDS sphere copy (count <= 640) */
    uint32_t layout;              /* a small-scene layout is uploaded */
    uint32_t layout_positions;    /* its padded position count, else 0 */
    uint32_t map_in_lds;          /* the render reads the position map from LDS */
    uint32_t flat_lo, flat_hi;    /* blocks of the flat run the scan uses (positions when layout) */
    uint32_t grid, grid_nx, grid_nz; /* a layer grid is uploaded, its size */
    uint32_t cull_positions;      /* kernels == 1: the culled layout's padded position count, else 0 */
    uint32_t cull_flat_lo;        /* kernels == 1: the first block of its flat section (= positions / 8: none), else 0 */
    uint32_t reserved[2];
} rtx_scene_info;
RTX_API int rtx_debug_scene_info(rtx_ctx *ctx, rtx_scene_info *out);

#ifdef __cplusplus
}
#endif
#endif /* RTX_H_ */
