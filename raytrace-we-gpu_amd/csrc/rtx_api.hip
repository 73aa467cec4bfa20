// rtx_api.hip — C-ABI context management for librtx.so (include/rtx.h).
//
// Replaces the D3D11 objects the reference's DxCSApp owns
// (CSVersion/DxCSApp.h:33-59): the IMMUTABLE WorldDef cbuffer becomes
// device arrays (rtx_upload_world), the DYNAMIC PerFrame cbuffer becomes
// kernel arguments (rtx_set_frame), the RWTexture2D UAV becomes a linear
// float4 framebuffer, Dispatch becomes rtx_render_rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/rtx.h"
#include "rtx_internal.h"
#include "rtx_cull.h"
#include "rtx_layout.h"
#include "rtx_film.h"
#include "rtx_paths.h"
#include "rtx_prefilter.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    return fail(RTX_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define RTX_HIP(call)                                   \
    do {                                                \
        hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return hip_fail(e_, #call); \
    } while (0)

struct EventPair {
    hipEvent_t start = nullptr, stop = nullptr;
};

// Launch timing: a ring of event pairs. When every pair is in use, the
// oldest launch's duration is folded into a running total if its stop event
// has completed (hipEventQuery, no wait); otherwise the ring doubles. A host
// that renders forever without rtx_stats_reset keeps as many pairs as it
// has launches in flight, and a launch never blocks on an older one.
constexpr size_t kEventRing = 64;  // initial ring size

// Device counter words (unsigned long long): [0] ray segments, [2] pixel-queue
// head (low half), [3] rtx_debug_pixel_cost's segments, [4] launch error bits
// (rtx::kErr*, low half; read back and cleared by check_errors), [1], [5] spare,
// [6, 6 + kErrDiagWords) the first promotion-valve firing's record
// (KParams::err_diag, rtx_internal.h).
constexpr size_t kErrWord = 4;
constexpr size_t kErrDiag = 6;
constexpr size_t kCounterWords = kErrDiag + rtx::kErrDiagWords;

}  // namespace

struct rtx_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // own_stream or an external one
    // scene (device)
    float *d_soa = nullptr;
    float *d_pre = nullptr;  // prefilter blocks (rtx_prefilter.h)
    float4 *d_pre4 = nullptr;  // prefilter data per sphere (tail coop)
    float smag = 0.0f;
    float flat_cy = 0.0f;  // scene's flat run of `pre` blocks (rtx_internal.h KScene)
    uint32_t flat_lo = 0, flat_hi = 0;
    // culled layout (rtx_internal.h KScene; none: null)
    float *d_cpre = nullptr;
    float *d_cbnd = nullptr;
    float *d_cbnd2 = nullptr;
    float *d_cbnd3 = nullptr;
    uint32_t *d_cperm = nullptr;
    float4 *d_ccen = nullptr;
    uint32_t n_cpad = 0, cflat_lo = 0;
    // layer grid of the flat run (small scenes; rtx_grid.h; none: null):
    // its LayerGrid, then the cells' block masks
    rtx::LayerGrid *d_grid = nullptr;
    uint32_t grid_nx = 0, grid_nz = 0;  // its size, for rtx_debug_scene_info (0: none)
    int scan_mode = RTX_SCAN_AUTO;  // rtx_set_scan_mode: applied by rtx_upload_world
    float4 *d_cen = nullptr;
    int *d_mtype = nullptr;
    float4 *d_mval = nullptr;
    uint32_t n = 0, n_pad = 0, depth = 0, spp = 0;
    bool have_world = false;
    // frame
    rtx_frame frame{};
    bool have_frame = false;
    // framebuffer
    float4 *d_fb = nullptr;
    size_t fb_pixels = 0;
    // progressive accumulation (linear sums) of accum_pixels pixels
    float4 *d_accum = nullptr;
    size_t accum_pixels = 0;
    uint32_t accum_frames = 0;
    // progressive refinement along the reference's RNG chain (rtx_refine):
    // per pixel (linear sample sum, seed after its last sample), the samples
    // in it (0: none, the next refine starts fresh) and the frame it is for
    float4 *d_chain = nullptr;
    size_t chain_pixels = 0;
    uint32_t chain_n = 0;
    rtx_frame chain_frame{};
    // ... and the rows it covers (rtx_refine_rows): part chain_part of
    // chain_nparts in tiles of chain_tile rows, chain_pixels = its rows * width
    // in the part's row order; the whole frame is (1, 0, 1) whatever tile_rows
    uint32_t chain_tile = 1, chain_part = 0, chain_nparts = 1;
    // ... and the cost map (rtx_refine_cost): per pixel the segments the last
    // refine launch spent on it, chain_pixels uint32 behind the chain state in
    // the same allocation (cost_map_of). cost_s_prev: the samples it covers;
    // the map is valid while that and chain_n are nonzero, so it falls with
    // the chain state. refine_keys: rtx_refine_set_keys; last_keys: what the
    // last refine launch was keyed by.
    uint32_t cost_s_prev = 0;
    int refine_keys = RTX_REFINE_KEYS_PREPASS;
    int last_keys = RTX_REFINE_KEYS_UNSCHEDULED;
    // adaptive refinement (rtx_refine_adaptive): the per-pixel maps beside the
    // chain state, allocated by the first adaptive call (adapt_maps).
    // adapt_valid: they describe the chain state; otherwise the state is
    // uniform (every count is chain_n, every error +inf) and the next adaptive
    // call fills them so. adapt_mixed: the counts may differ (some call traced
    // a proper subset). Both only mean something while chain_n != 0.
    uint32_t *d_adapt = nullptr;
    size_t adapt_pixels = 0;
    bool adapt_valid = false, adapt_mixed = false;
    // feature buffers (rtx_pick, rtx_mask_from_ids): scratch of feat_bytes
    // bytes — 64 bytes of words (rtx_pick's record; the mask's set count),
    // then the mask's listed bytes — grown on demand
    unsigned char *d_feat = nullptr;
    size_t feat_bytes = 0;
    // rtx_cast_rays: the box of the world's body (rtx_cast.h, from
    // rtx_upload_world), the COHERENT order's scratch — kCastBuckets counts,
    // then keys and perm of cast_rays words each — grown on demand, and what
    // the last call ran
    rtx::CastBox cast_box{};
    uint32_t *d_cast = nullptr;
    size_t cast_rays = 0;
    int cast_last = RTX_CAST_ORDER_GIVEN;
    int paths_last = RTX_CAST_ORDER_GIVEN;  // rtx_trace_paths: the order its last call ran
    int film_last = RTX_CAST_ORDER_GIVEN;   // rtx_trace_film: the order its last call ran
    // rtx_trace_paths_keyed: the probe's segment counts (paths_probe_cap words,
    // grown on demand; its own buffer, so d_cast's size rule stays), and
    // whether d_cast's perm still holds the cost order of paths_perm_n queries
    // (rtx_debug_paths_order): every call that sorts into d_cast clears it first
    uint32_t *d_paths_probe = nullptr;
    size_t paths_probe_cap = 0;
    bool paths_perm_valid = false;
    uint32_t paths_perm_n = 0;
    // measurement
    unsigned long long *d_counters = nullptr;
    unsigned long long *d_wave_times = nullptr;  // diagnostic (rtx_debug_wave_times)
    size_t wave_times_cap = 0;
    // LPT scheduling scratch (persistent kernel): cost + perm per pixel
    uint32_t *d_sched = nullptr;
    size_t sched_pixels = 0;
    // per-sample RNG kernel's per-wave sample-colour scratch
    float *d_ps = nullptr;
    size_t ps_floats = 0;
    std::vector<EventPair> events = std::vector<EventPair>(kEventRing);  // ring: [ev_head, ev_head + ev_count)
    size_t ev_head = 0, ev_count = 0;
    rtx::KTune tune = rtx::default_tune();  // rtx_set_schedule
    hipStream_t aux_stream = nullptr;       // k_trace (tier 1 beside the render), created on first use
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    uint64_t epoch = 0;                     // render launches: promotion-queue entry epochs
    double ms_folded = 0.0;         // durations of launches whose pair was recycled
    uint64_t samples = 0;
    uint64_t launches = 0;
    bool n_changed = false;  // world resized since the last rtx_stats_reset
};

namespace {

int set_device(rtx_ctx *c) {
    RTX_HIP(hipSetDevice(c->device));
    return RTX_OK;
}

// After a stream synchronisation: the error bits the launches since the last
// check set (KParams::errors), reported once and cleared. A set bit means a
// launch left pixels unwritten (rtx_kernels.hip take_promoted).
int check_errors(rtx_ctx *c, const char *what) {
    unsigned long long w[kCounterWords - kErrWord];  // the error word, [5], the valve record
    RTX_HIP(hipMemcpyAsync(w, c->d_counters + kErrWord, sizeof(w), hipMemcpyDeviceToHost, c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    const unsigned long long bits = w[0];
    if (bits == 0) return RTX_OK;
    RTX_HIP(hipMemsetAsync(c->d_counters + kErrWord, 0, sizeof(w), c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    const double valve_ms = (double)rtx::kPromValveTicks * 1e-5;  // s_memrealtime: 100 MHz
    char buf[160];
    std::string why;
    if (bits & rtx::kErrPromTimeout) {
        std::snprintf(buf, sizeof buf, " a promotion server polled for %.0f ms seeing no pixel written and no "
                      "heartbeat, and left;", valve_ms);
        why += buf;
    }
    if (bits & rtx::kErrPromEntryWait) {
        std::snprintf(buf, sizeof buf, " a claimed promotion entry was not published within %.0f ms;", valve_ms);
        why += buf;
    }
    if (bits & rtx::kErrPromTorn) why += " a promotion entry was out of range;";
    if (bits & rtx::kErrKernarg) why += " a kernel's argument segment did not begin with its KParams (check build);";
    const unsigned long long d = w[kErrDiag - kErrWord];
    if (d != 0) {
        const unsigned lo = (unsigned)d, age = (unsigned)(d >> 32);
        std::snprintf(buf, sizeof buf, " first firing: bit %u by a %s server, %.2f ms since it saw progress, the "
                      "heartbeat %.2f ms old, %u stalls of the server itself;", lo & 0xfu,
                      ((lo >> 4) & 0xfu) == 2u ? "k_trace" : "k_render", (double)(lo >> 16) * 1.024e-2,
                      (double)age * 1.024e-2, (lo >> 8) & 0xffu);
        why += buf;
        // the last launch's queue counters (zeroed at its start, still in memory)
        uint32_t q[5] = {0, 0, 0, 0, 0};
        if (c->d_sched && c->sched_pixels &&
            hipMemcpy(q, c->d_sched + 2 * c->sched_pixels + 2 * rtx::kCostBuckets + 8, sizeof q,
                      hipMemcpyDeviceToHost) == hipSuccess) {
            std::snprintf(buf, sizeof buf, " last launch's queue: claimed %u, taken %u, k_render pixels written %u, "
                          "k_render started %u", q[0], q[1], q[2], q[3]);
            why += buf;
        }
    }
    return fail(RTX_ERR_INCOMPLETE, std::string(what) + ": a render launch left pixels unwritten:" + why);
}

void free_world(rtx_ctx *c) {
    (void)hipFree(c->d_soa);
    (void)hipFree(c->d_pre);
    (void)hipFree(c->d_pre4);
    (void)hipFree(c->d_cen);
    (void)hipFree(c->d_mtype);
    (void)hipFree(c->d_mval);
    (void)hipFree(c->d_cpre);
    (void)hipFree(c->d_cbnd);
    (void)hipFree(c->d_cbnd2);
    (void)hipFree(c->d_cbnd3);
    (void)hipFree(c->d_cperm);
    (void)hipFree(c->d_ccen);
    (void)hipFree(c->d_grid);
    c->d_grid = nullptr;
    c->grid_nx = c->grid_nz = 0;
    c->d_cpre = c->d_cbnd = c->d_cbnd2 = c->d_cbnd3 = nullptr;
    c->d_cperm = nullptr;
    c->d_ccen = nullptr;
    c->n_cpad = c->cflat_lo = 0;
    c->d_soa = nullptr;
    c->d_pre = nullptr;
    c->d_pre4 = nullptr;
    c->d_cen = nullptr;
    c->d_mtype = nullptr;
    c->d_mval = nullptr;
    c->have_world = false;
}

rtx::KScene scene_of(const rtx_ctx *c) {
    rtx::KScene s;
    s.soa = c->d_soa;
    s.pre = c->d_pre;
    s.pre4 = c->d_pre4;
    s.smag = c->smag;
    s.flat_cy = c->flat_cy;
    s.flat_lo = c->flat_lo;
    s.flat_hi = c->flat_hi;
    s.cen = c->d_cen;
    s.mtype = c->d_mtype;
    s.mval = c->d_mval;
    s.n = c->n;
    s.n_pad = c->n_pad;
    s.cpre = c->d_cpre;
    s.cbnd = c->d_cbnd;
    s.cbnd2 = c->d_cbnd2;
    s.cbnd3 = c->d_cbnd3;
    s.cperm = c->d_cperm;
    s.ccen = c->d_ccen;
    s.n_cpad = c->n_cpad;
    s.cflat_lo = c->cflat_lo;
    s.grid = c->d_grid;
    return s;
}

}  // namespace

namespace rtx {  // for rtx_group.hip (rtx_internal.h)
int api_fail(int code, const char *msg) { return fail(code, msg); }
hipStream_t ctx_stream(const ::rtx_ctx *c) { return c->stream; }
bool ctx_world_spp(const ::rtx_ctx *c, uint32_t *spp) {
    *spp = c->spp;
    return c->have_world;
}
}  // namespace rtx

extern "C" {

int rtx_version(void) { return RTX_VERSION; }

#ifndef RTX_SRC_SHA
#define RTX_SRC_SHA "unknown"
#endif
// Build provenance: the hash of the sources this library was compiled from
// (Makefile SRC_SHA: sha256 over csrc/* and include/rtx.h, first 16 hex
// digits) and the offload target, so a run can show that the library it
// loaded is the one its tree's sources build.
// A variant build (Makefile variants/adhoc, tools/build_commit_variant.sh:
// other compile-time choices from the same sources) also names itself, so
// it is never mistaken for the product library.
#ifndef RTX_VARIANT
#define RTX_VARIANT "product"
#endif
const char *rtx_build_info(void) { return "src_sha16=" RTX_SRC_SHA " arch=gfx950 variant=" RTX_VARIANT; }

const char *rtx_last_error(void) { return g_last_error.c_str(); }

int rtx_device_count(int *count) {
    if (!count) return fail(RTX_ERR_INVALID, "rtx_device_count: null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return hip_fail(e, "hipGetDeviceCount");
    }
    *count = n;
    return RTX_OK;
}

int rtx_create(int hip_device, rtx_ctx **out) {
    if (!out) return fail(RTX_ERR_INVALID, "rtx_create: null out");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    if (hip_device < 0 || hip_device >= ndev)
        return fail(RTX_ERR_INVALID, "rtx_create: device " + std::to_string(hip_device) +
                                         " out of range (" + std::to_string(ndev) + " devices)");
    rtx_ctx *c = new (std::nothrow) rtx_ctx();
    if (!c) return fail(RTX_ERR_NOMEM, "rtx_create: out of host memory");
    c->device = hip_device;
    int rc = set_device(c);
    if (rc != RTX_OK) {
        delete c;
        return rc;
    }
    e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return hip_fail(e, "hipStreamCreate");
    }
    c->stream = c->own_stream;
    e = hipMalloc(&c->d_counters, kCounterWords * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(c->d_counters, 0, kCounterWords * sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipStreamDestroy(c->own_stream);
        delete c;
        return hip_fail(e, "hipMalloc(counters)");
    }
    *out = c;
    return RTX_OK;
}

void rtx_destroy(rtx_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_world(c);
    (void)hipFree(c->d_fb);
    (void)hipFree(c->d_accum);
    (void)hipFree(c->d_chain);
    (void)hipFree(c->d_adapt);
    (void)hipFree(c->d_feat);
    (void)hipFree(c->d_cast);
    (void)hipFree(c->d_paths_probe);
    (void)hipFree(c->d_counters);
    (void)hipFree(c->d_wave_times);
    (void)hipFree(c->d_sched);
    (void)hipFree(c->d_ps);
    for (auto &p : c->events) {
        if (p.start) (void)hipEventDestroy(p.start);
        if (p.stop) (void)hipEventDestroy(p.stop);
    }
    if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    (void)hipStreamDestroy(c->own_stream);
    delete c;
}

int rtx_set_stream(rtx_ctx *c, void *s) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_set_stream: null ctx");
    c->stream = reinterpret_cast<hipStream_t>(s);  // NULL: HIP's null stream (torch's default stream)
    return RTX_OK;
}

int rtx_use_own_stream(rtx_ctx *c) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_use_own_stream: null ctx");
    c->stream = c->own_stream;
    return RTX_OK;
}

int rtx_schedule_defaults(rtx_schedule *out) {
    if (!out) return fail(RTX_ERR_INVALID, "rtx_schedule_defaults: null out");
    const rtx::KTune t = rtx::default_tune();
    *out = rtx_schedule{};
    out->tier1_bar = (float)t.a1;
    out->tier1_bar_small = (float)t.a1_small;
    out->tier1_bar_low = (float)t.a1_low;
    out->tier2_bar_small = (float)t.a2_small;
    out->tier2_bar_medium = (float)t.a2_medium;
    out->tier2_bar = (float)std::min(t.a2_large, 1e30);
    out->small_share = (float)t.rho;
    out->low_share = (float)t.rho_low;
    out->medium_share = (float)t.rho2;
    out->hot_fraction = (float)t.prio_frac;
    out->occupancy_small = (float)t.occ_small;
    out->occupancy_low = (float)t.occ_low;
    out->occupancy_normal = (float)t.occ_normal;
    out->tail_coop_max = t.coop_max;
    out->tail_coop_max_large = t.coop_max_large;
    out->trace_small = (float)t.trace_small;
    out->trace_low = (float)t.trace_low;
    out->trace_medium = (float)t.trace_medium;
    out->trace_large = (float)t.trace_large;
    out->promote_small = (float)t.prom_small;
    out->promote_low = (float)t.prom_low;
    out->promote_medium = (float)t.prom_medium;
    out->promote_large = (float)t.prom_large;
    out->promote_big_scene = (float)t.prom_big;
    out->tier1_priority = t.prio_t1;
    out->tier2_priority = t.prio_t2;
    out->hot_priority = t.prio_hot;
    out->refill_chunk = t.chunk;
    out->trace_group = t.trace_group;
    out->trace_solo_bar = (float)std::min(t.trace_solo, 1e30);
    out->prepass_cap_split = t.cap_split;
    out->prio_bar1 = (float)t.dyn1;
    out->prio_bar2 = (float)t.dyn2;
    out->prio_bar3 = (float)t.dyn3;
    return RTX_OK;
}

int rtx_set_schedule(rtx_ctx *c, const rtx_schedule *s) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_set_schedule: null ctx");
    if (!s) {
        c->tune = rtx::default_tune();
        return RTX_OK;
    }
    const struct { const char *name; float v; } pos[] = {
        {"tier1_bar", s->tier1_bar},         {"tier1_bar_small", s->tier1_bar_small},
        {"tier1_bar_low", s->tier1_bar_low}, {"tier2_bar_small", s->tier2_bar_small},
        {"tier2_bar_medium", s->tier2_bar_medium}, {"tier2_bar", s->tier2_bar}, {"small_share", s->small_share},
        {"low_share", s->low_share},         {"medium_share", s->medium_share},
        {"trace_solo_bar", s->trace_solo_bar}};
    for (const auto &f : pos)
        if (!(f.v > 0.0f && f.v <= 1e30f))
            return fail(RTX_ERR_INVALID, std::string("rtx_set_schedule: ") + f.name + " must be finite and > 0");
    if (!(s->hot_fraction >= 0.0f && s->hot_fraction <= 1.0f))
        return fail(RTX_ERR_INVALID, "rtx_set_schedule: hot_fraction must be in [0, 1]");
    const float occ[] = {s->occupancy_small, s->occupancy_low, s->occupancy_normal};
    for (float o : occ)
        if (!(o > 0.0f && o <= 1.0f)) return fail(RTX_ERR_INVALID, "rtx_set_schedule: occupancies must be in (0, 1]");
    if (s->tail_coop_max < 1 || s->tail_coop_max > 64)
        return fail(RTX_ERR_INVALID, "rtx_set_schedule: tail_coop_max must be in 1..64");
    if (s->tail_coop_max_large < 1 || s->tail_coop_max_large > 64)
        return fail(RTX_ERR_INVALID, "rtx_set_schedule: tail_coop_max_large must be in 1..64");
    const float pr[] = {s->promote_small, s->promote_low, s->promote_medium, s->promote_large, s->promote_big_scene};
    for (float v : pr)
        if (!(v >= 0.0f && v <= 1e9f)) return fail(RTX_ERR_INVALID, "rtx_set_schedule: promote_* must be in [0, 1e9]");
    const float tr[] = {s->trace_small, s->trace_low, s->trace_medium, s->trace_large};
    for (float v : tr)
        if (!(v >= 0.0f && v <= 0.5f)) return fail(RTX_ERR_INVALID, "rtx_set_schedule: trace_* must be in [0, 0.5]");
    if (s->tier1_priority > 3 || s->tier2_priority > 3 || s->hot_priority > 3)
        return fail(RTX_ERR_INVALID, "rtx_set_schedule: priorities must be in 0..3");
    if (s->refill_chunk > 4096) return fail(RTX_ERR_INVALID, "rtx_set_schedule: refill_chunk must be in 0..4096");
    if (s->trace_group != 1 && s->trace_group != 2 && s->trace_group != 4 && s->trace_group != 8)
        return fail(RTX_ERR_INVALID, "rtx_set_schedule: trace_group must be 1, 2, 4 or 8");
    if (s->prepass_cap_split > 4096)
        return fail(RTX_ERR_INVALID, "rtx_set_schedule: prepass_cap_split must be in 0..4096");
    if (!(s->prio_bar1 == 0.0f || (s->prio_bar1 > 0.0f && s->prio_bar1 <= s->prio_bar2 &&
                                   s->prio_bar2 <= s->prio_bar3 && s->prio_bar3 <= 1e30f)))
        return fail(RTX_ERR_INVALID, "rtx_set_schedule: prio_bar1..3 must be 0 or 0 < bar1 <= bar2 <= bar3 <= 1e30");
    if (s->reserved != 0) return fail(RTX_ERR_INVALID, "rtx_set_schedule: reserved must be 0");
    rtx::KTune t;
    t.a1 = s->tier1_bar;
    t.a1_small = s->tier1_bar_small;
    t.a1_low = s->tier1_bar_low;
    t.a2_small = s->tier2_bar_small;
    t.a2_medium = s->tier2_bar_medium;
    t.a2_large = s->tier2_bar;
    t.rho = s->small_share;
    t.rho_low = s->low_share;
    t.rho2 = s->medium_share;
    t.prio_frac = s->hot_fraction;
    t.occ_small = s->occupancy_small;
    t.occ_low = s->occupancy_low;
    t.occ_normal = s->occupancy_normal;
    t.coop_max = s->tail_coop_max;
    t.coop_max_large = s->tail_coop_max_large;
    t.trace_small = s->trace_small;
    t.trace_low = s->trace_low;
    t.trace_medium = s->trace_medium;
    t.trace_large = s->trace_large;
    t.prom_small = s->promote_small;
    t.prom_low = s->promote_low;
    t.prom_medium = s->promote_medium;
    t.prom_large = s->promote_large;
    t.prom_big = s->promote_big_scene;
    t.prio_t1 = s->tier1_priority;
    t.prio_t2 = s->tier2_priority;
    t.prio_hot = s->hot_priority;
    t.chunk = s->refill_chunk;
    t.trace_group = s->trace_group;
    t.trace_solo = s->trace_solo_bar;
    t.cap_split = s->prepass_cap_split;
    t.dyn1 = s->prio_bar1;
    t.dyn2 = s->prio_bar1 > 0.0f ? s->prio_bar2 : 0.0f;
    t.dyn3 = s->prio_bar1 > 0.0f ? s->prio_bar3 : 0.0f;
    c->tune = t;
    return RTX_OK;
}

int rtx_get_schedule(rtx_ctx *c, rtx_schedule *out) {
    if (!c || !out) return fail(RTX_ERR_INVALID, "rtx_get_schedule: null argument");
    const rtx::KTune &t = c->tune;
    *out = rtx_schedule{};
    out->tier1_bar = (float)t.a1;
    out->tier1_bar_small = (float)t.a1_small;
    out->tier1_bar_low = (float)t.a1_low;
    out->tier2_bar_small = (float)t.a2_small;
    out->tier2_bar_medium = (float)t.a2_medium;
    out->tier2_bar = (float)std::min(t.a2_large, 1e30);
    out->small_share = (float)t.rho;
    out->low_share = (float)t.rho_low;
    out->medium_share = (float)t.rho2;
    out->hot_fraction = (float)t.prio_frac;
    out->occupancy_small = (float)t.occ_small;
    out->occupancy_low = (float)t.occ_low;
    out->occupancy_normal = (float)t.occ_normal;
    out->tail_coop_max = t.coop_max;
    out->tail_coop_max_large = t.coop_max_large;
    out->trace_small = (float)t.trace_small;
    out->trace_low = (float)t.trace_low;
    out->trace_medium = (float)t.trace_medium;
    out->trace_large = (float)t.trace_large;
    out->promote_small = (float)t.prom_small;
    out->promote_low = (float)t.prom_low;
    out->promote_medium = (float)t.prom_medium;
    out->promote_large = (float)t.prom_large;
    out->promote_big_scene = (float)t.prom_big;
    out->tier1_priority = t.prio_t1;
    out->tier2_priority = t.prio_t2;
    out->hot_priority = t.prio_hot;
    out->refill_chunk = t.chunk;
    out->trace_group = t.trace_group;
    out->trace_solo_bar = (float)std::min(t.trace_solo, 1e30);
    out->prepass_cap_split = t.cap_split;
    out->prio_bar1 = (float)t.dyn1;
    out->prio_bar2 = (float)t.dyn2;
    out->prio_bar3 = (float)t.dyn3;
    return RTX_OK;
}

int rtx_upload_world(rtx_ctx *c, const rtx_world *w) {
    if (!c || !w) return fail(RTX_ERR_INVALID, "rtx_upload_world: null argument");
    if (w->reserved != 0) return fail(RTX_ERR_INVALID, "rtx_upload_world: reserved must be 0");
    if (w->count > 0 && (!w->spheres || !w->mat_types || !w->mat_values))
        return fail(RTX_ERR_INVALID, "rtx_upload_world: null array with count > 0");
    // Finite scene values of magnitude <= 1e15 keep every ray-sphere
    // discriminant of a ray inside the prefilter's safe range free of fp32
    // overflow (rtx_prefilter.h line_test_setup: S^2 and a S^2 <= 1e36). The
    // radius may have either sign or be zero, and the materials are not
    // checked (include/rtx.h).
    for (uint32_t i = 0; i < w->count; ++i)
        for (int k = 0; k < 4; ++k) {
            const float v = w->spheres[4 * i + k];
            if (!(v >= -1e15f && v <= 1e15f))
                return fail(RTX_ERR_INVALID, "rtx_upload_world: sphere " + std::to_string(i) +
                                                 " has a non-finite or |value| > 1e15 component");
        }
    // The prefiltered scan's list entries hold a 24-bit local sphere index.
    if (w->count > (1u << 24) - rtx::kPad)
        return fail(RTX_ERR_INVALID, "rtx_upload_world: more than 16,777,208 spheres");
    int rc = set_device(c);
    if (rc) return rc;
    const uint32_t n = w->count;
    const uint32_t n_pad = (n + rtx::kPad - 1) / rtx::kPad * rtx::kPad;
    std::vector<float> soa(4 * (size_t)n_pad), pre(4 * (size_t)n_pad);
    double smag = 0.0;  // max |c| + |r|, for the prefilter's overflow guard
    std::vector<float4> cen(n), mval(n), pre4(n);
    std::vector<int> mtype(n);
    for (uint32_t i = 0; i < n_pad; ++i) {
        // padding: copies of sphere n-1 (see rtx::KScene)
        const uint32_t k = i < n ? i : n - 1;
        const float r = w->spheres[4 * k + 3];
        float *blk = &soa[32 * (size_t)(i / 8)];
        blk[i % 8] = w->spheres[4 * k + 0];
        blk[8 + i % 8] = w->spheres[4 * k + 1];
        blk[16 + i % 8] = w->spheres[4 * k + 2];
        const float r2 = r * r;
        blk[24 + i % 8] = -r2;
        float *pb = &pre[32 * (size_t)(i / 8)];
        pb[i % 8] = blk[i % 8];
        pb[8 + i % 8] = blk[8 + i % 8];
        pb[16 + i % 8] = blk[16 + i % 8];
        pb[24 + i % 8] = rtx::prefilter_R(blk[i % 8], blk[8 + i % 8], blk[16 + i % 8], r2);
        const double cx = blk[i % 8], cy = blk[8 + i % 8], cz = blk[16 + i % 8];
        smag = std::max(smag, std::sqrt(cx * cx + cy * cy + cz * cz) + std::fabs((double)r));
        if (i < n) pre4[i] = make_float4(pb[i % 8], pb[8 + i % 8], pb[16 + i % 8], pb[24 + i % 8]);
    }
    float smag_f = (float)smag;
    if ((double)smag_f < smag) smag_f = std::nextafter(smag_f, INFINITY);
    // The longest run of flat blocks (rtx_prefilter.h: all 8 centre heights
    // equal, bit for bit, and equal along the run): the scan's 5-op test.
    uint32_t flat_lo = 0, flat_hi = 0;
    float flat_cy = 0.0f;
    {
        auto bits = [&](uint32_t b, int k) { return __builtin_bit_cast(uint32_t, pre[32 * (size_t)b + 8 + k]); };
        auto flat = [&](uint32_t b) {
            for (int k = 1; k < 8; ++k)
                if (bits(b, k) != bits(b, 0)) return false;
            return true;
        };
        const uint32_t nblk = n_pad / 8;
        for (uint32_t b = 0; b < nblk;) {
            if (!flat(b)) {
                ++b;
                continue;
            }
            uint32_t e = b + 1;
            while (e < nblk && flat(e) && bits(e, 0) == bits(b, 0)) ++e;
            if (e - b > flat_hi - flat_lo) flat_lo = b, flat_hi = e, flat_cy = pre[32 * (size_t)b + 8];
            b = e;
        }
    }
    for (uint32_t i = 0; i < n; ++i) {
        cen[i] = make_float4(w->spheres[4 * i + 0], w->spheres[4 * i + 1], w->spheres[4 * i + 2],
                             w->spheres[4 * i + 3]);
        // The shader compares the float code with 0, 1, 2 (:209,219,229);
        // anything else does not scatter.
        const float t = w->mat_types[i];
        mtype[i] = (t == 0.0f) ? 0 : (t == 1.0f) ? 1 : (t == 2.0f) ? 2 : 3;
        mval[i] = make_float4(w->mat_values[4 * i + 0], w->mat_values[4 * i + 1],
                              w->mat_values[4 * i + 2], w->mat_values[4 * i + 3]);
    }
    rtx::CullLayout cl;  // the culled layout (rtx_cull.h)
    const bool linear = c->scan_mode == RTX_SCAN_LINEAR;  // every block of every segment: no grid, no culled copy
    const bool cull = !linear && n_pad > rtx::kScanPfMin;  // the large-scene (kPF) kernels scan it
    static_assert(sizeof(float4) == 4 * sizeof(float), "pre4 is read as (cx, cy, cz, R) float records");
    if (cull) cl = rtx::build_cull(w->spheres, n, reinterpret_cast<const float *>(pre4.data()), flat_hi > flat_lo, flat_cy);
    // the small-scene lane-mode scan's layer grid over the flat run (rtx_grid.h)
    rtx::LayerGrid grid{};
    std::vector<unsigned long long> gcell;
    // ... and its spatial layout (rtx_layout.h): the lane-mode scan's own copy
    // of the spheres, the layer in compact blocks. It takes the culled
    // layout's fields (cpre, cperm, n_cpad, cflat_lo: never both, a scene is
    // small or large), and the flat run and the grid then describe its blocks.
    rtx::SceneLayout lay;
    if (RTX_LAYOUT && !linear && n != 0 && n_pad <= rtx::kScanPfMin) {
        lay = rtx::build_scene_layout(w->spheres, n, rtx::kLayoutDefault);
        if (lay.valid && !rtx::layout_lds_ok(n, (uint32_t)lay.perm.size())) lay = rtx::SceneLayout();
    }
    bool has_grid;
    if (lay.valid) {
        flat_lo = lay.flat_lo, flat_hi = lay.flat_hi, flat_cy = lay.flat_cy;
        has_grid = lay.has_grid;
        grid = lay.grid;
        gcell.swap(lay.cell);
    } else {
        has_grid = !linear && n_pad <= rtx::kScanPfMin && flat_hi > flat_lo &&
                   rtx::build_layer_grid(w->spheres, 8 * flat_lo, std::min(8 * flat_hi, n), grid, gcell);
    }
    RTX_HIP(hipStreamSynchronize(c->stream));
    free_world(c);
    const size_t cap = n ? n : 1;
    RTX_HIP(hipMalloc(&c->d_soa, (n_pad ? 4 * (size_t)n_pad : 4) * sizeof(float)));
    RTX_HIP(hipMalloc(&c->d_pre, (n_pad ? 4 * (size_t)n_pad : 4) * sizeof(float)));
    RTX_HIP(hipMalloc(&c->d_pre4, cap * sizeof(float4)));
    RTX_HIP(hipMalloc(&c->d_cen, cap * sizeof(float4)));
    RTX_HIP(hipMalloc(&c->d_mtype, cap * sizeof(int)));
    RTX_HIP(hipMalloc(&c->d_mval, cap * sizeof(float4)));
    // All copies on the context stream (a non-blocking stream does not
    // order against the legacy null stream), then wait for them.
    if (n) {
        RTX_HIP(hipMemcpyAsync(c->d_soa, soa.data(), soa.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        RTX_HIP(hipMemcpyAsync(c->d_pre, pre.data(), pre.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        RTX_HIP(hipMemcpyAsync(c->d_pre4, pre4.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        RTX_HIP(hipMemcpyAsync(c->d_cen, cen.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        RTX_HIP(hipMemcpyAsync(c->d_mtype, mtype.data(), n * sizeof(int), hipMemcpyHostToDevice, c->stream));
        RTX_HIP(hipMemcpyAsync(c->d_mval, mval.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        RTX_HIP(hipStreamSynchronize(c->stream));
    }
    if (cull) {
        RTX_HIP(hipMalloc(&c->d_cpre, cl.pre.size() * sizeof(float)));
        RTX_HIP(hipMalloc(&c->d_cbnd, cl.bnd.size() * sizeof(float)));
        RTX_HIP(hipMalloc(&c->d_cbnd2, cl.bnd2.size() * sizeof(float)));
        RTX_HIP(hipMalloc(&c->d_cbnd3, cl.bnd3.size() * sizeof(float)));
        RTX_HIP(hipMemcpyAsync(c->d_cbnd3, cl.bnd3.data(), cl.bnd3.size() * sizeof(float), hipMemcpyHostToDevice,
                               c->stream));
        RTX_HIP(hipMemcpyAsync(c->d_cbnd2, cl.bnd2.data(), cl.bnd2.size() * sizeof(float), hipMemcpyHostToDevice,
                               c->stream));
        RTX_HIP(hipMalloc(&c->d_cperm, cl.perm.size() * sizeof(uint32_t)));
        RTX_HIP(hipMalloc(&c->d_ccen, cl.perm.size() * sizeof(float4)));
        std::vector<float4> ccen(cl.perm.size());
        for (size_t p = 0; p < ccen.size(); ++p) ccen[p] = cen[cl.perm[p]];
        RTX_HIP(hipMemcpyAsync(c->d_ccen, ccen.data(), ccen.size() * sizeof(float4), hipMemcpyHostToDevice, c->stream));
        RTX_HIP(hipMemcpyAsync(c->d_cpre, cl.pre.data(), cl.pre.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        RTX_HIP(hipMemcpyAsync(c->d_cbnd, cl.bnd.data(), cl.bnd.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        RTX_HIP(hipMemcpyAsync(c->d_cperm, cl.perm.data(), cl.perm.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                               c->stream));
        RTX_HIP(hipStreamSynchronize(c->stream));
        c->n_cpad = (uint32_t)cl.perm.size();
        c->cflat_lo = cl.flat_lo;
    }
    if (lay.valid) {
        RTX_HIP(hipMalloc(&c->d_cpre, lay.pre.size() * sizeof(float)));
        RTX_HIP(hipMalloc(&c->d_cperm, lay.perm.size() * sizeof(uint32_t)));
        RTX_HIP(hipMemcpyAsync(c->d_cpre, lay.pre.data(), lay.pre.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        RTX_HIP(hipMemcpyAsync(c->d_cperm, lay.perm.data(), lay.perm.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                               c->stream));
        RTX_HIP(hipStreamSynchronize(c->stream));
        c->n_cpad = (uint32_t)lay.perm.size();
        c->cflat_lo = lay.flat_lo;
    }
    if (has_grid) {
        static_assert(sizeof(rtx::LayerGrid) % 8 == 0, "the cells follow the LayerGrid, 8-byte aligned");
        std::vector<unsigned long long> buf(sizeof(rtx::LayerGrid) / 8 + gcell.size());
        std::memcpy(buf.data(), &grid, sizeof grid);
        std::memcpy(buf.data() + sizeof(rtx::LayerGrid) / 8, gcell.data(), gcell.size() * sizeof(unsigned long long));
        RTX_HIP(hipMalloc(&c->d_grid, buf.size() * sizeof(unsigned long long)));
        RTX_HIP(hipMemcpyAsync(c->d_grid, buf.data(), buf.size() * sizeof(unsigned long long), hipMemcpyHostToDevice,
                               c->stream));
        RTX_HIP(hipStreamSynchronize(c->stream));
        c->grid_nx = grid.nx;
        c->grid_nz = grid.nz;
    }
    if (c->n != n) c->n_changed = true;
    c->n = n;
    c->n_pad = n_pad;
    c->smag = smag_f;
    c->flat_cy = flat_cy;
    c->flat_lo = flat_lo;
    c->flat_hi = flat_hi;
    c->depth = w->depth;
    c->spp = w->spp;
    {
        std::vector<float> radii(n);
        c->cast_box = rtx::cast_box(w->spheres, n, radii.data());
    }
    c->have_world = true;
    c->chain_n = 0;  // a chain state belongs to the world it was traced in
    return RTX_OK;
}

// What the upload above built and what the launches will take for it: the
// context's fields and rtx::scene_kernels, no launch.
int rtx_debug_scene_info(rtx_ctx *c, rtx_scene_info *out) {
    if (!c || !out) return fail(RTX_ERR_INVALID, "rtx_debug_scene_info: null argument");
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_debug_scene_info: no world uploaded");
    const rtx::KScene s = scene_of(c);
    const rtx::SceneKernels k = rtx::scene_kernels(s);
    std::memset(out, 0, sizeof *out);
    out->count = s.n;
    out->n_pad = s.n_pad;
    out->kernels = k.kernels;
    out->sphere_copy_lds = k.sphere_copy_lds;
    out->layout = k.kernels == 0 && s.cpre != nullptr;  // a small scene holds only a layout in these fields
    out->layout_positions = out->layout ? s.n_cpad : 0;
    out->map_in_lds = k.map_in_lds;
    out->flat_lo = s.flat_lo;
    out->flat_hi = s.flat_hi;
    out->grid = s.grid != nullptr;
    out->grid_nx = c->grid_nx;
    out->grid_nz = c->grid_nz;
    out->cull_positions = k.kernels == 1 ? s.n_cpad : 0;
    out->cull_flat_lo = k.kernels == 1 ? s.cflat_lo : 0;
    return RTX_OK;
}

int rtx_set_scan_mode(rtx_ctx *c, int mode) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_set_scan_mode: null ctx");
    if (mode != RTX_SCAN_AUTO && mode != RTX_SCAN_LINEAR) return fail(RTX_ERR_INVALID, "rtx_set_scan_mode: unknown mode");
    c->scan_mode = mode;
    return RTX_OK;
}

int rtx_set_frame(rtx_ctx *c, const rtx_frame *f) {
    if (!c || !f) return fail(RTX_ERR_INVALID, "rtx_set_frame: null argument");
    if (f->width == 0 || f->height == 0)
        return fail(RTX_ERR_INVALID, "rtx_set_frame: zero width or height");
    if (f->rng_mode > 1) return fail(RTX_ERR_INVALID, "rtx_set_frame: unknown rng_mode");
    if ((f->flags & ~(uint32_t)RTX_FRAME_LAMBERT_GUARD) != 0 || f->reserved != 0)
        return fail(RTX_ERR_INVALID, "rtx_set_frame: unknown flags or nonzero reserved");
    if (!(f->lens_u[3] >= 0.0f)) return fail(RTX_ERR_INVALID, "rtx_set_frame: negative lens radius");
    if ((uint64_t)f->width * f->height > (1ull << 31))
        return fail(RTX_ERR_INVALID, "rtx_set_frame: more than 2^31 pixels");
    // a chain state belongs to its frame: other bytes restart it, the same
    // bytes again (a host's per-Update call) keep it
    if (c->chain_n != 0 && std::memcmp(f, &c->chain_frame, sizeof *f) != 0) c->chain_n = 0;
    c->frame = *f;
    c->have_frame = true;
    return RTX_OK;
}

uint32_t rtx_part_rows(uint32_t height, uint32_t tile_rows, uint32_t part, uint32_t nparts) {
    if (tile_rows == 0 || nparts == 0 || part >= nparts) return 0;
    const uint32_t tiles = (height + tile_rows - 1) / tile_rows;
    if (part >= tiles) return 0;
    const uint32_t my_tiles = (tiles - part + nparts - 1) / nparts;  // tiles part, part+nparts, ...
    uint32_t rows = my_tiles * tile_rows;
    const uint32_t last_tile = part + (my_tiles - 1) * nparts;
    if (last_tile == tiles - 1) rows -= tiles * tile_rows - height;  // ragged final tile
    return rows;
}

// A refine launch's chain arguments (KParams::chain_in, chain_out, out_n) and
// its sample count, which replaces the world's spp.
struct RefineArgs {
    const float4 *chain_in;
    float4 *chain_out;
    uint32_t samples, out_n;
    uint32_t *cost_map;  // KSchedule::cost_map
    uint32_t carry_spp;  // ... carry_spp (0: pre-pass keys)
    const rtx::KAdaptive *adaptive = nullptr;  // an adaptive launch: its maps and active count
};
// The chain state's allocation: chain_pixels float4, then the cost map.
static size_t chain_bytes(size_t px) { return px * (sizeof(float4) + sizeof(uint32_t)); }
static uint32_t *cost_map_of(const rtx_ctx *c) { return reinterpret_cast<uint32_t *>(c->d_chain + c->chain_pixels); }
static bool cost_map_valid(const rtx_ctx *c) { return c->d_chain && c->chain_n != 0 && c->cost_s_prev != 0; }
static int render_impl(rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts, void *d_out,
                       float4 *accum, uint32_t accum_frames, uint32_t frame_index,
                       const RefineArgs *refine = nullptr);

// Scheduling scratch (words): cost[npix] perm[npix] buckets[2K + kSchedWords], then the
// per-pixel pre-pass state (float4, 16-byte aligned).
static size_t sched_state_off(size_t npix) { return (2 * npix + 2 * rtx::kCostBuckets + rtx::kSchedWords + 3) & ~(size_t)3; }
constexpr uint32_t kPromCap = 65536;  // promotion queue entries (8 words each)

int rtx_render_rows(rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts, void *d_out) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_render_rows: null ctx");
    return render_impl(c, tile_rows, part, nparts, d_out, nullptr, 0, c->frame.frame_index);
}

int rtx_accumulate(rtx_ctx *c, int reset) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_accumulate: null ctx");
    if (!c->have_frame) return fail(RTX_ERR_STATE, "rtx_accumulate: no frame set");
    int rc = set_device(c);
    if (rc) return rc;
    const size_t px = (size_t)c->frame.width * c->frame.height;
    // a frame of another size restarts the accumulation (the accumulator is
    // indexed by pixel: it must hold exactly width*height sums)
    if (reset || c->accum_frames == 0 || !c->d_accum || c->accum_pixels != px) {
        if (!c->d_accum || c->accum_pixels != px) {
            RTX_HIP(hipStreamSynchronize(c->stream));
            (void)hipFree(c->d_accum);
            c->d_accum = nullptr;
            c->accum_pixels = 0;
            RTX_HIP(hipMalloc(&c->d_accum, px * sizeof(float4)));
            c->accum_pixels = px;
        }
        RTX_HIP(hipMemsetAsync(c->d_accum, 0, px * sizeof(float4), c->stream));
        c->accum_frames = 0;
    }
    rc = render_impl(c, 1, 0, 1, nullptr, c->d_accum, c->accum_frames + 1, c->accum_frames);
    if (rc == RTX_OK) c->accum_frames++;
    return rc;
}

uint32_t rtx_accumulated_frames(rtx_ctx *c) { return c ? c->accum_frames : 0; }

int rtx_render_sum(rtx_ctx *c, uint32_t frame_index, void *d_sum) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_render_sum: null ctx");
    if (!d_sum) return fail(RTX_ERR_INVALID, "rtx_render_sum: null d_sum");
    if (frame_index > 0x7fffffffu)  // the seed uses 0x80000000 | frame_index
        return fail(RTX_ERR_INVALID, "rtx_render_sum: frame_index above 0x7fffffff");
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_render_sum: no world uploaded");
    if (!c->have_frame) return fail(RTX_ERR_STATE, "rtx_render_sum: no frame set");
    int rc = set_device(c);
    if (rc) return rc;
    // The accumulate launch pointed at a zeroed buffer: frame 1 of 1 into
    // d_sum. 0 + s == s bit for bit, NaN and inf included, unless s is -0,
    // and a pixel's sum never is: it starts at +0 and x + y is
    // -0 only for two -0 terms. The gamma image the launch also writes lands
    // in the context's own framebuffer and is ignored.
    const size_t px = (size_t)c->frame.width * c->frame.height;
    RTX_HIP(hipMemsetAsync(d_sum, 0, px * sizeof(float4), c->stream));
    return render_impl(c, 1, 0, 1, nullptr, reinterpret_cast<float4 *>(d_sum), 1, frame_index);
}

int rtx_fold_frames(rtx_ctx *c, void *d_accum, const void *d_sums, uint32_t m, size_t slot_pixels, size_t pixels,
                    uint32_t divisor, void *d_image) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_fold_frames: null ctx");
    if (!d_accum || !d_sums || !d_image) return fail(RTX_ERR_INVALID, "rtx_fold_frames: null argument");
    if (m == 0 || m > RTX_FOLD_MAX) return fail(RTX_ERR_INVALID, "rtx_fold_frames: m outside 1 .. RTX_FOLD_MAX");
    if (pixels == 0 || slot_pixels < pixels)
        return fail(RTX_ERR_INVALID, "rtx_fold_frames: needs slot_pixels >= pixels >= 1");
    if (slot_pixels > ((size_t)1 << 40))  // m * slot_pixels * 16 stays far inside 64 bits
        return fail(RTX_ERR_INVALID, "rtx_fold_frames: slot_pixels above 2^40");
    if (divisor == 0) return fail(RTX_ERR_INVALID, "rtx_fold_frames: divisor is 0");
    int rc = set_device(c);
    if (rc) return rc;
    hipError_t e = rtx::launch_fold_frames(reinterpret_cast<float4 *>(d_accum), reinterpret_cast<const float4 *>(d_sums),
                                           m, slot_pixels, pixels, divisor, reinterpret_cast<float4 *>(d_image),
                                           c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_fold_frames");
    return RTX_OK;
}

static rtx::KParams make_params(const rtx_ctx *c, uint32_t rows, uint32_t tile_rows, uint32_t part,
                                uint32_t nparts, float4 *out, float4 *accum, uint32_t accum_frames,
                                uint32_t frame_index) {
    const rtx_frame &f = c->frame;
    rtx::KParams p{};
    p.scene = scene_of(c);
    p.out = out;
    p.counters = c->d_counters;
    p.queue = reinterpret_cast<uint32_t *>(c->d_counters + 2);
    p.errors = reinterpret_cast<uint32_t *>(c->d_counters + kErrWord);
    p.err_diag = c->d_counters + kErrDiag;
    p.depth = c->depth;
    p.spp = c->spp;
    p.width = f.width;
    p.rows_local = rows;
    p.tile_rows = tile_rows;
    p.part = part;
    p.nparts = nparts;
    p.rng_mode = f.rng_mode;
    p.frame_index = frame_index;
    p.flags = f.flags;
    p.accum = accum;
    p.accum_frames = accum_frames;
    for (int k = 0; k < 3; ++k) {
        p.lens_u[k] = f.lens_u[k];
        p.lens_v[k] = f.lens_v[k];
    }
    p.lens_r = f.lens_u[3];
    p.wave_times = c->d_wave_times;
    p.wave_cap = (uint32_t)std::min<size_t>(c->wave_times_cap, 0xffffffffu);
    for (int k = 0; k < 3; ++k) {
        p.org[k] = f.origin[k];
        p.hor[k] = f.horizontal[k];
        p.ver[k] = f.vertical[k];
        p.llc[k] = f.lower_left[k];
    }
    p.img_w = f.img_w;
    p.img_h = f.img_h;
    return p;
}

static int render_impl(rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts, void *d_out,
                       float4 *accum, uint32_t accum_frames, uint32_t frame_index, const RefineArgs *refine) {
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_render_rows: no world uploaded");
    if (!c->have_frame) return fail(RTX_ERR_STATE, "rtx_render_rows: no frame set");
    if (tile_rows == 0 || nparts == 0 || part >= nparts)
        return fail(RTX_ERR_INVALID, "rtx_render_rows: bad partition");
    int rc = set_device(c);
    if (rc) return rc;
    const rtx_frame &f = c->frame;
    const uint32_t rows = rtx_part_rows(f.height, tile_rows, part, nparts);
    float4 *out = reinterpret_cast<float4 *>(d_out);
    if (!out) {
        if (nparts != 1) return fail(RTX_ERR_INVALID, "rtx_render_rows: d_out NULL needs nparts == 1");
        const size_t px = (size_t)f.width * f.height;
        if (c->fb_pixels != px) {
            RTX_HIP(hipStreamSynchronize(c->stream));
            (void)hipFree(c->d_fb);
            c->d_fb = nullptr;
            c->fb_pixels = 0;
            RTX_HIP(hipMalloc(&c->d_fb, px * sizeof(float4)));
            c->fb_pixels = px;
        }
        out = c->d_fb;
    }
    rtx::KParams p = make_params(c, rows, tile_rows, part, nparts, out, accum, accum_frames, frame_index);
    if (refine) {
        p.spp = refine->samples;
        p.chain_in = refine->chain_in;
        p.chain_out = refine->chain_out;
        p.out_n = refine->out_n;
    }

    if (c->ev_count == c->events.size()) {
        EventPair &old = c->events[c->ev_head];
        const hipError_t q = hipEventQuery(old.stop);
        if (q == hipSuccess) {  // recycle the oldest pair: fold its duration
            float t = 0.0f;
            RTX_HIP(hipEventElapsedTime(&t, old.start, old.stop));
            c->ms_folded += t;
            c->ev_head = (c->ev_head + 1) % c->events.size();
            c->ev_count--;
        } else if (q == hipErrorNotReady) {  // still running: grow the ring, no wait
            std::vector<EventPair> grown(2 * c->events.size());
            for (size_t i = 0; i < c->ev_count; ++i) grown[i] = c->events[(c->ev_head + i) % c->events.size()];
            c->events.swap(grown);
            c->ev_head = 0;
        } else {
            return hip_fail(q, "hipEventQuery");
        }
    }
    EventPair &ev = c->events[(c->ev_head + c->ev_count) % c->events.size()];
    if (!ev.start) RTX_HIP(hipEventCreate(&ev.start));
    if (!ev.stop) RTX_HIP(hipEventCreate(&ev.stop));
    RTX_HIP(hipEventRecord(ev.start, c->stream));
    const size_t npix = (size_t)rows * f.width;
    if (c->sched_pixels < npix) {
        RTX_HIP(hipStreamSynchronize(c->stream));
        (void)hipFree(c->d_sched);
        c->d_sched = nullptr;
        c->sched_pixels = 0;
        // cost, perm, buckets; then 16-byte aligned per-pixel state
        // ... the promotion queue, then the slot-ordered image staging (float4) and the inverse permutation
        RTX_HIP(hipMalloc(&c->d_sched,
                          (sched_state_off(npix) + 4 * npix + 8 * (size_t)kPromCap + 5 * npix) * sizeof(uint32_t)));
        // the promotion queue's epoch words start below every launch's epoch
        RTX_HIP(hipMemsetAsync(c->d_sched + sched_state_off(npix) + 4 * npix, 0,
                               8 * (size_t)kPromCap * sizeof(uint32_t), c->stream));
        c->sched_pixels = npix;
    }
    const size_t ps_need = rtx::ps_scratch_floats(p);
    if (ps_need > c->ps_floats) {
        RTX_HIP(hipStreamSynchronize(c->stream));
        (void)hipFree(c->d_ps);
        c->d_ps = nullptr;
        c->ps_floats = 0;
        RTX_HIP(hipMalloc(&c->d_ps, ps_need * sizeof(float)));
        c->ps_floats = ps_need;
    }
    rtx::KSchedule sched;
    sched.ps_scratch = c->d_ps;
    sched.ps_floats = c->ps_floats;
    sched.cost = c->d_sched;
    sched.perm = c->d_sched + c->sched_pixels;
    sched.buckets = c->d_sched + 2 * c->sched_pixels;
    sched.state = reinterpret_cast<float4 *>(c->d_sched + sched_state_off(c->sched_pixels));
    sched.npix = (uint32_t)c->sched_pixels;
    sched.nbuckets = rtx::kCostBuckets;
    sched.tune = c->tune;
    if (!c->aux_stream) {
        RTX_HIP(hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
        RTX_HIP(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        RTX_HIP(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    }
    sched.aux = c->aux_stream;
    sched.prom_q = c->d_sched + sched_state_off(c->sched_pixels) + 4 * c->sched_pixels;
    sched.prom_cap = kPromCap;
    sched.stage = reinterpret_cast<float4 *>(sched.prom_q + 8 * (size_t)kPromCap);  // 16-byte aligned
    sched.inv = sched.prom_q + 8 * (size_t)kPromCap + 4 * c->sched_pixels;
    sched.epoch = (uint32_t)++c->epoch;
    sched.ev_fork = c->ev_fork;
    sched.ev_join = c->ev_join;
    sched.cost_map = refine ? refine->cost_map : nullptr;
    sched.carry_spp = refine ? refine->carry_spp : 0u;
    const rtx::KAdaptive *ad = refine ? refine->adaptive : nullptr;
    hipError_t e = ad ? rtx::launch_render_adaptive(p, sched, *ad, c->stream) : rtx::launch_render(p, sched, c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_render");
    RTX_HIP(hipEventRecord(ev.stop, c->stream));
    c->ev_count++;
    c->launches++;
    c->samples += (ad ? (uint64_t)ad->active : (uint64_t)rows * f.width) * p.spp;
    return RTX_OK;
}

int rtx_render(rtx_ctx *c) { return rtx_render_rows(c, 1, 0, 1, nullptr); }

// ---- progressive refinement along the reference's RNG chain ---------------
// The argument rules rtx_refine_rows and rtx_refine_import_rows share, decided
// before the context is looked at (and before any HIP call).
static int refine_rows_args(const char *fn, const rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts,
                            uint32_t samples) {
    auto bad = [&](const char *why) { return fail(RTX_ERR_INVALID, std::string(fn) + ": " + why); };
    if (!c) return bad("null ctx");
    if (samples == 0) return bad("samples is 0");
    if (tile_rows == 0 || nparts == 0 || part >= nparts) return bad("bad partition (tile_rows, part, nparts)");
    return RTX_OK;
}
// ... and the state rules, which need the context's world and frame.
static int refine_rows_state(const char *fn, const rtx_ctx *c) {
    if (!c->have_world) return fail(RTX_ERR_STATE, std::string(fn) + ": no world uploaded");
    if (!c->have_frame) return fail(RTX_ERR_STATE, std::string(fn) + ": no frame set");
    if (c->frame.rng_mode == RTX_RNG_PER_SAMPLE)
        return fail(RTX_ERR_INVALID, std::string(fn) + ": the per-sample RNG has no chain to continue (rtx_accumulate "
                                                       "is its progressive form)");
    return RTX_OK;
}
// The chain state's allocation for px pixels of shape (tile_rows, part, nparts);
// another size drains the stream and replaces it (N falls to 0).
static int ensure_chain(rtx_ctx *c, size_t px) {
    if (c->d_chain && c->chain_pixels == px) return RTX_OK;
    RTX_HIP(hipStreamSynchronize(c->stream));
    (void)hipFree(c->d_chain);
    c->d_chain = nullptr;
    c->chain_pixels = 0;
    c->chain_n = 0;
    RTX_HIP(hipMalloc(&c->d_chain, chain_bytes(px)));
    c->chain_pixels = px;
    return RTX_OK;
}
static bool chain_shape_is(const rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts) {
    return c->chain_tile == tile_rows && c->chain_part == part && c->chain_nparts == nparts;
}

static int refine_rows_impl(const char *fn, rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts,
                            uint32_t samples, int reset, void *d_out) {
    int rc = refine_rows_args(fn, c, tile_rows, part, nparts, samples);
    if (rc) return rc;
    if (!d_out && nparts > 1) return fail(RTX_ERR_INVALID, std::string(fn) + ": d_out NULL needs nparts == 1");
    rc = refine_rows_state(fn, c);
    if (rc) return rc;
    if (nparts == 1) tile_rows = 1;  // one whole-frame shape, and rtx_refine's launch, whatever tile_rows
    const uint32_t rows = rtx_part_rows(c->frame.height, tile_rows, part, nparts);
    if (rows == 0) return RTX_OK;  // a part without rows: nothing to launch, the state stays
    const size_t px = (size_t)c->frame.width * rows;
    const bool fresh = reset || c->chain_n == 0 || !c->d_chain || c->chain_pixels != px ||
                       !chain_shape_is(c, tile_rows, part, nparts) ||
                       std::memcmp(&c->frame, &c->chain_frame, sizeof c->frame) != 0;
    const uint32_t have = fresh ? 0u : c->chain_n;
    if (samples > 0xffffffffu - have) return fail(RTX_ERR_INVALID, std::string(fn) + ": more than 2^32 - 1 samples in all");
    if (!fresh && c->adapt_valid && c->adapt_mixed)
        return fail(RTX_ERR_STATE, std::string(fn) + ": the state's per-pixel sample counts differ after adaptive "
                                                     "steps: continue with rtx_refine_adaptive, or reset");
    rc = set_device(c);
    if (rc) return rc;
    rc = ensure_chain(c, px);
    if (rc) return rc;
    // the previous launch's cost map keys this one when the mode asks for it
    // and the map can (rtx_refine_keys.h); a fresh chain has none
    const uint32_t s_prev = fresh || c->chain_n == 0 ? 0u : c->cost_s_prev;
    const bool carried = rtx::launch_is_carried(c->refine_keys, s_prev, samples, c->n_pad > rtx::kScanPfMin);
    c->chain_n = 0;  // until the launch is enqueued
    c->cost_s_prev = 0;
    c->adapt_valid = c->adapt_mixed = false;  // uniform counts after this launch: the next adaptive call fills its maps
    c->chain_tile = tile_rows;
    c->chain_part = part;
    c->chain_nparts = nparts;
    RefineArgs a;
    a.cost_map = cost_map_of(c);
    a.carry_spp = carried ? s_prev : 0u;
    a.chain_in = fresh ? nullptr : c->d_chain;  // NULL: every pixel starts its chain (pixel_seed)
    a.chain_out = c->d_chain;
    a.samples = samples;
    a.out_n = have + samples;
    if (c->depth == 0) {
        // no segment is traced and the image is zeros (rtx_render's trivial
        // launch); the state keeps its sums (zeros for a fresh one) and N counts on
        if (fresh) RTX_HIP(hipMemsetAsync(c->d_chain, 0, px * sizeof(float4), c->stream));
        a.chain_in = a.chain_out = nullptr;
    }
    rc = render_impl(c, tile_rows, part, nparts, d_out, nullptr, 0, c->frame.frame_index, &a);
    if (rc != RTX_OK) return rc;
    c->chain_n = have + samples;
    c->chain_frame = c->frame;
    // every launch that traced segments leaves its map (none at depth 0, or
    // where a count could wrap)
    c->cost_s_prev = rtx::cost_map_after(samples, c->depth);
    c->last_keys = c->depth == 0 || samples < rtx::kLptMinSpp ? RTX_REFINE_KEYS_UNSCHEDULED
                   : carried                                  ? RTX_REFINE_KEYS_CARRIED
                                                              : RTX_REFINE_KEYS_PREPASS;
    return RTX_OK;
}

int rtx_refine(rtx_ctx *c, uint32_t samples, int reset) {
    return refine_rows_impl("rtx_refine", c, 1, 0, 1, samples, reset, nullptr);
}

int rtx_refine_rows(rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts, uint32_t samples, int reset,
                    void *d_out) {
    return refine_rows_impl("rtx_refine_rows", c, tile_rows, part, nparts, samples, reset, d_out);
}

int rtx_refine_shape(rtx_ctx *c, uint32_t *tile_rows, uint32_t *part, uint32_t *nparts) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_refine_shape: null ctx");
    if (c->chain_n == 0 || !c->d_chain) return fail(RTX_ERR_STATE, "rtx_refine_shape: no chain state");
    if (tile_rows) *tile_rows = c->chain_tile;
    if (part) *part = c->chain_part;
    if (nparts) *nparts = c->chain_nparts;
    return RTX_OK;
}

int rtx_refine_set_keys(rtx_ctx *c, int mode) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_refine_set_keys: null ctx");
    if (mode != RTX_REFINE_KEYS_PREPASS && mode != RTX_REFINE_KEYS_CARRIED)
        return fail(RTX_ERR_INVALID, "rtx_refine_set_keys: unknown mode");
    c->refine_keys = mode;  // the chain state and the map stay
    return RTX_OK;
}

int rtx_refine_last_keys(rtx_ctx *c) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_refine_last_keys: null ctx");
    return c->last_keys;
}

int rtx_refine_cost(rtx_ctx *c, uint32_t *host_cost, size_t bytes, uint32_t *samples) {
    if (!c || !host_cost || !samples) return fail(RTX_ERR_INVALID, "rtx_refine_cost: null argument");
    if (!cost_map_valid(c)) return fail(RTX_ERR_STATE, "rtx_refine_cost: no valid cost map");
    if (bytes != c->chain_pixels * sizeof(uint32_t))
        return fail(RTX_ERR_INVALID, "rtx_refine_cost: bytes != the state's pixels * 4 (width*height, or a part's "
                                     "rows * width)");
    int rc = set_device(c);
    if (rc) return rc;
    RTX_HIP(hipMemcpyAsync(host_cost, cost_map_of(c), bytes, hipMemcpyDeviceToHost, c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    *samples = c->cost_s_prev;
    return check_errors(c, "rtx_refine_cost");
}

uint32_t rtx_refined_samples(rtx_ctx *c) { return c ? c->chain_n : 0; }

void *rtx_refine_state(rtx_ctx *c) { return c && c->chain_n != 0 ? c->d_chain : nullptr; }

int rtx_refine_export(rtx_ctx *c, float *host_state, size_t bytes) {
    if (!c || !host_state) return fail(RTX_ERR_INVALID, "rtx_refine_export: null argument");
    if (c->chain_n == 0 || !c->d_chain) return fail(RTX_ERR_STATE, "rtx_refine_export: no chain state");
    if (bytes != c->chain_pixels * sizeof(float4))
        return fail(RTX_ERR_INVALID, "rtx_refine_export: bytes != the state's pixels * 16 (width*height, or a part's "
                                     "rows * width)");
    int rc = set_device(c);
    if (rc) return rc;
    RTX_HIP(hipMemcpyAsync(host_state, c->d_chain, bytes, hipMemcpyDeviceToHost, c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    return check_errors(c, "rtx_refine_export");
}

static int refine_import_impl(const char *fn, rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts,
                              const float *host_state, size_t bytes, uint32_t samples, void *d_out) {
    int rc = refine_rows_args(fn, c, tile_rows, part, nparts, samples);
    if (rc) return rc;
    rc = refine_rows_state(fn, c);
    if (rc) return rc;
    if (nparts == 1) tile_rows = 1;  // the whole-frame shape
    const uint32_t rows = rtx_part_rows(c->frame.height, tile_rows, part, nparts);
    const size_t px = (size_t)c->frame.width * rows;
    if (bytes != px * sizeof(float4))
        return fail(RTX_ERR_INVALID, std::string(fn) + ": bytes != rows*width*16 (the whole frame: width*height*16)");
    if (rows == 0) return RTX_OK;  // a part without rows: the state stays
    if (!host_state) return fail(RTX_ERR_INVALID, std::string(fn) + ": null host_state");
    rc = set_device(c);
    if (rc) return rc;
    c->chain_n = 0;
    c->cost_s_prev = 0;  // an installed state has no cost map: the next step takes the pre-pass
    c->adapt_valid = c->adapt_mixed = false;  // ... and is uniform
    rc = ensure_chain(c, px);
    if (rc) return rc;
    float4 *out = reinterpret_cast<float4 *>(d_out);
    if (!out && nparts == 1) {  // the context framebuffer, as rtx_refine's
        if (c->fb_pixels != px) {
            RTX_HIP(hipStreamSynchronize(c->stream));
            (void)hipFree(c->d_fb);
            c->d_fb = nullptr;
            c->fb_pixels = 0;
            RTX_HIP(hipMalloc(&c->d_fb, px * sizeof(float4)));
            c->fb_pixels = px;
        }
        out = c->d_fb;
    }
    // synchronous, like rtx_copy_to_device: the caller's array is free on return
    RTX_HIP(hipMemcpyAsync(c->d_chain, host_state, bytes, hipMemcpyHostToDevice, c->stream));
    if (out) {  // (a part without d_out: no image)
        hipError_t e = rtx::launch_chain_image(c->d_chain, out, px, samples, c->stream);
        if (e != hipSuccess) return hip_fail(e, "launch_chain_image");
    }
    RTX_HIP(hipStreamSynchronize(c->stream));
    c->chain_n = samples;
    c->chain_frame = c->frame;
    c->chain_tile = tile_rows;
    c->chain_part = part;
    c->chain_nparts = nparts;
    return RTX_OK;
}

int rtx_refine_import(rtx_ctx *c, const float *host_state, size_t bytes, uint32_t samples) {
    if (!c || !host_state) return fail(RTX_ERR_INVALID, "rtx_refine_import: null argument");
    return refine_import_impl("rtx_refine_import", c, 1, 0, 1, host_state, bytes, samples, nullptr);
}

int rtx_refine_import_rows(rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts, const float *host_state,
                           size_t bytes, uint32_t samples, void *d_out) {
    return refine_import_impl("rtx_refine_import_rows", c, tile_rows, part, nparts, host_state, bytes, samples, d_out);
}

// ---- adaptive refinement (rtx_adaptive.h) ----------------------------------
float rtx_adaptive_error(const float sum_old[3], uint32_t n_old, const float sum_new[3], uint32_t n_new) {
    return rtx::adaptive_error_with(sum_old, n_old, sum_new, n_new, [](float v) { return sqrtf(v); });
}

// The adaptive maps' allocation: count[px] uint32, err[px] float, the active
// count (one word, padded to 4), then the flags, px bytes.
static size_t adapt_bytes(size_t px) { return (2 * px + 4) * sizeof(uint32_t) + px; }
static rtx::KAdaptive adapt_maps(const rtx_ctx *c) {
    rtx::KAdaptive a{};
    a.count = c->d_adapt;
    a.err = reinterpret_cast<float *>(c->d_adapt + c->adapt_pixels);
    a.n_active = c->d_adapt + 2 * c->adapt_pixels;
    a.flags = reinterpret_cast<uint8_t *>(c->d_adapt + 2 * c->adapt_pixels + 4);
    return a;
}
// A chain state of a row part (nparts > 1): the whole-frame entry points
// refuse it (their maps and their 3 x 3 window are a whole frame's).
static bool part_state(const rtx_ctx *c) { return c->chain_n != 0 && c->d_chain && c->chain_nparts > 1; }
static const char *const kPartStateWhy =
    "the chain state covers a row part (nparts > 1): continue it with rtx_refine_adaptive_rows / "
    "rtx_refine_pending_rows and read it with rtx_refine_counts_rows / rtx_refine_error_rows; or reset";
// A call's partition: part `part` of `nparts` in tiles of `tile_rows` (the
// whole frame: (1, 0, 1) whatever tile_rows, as rtx_refine_rows).
struct AdaptShape {
    uint32_t tile_rows, part, nparts;
    bool whole_only;  // rtx_refine_adaptive / rtx_refine_pending: a part state is refused, not restarted
};
static const AdaptShape kWholeFrame = {1u, 0u, 1u, true};
static uint32_t shape_rows(const rtx_ctx *c, const AdaptShape &s) {
    return rtx_part_rows(c->frame.height, s.tile_rows, s.part, s.nparts);
}
// Whether a call continues the context's chain state (else it starts fresh).
static bool chain_continues(const rtx_ctx *c, const AdaptShape &s, int reset) {
    const size_t px = (size_t)c->frame.width * shape_rows(c, s);
    return !reset && c->chain_n != 0 && c->d_chain && c->chain_pixels == px &&
           chain_shape_is(c, s.tile_rows, s.part, s.nparts) &&
           std::memcmp(&c->frame, &c->chain_frame, sizeof c->frame) == 0;
}
// The argument and state rules the calls share, decided before any HIP call.
// *s: the call's partition, normalised here. need_out: rtx_refine_adaptive_rows.
static int adaptive_check(const rtx_ctx *c, const char *fn, AdaptShape *s, uint32_t samples, float threshold,
                          uint32_t max_samples, int reset, const void *d_halo, bool need_out, const void *d_out) {
    char buf[320];
    auto bad = [&](int code, const char *why) {
        std::snprintf(buf, sizeof buf, "%s: %s", fn, why);
        return fail(code, buf);
    };
    if (!c) return bad(RTX_ERR_INVALID, "null ctx");
    if (const char *why = rtx::adaptive_args_error(samples, threshold, max_samples)) return bad(RTX_ERR_INVALID, why);
    if (s->tile_rows == 0 || s->nparts == 0 || s->part >= s->nparts)
        return bad(RTX_ERR_INVALID, "bad partition (tile_rows, part, nparts)");
    if (need_out && !d_out && s->nparts > 1) return bad(RTX_ERR_INVALID, "d_out NULL needs nparts == 1");
    if (s->nparts == 1) s->tile_rows = 1;
    if (!c->have_world) return bad(RTX_ERR_STATE, "no world uploaded");
    if (!c->have_frame) return bad(RTX_ERR_STATE, "no frame set");
    if (c->frame.rng_mode == RTX_RNG_PER_SAMPLE) return bad(RTX_ERR_INVALID, "the per-sample RNG has no chain to continue");
    if (const char *why = rtx::ctx_adaptive_refusal(c, samples)) return bad(RTX_ERR_INVALID, why);
    if (s->whole_only && !reset && part_state(c)) return bad(RTX_ERR_STATE, kPartStateWhy);
    const bool goes_on = chain_continues(c, *s, reset);
    if (samples > 0xffffffffu - (goes_on ? c->chain_n : 0u)) return bad(RTX_ERR_INVALID, "more than 2^32 - 1 samples in all");
    // (a fresh or uniform state reads no halo: every err is +inf)
    if (s->nparts > 1 && !d_halo && goes_on && c->adapt_valid)
        return bad(RTX_ERR_INVALID, "d_halo NULL needs nparts == 1, or a fresh or uniform state");
    return RTX_OK;
}
// What a uniform state of `have` samples answers without its maps: every error
// is +inf (>= any threshold), so only the cap decides.
static uint32_t uniform_active(size_t px, uint32_t have, uint32_t samples, uint32_t max_samples) {
    return max_samples == 0u || (uint64_t)have + samples <= max_samples ? (uint32_t)px : 0u;
}
// The flags of a call over valid maps and their number (synchronous: the
// 4-byte count comes back to the host, which sizes the launch by it). The
// whole frame takes k_adaptive_mask, a part k_adaptive_mask_rows with d_halo;
// d_mask (rtx_refine_masked, whole frame): k_masked_flags, the caller's mask
// in the place of the error test.
static int adaptive_mask(rtx_ctx *c, const AdaptShape &s, uint32_t samples, float threshold, uint32_t max_samples,
                         const void *d_halo, rtx::KAdaptive *a, const void *d_mask = nullptr) {
    *a = adapt_maps(c);
    hipError_t e;
    if (d_mask)
        e = rtx::launch_masked_flags(*a, static_cast<const uint8_t *>(d_mask), c->frame.width, c->frame.height, samples,
                                     max_samples, c->stream);
    else if (s.nparts == 1)
        e = rtx::launch_adaptive_mask(*a, c->frame.width, c->frame.height, samples, threshold, max_samples, c->stream);
    else
        e = rtx::launch_adaptive_mask_rows(*a, static_cast<const float *>(d_halo), c->frame.width, shape_rows(c, s),
                                           c->frame.height, s.tile_rows, s.part, s.nparts, samples, threshold,
                                           max_samples, c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_adaptive_mask");
    RTX_HIP(hipMemcpyAsync(&a->active, a->n_active, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    return RTX_OK;
}

// rtx_refine_adaptive, rtx_refine_adaptive_rows and rtx_refine_masked (checked
// already; d_mask: the masked call, which continues a whole-frame state).
static int adaptive_impl(rtx_ctx *c, const AdaptShape &s, uint32_t samples, float threshold, uint32_t max_samples,
                         int reset, const void *d_halo, void *d_out, uint32_t *active, const void *d_mask = nullptr) {
    const uint32_t rows = shape_rows(c, s);
    if (rows == 0) {  // a part without rows: nothing to launch, the state stays
        if (active) *active = 0;
        return RTX_OK;
    }
    const size_t px = (size_t)c->frame.width * rows;
    const bool fresh = !chain_continues(c, s, reset);
    const uint32_t have = fresh ? 0u : c->chain_n;
    int rc = set_device(c);
    if (rc) return rc;
    rc = ensure_chain(c, px);
    if (rc) return rc;
    if (fresh) c->chain_tile = s.tile_rows, c->chain_part = s.part, c->chain_nparts = s.nparts;
    if (!c->d_adapt || c->adapt_pixels != px) {
        RTX_HIP(hipStreamSynchronize(c->stream));
        (void)hipFree(c->d_adapt);
        c->d_adapt = nullptr;
        c->adapt_pixels = 0;
        c->adapt_valid = false;
        RTX_HIP(hipMalloc(&c->d_adapt, adapt_bytes(px)));
        c->adapt_pixels = px;
    }
    const bool uniform = fresh || !c->adapt_valid;
    if (uniform) {  // a uniform state of `have` samples, no estimate yet
        const rtx::KAdaptive m = adapt_maps(c);
        RTX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m.count), (int)have, px, c->stream));
        RTX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(m.err), 0x7f800000, px, c->stream));
        c->adapt_valid = !fresh;  // (a fresh start: only once its launch is enqueued)
        c->adapt_mixed = false;
    }
    rtx::KAdaptive ka;
    // (a uniform state reads no halo: a caller's buffer may hold anything then)
    rc = adaptive_mask(c, s, samples, threshold, max_samples, uniform ? nullptr : d_halo, &ka, d_mask);
    if (rc) return rc;
    if (active) *active = ka.active;
    if (ka.active == 0) {  // (never a fresh start: its errors are +inf and its counts 0)
        c->last_keys = RTX_REFINE_KEYS_UNSCHEDULED;
        return RTX_OK;
    }
    // a caller's d_out holds every pixel of the part after the call, whatever
    // was in it: the pixels this call leaves alone come from the state
    if (d_out && ka.active != px) {
        hipError_t e = rtx::launch_chain_image_counts(c->d_chain, ka.count, ka.flags, reinterpret_cast<float4 *>(d_out),
                                                      px, c->stream);
        if (e != hipSuccess) return hip_fail(e, "launch_chain_image_counts");
    }
    // keyed by the cost map wherever it is valid, whatever rtx_refine_set_keys
    // says and however few samples it covers; else every key is equal
    const uint32_t s_prev = fresh ? 0u : c->cost_s_prev;
    c->chain_n = 0;  // until the launch is enqueued
    c->cost_s_prev = 0;
    c->adapt_valid = false;
    RefineArgs a;
    a.cost_map = cost_map_of(c);
    a.carry_spp = s_prev;
    a.chain_in = fresh ? nullptr : c->d_chain;  // NULL: every count is 0, every pixel starts its chain
    a.chain_out = c->d_chain;
    a.samples = samples;
    a.out_n = 0;  // (each pixel divides by its own count)
    a.adaptive = &ka;
    rc = render_impl(c, s.tile_rows, s.part, s.nparts, d_out, nullptr, 0, c->frame.frame_index, &a);
    if (rc != RTX_OK) return rc;
    c->chain_n = have + samples;
    c->chain_frame = c->frame;
    c->cost_s_prev = rtx::cost_map_after(samples, c->depth);
    c->last_keys = RTX_REFINE_KEYS_CARRIED;
    c->adapt_valid = true;
    if (ka.active != px) c->adapt_mixed = true;
    return RTX_OK;
}

// rtx_refine_pending and rtx_refine_pending_rows (checked already).
static int pending_impl(rtx_ctx *c, const AdaptShape &s, uint32_t samples, float threshold, uint32_t max_samples,
                        const void *d_halo, uint32_t *active) {
    const size_t px = (size_t)c->frame.width * shape_rows(c, s);
    const bool fresh = !chain_continues(c, s, 0);
    if (px == 0 || fresh || !c->adapt_valid || !c->d_adapt || c->adapt_pixels != px) {
        *active = uniform_active(px, fresh ? 0u : c->chain_n, samples, max_samples);
        return RTX_OK;
    }
    int rc = set_device(c);
    if (rc) return rc;
    rtx::KAdaptive ka;
    rc = adaptive_mask(c, s, samples, threshold, max_samples, d_halo, &ka);
    if (rc) return rc;
    *active = ka.active;
    return RTX_OK;
}

int rtx_refine_adaptive(rtx_ctx *c, uint32_t samples, float threshold, uint32_t max_samples, int reset,
                        uint32_t *active) {
    AdaptShape s = kWholeFrame;
    const int rc = adaptive_check(c, "rtx_refine_adaptive", &s, samples, threshold, max_samples, reset, nullptr, false,
                                  nullptr);
    if (rc) return rc;
    return adaptive_impl(c, s, samples, threshold, max_samples, reset, nullptr, nullptr, active);
}

int rtx_refine_adaptive_rows(rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts, uint32_t samples,
                             float threshold, uint32_t max_samples, int reset, const void *d_halo, void *d_out,
                             uint32_t *active) {
    AdaptShape s = {tile_rows, part, nparts, false};
    const int rc = adaptive_check(c, "rtx_refine_adaptive_rows", &s, samples, threshold, max_samples, reset, d_halo, true,
                                  d_out);
    if (rc) return rc;
    return adaptive_impl(c, s, samples, threshold, max_samples, reset, d_halo, d_out, active);
}

int rtx_refine_pending(rtx_ctx *c, uint32_t samples, float threshold, uint32_t max_samples, uint32_t *active) {
    AdaptShape s = kWholeFrame;
    const int rc = adaptive_check(c, "rtx_refine_pending", &s, samples, threshold, max_samples, 0, nullptr, false, nullptr);
    if (rc) return rc;
    if (!active) return fail(RTX_ERR_INVALID, "rtx_refine_pending: null active");
    return pending_impl(c, s, samples, threshold, max_samples, nullptr, active);
}

int rtx_refine_pending_rows(rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts, uint32_t samples,
                            float threshold, uint32_t max_samples, const void *d_halo, uint32_t *active) {
    AdaptShape s = {tile_rows, part, nparts, false};
    const int rc = adaptive_check(c, "rtx_refine_pending_rows", &s, samples, threshold, max_samples, 0, d_halo, false,
                                  nullptr);
    if (rc) return rc;
    if (!active) return fail(RTX_ERR_INVALID, "rtx_refine_pending_rows: null active");
    return pending_impl(c, s, samples, threshold, max_samples, d_halo, active);
}

int rtx_refine_masked(rtx_ctx *c, uint32_t samples, const void *d_mask, uint32_t max_samples, uint32_t *active) {
    const char *fn = "rtx_refine_masked";
    if (!d_mask && c) return fail(RTX_ERR_INVALID, "rtx_refine_masked: null mask");
    AdaptShape s = kWholeFrame;
    // (the threshold plays no part: the mask stands in for the error test)
    const int rc = adaptive_check(c, fn, &s, samples, 0.0f, max_samples, 0, nullptr, false, nullptr);
    if (rc) return rc;
    if (!chain_continues(c, s, 0))
        return fail(RTX_ERR_STATE, "rtx_refine_masked: no whole-frame chain state for this world and frame (start one with "
                                   "rtx_refine, rtx_refine_adaptive or rtx_refine_import)");
    return adaptive_impl(c, s, samples, 0.0f, max_samples, 0, nullptr, nullptr, active, d_mask);
}

int rtx_refine_edges(rtx_ctx *c, void *d_edges) {
    if (!c || !d_edges) return fail(RTX_ERR_INVALID, "rtx_refine_edges: null argument");
    if (c->chain_n == 0 || !c->d_chain) return fail(RTX_ERR_STATE, "rtx_refine_edges: no chain state");
    int rc = set_device(c);
    if (rc) return rc;
    const bool maps = c->adapt_valid && c->d_adapt && c->adapt_pixels == c->chain_pixels;
    const uint32_t width = c->chain_frame.width;  // (the state's frame: c->frame may have moved on)
    const uint32_t rows = (uint32_t)(c->chain_pixels / width);
    hipError_t e = rtx::launch_adaptive_edges(maps ? adapt_maps(c).err : nullptr, width, rows, c->chain_tile,
                                              static_cast<float *>(d_edges), c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_adaptive_edges");
    return RTX_OK;
}

// The four readers: map 0 / 1, or a uniform state's value. `rows`: a state of
// any shape in its own row order; else a part state is refused.
static int adaptive_read(rtx_ctx *c, const char *fn, int which, bool rows, void *host, size_t bytes) {
    char buf[128];
    if (!c || !host) {
        std::snprintf(buf, sizeof buf, "%s: null argument", fn);
        return fail(RTX_ERR_INVALID, buf);
    }
    if (c->chain_n == 0 || !c->d_chain) {
        std::snprintf(buf, sizeof buf, "%s: no chain state", fn);
        return fail(RTX_ERR_STATE, buf);
    }
    if (!rows && part_state(c)) return fail(RTX_ERR_STATE, std::string(fn) + ": " + kPartStateWhy);
    if (bytes != c->chain_pixels * sizeof(uint32_t)) {
        std::snprintf(buf, sizeof buf, rows ? "%s: bytes != the state's rows * width * 4" : "%s: bytes != width*height*4",
                      fn);
        return fail(RTX_ERR_INVALID, buf);
    }
    if (!c->adapt_valid || !c->d_adapt || c->adapt_pixels != c->chain_pixels) {
        const uint32_t v = which == 0 ? c->chain_n : 0x7f800000u;
        uint32_t *w = static_cast<uint32_t *>(host);
        for (size_t i = 0; i < c->chain_pixels; ++i) w[i] = v;
        return RTX_OK;
    }
    int rc = set_device(c);
    if (rc) return rc;
    RTX_HIP(hipMemcpyAsync(host, c->d_adapt + (size_t)which * c->adapt_pixels, bytes, hipMemcpyDeviceToHost, c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    return check_errors(c, fn);
}
int rtx_refine_counts(rtx_ctx *c, uint32_t *host, size_t bytes) {
    return adaptive_read(c, "rtx_refine_counts", 0, false, host, bytes);
}
int rtx_refine_error(rtx_ctx *c, float *host, size_t bytes) {
    return adaptive_read(c, "rtx_refine_error", 1, false, host, bytes);
}
int rtx_refine_counts_rows(rtx_ctx *c, uint32_t *host, size_t bytes) {
    return adaptive_read(c, "rtx_refine_counts_rows", 0, true, host, bytes);
}
int rtx_refine_error_rows(rtx_ctx *c, float *host, size_t bytes) {
    return adaptive_read(c, "rtx_refine_error_rows", 1, true, host, bytes);
}

extern "C++" {
namespace rtx {  // for rtx_group.hip (rtx_internal.h)
const char *ctx_adaptive_refusal(const ::rtx_ctx *c, uint32_t samples) {
    if (c->depth == 0) return "depth is 0: nothing to estimate an error from";
    if (!cost_map_fits(samples, c->depth)) return "samples * depth does not fit 32 bits";
    return nullptr;
}
int ctx_state_image(::rtx_ctx *c, void *d_out) {
    if (!c || !d_out) return fail(RTX_ERR_INVALID, "ctx_state_image: null argument");
    if (c->chain_n == 0 || !c->d_chain) return fail(RTX_ERR_STATE, "ctx_state_image: no chain state");
    int rc = set_device(c);
    if (rc) return rc;
    float4 *out = reinterpret_cast<float4 *>(d_out);
    hipError_t e;
    if (c->adapt_valid && c->d_adapt && c->adapt_pixels == c->chain_pixels)
        e = launch_chain_image_counts(c->d_chain, adapt_maps(c).count, nullptr, out, c->chain_pixels, c->stream);
    else  // a uniform state
        e = launch_chain_image(c->d_chain, out, c->chain_pixels, c->chain_n, c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_chain_image");
    return RTX_OK;
}
}  // namespace rtx
}  // extern "C++"

int rtx_deinterleave_rows(rtx_ctx *c, const void *d_gathered, uint32_t width, uint32_t height,
                          uint32_t tile_rows, uint32_t nparts, void *d_image) {
    if (!c || !d_gathered || !d_image) return fail(RTX_ERR_INVALID, "rtx_deinterleave_rows: null argument");
    if (tile_rows == 0 || nparts == 0) return fail(RTX_ERR_INVALID, "rtx_deinterleave_rows: bad partition");
    int rc = set_device(c);
    if (rc) return rc;
    const uint32_t max_rows = rtx_part_rows(height, tile_rows, 0, nparts);  // part 0 is largest
    hipError_t e = rtx::launch_deinterleave(reinterpret_cast<const float4 *>(d_gathered),
                                            reinterpret_cast<float4 *>(d_image), width, height,
                                            tile_rows, nparts, max_rows, c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_deinterleave");
    return RTX_OK;
}

int rtx_sync(rtx_ctx *c) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_sync: null ctx");
    int rc = set_device(c);
    if (rc) return rc;
    RTX_HIP(hipStreamSynchronize(c->stream));
    return check_errors(c, "rtx_sync");
}

void *rtx_framebuffer(rtx_ctx *c) { return c ? c->d_fb : nullptr; }

int rtx_download(rtx_ctx *c, float *host, size_t bytes) {
    if (!c || !host) return fail(RTX_ERR_INVALID, "rtx_download: null argument");
    if (!c->d_fb) return fail(RTX_ERR_STATE, "rtx_download: nothing rendered into the context framebuffer");
    if (bytes != c->fb_pixels * sizeof(float4))
        return fail(RTX_ERR_INVALID, "rtx_download: bytes != width*height*16");
    int rc = set_device(c);
    if (rc) return rc;
    RTX_HIP(hipMemcpyAsync(host, c->d_fb, bytes, hipMemcpyDeviceToHost, c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    return check_errors(c, "rtx_download");
}

int rtx_stats_reset(rtx_ctx *c) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_stats_reset: null ctx");
    int rc = set_device(c);
    if (rc) return rc;
    rc = check_errors(c, "rtx_stats_reset");  // an unreported error of earlier launches
    RTX_HIP(hipMemsetAsync(c->d_counters, 0, kCounterWords * sizeof(unsigned long long), c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    c->ev_head = 0;
    c->ev_count = 0;
    c->ms_folded = 0.0;
    c->samples = 0;
    c->launches = 0;
    c->n_changed = false;
    return rc;
}

int rtx_get_stats(rtx_ctx *c, rtx_stats *out) {
    if (!c || !out) return fail(RTX_ERR_INVALID, "rtx_get_stats: null argument");
    if (c->n_changed) return fail(RTX_ERR_STATE, "rtx_get_stats: world changed since rtx_stats_reset");
    int rc = set_device(c);
    if (rc) return rc;
    RTX_HIP(hipStreamSynchronize(c->stream));
    rc = check_errors(c, "rtx_get_stats");
    if (rc) return rc;
    unsigned long long h[4];
    RTX_HIP(hipMemcpyAsync(h, c->d_counters, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    double ms = c->ms_folded;
    for (size_t i = 0; i < c->ev_count; ++i) {
        const EventPair &p = c->events[(c->ev_head + i) % c->events.size()];
        float t = 0.0f;
        RTX_HIP(hipEventElapsedTime(&t, p.start, p.stop));
        ms += t;
    }
    out->kernel_ms = ms;
    out->launches = c->launches;
    out->samples = c->samples;
    out->segments = h[0];
    out->sphere_tests = h[0] * (uint64_t)c->n;
    return RTX_OK;
}

int rtx_alloc(rtx_ctx *c, size_t bytes, void **d_ptr) {
    if (!c || !d_ptr) return fail(RTX_ERR_INVALID, "rtx_alloc: null argument");
    *d_ptr = nullptr;
    int rc = set_device(c);
    if (rc) return rc;
    hipError_t e = hipMalloc(d_ptr, bytes ? bytes : 1);
    if (e == hipErrorOutOfMemory) return fail(RTX_ERR_NOMEM, "rtx_alloc: out of device memory");
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    return RTX_OK;
}

int rtx_free(rtx_ctx *c, void *d_ptr) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_free: null ctx");
    if (!d_ptr) return RTX_OK;
    int rc = set_device(c);
    if (rc) return rc;
    RTX_HIP(hipStreamSynchronize(c->stream));
    RTX_HIP(hipFree(d_ptr));
    return RTX_OK;
}

int rtx_copy_to_host(rtx_ctx *c, void *host, const void *d_src, size_t bytes) {
    if (!c || ((!host || !d_src) && bytes)) return fail(RTX_ERR_INVALID, "rtx_copy_to_host: null argument");
    if (!bytes) return RTX_OK;
    int rc = set_device(c);
    if (rc) return rc;
    RTX_HIP(hipMemcpyAsync(host, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    return RTX_OK;
}

int rtx_copy_to_device(rtx_ctx *c, void *d_dst, const void *host, size_t bytes) {
    if (!c || ((!host || !d_dst) && bytes)) return fail(RTX_ERR_INVALID, "rtx_copy_to_device: null argument");
    if (!bytes) return RTX_OK;
    int rc = set_device(c);
    if (rc) return rc;
    RTX_HIP(hipMemcpyAsync(d_dst, host, bytes, hipMemcpyHostToDevice, c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    return RTX_OK;
}

// ---- first-hit feature buffers, picking, the id mask (rtx_features.h) --------
static rtx::KFeatures features_of(const rtx_ctx *c, uint32_t rows, uint32_t tile_rows, uint32_t part, uint32_t nparts) {
    const rtx_frame &f = c->frame;
    rtx::KFeatures k{};
    for (int i = 0; i < 3; ++i) {
        k.org[i] = f.origin[i];
        k.hor[i] = f.horizontal[i];
        k.ver[i] = f.vertical[i];
        k.llc[i] = f.lower_left[i];
    }
    k.img_w = f.img_w;
    k.img_h = f.img_h;
    k.width = f.width;
    k.rows_local = rows;
    k.tile_rows = tile_rows;
    k.part = part;
    k.nparts = nparts;
    return k;
}
// The context's feature scratch: 64 bytes of words, then `more` bytes.
static int ensure_feat(rtx_ctx *c, size_t more) {
    const size_t need = 64 + more;
    if (c->d_feat && c->feat_bytes >= need) return RTX_OK;
    RTX_HIP(hipStreamSynchronize(c->stream));
    (void)hipFree(c->d_feat);
    c->d_feat = nullptr;
    c->feat_bytes = 0;
    RTX_HIP(hipMalloc(&c->d_feat, need));
    c->feat_bytes = need;
    return RTX_OK;
}

int rtx_features_rows(rtx_ctx *c, uint32_t tile_rows, uint32_t part, uint32_t nparts, void *d_geom, void *d_surf) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_features_rows: null ctx");
    if (!d_geom && !d_surf) return fail(RTX_ERR_INVALID, "rtx_features_rows: both planes are NULL");
    if (tile_rows == 0 || nparts == 0 || part >= nparts)
        return fail(RTX_ERR_INVALID, "rtx_features_rows: bad partition (tile_rows, part, nparts)");
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_features_rows: no world uploaded");
    if (!c->have_frame) return fail(RTX_ERR_STATE, "rtx_features_rows: no frame set");
    const uint32_t rows = rtx_part_rows(c->frame.height, tile_rows, part, nparts);
    if (rows == 0 || c->frame.width == 0) return RTX_OK;  // a part without rows: nothing to launch
    int rc = set_device(c);
    if (rc) return rc;
    const hipError_t e = rtx::launch_features(scene_of(c), features_of(c, rows, tile_rows, part, nparts),
                                              static_cast<float4 *>(d_geom), static_cast<float4 *>(d_surf), nullptr,
                                              c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_features");
    return RTX_OK;
}

int rtx_features(rtx_ctx *c, void *d_geom, void *d_surf) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_features: null ctx");
    if (!d_geom && !d_surf) return fail(RTX_ERR_INVALID, "rtx_features: both planes are NULL");
    return rtx_features_rows(c, 1, 0, 1, d_geom, d_surf);
}

int rtx_pick(rtx_ctx *c, uint32_t x, uint32_t y, rtx_hit *out) {
    if (!c || !out) return fail(RTX_ERR_INVALID, "rtx_pick: null argument");
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_pick: no world uploaded");
    if (!c->have_frame) return fail(RTX_ERR_STATE, "rtx_pick: no frame set");
    if (x >= c->frame.width || y >= c->frame.height) return fail(RTX_ERR_INVALID, "rtx_pick: the pixel is outside the frame");
    int rc = set_device(c);
    if (rc) return rc;
    rc = ensure_feat(c, 0);
    if (rc) return rc;
    // the planes' kernel on the one pixel: a 1 x 1 part whose only row is y
    rtx::KFeatures k = features_of(c, 1, 1, y, c->frame.height);
    k.width = 1;
    k.x0 = x;
    float4 *d = reinterpret_cast<float4 *>(c->d_feat);  // geom, surf, extra[2]
    hipError_t e = rtx::launch_features(scene_of(c), k, d, d + 1, d + 2, c->stream);
    float4 h[4];
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof h, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(e, "rtx_pick");
    std::memset(out, 0, sizeof *out);
    out->index = (int32_t)h[1].w;
    out->hit = out->index >= 0 ? 1u : 0u;
    out->depth = h[0].w;
    if (out->hit) {
        out->front_face = h[3].x != 0.0f ? 1u : 0u;
        out->material = (uint32_t)h[3].y;
        out->t = h[2].w;
        out->p[0] = h[2].x, out->p[1] = h[2].y, out->p[2] = h[2].z;
        out->normal[0] = h[0].x, out->normal[1] = h[0].y, out->normal[2] = h[0].z;
        out->albedo[0] = h[1].x, out->albedo[1] = h[1].y, out->albedo[2] = h[1].z;
        out->mat_param = h[3].z;
    }
    return RTX_OK;
}

int rtx_mask_from_ids(rtx_ctx *c, const void *d_surf, const uint32_t *ids, uint32_t n, uint32_t grow, void *d_mask,
                      uint32_t *set) {
    if (!c || !d_surf || !ids || !d_mask) return fail(RTX_ERR_INVALID, "rtx_mask_from_ids: null argument");
    if (n == 0 || n > rtx::kFeatureIdsMax) return fail(RTX_ERR_INVALID, "rtx_mask_from_ids: n outside 1 .. 256");
    if (grow > rtx::kFeatureGrowMax) return fail(RTX_ERR_INVALID, "rtx_mask_from_ids: grow above 8");
    if (!c->have_frame) return fail(RTX_ERR_STATE, "rtx_mask_from_ids: no frame set");
    const size_t px = (size_t)c->frame.width * c->frame.height;
    int rc = set_device(c);
    if (rc) return rc;
    rc = ensure_feat(c, px);
    if (rc) return rc;
    uint32_t *d_set = reinterpret_cast<uint32_t *>(c->d_feat);
    const hipError_t e = rtx::launch_feature_mask(static_cast<const float4 *>(d_surf), c->frame.width, c->frame.height,
                                                  ids, n, grow, c->d_feat + 64, static_cast<uint8_t *>(d_mask), d_set,
                                                  c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_feature_mask");
    if (set) {
        RTX_HIP(hipMemcpyAsync(set, d_set, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        RTX_HIP(hipStreamSynchronize(c->stream));
    }
    return RTX_OK;
}

// ---- batched closest-hit ray queries (rtx_cast.h) -----------------------------
static_assert(sizeof(rtx_ray) == 32 && sizeof(rtx_ray_hit) == 32, "rtx_cast_rays: two float4 per record");
// The COHERENT order's scratch for n rays. Once it fits there is no host wait.
static int ensure_cast(rtx_ctx *c, size_t n) {
    if (c->d_cast && c->cast_rays >= n) return RTX_OK;
    RTX_HIP(hipStreamSynchronize(c->stream));
    (void)hipFree(c->d_cast);
    c->d_cast = nullptr;
    c->cast_rays = 0;
    RTX_HIP(hipMalloc(&c->d_cast, (rtx::kCastBuckets + 2 * n) * sizeof(uint32_t)));
    c->cast_rays = n;
    return RTX_OK;
}

int rtx_cast_rays(rtx_ctx *c, const void *d_rays, uint32_t n, float t_min, uint32_t order, void *d_hits,
                  void *d_occluded) {
    // the argument rules first: none of them looks at the context
    if (!c) return fail(RTX_ERR_INVALID, "rtx_cast_rays: null ctx");
    if (n != 0 && !d_rays) return fail(RTX_ERR_INVALID, "rtx_cast_rays: d_rays is NULL");
    if (n != 0 && !d_hits && !d_occluded) return fail(RTX_ERR_INVALID, "rtx_cast_rays: both outputs are NULL");
    // the resolve compares roots by their bit patterns, which order like the values only for roots > 0
    if (!(t_min > 0.0f && t_min <= 3.4028235e38f))
        return fail(RTX_ERR_INVALID, "rtx_cast_rays: t_min must be finite and > 0");
    if (order != RTX_CAST_ORDER_AUTO && order != RTX_CAST_ORDER_GIVEN && order != RTX_CAST_ORDER_COHERENT)
        return fail(RTX_ERR_INVALID, "rtx_cast_rays: unknown order");
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_cast_rays: no world uploaded");
    if (n == 0) return RTX_OK;
    const rtx::KScene s = scene_of(c);
    const bool sort = order == RTX_CAST_ORDER_COHERENT ||
                      (order == RTX_CAST_ORDER_AUTO && rtx::cast_auto_coherent(n, rtx::scene_kernels(s).kernels));
    int rc = set_device(c);
    if (rc) return rc;
    const float4 *rays = static_cast<const float4 *>(d_rays);
    const uint32_t *perm = nullptr;
    if (sort) {
        c->paths_perm_valid = false;  // (the scratch is about to hold another order)
        rc = ensure_cast(c, n);
        if (rc) return rc;
        const rtx::KCastScratch k{c->d_cast, c->d_cast + rtx::kCastBuckets, c->d_cast + rtx::kCastBuckets + c->cast_rays};
        const hipError_t e = rtx::launch_cast_order(rays, n, c->cast_box, k, c->stream);
        if (e != hipSuccess) return hip_fail(e, "launch_cast_order");
        perm = k.perm;
    }
    const hipError_t e = rtx::launch_cast(s, rays, n, t_min, perm, static_cast<float4 *>(d_hits),
                                          static_cast<uint8_t *>(d_occluded), c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_cast");
    c->cast_last = sort ? RTX_CAST_ORDER_COHERENT : RTX_CAST_ORDER_GIVEN;
    return RTX_OK;
}

int rtx_cast_last_order(rtx_ctx *c) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_cast_last_order: null ctx");
    return c->cast_last;
}

// ---- path queries along caller-chosen rays (rtx_paths.h) ----------------------
static_assert(sizeof(rtx_path_query) == rtx::kPathRayBytes && sizeof(rtx_path_result) == rtx::kPathResultBytes,
              "rtx_trace_paths: two float4 per query, one per result");
static_assert(offsetof(rtx_path_query, o) == offsetof(rtx_ray, o) && offsetof(rtx_path_query, d) == offsetof(rtx_ray, d),
              "the COHERENT passes read a query's o and d where a ray's are");
static_assert(RTX_PATHS_LAMBERT_GUARD == rtx::kPathsLambertGuard && RTX_PATHS_CONTINUE == rtx::kPathsContinue &&
                  RTX_CAST_ORDER_COHERENT == rtx::kPathsOrderMax && rtx::kFrameLambertGuard == 1u,
              "rtx_paths.h restates these");

int rtx_trace_paths(rtx_ctx *c, const void *d_queries, uint32_t n, uint32_t samples, uint32_t flags, uint32_t order,
                    void *d_results, void *d_segments) {
    // the argument rules first (rtx_paths.h): none of them looks at the context
    if (!c) return fail(RTX_ERR_INVALID, "rtx_trace_paths: null ctx");
    switch (rtx::paths_args(d_queries != nullptr, d_results != nullptr, n, samples, flags, order)) {
    case rtx::kPathsArgQueries: return fail(RTX_ERR_INVALID, "rtx_trace_paths: d_queries is NULL");
    case rtx::kPathsArgResults: return fail(RTX_ERR_INVALID, "rtx_trace_paths: d_results is NULL");
    case rtx::kPathsArgSamples: return fail(RTX_ERR_INVALID, "rtx_trace_paths: samples is 0");
    case rtx::kPathsArgFlags: return fail(RTX_ERR_INVALID, "rtx_trace_paths: unknown flags");
    case rtx::kPathsArgOrder: return fail(RTX_ERR_INVALID, "rtx_trace_paths: unknown order");
    case rtx::kPathsArgOk: break;
    }
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_trace_paths: no world uploaded");
    switch (rtx::paths_world(samples, c->depth)) {
    case rtx::kPathsWorldDepth0: return fail(RTX_ERR_INVALID, "rtx_trace_paths: the world's depth is 0");
    case rtx::kPathsWorldCount: return fail(RTX_ERR_INVALID, "rtx_trace_paths: samples * depth does not fit 32 bits");
    case rtx::kPathsWorldOk: break;
    }
    if (n == 0) return RTX_OK;
    rtx::KPaths p;
    p.scene = scene_of(c);
    p.depth = c->depth;
    p.flags = rtx::paths_frame_flags(flags);
    p.samples = samples;
    p.n = n;
    p.mode = flags & rtx::kPathsContinue;
    // AUTO is GIVEN: only a query's first segment follows the batch's order
    // (RESULTS.md: where COHERENT was measured against GIVEN)
    const bool sort = order == RTX_CAST_ORDER_COHERENT;
    int rc = set_device(c);
    if (rc) return rc;
    const float4 *queries = static_cast<const float4 *>(d_queries);
    const uint32_t *perm = nullptr;
    c->paths_perm_valid = false;  // (rtx_debug_paths_order: this call is not a cost-ordered one)
    if (sort) {  // rtx_cast_rays' passes and scratch, unchanged: a query holds o and d where a ray does
        rc = ensure_cast(c, n);
        if (rc) return rc;
        const rtx::KCastScratch k{c->d_cast, c->d_cast + rtx::kCastBuckets, c->d_cast + rtx::kCastBuckets + c->cast_rays};
        const hipError_t e = rtx::launch_cast_order(queries, n, c->cast_box, k, c->stream);
        if (e != hipSuccess) return hip_fail(e, "launch_cast_order");
        perm = k.perm;
    }
    const hipError_t e = rtx::launch_paths(p, queries, perm, static_cast<float4 *>(d_results),
                                           static_cast<uint32_t *>(d_segments), c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_paths");
    c->paths_last = sort ? RTX_CAST_ORDER_COHERENT : RTX_CAST_ORDER_GIVEN;
    return RTX_OK;
}

int rtx_paths_last_order(rtx_ctx *c) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_paths_last_order: null ctx");
    return c->paths_last;
}

// ---- path queries in cost order (rtx_paths.h: the cost order) ------------------
static_assert(RTX_PATHS_ORDER_COST == rtx::kPathsOrderCost && rtx::kPathsCostBuckets == rtx::kCastBuckets,
              "rtx_paths.h restates these");
// The probe's segment counts for n queries. Once it fits there is no host wait.
static int ensure_paths_probe(rtx_ctx *c, size_t n) {
    if (c->d_paths_probe && c->paths_probe_cap >= n) return RTX_OK;
    RTX_HIP(hipStreamSynchronize(c->stream));
    (void)hipFree(c->d_paths_probe);
    c->d_paths_probe = nullptr;
    c->paths_probe_cap = 0;
    RTX_HIP(hipMalloc(&c->d_paths_probe, n * sizeof(uint32_t)));
    c->paths_probe_cap = n;
    return RTX_OK;
}

int rtx_trace_paths_keyed(rtx_ctx *c, const void *d_queries, uint32_t n, uint32_t samples, uint32_t flags,
                          const void *d_keys, uint32_t probe, void *d_results, void *d_segments) {
    // the argument rules first (rtx_paths.h): none of them looks at the context
    if (!c) return fail(RTX_ERR_INVALID, "rtx_trace_paths_keyed: null ctx");
    switch (rtx::paths_keyed_args(d_queries != nullptr, d_results != nullptr, n, samples, flags, d_keys != nullptr,
                                  probe)) {
    case rtx::kPathsKeyedArgQueries: return fail(RTX_ERR_INVALID, "rtx_trace_paths_keyed: d_queries is NULL");
    case rtx::kPathsKeyedArgResults: return fail(RTX_ERR_INVALID, "rtx_trace_paths_keyed: d_results is NULL");
    case rtx::kPathsKeyedArgSamples: return fail(RTX_ERR_INVALID, "rtx_trace_paths_keyed: samples is 0");
    case rtx::kPathsKeyedArgFlags: return fail(RTX_ERR_INVALID, "rtx_trace_paths_keyed: unknown flags");
    case rtx::kPathsKeyedArgProbe: return fail(RTX_ERR_INVALID, "rtx_trace_paths_keyed: probe must be 0 with d_keys");
    case rtx::kPathsKeyedArgOk: break;
    }
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_trace_paths_keyed: no world uploaded");
    switch (rtx::paths_world(samples, c->depth)) {
    case rtx::kPathsWorldDepth0: return fail(RTX_ERR_INVALID, "rtx_trace_paths_keyed: the world's depth is 0");
    case rtx::kPathsWorldCount:
        return fail(RTX_ERR_INVALID, "rtx_trace_paths_keyed: samples * depth does not fit 32 bits");
    case rtx::kPathsWorldOk: break;
    }
    if (n == 0) return RTX_OK;
    rtx::KPaths p;
    p.scene = scene_of(c);
    p.depth = c->depth;
    p.flags = rtx::paths_frame_flags(flags);
    p.samples = samples;
    p.n = n;
    p.mode = flags & rtx::kPathsContinue;
    int rc = set_device(c);
    if (rc) return rc;
    const float4 *queries = static_cast<const float4 *>(d_queries);
    float4 *results = static_cast<float4 *>(d_results);
    uint32_t *segments = static_cast<uint32_t *>(d_segments);
    c->paths_perm_valid = false;
    const uint32_t pr = d_keys ? 0u : (probe != 0u ? probe : rtx::paths_default_probe(p.scene.n_pad));
    if (!d_keys && !rtx::paths_two_phase(samples, pr)) {  // nothing left to order: one plain launch
        const hipError_t e = rtx::launch_paths(p, queries, nullptr, results, segments, c->stream);
        if (e != hipSuccess) return hip_fail(e, "launch_paths");
        c->paths_last = RTX_CAST_ORDER_GIVEN;
        return RTX_OK;
    }
    rc = ensure_cast(c, n);
    if (rc) return rc;
    const uint32_t *src = static_cast<const uint32_t *>(d_keys);
    if (!d_keys) {  // phase A: the probe, in the given order, its counts kept aside
        rc = ensure_paths_probe(c, n);
        if (rc) return rc;
        p.samples = pr;
        const hipError_t e = rtx::launch_paths(p, queries, nullptr, results, c->d_paths_probe, c->stream);
        if (e != hipSuccess) return hip_fail(e, "launch_paths");
        src = c->d_paths_probe;
        p.samples = samples - pr;
        p.mode = rtx::kPathsContinue;
    }
    // the sort reads src in its first pass only, before the trace below is enqueued: d_keys may be d_segments
    const rtx::KCastScratch k{c->d_cast, c->d_cast + rtx::kCastBuckets, c->d_cast + rtx::kCastBuckets + c->cast_rays};
    hipError_t e = rtx::launch_paths_cost_order(src, n, k, c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_paths_cost_order");
    e = rtx::launch_paths(p, queries, k.perm, results, segments, c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_paths");
    if (!d_keys && segments) {  // the whole call's count: the probe's plus the rest's
        e = rtx::launch_paths_add_segments(segments, c->d_paths_probe, n, c->stream);
        if (e != hipSuccess) return hip_fail(e, "launch_paths_add_segments");
    }
    c->paths_last = RTX_PATHS_ORDER_COST;
    c->paths_perm_valid = true;
    c->paths_perm_n = n;
    return RTX_OK;
}

int rtx_debug_paths_order(rtx_ctx *c, uint32_t *host_perm, size_t bytes) {
    if (!c || !host_perm) return fail(RTX_ERR_INVALID, "rtx_debug_paths_order: null argument");
    if (!c->paths_perm_valid || c->paths_last != RTX_PATHS_ORDER_COST || !c->d_cast)
        return fail(RTX_ERR_STATE, "rtx_debug_paths_order: the last path call's cost order is not at hand");
    if (bytes != (size_t)c->paths_perm_n * sizeof(uint32_t))
        return fail(RTX_ERR_INVALID, "rtx_debug_paths_order: bytes != n * 4");
    int rc = set_device(c);
    if (rc) return rc;
    const uint32_t *perm = c->d_cast + rtx::kCastBuckets + c->cast_rays;
    RTX_HIP(hipMemcpyAsync(host_perm, perm, bytes, hipMemcpyDeviceToHost, c->stream));
    RTX_HIP(hipStreamSynchronize(c->stream));
    return RTX_OK;
}

// ---- film queries: a pixel of a frame of its own (rtx_film.h) -------------------
static_assert(sizeof(rtx_film_query) == rtx::kFilmBytes && sizeof(rtx_film_lens_query) == rtx::kFilmLensBytes,
              "rtx_trace_film: four float4 per query, six with a lens");
static_assert(offsetof(rtx_film_query, o) == 4 * rtx::kFilmO && offsetof(rtx_film_query, seed) == 4 * rtx::kFilmSeed &&
                  offsetof(rtx_film_query, lower_left) == 4 * rtx::kFilmL &&
                  offsetof(rtx_film_query, tag) == 4 * rtx::kFilmTag &&
                  offsetof(rtx_film_query, horizontal) == 4 * rtx::kFilmH &&
                  offsetof(rtx_film_query, fx) == 4 * rtx::kFilmFx &&
                  offsetof(rtx_film_query, vertical) == 4 * rtx::kFilmV &&
                  offsetof(rtx_film_query, fy) == 4 * rtx::kFilmFy &&
                  offsetof(rtx_film_lens_query, lens_u) == 4 * rtx::kFilmLensU &&
                  offsetof(rtx_film_lens_query, lens_r) == 4 * rtx::kFilmLensR &&
                  offsetof(rtx_film_lens_query, lens_v) == 4 * rtx::kFilmLensV &&
                  offsetof(rtx_film_lens_query, reserved) == 4 * rtx::kFilmReserved,
              "rtx_film.h restates the record");
static_assert(RTX_FILM_LENS == rtx::kFilmLens && RTX_CAST_ORDER_AUTO == rtx::kFilmOrderAuto &&
                  RTX_CAST_ORDER_GIVEN == rtx::kFilmOrderGiven && RTX_CAST_ORDER_COHERENT == rtx::kFilmOrderCoherent &&
                  RTX_FILM_EQUIRECT == rtx::kFilmEquirect && RTX_FILM_FISHEYE == rtx::kFilmFisheye,
              "rtx_film.h restates these");

int rtx_trace_film(rtx_ctx *c, const void *d_queries, uint32_t n, uint32_t samples, float img_w, float img_h,
                   uint32_t flags, uint32_t order, void *d_results, void *d_segments) {
    // the argument rules first (rtx_film.h): none of them looks at the context
    if (!c) return fail(RTX_ERR_INVALID, "rtx_trace_film: null ctx");
    switch (rtx::film_args(d_queries != nullptr, d_results != nullptr, n, samples, flags, order)) {
    case rtx::kFilmArgQueries: return fail(RTX_ERR_INVALID, "rtx_trace_film: d_queries is NULL");
    case rtx::kFilmArgResults: return fail(RTX_ERR_INVALID, "rtx_trace_film: d_results is NULL");
    case rtx::kFilmArgSamples: return fail(RTX_ERR_INVALID, "rtx_trace_film: samples is 0");
    case rtx::kFilmArgFlags: return fail(RTX_ERR_INVALID, "rtx_trace_film: unknown flags");
    case rtx::kFilmArgOrder:
        return fail(RTX_ERR_INVALID, order == RTX_CAST_ORDER_COHERENT
                                         ? "rtx_trace_film: the coherent order does not apply to film records"
                                         : "rtx_trace_film: unknown order");
    case rtx::kFilmArgOk: break;
    }
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_trace_film: no world uploaded");
    switch (rtx::paths_world(samples, c->depth)) {
    case rtx::kPathsWorldDepth0: return fail(RTX_ERR_INVALID, "rtx_trace_film: the world's depth is 0");
    case rtx::kPathsWorldCount: return fail(RTX_ERR_INVALID, "rtx_trace_film: samples * depth does not fit 32 bits");
    case rtx::kPathsWorldOk: break;
    }
    if (n == 0) return RTX_OK;
    rtx::KFilm f;
    f.p.scene = scene_of(c);
    f.p.depth = c->depth;
    f.p.flags = rtx::paths_frame_flags(flags);
    f.p.samples = samples;
    f.p.n = n;
    f.p.mode = flags & rtx::kPathsContinue;
    f.img_w = img_w;
    f.img_h = img_h;
    const bool lens = (flags & rtx::kFilmLens) != 0u;
    int rc = set_device(c);
    if (rc) return rc;
    const float4 *queries = static_cast<const float4 *>(d_queries);
    float4 *results = static_cast<float4 *>(d_results);
    uint32_t *segments = static_cast<uint32_t *>(d_segments);
    const uint32_t pr = rtx::paths_default_probe(f.p.scene.n_pad);
    if (order != RTX_PATHS_ORDER_COST || !rtx::paths_two_phase(samples, pr)) {  // AUTO is GIVEN; nothing left to order
        const hipError_t e = rtx::launch_film(f, lens, queries, nullptr, results, segments, c->stream);
        if (e != hipSuccess) return hip_fail(e, "launch_film");
        c->film_last = RTX_CAST_ORDER_GIVEN;
        return RTX_OK;
    }
    // rtx_trace_paths_keyed's probe: pr samples in the given order with their
    // counts kept aside, the sort, the rest as a continuing launch through perm
    c->paths_perm_valid = false;  // (the scratch is about to hold another order)
    rc = ensure_cast(c, n);
    if (rc) return rc;
    rc = ensure_paths_probe(c, n);
    if (rc) return rc;
    f.p.samples = pr;
    hipError_t e = rtx::launch_film(f, lens, queries, nullptr, results, c->d_paths_probe, c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_film");
    f.p.samples = samples - pr;
    f.p.mode = rtx::kPathsContinue;
    const rtx::KCastScratch k{c->d_cast, c->d_cast + rtx::kCastBuckets, c->d_cast + rtx::kCastBuckets + c->cast_rays};
    e = rtx::launch_paths_cost_order(c->d_paths_probe, n, k, c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_paths_cost_order");
    e = rtx::launch_film(f, lens, queries, k.perm, results, segments, c->stream);
    if (e != hipSuccess) return hip_fail(e, "launch_film");
    if (segments) {  // the whole call's count: the probe's plus the rest's
        e = rtx::launch_paths_add_segments(segments, c->d_paths_probe, n, c->stream);
        if (e != hipSuccess) return hip_fail(e, "launch_paths_add_segments");
    }
    c->film_last = RTX_PATHS_ORDER_COST;
    return RTX_OK;
}

int rtx_film_last_order(rtx_ctx *c) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_film_last_order: null ctx");
    return c->film_last;
}

int rtx_debug_pixel_cost(rtx_ctx *c, uint32_t spp, uint32_t *host_cost) {
    if (!c || !host_cost) return fail(RTX_ERR_INVALID, "rtx_debug_pixel_cost: null argument");
    if (!c->have_world || !c->have_frame) return fail(RTX_ERR_STATE, "rtx_debug_pixel_cost: no world/frame");
    int rc = set_device(c);
    if (rc) return rc;
    const rtx_frame &f = c->frame;
    const size_t npix = (size_t)f.width * f.height;
    uint32_t *d = nullptr;
    RTX_HIP(hipMalloc(&d, npix * sizeof(uint32_t)));
    rtx::KParams p = make_params(c, f.height, 1, 0, 1, nullptr, nullptr, 0, f.frame_index);
    if (spp) p.spp = spp;
    p.cost_out = d;
    p.counters = c->d_counters + 3;
    p.wave_times = nullptr;
    hipError_t e = rtx::launch_cost(p, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(host_cost, d, npix * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return hip_fail(e, "rtx_debug_pixel_cost");
    return RTX_OK;
}

int rtx_debug_wave_times(rtx_ctx *c, size_t max_waves, unsigned long long *host_pairs) {
    if (!c) return fail(RTX_ERR_INVALID, "rtx_debug_wave_times: null ctx");
    int rc = set_device(c);
    if (rc) return rc;
    if (max_waves != c->wave_times_cap) {  // (re)arm: allocate and enable recording
        RTX_HIP(hipStreamSynchronize(c->stream));
        (void)hipFree(c->d_wave_times);
        c->d_wave_times = nullptr;
        c->wave_times_cap = 0;
        if (max_waves) {
            RTX_HIP(hipMalloc(&c->d_wave_times, max_waves * 2 * sizeof(unsigned long long)));
            RTX_HIP(hipMemsetAsync(c->d_wave_times, 0, max_waves * 2 * sizeof(unsigned long long), c->stream));
            c->wave_times_cap = max_waves;
        }
        return RTX_OK;
    }
    if (host_pairs && max_waves) {
        RTX_HIP(hipMemcpyAsync(host_pairs, c->d_wave_times, max_waves * 2 * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, c->stream));
        RTX_HIP(hipStreamSynchronize(c->stream));
    }
    return RTX_OK;
}

int rtx_debug_hit_world_from(rtx_ctx *c, const float *rays, uint32_t nrays, float t_min, float t_max,
                             uint32_t start_block, float *out) {
    if (!c || (nrays && (!rays || !out))) return fail(RTX_ERR_INVALID, "rtx_debug_hit_world: null argument");
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_debug_hit_world: no world uploaded");
    // the resolve compares roots by their bit patterns (rtx_kernels.hip
    // hit_key), which order like the values only for roots > 0
    if (!(t_min > 0.0f && t_min <= 3.4e38f))
        return fail(RTX_ERR_INVALID, "rtx_debug_hit_world: t_min must be finite and > 0");
    if (t_max != t_max) return fail(RTX_ERR_INVALID, "rtx_debug_hit_world: t_max is NaN");
    if (nrays == 0) return RTX_OK;
    if (t_max < t_min) {  // no root lies in [t_min, t_max]: every ray misses
        for (size_t i = 0; i < (size_t)nrays; ++i) {
            for (int k = 0; k < 9; ++k) out[10 * i + k] = 0.0f;
            out[10 * i + 9] = -1.0f;
        }
        return RTX_OK;
    }
    int rc = set_device(c);
    if (rc) return rc;
    float *d_rays = nullptr, *d_out = nullptr;
    RTX_HIP(hipMalloc(&d_rays, (size_t)nrays * 6 * sizeof(float)));
    hipError_t e = hipMalloc(&d_out, (size_t)nrays * 10 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(d_rays, rays, (size_t)nrays * 6 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = rtx::launch_debug_hit_world(scene_of(c), d_rays, nrays, t_min, t_max, start_block, d_out, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)nrays * 10 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_rays);
    (void)hipFree(d_out);
    if (e != hipSuccess) return hip_fail(e, "rtx_debug_hit_world");
    return RTX_OK;
}

int rtx_debug_hit_world(rtx_ctx *c, const float *rays, uint32_t nrays, float t_min, float t_max, float *out) {
    return rtx_debug_hit_world_from(c, rays, nrays, t_min, t_max, 0, out);
}

int rtx_debug_scan_rate(rtx_ctx *c, uint32_t reps, float *ms, unsigned long long *wave_segments) {
    if (!c || !ms || !wave_segments) return fail(RTX_ERR_INVALID, "rtx_debug_scan_rate: null argument");
    if (!c->have_world) return fail(RTX_ERR_STATE, "rtx_debug_scan_rate: no world uploaded");
    if (!c->have_frame) return fail(RTX_ERR_STATE, "rtx_debug_scan_rate: no frame set");
    int rc = set_device(c);
    if (rc) return rc;
    const rtx_frame &f = c->frame;
    rtx::KParams p = make_params(c, f.height, 1, 0, 1, nullptr, nullptr, 0, f.frame_index);
    if (!rtx::debug_scan_rate_supported(p))  // refused before any HIP call: every HIP error below is hip_fail's
        return fail(RTX_ERR_INVALID, "rtx_debug_scan_rate: scenes up to 640 spheres and a non-empty frame only");
    unsigned long long *sink = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    uint32_t waves = 0;
    RTX_HIP(hipMalloc(&sink, sizeof(unsigned long long)));
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipMemsetAsync(sink, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) e = hipEventRecord(e0, c->stream);
    if (e == hipSuccess) e = rtx::launch_debug_scan_rate(p, reps, sink, &waves, c->stream);
    if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(ms, e0, e1);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    (void)hipFree(sink);
    if (e != hipSuccess) return hip_fail(e, "rtx_debug_scan_rate");
    *wave_segments = (unsigned long long)waves * reps;
    return RTX_OK;
}

int rtx_debug_math(rtx_ctx *c, int fn, const float *in0, const float *in1, uint32_t n, float *out) {
    if (!c || (n && (!in0 || !out))) return fail(RTX_ERR_INVALID, "rtx_debug_math: null argument");
    if (fn < RTX_FN_SQRT || fn > RTX_FN_LAMBERT_DIR_GUARD)
        return fail(RTX_ERR_INVALID, "rtx_debug_math: unknown fn");
    const bool vec = fn >= RTX_FN_LAMBERT_DIR;  // in0 = p[3n], in1 = (normal, rius)[6n]
    if (vec && n && !in1) return fail(RTX_ERR_INVALID, "rtx_debug_math: lambert functions need in1");
    if (n == 0) return RTX_OK;
    int rc = set_device(c);
    if (rc) return rc;
    float *d0 = nullptr, *d1 = nullptr, *dout = nullptr;
    const size_t outn = (size_t)n * 3;
    const size_t n0 = vec ? (size_t)n * 3 : (size_t)n, n1 = vec ? (size_t)n * 6 : (size_t)n;
    RTX_HIP(hipMalloc(&d0, n0 * sizeof(float)));
    hipError_t e = hipMalloc(&dout, outn * sizeof(float));
    if (e == hipSuccess && in1) e = hipMalloc(&d1, n1 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(d0, in0, n0 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && in1) e = hipMemcpyAsync(d1, in1, n1 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(dout, 0, outn * sizeof(float), c->stream);
    if (e == hipSuccess) e = rtx::launch_debug_math(fn, d0, d1, n, dout, c->stream);
    const size_t copy_n = (fn >= RTX_FN_HASH1) ? outn : (size_t)n;
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, copy_n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d0);
    (void)hipFree(d1);
    (void)hipFree(dout);
    if (e != hipSuccess) return hip_fail(e, "rtx_debug_math");
    return RTX_OK;
}

}  // extern "C"
