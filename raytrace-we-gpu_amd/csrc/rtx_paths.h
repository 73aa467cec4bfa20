// rtx_paths.h — the host-side rules of path queries along caller-chosen rays
// (include/rtx.h rtx_path_seed, rtx_trace_paths): a query record's layout, the
// seed of a pixel's RNG chain, the entry point's argument rules and the
// launch's index arithmetic. HIP-free: the host (rtx_host.cpp, rtx_api.hip),
// the kernel (rtx_kernels.hip k_paths) and the CPU checkers
// (tests/paths_check.cpp, tests/paths_args_check.cpp) run this one text.
//
// The rule the seed serves. In a frame whose horizontal and vertical rows are
// zero, get_ray gives every pixel the same ray, d = fl(lower_left - origin)
// componentwise, whatever the jitter; a pixel's (x, y) then enters only
// through its seed. A path query with ray (o, d) and the seed of pixel (x, y)
// is therefore, by definition, that pixel of that "zero-film twin" frame, and
// the CPU oracle's render_rows_linear computes it (tests/paths_cases.py).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_PATHS_HD __host__ __device__ inline
#else
#define RTX_PATHS_HD inline
#endif

namespace rtx {

// A query record is two float4: (o.xyz, seed), (d.xyz, tag). rtx_cast_rays'
// COHERENT passes (rtx_cast.h) read a ray record's origin and direction at the
// same floats, so they sort such records as they stand.
constexpr uint32_t kPathRayBytes = 32u;
constexpr uint32_t kPathRayO = 0u;     // float index of o[0]
constexpr uint32_t kPathRaySeed = 3u;  // ... of seed
constexpr uint32_t kPathRayD = 4u;     // ... of d[0]
constexpr uint32_t kPathRayTag = 7u;   // ... of tag (the caller's, unread)

// baseHash(uint2 p) of the reference's compute shader (ShaderCompute.hlsl:
// 23-28), as rtx_device_math.h base_hash.
RTX_PATHS_HD uint32_t path_base_hash(uint32_t px, uint32_t py) {
    const uint32_t qx = 1103515245u * ((px >> 1) ^ py);
    const uint32_t qy = 1103515245u * ((py >> 1) ^ px);
    const uint32_t h = 1103515245u * (qx ^ (qy >> 3));
    return h ^ (h >> 16);
}
// The hash behind pixel (x, y)'s chain seed in frame `frame_index`: the chain
// mode of the render's pixel_seed (rtx_kernels.hip).
RTX_PATHS_HD uint32_t path_seed_hash(uint32_t x, uint32_t y, uint32_t frame_index) {
    uint32_t h = path_base_hash(x, y);
    if (frame_index != 0u) h = path_base_hash(h, 0x80000000u | frame_index);
    return h;
}
// ... and the seed: float(h) / 2^32, the conversion rounded to nearest even
// and the divide exact (a power of two).
RTX_PATHS_HD float path_seed(uint32_t x, uint32_t y, uint32_t frame_index) {
    return (float)path_seed_hash(x, y, frame_index) / 4294967296.0f;
}

// samples * depth must stay below 2^32: a query's segment count is a uint32.
RTX_PATHS_HD bool paths_count_ok(uint32_t samples, uint32_t depth) {
    return (uint64_t)samples * (uint64_t)depth < (1ull << 32);
}

// ---- rtx_trace_paths: the argument rules and the launch's arithmetic ---------
// A result record is one float4: (sum.xyz, the chain's seed after the last
// sample): a one-pixel chain state (rtx_refine_export's layout).
constexpr uint32_t kPathResultBytes = 16u;
constexpr uint32_t kPathsLambertGuard = 1u;  // = RTX_PATHS_LAMBERT_GUARD
constexpr uint32_t kPathsContinue = 2u;      // = RTX_PATHS_CONTINUE
constexpr uint32_t kPathsFlagMask = kPathsLambertGuard | kPathsContinue;
constexpr uint32_t kPathsOrderMax = 2u;      // RTX_CAST_ORDER_AUTO, _GIVEN, _COHERENT = 0, 1, 2

// What rtx_trace_paths refuses before it looks at the context, in the order it
// tests them (a null ctx comes before all of these).
enum PathsArg : int {
    kPathsArgOk = 0,
    kPathsArgQueries,  // n > 0 with d_queries NULL
    kPathsArgResults,  // n > 0 with d_results NULL
    kPathsArgSamples,  // samples == 0
    kPathsArgFlags,    // a bit outside kPathsFlagMask
    kPathsArgOrder,    // order > kPathsOrderMax
};
RTX_PATHS_HD PathsArg paths_args(bool have_queries, bool have_results, uint32_t n, uint32_t samples, uint32_t flags,
                                 uint32_t order) {
    if (n != 0u && !have_queries) return kPathsArgQueries;
    if (n != 0u && !have_results) return kPathsArgResults;
    if (samples == 0u) return kPathsArgSamples;
    if ((flags & ~kPathsFlagMask) != 0u) return kPathsArgFlags;
    if (order > kPathsOrderMax) return kPathsArgOrder;
    return kPathsArgOk;
}
// ... and once the world is known: its depth.
enum PathsWorld : int { kPathsWorldOk = 0, kPathsWorldDepth0, kPathsWorldCount };
RTX_PATHS_HD PathsWorld paths_world(uint32_t samples, uint32_t depth) {
    if (depth == 0u) return kPathsWorldDepth0;
    if (!paths_count_ok(samples, depth)) return kPathsWorldCount;
    return kPathsWorldOk;
}
// The frame flags path_segment sees (rtx_internal.h kFrameLambertGuard = 1).
RTX_PATHS_HD uint32_t paths_frame_flags(uint32_t flags) { return (flags & kPathsLambertGuard) != 0u ? 1u : 0u; }

// The exact grid: ceil(n / block) workgroups, for every n below 2^32 (n +
// block - 1 in 32 bits wraps from n = 2^32 - block + 1).
RTX_PATHS_HD uint32_t paths_blocks(uint32_t n, uint32_t block) {
    return (uint32_t)(((uint64_t)n + block - 1u) / block);
}
// Lane g of that grid: whether it owns a query (g counted in 64 bits: the
// grid's last lanes lie past 2^32 - 1 for the largest n), and which — the g-th
// of the order `perm` (an entry, whatever it holds, is clamped to n - 1) or
// query g itself. n > 0.
RTX_PATHS_HD bool paths_lane_live(uint64_t g, uint32_t n) { return g < (uint64_t)n; }
RTX_PATHS_HD uint32_t paths_lane_query(uint32_t g, bool have_perm, uint32_t perm_g, uint32_t n) {
    if (!have_perm) return g;
    return perm_g < n - 1u ? perm_g : n - 1u;
}
// Byte offsets of query i's two float4, of its result and of its segment word:
// 64-bit, so that i * 32 does not wrap from i = 2^27.
RTX_PATHS_HD uint64_t paths_query_offset(uint32_t i) { return (uint64_t)i * kPathRayBytes; }
RTX_PATHS_HD uint64_t paths_result_offset(uint32_t i) { return (uint64_t)i * kPathResultBytes; }
RTX_PATHS_HD uint64_t paths_segment_offset(uint32_t i) { return (uint64_t)i * 4u; }

// ---- rtx_trace_paths_keyed: the cost order -------------------------------------
// Lane g of the one k_paths launch takes the g-th query in non-increasing order
// of min(key, 65535): the longest queries first, so that a wave's 64 lanes
// hold queries of similar length. The keys are the caller's (d_keys) or the
// segment counts of the library's own probe, a first call of p samples. A
// schedule and nothing else: every record is what the given order writes.
constexpr uint32_t kPathsOrderCost = 3u;   // = RTX_PATHS_ORDER_COST (rtx_paths_last_order; never an `order` argument)
constexpr uint32_t kPathsKeyMax = 65535u;  // keys above it sort with it
constexpr uint32_t kPathsCostBuckets = kPathsKeyMax + 1u;  // = kCastBuckets (asserted where rtx_cast.h is in sight)

// What rtx_trace_paths_keyed refuses before it looks at the context, in the
// order it tests them (a null ctx comes before all of these).
enum PathsKeyedArg : int {
    kPathsKeyedArgOk = 0,
    kPathsKeyedArgQueries,  // n > 0 with d_queries NULL
    kPathsKeyedArgResults,  // n > 0 with d_results NULL
    kPathsKeyedArgSamples,  // samples == 0
    kPathsKeyedArgFlags,    // a bit outside kPathsFlagMask
    kPathsKeyedArgProbe,    // d_keys given and probe != 0
};
RTX_PATHS_HD PathsKeyedArg paths_keyed_args(bool have_queries, bool have_results, uint32_t n, uint32_t samples,
                                            uint32_t flags, bool have_keys, uint32_t probe) {
    if (n != 0u && !have_queries) return kPathsKeyedArgQueries;
    if (n != 0u && !have_results) return kPathsKeyedArgResults;
    if (samples == 0u) return kPathsKeyedArgSamples;
    if ((flags & ~kPathsFlagMask) != 0u) return kPathsKeyedArgFlags;
    if (have_keys && probe != 0u) return kPathsKeyedArgProbe;
    return kPathsKeyedArgOk;
}
// The probe's samples when the caller passes 0: the refine pre-pass's rule, 2,
// or 1 for a world of more than 1,024 spheres after padding.
RTX_PATHS_HD uint32_t paths_default_probe(uint32_t n_pad) { return n_pad > 1024u ? 1u : 2u; }
// Whether a probed call of `samples` with probe p sorts at all: with nothing
// left after the probe it is one plain launch in the given order.
RTX_PATHS_HD bool paths_two_phase(uint32_t samples, uint32_t p) { return samples > p; }
// The counting sort's bucket of a key: buckets ascend, keys descend. Below
// kPathsCostBuckets for every input.
RTX_PATHS_HD uint32_t paths_cost_bucket(uint32_t key) {
    return kPathsKeyMax - (key < kPathsKeyMax ? key : kPathsKeyMax);
}

}  // namespace rtx
