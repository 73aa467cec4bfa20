// rtx_paths.h — the host-side rules of path queries along caller-chosen rays
// (include/rtx.h rtx_path_seed): a query record's layout and the seed of a
// pixel's RNG chain. HIP-free: the host (rtx_host.cpp) and the CPU checker
// (tests/paths_check.cpp) run this one text, and a device entry point that
// traces such queries is to run it too.
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

}  // namespace rtx
