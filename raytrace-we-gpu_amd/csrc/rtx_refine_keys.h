// rtx_refine_keys.h — the carried queue key of a refine launch and the host's
// rule for when a launch takes it (include/rtx.h rtx_refine_set_keys).
// HIP-free: the kernels (rtx_kernels.hip k_carried_hist / k_carried_scatter),
// the host (rtx_api.hip) and a CPU checker (tests/carried_key_check.cpp) all
// run this one text.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_KEYS_HD __host__ __device__ inline
#else
#define RTX_KEYS_HD inline
#endif

namespace rtx {

constexpr uint32_t kCostBuckets = 256;  // queue keys: bucket 0 = most expensive
#ifndef RTX_COST_SPP
#define RTX_COST_SPP 2
#endif
constexpr uint32_t kCostSpp = RTX_COST_SPP;  // pre-pass samples per pixel (kept: the render resumes after them)
#ifndef RTX_COST_SPP_LARGE
#define RTX_COST_SPP_LARGE 1
#endif
constexpr uint32_t kCostSppLarge = RTX_COST_SPP_LARGE;  // ... for scenes above kScanPfMin spheres (C5: 1,997 vs 2,018 ms)
constexpr uint32_t kLptMinSpp = 8;  // below this the pre-pass costs more than it saves: exact grid

// rtx_refine_set_keys modes and what rtx_refine_last_keys reports (= the
// RTX_REFINE_KEYS_* values of include/rtx.h)
constexpr int kKeysPrepass = 0, kKeysCarried = 1, kKeysUnscheduled = 2;

// Queue key of pixel i from the cost map of the previous refine launch
// (`map`: width * rows segment counts, each over s_prev >= 1 samples of its
// pixel): cost_key's unit and window — the sum over the 3 x 3 window, clamped
// at the edges, scaled to 9 one-sample costs and rounded as cost_key rounds,
// then the bucket. 64-bit: 9 entries below 2^32, times 9, plus half a window
// of at most 9 * (2^32 - 1) stays below 2^41.
RTX_KEYS_HD uint32_t carried_key(const uint32_t *map, uint32_t i, uint32_t width, uint32_t rows, uint32_t s_prev) {
    const int x = (int)(i % width), y = (int)(i / width);
    uint64_t sum = 0;
    for (int dy = -1; dy <= 1; ++dy) {
        const int yc = y + dy < 0 ? 0 : y + dy > (int)rows - 1 ? (int)rows - 1 : y + dy;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xc = x + dx < 0 ? 0 : x + dx > (int)width - 1 ? (int)width - 1 : x + dx;
            sum += map[(uint64_t)(uint32_t)yc * width + (uint32_t)xc];
        }
    }
    const uint64_t win = 9ull * s_prev;
    if (win != 9ull) sum = (sum * 9ull + win / 2ull) / win;
    const uint64_t top = kCostBuckets - 1u;
    return (uint32_t)(top - (sum < top ? sum : top));
}

// A launch's counts fit the map's uint32 entries: a pixel traces at most
// depth segments per sample.
RTX_KEYS_HD bool cost_map_fits(uint32_t samples, uint32_t depth) {
    return (uint64_t)samples * depth < (1ull << 32);
}

// s_prev after a refine launch of `samples` samples at `depth` (0: no valid
// map): a launch that traced nothing, or whose counts could wrap, leaves none.
RTX_KEYS_HD uint32_t cost_map_after(uint32_t samples, uint32_t depth) {
    return depth != 0u && cost_map_fits(samples, depth) ? samples : 0u;
}

// Whether a refine launch of `samples` samples is keyed by the map: the mode
// asks for it, the map is valid (s_prev != 0) and covers at least the samples
// a pre-pass would trace for the scene class, and the launch is scheduled at
// all (kLptMinSpp). Otherwise the launch runs the pre-pass path unchanged.
RTX_KEYS_HD bool launch_is_carried(int mode, uint32_t s_prev, uint32_t samples, bool large_scene) {
    return mode == kKeysCarried && s_prev != 0u && samples >= kLptMinSpp &&
           s_prev >= (large_scene ? kCostSppLarge : kCostSpp);
}

}  // namespace rtx
