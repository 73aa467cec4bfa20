// rtx_features.h — the rules of the first-hit feature buffers (include/rtx.h
// rtx_features, rtx_pick), of the id mask (rtx_mask_from_ids) and of masked
// refinement (rtx_refine_masked). HIP-free: the kernels (rtx_kernels.hip
// k_features, k_feature_listed, k_feature_mask, k_masked_flags), the host
// (rtx_app.cpp) and the CPU checker (tests/features_check.cpp) all run this
// one text.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_FEAT_HD __host__ __device__ inline
#else
#define RTX_FEAT_HD inline
#endif
// hipcc contracts a * b + c into an fma by default; the ray and the depth are
// fixed sequences of fp32 operations, so their functions switch contraction
// off for themselves (as rtx_adaptive.h does).
#if defined(__clang__)
#define RTX_FEAT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RTX_FEAT_NO_CONTRACT  // (other compilers: build with -ffp-contract=off)
#endif

namespace rtx {

// The centre ray of pixel (x, y), y counted from the image's bottom row, in
// the frame's four view rows (rtx_frame: origin, horizontal, vertical,
// lower_left): get_ray's operations (ShaderCompute.hlsl:118-127) at the pixel
// centre, no jitter, no lens offset, no fma. The origin is org itself.
//   u = ((float)x + 0.5f) / (img_w - 1.0f),  v = ((float)y + 0.5f) / (img_h - 1.0f)
//   d = ((llc + u * hor) + v * ver) - org
RTX_FEAT_HD void feature_ray(const float *org, const float *hor, const float *ver, const float *llc, float img_w,
                             float img_h, uint32_t x, uint32_t y, float *d) {
    RTX_FEAT_NO_CONTRACT
    const float u = ((float)x + 0.5f) / (img_w - 1.0f);
    const float v = ((float)y + 0.5f) / (img_h - 1.0f);
    for (int k = 0; k < 3; ++k) {
        const float a = u * hor[k];
        const float b = llc[k] + a;
        const float c = v * ver[k];
        d[k] = (b + c) - org[k];
    }
}

// The distance of a hit at parameter t along direction d, in world units:
//   depth = t * sqrt((d.x * d.x + d.y * d.y) + d.z * d.z)
// plain fp32 multiplies and adds; `sq` is the caller's correctly rounded fp32
// square root (the kernels pass sqrt_rn, a host sqrtf).
template <class Sqrt>
RTX_FEAT_HD float feature_depth(float t, const float *d, Sqrt sq) {
    RTX_FEAT_NO_CONTRACT
    const float xx = d[0] * d[0];
    const float yy = d[1] * d[1];
    const float zz = d[2] * d[2];
    const float s = (xx + yy) + zz;
    return t * sq(s);
}

// ---- the id mask (rtx_mask_from_ids) ----------------------------------------
// A pixel's id is its surf plane's w: (float)(scene index) of its first hit,
// -1 on a miss. A pixel is LISTED iff it hit something and that index is one
// of ids[0 .. n). A miss is never listed — an entry 0xffffffff ("-1") in the
// list names no sphere — and neither is a NaN or negative w.
RTX_FEAT_HD bool feature_id_listed(float w, const uint32_t *ids, uint32_t n) {
    if (!(w >= 0.0f) || w >= 4294967296.0f) return false;
    const uint32_t id = (uint32_t)w;
    for (uint32_t k = 0; k < n; ++k)
        if (ids[k] == id) return true;
    return false;
}

// mask[i] of a width x height image: some pixel within Chebyshev distance
// `grow` of pixel i, inside the image, is listed (listed: one byte per pixel,
// nonzero = listed, framebuffer order).
RTX_FEAT_HD bool feature_mask_grown(const uint8_t *listed, uint32_t i, uint32_t width, uint32_t height, uint32_t grow) {
    const int64_t x = (int64_t)(i % width), y = (int64_t)(i / width), g = (int64_t)grow;
    const int64_t y0 = y - g < 0 ? 0 : y - g, y1 = y + g >= (int64_t)height ? (int64_t)height - 1 : y + g;
    const int64_t x0 = x - g < 0 ? 0 : x - g, x1 = x + g >= (int64_t)width ? (int64_t)width - 1 : x + g;
    for (int64_t yy = y0; yy <= y1; ++yy)
        for (int64_t xx = x0; xx <= x1; ++xx)
            if (listed[(uint64_t)yy * width + (uint64_t)xx]) return true;
    return false;
}

constexpr uint32_t kFeatureIdsMax = 256u;  // rtx_mask_from_ids: 1 <= n <= this
constexpr uint32_t kFeatureGrowMax = 8u;   // ... and grow <= this

// ---- masked refinement (rtx_refine_masked) ----------------------------------
// Whether a call (samples, max_samples) traces a pixel with mask byte m whose
// sum holds `count` samples: rtx_refine_adaptive's rule with the caller's mask
// in the place of the "noisy" test.
RTX_FEAT_HD bool masked_active(uint8_t m, uint32_t count, uint32_t samples, uint32_t max_samples) {
    return m != 0u && (max_samples == 0u || (uint64_t)count + samples <= max_samples);
}

}  // namespace rtx
