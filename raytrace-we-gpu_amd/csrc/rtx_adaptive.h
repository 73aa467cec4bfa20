// rtx_adaptive.h — the rule of adaptive refinement (include/rtx.h
// rtx_refine_adaptive): a pixel's error estimate after a step and which pixels
// a call traces. HIP-free: the kernels (rtx_kernels.hip write_pixel,
// k_adaptive_mask), the host (rtx_api.hip rtx_adaptive_error) and a CPU
// checker (tests/adaptive_check.cpp) all run this one text.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_ADAPT_HD __host__ __device__ inline
#else
#define RTX_ADAPT_HD inline
#endif
// hipcc contracts a * b + c into an fma by default; the estimate is a fixed
// sequence of fp32 operations, so its functions switch contraction off for
// themselves (a pragma at file scope would reach the including file's code).
#if defined(__clang__)
#define RTX_ADAPT_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RTX_ADAPT_NO_CONTRACT  // (other compilers: build with -ffp-contract=off)
#endif

namespace rtx {

// Error E of a pixel whose step took it from n_old to n_new > n_old samples;
// sum_old and sum_new are its linear sample sums (x, y, z) before and after.
//   n_old == 0 -> +inf (no estimate yet)
//   m0 = sum_old / n_old, m1 = sum_new / n_new
//   d = (|m1.x - m0.x| + |m1.y - m0.y|) + |m1.z - m0.z|
//   l = (m1.x + m1.y) + m1.z
//   E = (d * sqrt(n_old / s)) / sqrt(l + 0.01f),  s = n_new - n_old
// |m1 - m0| * sqrt(n_old / s) estimates the standard error of the new mean;
// the denominator makes it relative, so dark pixels do not starve the bright
// ones. Linear values on purpose. fp32 in this order with IEEE division and
// square root: `sq` is the caller's correctly rounded fp32 square root (the
// kernels pass sqrt_rn, a host sqrtf), `/` is correctly rounded on both sides.
// NaN sums give a NaN E.
template <class Sqrt>
RTX_ADAPT_HD float adaptive_error_with(const float *sum_old, uint32_t n_old, const float *sum_new, uint32_t n_new,
                                       Sqrt sq) {
    RTX_ADAPT_NO_CONTRACT
    if (n_old == 0u) return INFINITY;
    const float a = (float)n_old, b = (float)n_new, sf = (float)(n_new - n_old);
    const float m0x = sum_old[0] / a, m0y = sum_old[1] / a, m0z = sum_old[2] / a;
    const float m1x = sum_new[0] / b, m1y = sum_new[1] / b, m1z = sum_new[2] / b;
    const float d = (fabsf(m1x - m0x) + fabsf(m1y - m0y)) + fabsf(m1z - m0z);
    const float l = (m1x + m1y) + m1z;
    return (d * sq(a / sf)) / sq(l + 0.01f);
}

// Whether a call (samples, threshold, max_samples) traces pixel i of a
// width x rows image with the per-pixel maps `err` (E of each pixel's last
// step) and `count` (samples in its sum). Both must hold:
//   some pixel q of i's 3 x 3 neighbourhood inside the image has
//   err[q] >= threshold (false for a NaN: a NaN pixel stays NaN, so sampling
//   it is waste). One step's estimate is a single noisy draw; the
//   neighbourhood plays the role of carried_key's 3 x 3 window;
//   max_samples == 0 or count[i] + samples <= max_samples.
RTX_ADAPT_HD bool adaptive_active(const float *err, const uint32_t *count, uint32_t i, uint32_t width, uint32_t rows,
                                  uint32_t samples, float threshold, uint32_t max_samples) {
    if (max_samples != 0u && (uint64_t)count[i] + samples > max_samples) return false;
    const int x = (int)(i % width), y = (int)(i / width);
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= (int)rows) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= (int)width) continue;
            if (err[(uint64_t)(uint32_t)yy * width + (uint32_t)xx] >= threshold) return true;
        }
    }
    return false;
}

// The argument rules of rtx_refine_adaptive and rtx_refine_pending that need
// no context (NULL: fine, else what is wrong).
RTX_ADAPT_HD const char *adaptive_args_error(uint32_t samples, float threshold, uint32_t max_samples) {
    if (samples == 0u) return "samples is 0";
    if (threshold != threshold) return "the threshold is NaN";
    if (max_samples != 0u && max_samples < samples) return "max_samples is below samples";
    return nullptr;
}

// Queue keys of an adaptive launch (k_adaptive_hist / k_adaptive_scatter):
// carried_key over the context's cost map with its s_prev, for active pixels
// only; with no valid map every key is equal. An inactive pixel keeps its own
// last step's entry, so a re-activated pixel's entry (and its neighbours') may
// stem from an older step of another size than s_prev: that mis-scales a key,
// which orders the queue, never a result.

}  // namespace rtx
