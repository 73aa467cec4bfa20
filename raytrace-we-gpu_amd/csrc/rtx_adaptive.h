// rtx_adaptive.h — the rule of adaptive refinement (include/rtx.h
// rtx_refine_adaptive): a pixel's error estimate after a step and which pixels
// a call traces, on the whole frame and on a row part of it. HIP-free: the
// kernels (rtx_kernels.hip write_pixel, k_adaptive_mask, k_adaptive_mask_rows),
// the host (rtx_api.hip rtx_adaptive_error) and the CPU checkers
// (tests/adaptive_check.cpp, tests/group_adaptive_check.cpp) all run this one
// text.
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

// ---- the rule on a row part (rtx_refine_adaptive_rows) ----------------------
// A frame of `height` rows in tiles of `tile_rows`; tile k belongs to part
// k % nparts as its local tile k / nparts (rtx_render_rows' partition). A
// part's maps hold its own rows only, so the err row just outside one of its
// tiles comes from a halo buffer the caller filled from the neighbours:
//   halo[2][tiles_of_part][width] fp32
//   plane 0, slot j: the err row just below local tile j's first row
//   plane 1, slot j: the err row just above its last row
// A slot whose row lies outside the image is never read. The same layout is a
// part's edges (k_adaptive_edges): plane 0 each tile's first err row, plane 1
// its last (one row twice for a 1-row tile).

// Tiles of `part`: tiles part, part + nparts, ... below ceil(height / tile_rows).
RTX_ADAPT_HD uint32_t adaptive_part_tiles(uint32_t height, uint32_t tile_rows, uint32_t part, uint32_t nparts) {
    const uint32_t tiles = (uint32_t)(((uint64_t)height + tile_rows - 1u) / tile_rows);
    return part >= tiles ? 0u : (tiles - part + nparts - 1u) / nparts;
}

// adaptive_active for local pixel i of part `part` (err, count: the part's
// maps in its row order). nparts == 1 reads the local maps alone and is
// adaptive_active. halo == NULL with nparts > 1 skips the rows outside a tile:
// right only where every err is +inf (a fresh or uniform state), since then
// the pixel's own entry already decides.
RTX_ADAPT_HD bool adaptive_active_rows(const float *err, const uint32_t *count, const float *halo, uint32_t i,
                                       uint32_t width, uint32_t height, uint32_t tile_rows, uint32_t part,
                                       uint32_t nparts, uint32_t samples, float threshold, uint32_t max_samples) {
    if (max_samples != 0u && (uint64_t)count[i] + samples > max_samples) return false;
    const uint32_t lr = i / width, j = lr / tile_rows, r = lr - j * tile_rows;
    const int x = (int)(i - lr * width);
    const uint32_t y0 = (part + j * nparts) * tile_rows;  // the tile's first row in the image
    const uint32_t left = height - y0;
    const uint32_t trows = left < tile_rows ? left : tile_rows;  // (the ragged final tile)
    const uint64_t plane = (uint64_t)adaptive_part_tiles(height, tile_rows, part, nparts) * width;
    for (int dy = -1; dy <= 1; ++dy) {
        const float *row;
        if (dy < 0 && r == 0u) {
            if (y0 == 0u) continue;  // below the image
            row = nparts == 1u ? err + (uint64_t)(lr - 1u) * width : halo ? halo + (uint64_t)j * width : nullptr;
        } else if (dy > 0 && r == trows - 1u) {
            if (y0 + trows >= height) continue;  // above the image
            row = nparts == 1u ? err + (uint64_t)(lr + 1u) * width : halo ? halo + plane + (uint64_t)j * width : nullptr;
        } else {
            row = err + (uint64_t)(uint32_t)((int)lr + dy) * width;
        }
        if (!row) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= (int)width) continue;
            if (row[xx] >= threshold) return true;
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
