// rtx_cast.h — the rules of rtx_cast_rays' COHERENT order (include/rtx.h): the
// box of the scene's body, a ray's origin and direction cells, the sort key,
// and the AUTO rule. HIP-free: the kernels (rtx_kernels.hip k_cast_keys,
// k_cast_scatter), the host (rtx_api.hip, at rtx_upload_world) and the CPU
// checker (tests/cast_check.cpp) all run this one text.
//
// The key is a schedule and nothing else: k_cast casts ray perm[i] in lane i
// and writes record perm[i], so any key gives the same records. What the key
// buys is that the 64 rays of a wave start close together and point the same
// way, and the lane-mode scan costs the union of a wave's candidate blocks.
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_CAST_HD __host__ __device__ inline
#else
#define RTX_CAST_HD inline
#endif
// The cells are fixed sequences of fp32 operations (host and device agree on a
// ray's key), so their functions switch contraction off for themselves (as
// rtx_features.h and rtx_adaptive.h do).
#if defined(__clang__)
#define RTX_CAST_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RTX_CAST_NO_CONTRACT  // (other compilers: build with -ffp-contract=off)
#endif

namespace rtx {

// The key's bits, high to low: kCastOriginBits of origin cell, dealt to the
// three axes by the box's shape (CastBox::bits) and interleaved, then
// 2 * kCastDirBits of direction cell (octahedral u, v), interleaved.
constexpr uint32_t kCastOriginBits = 10u;
constexpr uint32_t kCastDirBits = 3u;
constexpr uint32_t kCastKeyBits = kCastOriginBits + 2u * kCastDirBits;
constexpr uint32_t kCastBuckets = 1u << kCastKeyBits;  // 65,536
static_assert(kCastBuckets <= 65536u, "rtx_cast_rays: at most 65,536 buckets");

// The box of the scene's body and how the origin bits are dealt to its axes:
// axis k has 2^bits[k] cells of extent / 2^bits[k] each from lo[k];
// scale[k] = 2^bits[k] / extent (0 with bits[k] = 0: every origin in cell 0).
struct CastBox {
    float lo[3];
    float scale[3];
    uint32_t bits[3];
};

// The body of a scene of n spheres (x, y, z, r each): the centres of the
// spheres whose |r| is at most 16 times the median |r| (a 1000-radius ground
// under unit spheres is not part of it). An axis whose extent is not a positive
// finite number, or a scene without such a sphere, keeps 0 bits. The bits go
// one at a time to the axis whose cells are the longest so far, so the cells
// end up as close to cubes as powers of two allow: a flat layer of spheres
// spends them on x and z. `radii`: scratch of n floats. Host only.
inline CastBox cast_box(const float *spheres, uint32_t n, float *radii) {
    CastBox b{};
    for (uint32_t i = 0; i < n; ++i) {
        const float r = fabsf(spheres[4 * (size_t)i + 3]);
        radii[i] = r == r ? r : INFINITY;  // (a NaN radius sorts last and is never part of the body)
    }
    float med = 0.0f;
    if (n != 0) {
        std::nth_element(radii, radii + n / 2, radii + n);
        med = radii[n / 2];
    }
    const float bar = 16.0f * med;
    float lo[3] = {0.0f, 0.0f, 0.0f}, hi[3] = {0.0f, 0.0f, 0.0f};
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) {
        if (!(fabsf(spheres[4 * (size_t)i + 3]) <= bar)) continue;
        for (int k = 0; k < 3; ++k) {
            const float c = spheres[4 * (size_t)i + k];
            if (!any || c < lo[k]) lo[k] = c;
            if (!any || c > hi[k]) hi[k] = c;
        }
        any = true;
    }
    double cell[3];
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = lo[k];
        const double e = any ? (double)hi[k] - (double)lo[k] : 0.0;
        cell[k] = (e > 0.0 && e < 1e30) ? e : 0.0;
    }
    for (uint32_t given = 0; given < kCastOriginBits; ++given) {
        int best = -1;
        for (int k = 0; k < 3; ++k)
            if (cell[k] > 0.0 && (best < 0 || cell[k] > cell[best])) best = k;
        if (best < 0) break;
        ++b.bits[best];
        cell[best] *= 0.5;
    }
    for (int k = 0; k < 3; ++k)
        b.scale[k] = b.bits[k] ? (float)((double)(1u << b.bits[k]) / ((double)hi[k] - (double)lo[k])) : 0.0f;
    return b;
}

// floor(v) clamped to [0, cells - 1] for any float v: NaN and everything below
// 1 give 0, everything from cells - 1 up (+inf too) gives cells - 1. The
// conversion only ever sees a value in [1, cells - 1).
RTX_CAST_HD uint32_t cast_cell(float v, uint32_t cells) {
    if (!(v >= 1.0f)) return 0u;
    const float top = (float)(cells - 1u);
    if (v >= top) return cells - 1u;
    return (uint32_t)v;
}

// The origin's cell on each axis of the box: (o - lo) * scale, clamped.
RTX_CAST_HD void cast_origin_cells(const CastBox &b, const float *o, uint32_t *c) {
    RTX_CAST_NO_CONTRACT
    for (int k = 0; k < 3; ++k) {
        const float rel = o[k] - b.lo[k];
        const float v = rel * b.scale[k];
        c[k] = b.bits[k] ? cast_cell(v, 1u << b.bits[k]) : 0u;
    }
}

// The direction's cell: the octahedral map of d / (|dx| + |dy| + |dz|) onto
// [-1, 1]^2 (the lower hemisphere, dy < 0, folded over the diagonals), each
// coordinate cut into 2^kCastDirBits cells. A zero, infinite or NaN direction
// makes NaN coordinates, which cast_cell sends to cell 0.
RTX_CAST_HD void cast_dir_cells(const float *d, uint32_t *c) {
    RTX_CAST_NO_CONTRACT
    const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
    const float s = (ax + ay) + az;
    float u = d[0] / s, v = d[2] / s;
    if (d[1] < 0.0f) {
        const float fu = 1.0f - fabsf(v), fv = 1.0f - fabsf(u);
        const float su = u < 0.0f ? -fu : fu, sv = v < 0.0f ? -fv : fv;
        u = su, v = sv;
    }
    const float cells = (float)(1u << kCastDirBits);
    const float hu = u * 0.5f, hv = v * 0.5f;
    const float pu = hu + 0.5f, pv = hv + 0.5f;
    c[0] = cast_cell(pu * cells, 1u << kCastDirBits);
    c[1] = cast_cell(pv * cells, 1u << kCastDirBits);
}

// The key of cells (origin x, y, z; direction u, v): the origin cells' bits
// interleaved from the top (an axis joins once its bits reach the level), then
// the two direction cells' bits interleaved. A bijection of the cells, below
// kCastBuckets; neighbouring keys are neighbouring cells.
RTX_CAST_HD uint32_t cast_key_of_cells(const CastBox &b, const uint32_t *oc, const uint32_t *dc) {
    uint32_t key = 0u;
    for (uint32_t level = kCastOriginBits; level-- > 0u;)
        for (int k = 0; k < 3; ++k)
            if (b.bits[k] > level) key = (key << 1) | ((oc[k] >> level) & 1u);
    for (uint32_t level = kCastDirBits; level-- > 0u;) {
        key = (key << 1) | ((dc[0] >> level) & 1u);
        key = (key << 1) | ((dc[1] >> level) & 1u);
    }
    return key;
}

// A ray's key, total over every bit pattern of (o, d).
RTX_CAST_HD uint32_t cast_key(const CastBox &b, const float *o, const float *d) {
    uint32_t oc[3], dc[2];
    cast_origin_cells(b, o, oc);
    cast_dir_cells(d, dc);
    return cast_key_of_cells(b, oc, dc);
}

// RTX_CAST_ORDER_AUTO for a batch of n rays on a scene of class `kernels`
// (rtx_internal.h SceneKernels: 0 small, 1 large culled, 2 large linear):
// whether the call sorts. From tools/cast_time.py (RESULTS.md "rtx_cast_rays"):
// on the 100k-sphere scene under the culled scan the sorted call, key passes
// included, beat the given order on the shuffled centre rays (2.07 M: 1.91
// against 2.58 ms) and on the AO batch (7.48 M: 4.61 against 5.06 ms) by more
// than three times the given order's window spread; on the 486-sphere scene
// it lost on both (0.24 against 0.13 ms, 0.69 against 0.22 ms). Smaller
// batches and the large linear class were not measured and keep the given
// order. AUTO cannot see whether a batch is coherent already: rays in pixel or
// patch order lose about 0.2 ms to the sort (0.68 against 0.45 ms), so a
// caller that knows its rays are ordered passes GIVEN.
constexpr uint32_t kCastAutoNever = 0xffffffffu;
constexpr uint32_t kCastAutoMinSmall = kCastAutoNever;
constexpr uint32_t kCastAutoMinCulled = 2000000u;
constexpr uint32_t kCastAutoMinLinear = kCastAutoNever;
RTX_CAST_HD bool cast_auto_coherent(uint32_t n, uint32_t kernels) {
    const uint32_t bar = kernels == 0u ? kCastAutoMinSmall : kernels == 1u ? kCastAutoMinCulled : kCastAutoMinLinear;
    return bar != kCastAutoNever && n >= bar;
}

}  // namespace rtx
