// rtx_cull.h — the culled layout of a large scene (n_pad > kScanPfMin;
// DESIGN.md §3e; rtx_internal.h KScene), built once at rtx_upload_world and
// shared by the upload (rtx_api.hip) and the CPU checker
// (tests/cull_check.cpp). Host code only.
//
// Sections of spheres — large ones (|r| > 8x the median), the other non-flat
// ones, the flat ones (height flat_cy, when the scene has a flat run) — each
// in Morton order of its centres (x, z for the flat section; x, y, z
// otherwise) and padded to whole blocks with copies of its last sphere whose
// prefilter R is -inf: never flagged (Q = -inf), except by a lane outside the
// prefilter's safe region (thr = -inf flags everything), which then resolves
// the copy to the same key as the sphere itself — no result changes either way.
// Three levels of bounds (rtx_prefilter.h cull_bound) sit above the blocks:
// one per block (8 spheres), per group (64) and per super-group (512), each
// level stored in AoSoA-8 rows of 8 entries.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "rtx_prefilter.h"

namespace rtx {

// The culled layout has three bound levels above the blocks (groups,
// super-groups, 512-block ranges; two levels: 187.5 vs 128.8 ms, RESULTS R9zb),
// and its flat section starts at a multiple of this many blocks: no bound test
// (8 entries) mixes flat and non-flat bounds
constexpr uint32_t kCullAlign = 512u;

struct CullLayout {
    std::vector<float> pre, bnd, bnd2, bnd3;
    std::vector<uint32_t> perm;
    std::vector<uint8_t> pad;  // position holds a padding copy
    uint32_t flat_lo = 0;
};

inline uint32_t cull_bits(float v) {
    uint32_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

// spheres: (cx, cy, cz, r)[n] as uploaded, n > 0; pre4: (cx, cy, cz,
// prefilter_R)[n], the records of the scene-order `pre`; has_flat, flat_cy:
// whether the scene has a scene-order flat run, and its height.
inline CullLayout build_cull(const float *spheres, uint32_t n, const float *pre4, bool has_flat, float flat_cy) {
    const float *S = spheres;
    std::vector<float> rs(n);
    for (uint32_t i = 0; i < n; ++i) rs[i] = fabsf(S[4 * i + 3]);
    std::nth_element(rs.begin(), rs.begin() + n / 2, rs.end());
    const float big = 8.0f * rs[n / 2];
    std::vector<uint32_t> sec[3];
    for (uint32_t i = 0; i < n; ++i) {
        const bool fl = has_flat && cull_bits(S[4 * i + 1]) == cull_bits(flat_cy);
        sec[fabsf(S[4 * i + 3]) > big ? 0 : fl ? 2 : 1].push_back(i);
    }
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) lo[k] = std::min(lo[k], (double)S[4 * i + k]), hi[k] = std::max(hi[k], (double)S[4 * i + k]);
    auto q = [&](uint32_t i, int k) -> uint64_t {
        const double span = hi[k] - lo[k];
        return span > 0.0 ? (uint64_t)std::min(1023.0, floor(((double)S[4 * i + k] - lo[k]) / span * 1024.0)) : 0;
    };
    auto morton = [&](uint32_t i, bool flat) {
        uint64_t key = 0;
        for (int bit = 0; bit < 10; ++bit) {
            if (flat)
                key |= ((q(i, 0) >> bit) & 1u) << (2 * bit) | ((q(i, 2) >> bit) & 1u) << (2 * bit + 1);
            else
                key |= ((q(i, 0) >> bit) & 1u) << (3 * bit) | ((q(i, 1) >> bit) & 1u) << (3 * bit + 1) |
                       ((q(i, 2) >> bit) & 1u) << (3 * bit + 2);
        }
        return key;
    };
    CullLayout L;
    for (int k = 0; k < 3; ++k) {
        if (sec[k].empty()) continue;
        std::stable_sort(sec[k].begin(), sec[k].end(),
                         [&](uint32_t a, uint32_t b) { return morton(a, k == 2) < morton(b, k == 2); });
        if (k == 2) {
            // the flat section starts at a multiple of kCullAlign blocks, so
            // that no bound test (8 entries of 1, 8 or 64 blocks) mixes flat
            // and non-flat bounds; the padding blocks' bounds never pass (R = -inf)
            while (!L.perm.empty() && (L.perm.size() / 8) % kCullAlign != 0) {
                const uint32_t last = L.perm.back();
                for (int i = 0; i < 8; ++i) L.perm.push_back(last), L.pad.push_back(1);
            }
            L.flat_lo = (uint32_t)L.perm.size() / 8;
        }
        for (uint32_t i : sec[k]) L.perm.push_back(i), L.pad.push_back(0);
        while (L.perm.size() % 8) L.perm.push_back(sec[k].back()), L.pad.push_back(1);
    }
    if (sec[2].empty()) L.flat_lo = (uint32_t)L.perm.size() / 8;
    const uint32_t np = (uint32_t)L.perm.size(), nblk = np / 8, ngrp = (nblk + 7) / 8;
    // the bound of positions [p0, p1): over their spheres; R = -inf when they are all padding
    auto bound_of = [&](uint32_t p0, uint32_t p1, bool fl) {
        std::vector<const float *> sp;
        bool all_pad = true;
        for (uint32_t p = p0; p < std::min(p1, np); ++p) sp.push_back(&S[4 * (size_t)L.perm[p]]), all_pad &= L.pad[p] != 0;
        CullBound cb = cull_bound(sp.data(), (int)sp.size(), fl, flat_cy, fl ? kCullSy : 1.0f);
        if (all_pad) cb.R = -INFINITY;
        return cb;
    };
    L.pre.assign(4 * (size_t)np, 0.0f);
    for (uint32_t p = 0; p < np; ++p) {
        const float *v = &pre4[4 * (size_t)L.perm[p]];
        float *blk = &L.pre[32 * (size_t)(p / 8)];
        blk[p % 8] = v[0], blk[8 + p % 8] = v[1], blk[16 + p % 8] = v[2], blk[24 + p % 8] = L.pad[p] ? -INFINITY : v[3];
    }
    L.bnd.assign(32 * (size_t)ngrp, 0.0f);
    for (uint32_t g = 0; g < ngrp; ++g)
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t b = 8 * g + j;
            float *gb = &L.bnd[32 * (size_t)g];
            if (b >= nblk) {  // past the last block: masked off by the kernel; flat height for a flat group
                gb[8 + j] = 8 * g >= L.flat_lo ? kCullSy * flat_cy : 0.0f;
                continue;
            }
            const CullBound cb = bound_of(8 * b, 8 * b + 8, b >= L.flat_lo);  // flat: stretched along y
            gb[j] = cb.cx, gb[8 + j] = cb.cy, gb[16 + j] = cb.cz, gb[24 + j] = cb.R;
        }
    // the top level: one bound over each group's 64 spheres, 8 groups per super-group
    const uint32_t nsg = (ngrp + 7) / 8;
    L.bnd2.assign(32 * (size_t)nsg, 0.0f);
    for (uint32_t s = 0; s < nsg; ++s)
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t g = 8 * s + j;
            float *gb = &L.bnd2[32 * (size_t)s];
            if (g >= ngrp) {
                gb[8 + j] = 64 * s >= L.flat_lo ? kCullSy * flat_cy : 0.0f;
                continue;
            }
            const CullBound cb = bound_of(64 * g, 64 * g + 64, 8 * g >= L.flat_lo);
            gb[j] = cb.cx, gb[8 + j] = cb.cy, gb[16 + j] = cb.cz, gb[24 + j] = cb.R;
        }
    // the third level: one bound over each super-group's 512 spheres, 8 per entry of bnd3
    const uint32_t nhg = (nsg + 7) / 8;
    L.bnd3.assign(32 * (size_t)nhg, 0.0f);
    for (uint32_t h = 0; h < nhg; ++h)
        for (uint32_t j = 0; j < 8; ++j) {
            const uint32_t sg = 8 * h + j;
            float *gb = &L.bnd3[32 * (size_t)h];
            if (sg >= nsg) {
                gb[8 + j] = 512 * h >= L.flat_lo ? kCullSy * flat_cy : 0.0f;
                continue;
            }
            const CullBound cb = bound_of(512 * sg, 512 * sg + 512, 64 * sg >= L.flat_lo);
            gb[j] = cb.cx, gb[8 + j] = cb.cy, gb[16 + j] = cb.cz, gb[24 + j] = cb.R;
        }
    return L;
}

}  // namespace rtx
