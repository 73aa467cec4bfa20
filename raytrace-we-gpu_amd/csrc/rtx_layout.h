// rtx_layout.h — the spatial layout of a small scene's sphere layer
// (DESIGN.md §3f), built once at rtx_upload_world and shared by the upload
// (rtx_api.hip), the CPU checker (tests/layout_check.cpp) and the block-count
// tool (tools/layout_blocks.cpp). Host code only.
//
// The lane-mode scan visits the flat run in blocks of 8 spheres, and the layer
// grid (rtx_grid.h) marks, per cell, every block with a disc in the cell. A
// block of 8 consecutive spheres in scene order is whatever the scene's author
// emitted in a row — for the RTIOW worlds a 1 x 8 strip of the layer — and a
// ray's stretch through the slab, let alone the union over a wave's 64 rays,
// crosses many thin strips. The same spheres grouped into compact patches are
// met by fewer stretches, so fewer blocks are marked and scanned. The order of
// the scan is free: the resolve's rule (smallest root, then the later scene
// index) does not depend on it (rtx_kernels.hip hit_world_pre_ld), and every
// list entry is mapped back to its scene index before it is resolved.
//
// The layer is the largest set of spheres whose centre heights are
// bit-identical, wherever they sit in scene order (two sets of equal size:
// the one whose first sphere comes first). A scene whose layer has fewer than
// kLayoutMinLayer or more than kLayoutMaxLayer spheres (64 blocks, the width
// of a cell's mask) has no layout.
//
// Positions: the off-layer spheres first, in scene order, then the layer in
// the spatial order; each section padded to a multiple of 8 with copies of its
// own last sphere (a copy maps to that sphere's scene index and carries
// R = -inf, so the prefilter does not flag it; were it flagged all the same,
// by a ray outside the test's safe range, it resolves to its sphere's own
// key: harmless). Every layer block is flat and the flat run, blocks
// [flat_lo, flat_hi), is contiguous by construction.
#pragma once

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <utility>
#include <vector>

#include "rtx_grid.h"
#include "rtx_prefilter.h"

namespace rtx {

constexpr uint32_t kLayoutMinLayer = 16;   // a smaller layer is not worth a layout
constexpr uint32_t kLayoutMaxLayer = 512;  // 64 blocks: the layer grid's mask

// The order of the layer's spheres.
//   kLayoutMedian  recursive median split of (x, z) along the longer extent,
//                  halves sized in whole blocks, leaves of 8
//   kLayoutTiles   fixed tiles of tx x tz mean sphere spacings, tile by tile
//   kLayoutScene   scene order (the comparison)
enum LayoutOrder : int { kLayoutScene = 0, kLayoutMedian = 1, kLayoutTiles = 2 };
// The order rtx_upload_world uses: chosen by tools/layout_blocks.cpp on the
// RTIOW worlds (RESULTS.md, "block order").
constexpr LayoutOrder kLayoutDefault = kLayoutMedian;

struct SceneLayout {
    bool valid = false;
    std::vector<float> pre;      // AoSoA-8 (cx cy cz R) by position, R = prefilter_R as in `pre`
    std::vector<uint32_t> perm;  // position -> scene index
    uint32_t flat_lo = 0, flat_hi = 0;  // the layer's blocks
    float flat_cy = 0.0f;               // the layer's height
    uint32_t n_layer = 0;               // layer spheres (without pads)
    bool has_grid = false;              // the layer grid over position blocks (bit j: block flat_lo + j)
    LayerGrid grid{};
    std::vector<unsigned long long> cell;
};

inline uint32_t layout_bits(float v) {
    uint32_t b;
    memcpy(&b, &v, sizeof b);
    return b;
}

// The layer of `n` spheres sph[4 i] = (cx, cy, cz, r): its scene indices,
// ascending. Empty when the scene has none of a usable size.
inline std::vector<uint32_t> layout_find_layer(const float *sph, uint32_t n) {
    std::map<uint32_t, std::pair<uint32_t, uint32_t>> sets;  // height bits -> (count, first index)
    for (uint32_t i = 0; i < n; ++i) {
        auto it = sets.find(layout_bits(sph[4 * (size_t)i + 1]));
        if (it == sets.end())
            sets.emplace(layout_bits(sph[4 * (size_t)i + 1]), std::make_pair(1u, i));
        else
            ++it->second.first;
    }
    uint32_t best_cnt = 0, best_first = 0, best_bits = 0;
    for (const auto &s : sets)
        if (s.second.first > best_cnt || (s.second.first == best_cnt && s.second.second < best_first))
            best_cnt = s.second.first, best_first = s.second.second, best_bits = s.first;
    std::vector<uint32_t> ids;
    if (best_cnt < kLayoutMinLayer || best_cnt > kLayoutMaxLayer) return ids;
    for (uint32_t i = 0; i < n; ++i)
        if (layout_bits(sph[4 * (size_t)i + 1]) == best_bits) ids.push_back(i);
    return ids;
}

// Recursive median split: ids[lo, hi) sorted by the coordinate of the longer
// extent (ties: scene index), cut at a whole number of blocks.
inline void layout_median_split(const float *sph, std::vector<uint32_t> &ids, size_t lo, size_t hi) {
    const size_t m = hi - lo;
    if (m <= 8) {
        std::sort(ids.begin() + lo, ids.begin() + hi);  // a leaf: scene order inside the block
        return;
    }
    float xlo = INFINITY, xhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
    for (size_t k = lo; k < hi; ++k) {
        const float x = sph[4 * (size_t)ids[k]], z = sph[4 * (size_t)ids[k] + 2];
        xlo = std::min(xlo, x), xhi = std::max(xhi, x), zlo = std::min(zlo, z), zhi = std::max(zhi, z);
    }
    const int ax = (zhi - zlo) > (xhi - xlo) ? 2 : 0;
    std::sort(ids.begin() + lo, ids.begin() + hi, [&](uint32_t a, uint32_t b) {
        const float ca = sph[4 * (size_t)a + ax], cb = sph[4 * (size_t)b + ax];
        return ca < cb || (ca == cb && a < b);
    });
    const size_t nb = (m + 7) / 8;
    const size_t mid = lo + 8 * (nb / 2);  // nb >= 2: both halves are non-empty
    layout_median_split(sph, ids, lo, mid);
    layout_median_split(sph, ids, mid, hi);
}

// Fixed tiles: tx x tz mean spacings (sqrt(area / m)), tiles in x-major
// order, scene order inside a tile; blocks are consecutive runs of 8.
inline void layout_tiles(const float *sph, std::vector<uint32_t> &ids, uint32_t tx, uint32_t tz) {
    float xlo = INFINITY, xhi = -INFINITY, zlo = INFINITY, zhi = -INFINITY;
    for (uint32_t i : ids) {
        const float x = sph[4 * (size_t)i], z = sph[4 * (size_t)i + 2];
        xlo = std::min(xlo, x), xhi = std::max(xhi, x), zlo = std::min(zlo, z), zhi = std::max(zhi, z);
    }
    const double area = std::max((double)(xhi - xlo) * (double)(zhi - zlo), 1e-30);
    const double s = std::sqrt(area / (double)ids.size());
    auto key = [&](uint32_t i) {
        const long kx = (long)std::floor((sph[4 * (size_t)i] - xlo) / (s * tx));
        const long kz = (long)std::floor((sph[4 * (size_t)i + 2] - zlo) / (s * tz));
        return std::make_pair(kx, kz);
    };
    std::sort(ids.begin(), ids.end(), [&](uint32_t a, uint32_t b) {
        const auto ka = key(a), kb = key(b);
        return ka < kb || (ka == kb && a < b);
    });
}

// The layer's spheres `ids` (scene order on entry) in the given order.
inline void layout_order(const float *sph, std::vector<uint32_t> &ids, LayoutOrder order, uint32_t tx = 4,
                         uint32_t tz = 2) {
    if (order == kLayoutMedian)
        layout_median_split(sph, ids, 0, ids.size());
    else if (order == kLayoutTiles)
        layout_tiles(sph, ids, tx, tz);
}

// The layout of a scene of `n` spheres, with the layer grid over its position
// blocks; valid = false when it has none.
inline SceneLayout build_scene_layout(const float *sph, uint32_t n, LayoutOrder order = kLayoutDefault,
                                      uint32_t tx = 4, uint32_t tz = 2) {
    SceneLayout L;
    std::vector<uint32_t> layer = layout_find_layer(sph, n);
    if (layer.empty()) return L;
    L.n_layer = (uint32_t)layer.size();
    L.flat_cy = sph[4 * (size_t)layer[0] + 1];
    std::vector<char> in_layer(n, 0);
    for (uint32_t i : layer) in_layer[i] = 1;
    layout_order(sph, layer, order, tx, tz);
    std::vector<char> pad;
    for (uint32_t i = 0; i < n; ++i)
        if (!in_layer[i]) L.perm.push_back(i), pad.push_back(0);
    while (L.perm.size() % 8) L.perm.push_back(L.perm.back()), pad.push_back(1);
    L.flat_lo = (uint32_t)(L.perm.size() / 8);
    for (uint32_t i : layer) L.perm.push_back(i), pad.push_back(0);
    while (L.perm.size() % 8) L.perm.push_back(L.perm.back()), pad.push_back(1);
    L.flat_hi = (uint32_t)(L.perm.size() / 8);
    const size_t np = L.perm.size();
    L.pre.assign(4 * np, 0.0f);
    for (size_t p = 0; p < np; ++p) {
        const float *s = sph + 4 * (size_t)L.perm[p];
        float *blk = &L.pre[32 * (p / 8)];
        blk[p % 8] = s[0], blk[8 + p % 8] = s[1], blk[16 + p % 8] = s[2];
        // a pad's R is -inf: the prefilter never flags it where the test is
        // in its safe range (its sphere is flagged at its own position; with
        // the same R every ray near a padded section's last sphere — one of
        // the RTIOW worlds' three large ones — would resolve it once per copy)
        blk[24 + p % 8] = pad[p] ? -INFINITY : prefilter_R(s[0], s[1], s[2], s[3] * s[3]);
    }
    L.has_grid = build_layer_grid_pos(sph, L.perm.data(), 8 * L.flat_lo, 8 * L.flat_hi, L.grid, L.cell);
    L.valid = true;
    return L;
}

}  // namespace rtx
