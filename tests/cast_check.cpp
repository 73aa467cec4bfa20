// cast_check.cpp — CPU checker of rtx_cast_rays' COHERENT order
// (raytrace-we-gpu_amd/csrc/rtx_cast.h), the text the kernels and
// rtx_upload_world run. Stand-alone: its own main, no HIP, no library. Build
// with -ffp-contract=off. Prints one JSON line; exit status 0 iff every check
// held.
//
//   1. the box of the scene's body: a 1000-radius ground is not part of it,
//      the origin bits add up to kCastOriginBits and go to the long axes; a
//      scene without an extent (no sphere, one sphere, every centre equal)
//      keeps no bits
//   2. over every box: seeded random rays, every hostile class of
//      tests/hostile_rays.h, and rays of random bit patterns (NaN payloads,
//      denormals, infinities, 1e38) — the key is below kCastBuckets, the same
//      when computed again, and a function of the cells that is one to one:
//      equal cells give equal keys, other cells another key
//   3. cast_cell on the values a conversion must never see
//   4. a reference counting sort over those keys (histogram, prefix, scatter)
//      yields a permutation of 0 .. n-1 with the keys in order
//   5. the record sizes of include/rtx.h
//   6. the AUTO rule: COHERENT for a large culled scene from 2,000,000 rays,
//      GIVEN for every other class and size
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "../include/rtx.h"
#include "../raytrace-we-gpu_amd/csrc/rtx_cast.h"
#include "hostile_rays.h"

using namespace rtx;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}
static float unit() { return (float)(rnd() >> 8) * (1.0f / 16777216.0f); }
static float span(float lo, float hi) { return lo + (hi - lo) * unit(); }
static float from_bits(uint32_t u) {
    float v;
    std::memcpy(&v, &u, 4);
    return v;
}

struct Ray { float o[3], d[3]; };

// The ground and n - 1 small spheres over x, z in +-ext at heights in [0.2, 0.2 + tall].
static std::vector<float> scene(uint32_t n, float ext_x, float ext_z, float tall) {
    std::vector<float> s(4 * (size_t)n);
    for (uint32_t i = 0; i < n; ++i) {
        s[4 * i + 0] = span(-ext_x, ext_x);
        s[4 * i + 1] = 0.2f + tall * unit();
        s[4 * i + 2] = span(-ext_z, ext_z);
        s[4 * i + 3] = span(0.1f, 0.3f);
    }
    if (n) s[0] = 0.0f, s[1] = -1000.0f, s[2] = 0.0f, s[3] = 1000.0f;
    return s;
}
static CastBox box_of(const std::vector<float> &s) {
    std::vector<float> radii(s.size() / 4 + 1);
    return cast_box(s.data(), (uint32_t)(s.size() / 4), radii.data());
}

int main() {
    long box_bad = 0, key_checks = 0, range_bad = 0, repeat_bad = 0, cells_bad = 0, cell_edge_bad = 0, sort_bad = 0;
    long hostile_checks = 0, bits_checks = 0, distinct_keys = 0;

    // 1. boxes
    std::vector<CastBox> boxes;
    {
        const std::vector<float> a = scene(486, 11.0f, 11.0f, 0.8f);  // a flat layer over a ground
        const CastBox b = box_of(a);
        boxes.push_back(b);
        if (b.bits[0] + b.bits[1] + b.bits[2] != kCastOriginBits) ++box_bad;
        if (!(b.lo[0] >= -11.0f && b.lo[1] >= 0.2f && b.lo[2] >= -11.0f)) ++box_bad;  // not the ground's -1000
        if (!(b.bits[0] >= 4u && b.bits[2] >= 4u && b.bits[1] <= 2u)) ++box_bad;      // the long axes
        for (int k = 0; k < 3; ++k)
            if (b.bits[k] && !(b.scale[k] > 0.0f && std::isfinite(b.scale[k]))) ++box_bad;
        const std::vector<float> c = scene(2500, 30.0f, 2.0f, 20.0f);  // a strip, tall
        const CastBox bc = box_of(c);
        boxes.push_back(bc);
        if (bc.bits[0] + bc.bits[1] + bc.bits[2] != kCastOriginBits || !(bc.bits[0] > bc.bits[2])) ++box_bad;
        // no extent: no sphere, one sphere, every centre equal, only the x axis
        std::vector<float> none, one = {1.0f, 2.0f, 3.0f, 0.5f}, same, line;
        for (int i = 0; i < 9; ++i) {
            const float s4[4] = {1.0f, 2.0f, 3.0f, 0.25f};
            same.insert(same.end(), s4, s4 + 4);
            const float l4[4] = {(float)i, 2.0f, 3.0f, 0.25f};
            line.insert(line.end(), l4, l4 + 4);
        }
        for (const std::vector<float> *s : {&none, &one, &same}) {
            const CastBox z = box_of(*s);
            boxes.push_back(z);
            if (z.bits[0] | z.bits[1] | z.bits[2]) ++box_bad;
            if (z.scale[0] != 0.0f || z.scale[1] != 0.0f || z.scale[2] != 0.0f) ++box_bad;
        }
        const CastBox bl = box_of(line);
        boxes.push_back(bl);
        if (bl.bits[0] != kCastOriginBits || bl.bits[1] || bl.bits[2]) ++box_bad;
        // radii of either sign, zero and 1e-30 (the degenerate worlds of the GPU tests)
        std::vector<float> odd = scene(600, 11.0f, 11.0f, 0.8f);
        for (uint32_t i = 1; i < 600; i += 4) hostile::degenerate_sphere(odd.data(), i, (int)(i / 4), true);
        const CastBox bo = box_of(odd);
        boxes.push_back(bo);
        if (bo.bits[0] + bo.bits[1] + bo.bits[2] != kCastOriginBits) ++box_bad;
    }

    // 2. keys
    const float centre[4] = {1.5f, 0.25f, -2.0f, 0.25f};
    std::vector<uint32_t> all_keys;
    for (const CastBox &b : boxes) {
        std::map<uint64_t, uint32_t> key_of_cells;
        std::map<uint32_t, uint64_t> cells_of_key;
        auto check = [&](const Ray &r) {
            uint32_t oc[3], dc[2];
            cast_origin_cells(b, r.o, oc);
            cast_dir_cells(r.d, dc);
            const uint32_t key = cast_key(b, r.o, r.d);
            ++key_checks;
            if (key >= kCastBuckets) ++range_bad;
            if (cast_key(b, r.o, r.d) != key || cast_key_of_cells(b, oc, dc) != key) ++repeat_bad;
            for (int k = 0; k < 3; ++k)
                if (oc[k] >= (1u << b.bits[k])) ++range_bad;
            if (dc[0] >= (1u << kCastDirBits) || dc[1] >= (1u << kCastDirBits)) ++range_bad;
            const uint64_t cells = ((uint64_t)oc[0] << 48) | ((uint64_t)oc[1] << 36) | ((uint64_t)oc[2] << 24) |
                                   ((uint64_t)dc[0] << 8) | dc[1];
            const auto a = key_of_cells.emplace(cells, key);
            if (a.first->second != key) ++cells_bad;  // equal cells, another key
            const auto c = cells_of_key.emplace(key, cells);
            if (c.first->second != cells) ++cells_bad;  // other cells, the same key
            all_keys.push_back(key);
        };
        for (int it = 0; it < 20000; ++it) {
            Ray r;
            for (int k = 0; k < 3; ++k) r.o[k] = span(-30.0f, 30.0f), r.d[k] = span(-1.0f, 1.0f);
            if (it % 7 == 0) r.o[1] = span(0.0f, 1.0f);
            check(r);
            if (it % 8 == 0) {  // ... and its hostile version, every class in turn
                hostile::hostile_ray(it / 8, centre, r.o, r.d);
                check(r);
                ++hostile_checks;
            }
        }
        for (int it = 0; it < 20000; ++it) {  // any bit pattern at all
            Ray r;
            for (int k = 0; k < 3; ++k) r.o[k] = from_bits(rnd()), r.d[k] = from_bits(rnd());
            check(r);
            ++bits_checks;
        }
        const float edge[] = {0.0f, -0.0f, 1e38f, -1e38f, 1e-45f, -1e-45f, 3e-39f, std::numeric_limits<float>::infinity(),
                              -std::numeric_limits<float>::infinity(), std::nanf(""), from_bits(0xffc00001u),
                              std::numeric_limits<float>::max(), std::numeric_limits<float>::min()};
        for (float eo : edge)
            for (float ed : edge)
                for (int k = 0; k < 3; ++k) {
                    Ray r = {{1.0f, 0.5f, -1.0f}, {0.3f, -0.2f, 0.9f}};
                    r.o[k] = eo;
                    r.d[(k + 1) % 3] = ed;
                    check(r);
                    Ray q = {{eo, eo, eo}, {ed, ed, ed}};
                    check(q);
                }
        distinct_keys += (long)cells_of_key.size();
    }

    // 3. cast_cell: floor, clamped, total
    {
        const float inf = std::numeric_limits<float>::infinity();
        struct E { float v; uint32_t cells, want; };
        const E e[] = {{std::nanf(""), 8, 0}, {-inf, 8, 0}, {inf, 8, 7}, {-1.0f, 8, 0}, {0.999f, 8, 0}, {1.0f, 8, 1},
                       {6.999f, 8, 6}, {7.0f, 8, 7}, {1e38f, 8, 7}, {4294967296.0f, 1024, 1023}, {1e-45f, 8, 0},
                       {5.0f, 1, 0}, {1022.5f, 1024, 1022}, {-0.0f, 2, 0}, {3e9f, 2, 1}};
        for (const E &x : e)
            if (cast_cell(x.v, x.cells) != x.want) ++cell_edge_bad;
    }

    // 4. the counting sort the three passes do, on the host
    {
        const size_t n = all_keys.size();
        std::vector<uint32_t> count(kCastBuckets, 0u), perm(n, 0xffffffffu);
        for (uint32_t k : all_keys) ++count[k];
        uint32_t pre = 0;
        for (uint32_t b = 0; b < kCastBuckets; ++b) {
            const uint32_t c = count[b];
            count[b] = pre;
            pre += c;
        }
        if (pre != n) ++sort_bad;
        for (size_t i = 0; i < n; ++i) perm[count[all_keys[i]]++] = (uint32_t)i;
        std::vector<uint8_t> seen(n, 0);
        for (size_t g = 0; g < n; ++g) {
            if (perm[g] >= n || seen[perm[g]]) {
                ++sort_bad;
                continue;
            }
            seen[perm[g]] = 1;
            if (g && all_keys[perm[g - 1]] > all_keys[perm[g]]) ++sort_bad;
        }
    }

    // 5. the records
    const long size_bad = (sizeof(rtx_ray) != 32) + (sizeof(rtx_ray_hit) != 32) + (offsetof(rtx_ray, t_max) != 12) +
                          (offsetof(rtx_ray, d) != 16) + (offsetof(rtx_ray_hit, index) != 4) +
                          (offsetof(rtx_ray_hit, normal) != 8) + (offsetof(rtx_ray_hit, front_face) != 20);

    // 6. AUTO (scene classes: 0 small, 1 large culled, 2 large linear)
    long auto_bad = 0;
    for (uint32_t n : {1u, 1999999u, 2000000u, 0xffffffffu})
        for (uint32_t cls = 0; cls < 3u; ++cls)
            if (cast_auto_coherent(n, cls) != (cls == 1u && n >= 2000000u)) ++auto_bad;

    std::printf("{\"boxes\": %zu, \"box_bad\": %ld, \"key_checks\": %ld, \"hostile_checks\": %ld, \"bits_checks\": %ld, "
                "\"range_bad\": %ld, \"repeat_bad\": %ld, \"cells_bad\": %ld, \"distinct_keys\": %ld, "
                "\"cell_edge_bad\": %ld, \"sorted\": %zu, \"sort_bad\": %ld, \"size_bad\": %ld, \"auto_bad\": %ld, \"buckets\": %u}\n",
                boxes.size(), box_bad, key_checks, hostile_checks, bits_checks, range_bad, repeat_bad, cells_bad,
                distinct_keys, cell_edge_bad, all_keys.size(), sort_bad, size_bad, auto_bad, kCastBuckets);
    return (box_bad || range_bad || repeat_bad || cells_bad || cell_edge_bad || sort_bad || size_bad || auto_bad) ? 1 : 0;
}
